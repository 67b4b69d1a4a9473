"""PCGAMG on the device: MatCoarsenAggregate on both routes against the model, the PC against a PCMG given the model's prolongators by
hand (bit for bit) and against the dense model (1e-10 relative, as tests/test_pcmg_gpu.py asks of PCMG), iteration counts, the stopping
rules, the refusals that need a device copy, the reuse option, destruction order, and the README's example."""
import numpy as np
import pytest

import gamg_ref as gr
import mg_ref as mr
from test_gamg_cpu import model, raises

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP, PETSC_ERR_ARG_WRONGSTATE = 56, 73


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture()
def opts(P):
    L = P.lib()

    def set_(text=""):
        L.PetscOptionsClear()
        if text:
            L.PetscOptionsInsertString(text.encode())
    set_()
    yield set_
    L.PetscOptionsClear()


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def gamg_ksp(P, A, ksptype="preonly", **kw):
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_type(ksptype)
    ksp.set_pc_type("gamg")
    ksp.set_operators(A)
    pc = ksp.get_pc()
    for k, v in kw.items():
        getattr(pc, "gamg_set_" + k)(v)
    return ksp, pc


def hand_built(P, A, H):
    """a PCMG given the model's prolongators and configured as PCGAMG configures its own"""
    L = P.lib()
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_type("preonly")
    ksp.set_pc_type("mg")
    ksp.set_operators(A)
    pc = ksp.get_pc()
    pc.mg_set_levels(H.n); pc.mg_set_galerkin(True)
    sizes = H.sizes[::-1]
    for l in range(1, H.n):
        pc.mg_set_interpolation(l, P.Mat.from_csr(*H.Ps[l], ncols=sizes[l - 1]))
        s = pc.mg_get_smoother(l)
        s.set_type("chebychev"); s.set_pc_type("jacobi"); s.set_norm_type("none"); s.set_tolerances(max_it=2)
        s.set_chebychev_eigenvalues(H.rho_mg[l], H.rho_mg[l] / 10.0)
    c = pc.mg_get_coarse_solve()
    c.set_pc_type("ilu")
    L.PCFactorSetLevels(c.get_pc().h, sizes[0])
    return ksp, pc


def apply(P, pc, v):
    x = P.Vec.from_array(v)
    y = x.duplicate()
    pc.apply(x, y)
    return y.array()


CASES = [("p7_5_4_3", gr.poisson7(5, 4, 3), 0.0, 10), ("p2d_16", gr.poisson2d(16), 0.0, 50), ("aniso12", gr.anisotropic(12), 0.1, 20)]


@pytest.mark.parametrize("name,csr,theta", [("p7_5_4_3", gr.poisson7(5, 4, 3), 0.0), ("upwind9", gr.upwind(9), 0.25), ("aniso12", gr.anisotropic(12), 0.1),
                                            ("holes", gr.with_empty_rows_and_isolated_nodes(), 0.5), ("sym3000", gr.random_graph(3000, 3, 5, True), 0.0)])
def test_device_route_equals_host_route_equals_the_model(P, opts, name, csr, theta):
    _, want, wn = gr.aggregate(*csr, theta)
    got = {}
    for route in ("device", "host"):
        opts("-mat_hipmi355x_coarsen " + route)
        A = P.Mat.from_csr(*csr)
        got[route] = A.aggregate(theta)
        dev, host, rounds = A.coarsen_counts()
        assert (dev, host) == ((1, 0) if route == "device" else (0, 1)) and (rounds >= 1) == (route == "device")
    opts()
    A = P.Mat.from_csr(*csr)
    A.aggregate(theta)
    assert A.coarsen_counts()[:2] == (1, 0)                             # the default with a device
    for route in got:
        assert got[route][1] == wn and np.array_equal(got[route][0], want), (name, route)


def test_changed_values_change_the_aggregates_only_through_the_strengths(P):
    ai, aj, aa = gr.anisotropic(12)
    A = P.Mat.from_csr(ai, aj, aa)
    base = A.aggregate(0.1)
    P.lib().MatScale(A.h, 3.0)                                          # every |a| and every bound scale alike: the same mask
    same = A.aggregate(0.1)
    assert same[1] == base[1] and np.array_equal(same[0], base[0])
    B = P.Mat.from_csr(ai, aj, np.where(np.abs(aa) < 0.5, aa * 500.0, aa))   # the weak direction made strong
    other = B.aggregate(0.1)
    _, want, wn = gr.aggregate(ai, aj, np.where(np.abs(aa) < 0.5, aa * 500.0, aa), 0.1)
    assert other[1] == wn and np.array_equal(other[0], want) and other[1] != base[1]
    assert A.coarsen_counts()[0] == 2


@pytest.mark.parametrize("name,csr,theta,limit", CASES, ids=[c[0] for c in CASES])
def test_apply_equals_the_hand_built_pcmg_and_the_dense_model(P, name, csr, theta, limit):
    H = gr.Hierarchy(*csr, theta=theta, coarse_eq_limit=limit)
    assert H.n >= 2
    A = P.Mat.from_csr(*csr)
    ksp, pc = gamg_ksp(P, A, threshold=theta, coarse_eq_limit=limit)
    pc.set_up()
    assert pc.gamg_level_sizes() == H.sizes and pc.mg_get_levels() == H.n
    ksp2, pc2 = hand_built(P, A, H)
    B = H.cycle()
    rng = np.random.default_rng(3)
    for v in (np.ones(H.sizes[0]), rng.standard_normal(H.sizes[0])):
        y, y2 = apply(P, pc, v), apply(P, pc2, v)
        assert np.array_equal(bits(y), bits(y2)), name
        ref = B.apply(v)
        assert np.linalg.norm(y - ref) <= 1e-10 * np.linalg.norm(ref), (name, np.linalg.norm(y - ref) / np.linalg.norm(ref))
    for l in range(1, H.n):                                             # the smoothers are what the issue says
        s = pc.mg_get_smoother(l)
        assert s.get_type() == "chebychev" and s.get_tolerances()[3] == 2
    assert pc.mg_get_coarse_solve().get_type() == "preonly"


def test_unsmoothed_prolongator_and_w_cycle(P):
    csr = gr.poisson2d(16)
    H = gr.Hierarchy(*csr, nsmooths=0, coarse_eq_limit=10)
    A = P.Mat.from_csr(*csr)
    ksp, pc = gamg_ksp(P, A, nsmooths=0, coarse_eq_limit=10)
    pc.mg_set_cycle_type("w")
    pc.set_up()
    assert pc.gamg_level_sizes() == H.sizes
    B = mr.MG(H.As_dense, H.Ps_dense, gr.cheby_smoother(H.As_dense, H.rho_mg), cycle="w")
    v = np.cos(np.arange(256.0))
    y, ref = apply(P, pc, v), B.apply(v)
    assert np.linalg.norm(y - ref) <= 1e-10 * np.linalg.norm(ref)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_cg_with_gamg_on_poisson2d_takes_the_models_count(P, n):
    want, jac, H = model(n)
    A = P.Mat.from_csr(*gr.poisson2d(n))
    b = P.Vec.from_array(np.sin(0.3 * np.arange(n * n)) + 0.5)

    def solve(pctype):
        ksp = P.KSP(comm=P.lib().COMM_SELF)
        ksp.set_type("cg"); ksp.set_norm_type("unpreconditioned"); ksp.set_tolerances(rtol=1e-8)
        ksp.set_pc_type(pctype); ksp.set_operators(A)
        x = b.duplicate()
        ksp.solve(b, x)
        r = b.duplicate()
        A.residual(b, x, r)
        assert ksp.reason > 0 and r.norm() <= 2e-8 * b.norm()
        return ksp, ksp.its

    ksp, its = solve("gamg")
    print("n = %d: cg + gamg %d iterations (model %d), levels %s" % (n, its, want, ksp.get_pc().gamg_level_sizes()))
    assert ksp.get_pc().gamg_level_sizes() == H.sizes and its == want
    if n == 64:
        assert its < solve("jacobi")[1]


P7_15 = {}


def p7_15():
    if not P7_15:
        csr = gr.poisson7(15, 15, 15)
        H = gr.Hierarchy(*csr)
        b = np.sin(0.3 * np.arange(15 ** 3)) + 0.5
        P7_15.update(csr=csr, H=H, b=b, its=mr.pcg(H.As_dense[-1], b, H.cycle().apply)[1])
    return P7_15


def test_fused_cg_with_gamg_on_p7_15_takes_the_models_count(P):
    m = p7_15()
    A = P.Mat.from_csr(*m["csr"])
    b = P.Vec.from_array(m["b"])
    ksp, pc = gamg_ksp(P, A, "cghipmi355x")
    ksp.set_norm_type("unpreconditioned"); ksp.set_tolerances(rtol=1e-8)
    x = b.duplicate()
    ksp.solve(b, x)
    print("P7(15): cghipmi355x + gamg %d iterations (model %d), levels %s" % (ksp.its, m["its"], pc.gamg_level_sizes()))
    assert ksp.reason > 0 and pc.gamg_level_sizes() == m["H"].sizes and ksp.its == m["its"]


def test_readme_example_runs_at_p7_15(P):
    n = 15
    ai, aj, aa = P.gen_poisson7(n, n, n)
    A = P.Mat.from_csr(ai, aj, aa)
    b = P.Vec.from_array(np.ones(n ** 3))
    x = b.duplicate()
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_operators(A)
    ksp.set_type("cghipmi355x")
    ksp.set_pc_type("gamg")                       # aggregates, prolongators and coarse operators come from A
    ksp.set_tolerances(rtol=1e-8)
    ksp.solve(b, x)
    r = b.duplicate()
    A.residual(b, x, r)
    assert ksp.reason > 0 and ksp.its <= 20 and r.norm() <= 1e-6 * b.norm()
    assert ksp.get_pc().gamg_level_sizes()[0] == n ** 3


def test_stopping_rules(P, opts):
    A = P.Mat.from_csr(*gr.poisson2d(16))
    ksp, pc = gamg_ksp(P, A, coarse_eq_limit=300)
    pc.set_up()
    assert pc.gamg_level_sizes() == [256] and pc.mg_get_levels() == 1   # the coarse limit: one level, a direct solve
    v = np.arange(256.0) + 1.0
    assert np.linalg.norm(gr.dense(gr.poisson2d(16), 256) @ apply(P, pc, v) - v) <= 1e-10 * np.linalg.norm(v)
    ksp, pc = gamg_ksp(P, A, nlevels=2, coarse_eq_limit=5)
    pc.set_up()
    assert pc.gamg_level_sizes() == gr.Hierarchy(*gr.poisson2d(16), nlevels=2, coarse_eq_limit=5).sizes and pc.mg_get_levels() == 2
    D = P.Mat.from_csr(*gr.from_rows(60, {i: {i: 1.0 + i} for i in range(60)}))
    ksp, pc = gamg_ksp(P, D)
    pc.set_up()
    assert pc.gamg_level_sizes() == [60]                                # stalled: every node is its own aggregate
    opts("-pc_gamg_coarse_eq_limit 5 -pc_mg_levels 2 -mg_levels_ksp_max_it 3")
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_pc_type("gamg"); ksp.set_operators(A); ksp.set_from_options()
    pc = ksp.get_pc()
    pc.set_up()
    assert len(pc.gamg_level_sizes()) == 2 and pc.mg_get_smoother(1).get_tolerances()[3] == 3   # options under mg_levels_ win


def test_refusals(P):
    rows = {i: {i: 2.0} for i in range(8)}
    rows[3] = {2: 1.0, 3: 0.0, 4: 1.0}
    Z = P.Mat.from_csr(*gr.from_rows(8, rows))
    ksp, pc = gamg_ksp(P, Z)
    with pytest.raises(P.PetscError) as e:
        pc.set_up()
    assert e.value.code == PETSC_ERR_ARG_WRONGSTATE and "row 3" in str(e.value)
    B = P.Mat.from_bsr(2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([2.0, 0, 0, 2.0, 2.0, 0, 0, 2.0]))
    ksp, pc = gamg_ksp(P, B)
    raises(P, PETSC_ERR_SUP, pc.set_up)
    ai, aj, aa = gr.path(6)
    M = P.Mat.from_csr_mpi(ai, aj, aa, 6, comm=P.lib().COMM_SELF)
    raises(P, PETSC_ERR_SUP, M.aggregate, 0.0)
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_pc_type("gamg"); ksp.set_operators(M)
    raises(P, PETSC_ERR_SUP, ksp.get_pc().set_up)


def test_reuse_keeps_the_interpolation_and_only_refills(P):
    csr = gr.poisson2d(16)
    A = P.Mat.from_csr(*csr)
    ksp, pc = gamg_ksp(P, A, reuse_interpolation=True)
    pc.set_up()
    sizes = pc.gamg_level_sizes()
    v = np.sin(np.arange(256.0))
    y1 = apply(P, pc, v)
    before = P.Mat.coarsen_counts_total()
    P.lib().MatScale(A.h, 2.0)
    ksp.set_operators(A)
    pc.set_up()
    after = P.Mat.coarsen_counts_total()
    assert after[:2] == before[:2] and pc.gamg_level_sizes() == sizes  # zero coarsenings
    y2 = apply(P, pc, v)
    assert np.linalg.norm(2.0 * y2 - y1) <= 1e-12 * np.linalg.norm(y1)  # B(2 A) = B(A) / 2: the refill ran
    ksp, pc = gamg_ksp(P, A)                                            # without the option the hierarchy is rebuilt
    pc.set_up()
    before = P.Mat.coarsen_counts_total()
    P.lib().MatScale(A.h, 0.5)
    ksp.set_operators(A)
    pc.set_up()
    after = P.Mat.coarsen_counts_total()
    assert sum(after[:2]) - sum(before[:2]) == len(sizes) and pc.gamg_level_sizes() == sizes
    assert np.array_equal(bits(apply(P, pc, v)), bits(y1))


def test_destruction_order_is_safe(P):
    A = P.Mat.from_csr(*gr.poisson2d(16))
    ksp, pc = gamg_ksp(P, A)
    pc.set_up()
    v = np.ones(256)
    y = apply(P, pc, v)
    A2 = P.Mat.from_csr(*gr.poisson2d(16))
    ksp2, pc2 = gamg_ksp(P, A2)
    pc2.set_up()
    ksp.destroy(); ksp.own = False                                      # the PC first, its operator after
    A.destroy()
    assert np.array_equal(bits(apply(P, pc2, v)), bits(y))
    ksp2.set_pc_type("jacobi")                                          # the type replaced: the hierarchy goes with it
    ksp2.set_pc_type("gamg")
    ksp2.get_pc().set_up()
    assert np.array_equal(bits(apply(P, ksp2.get_pc(), v)), bits(y))
