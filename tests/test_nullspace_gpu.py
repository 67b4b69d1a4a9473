"""Null spaces through the harness on the device: MatNullSpaceRemove, MatNullSpaceTest, KSPSetNullSpace.

Operator: the 3-D 7-point pure-Neumann Laplacian (nullspace_ref.neumann7) at 6 x 5 x 4 (120 rows, reductions in one workgroup) and
17 x 17 x 17 (4913 rows, the hand-off between workgroups).  Reference: tests/nullspace_ref.py, reductions in the device's order
(orc.device_reduction_order()), compared bit for bit: a PCG (the removal behind KSP_PCApply) and a GMRES (behind KSP_PCApplyBAorAB).
The registered types (and plain bcgs, which has no restatement there) are held to the bits of the plain types."""
import ctypes as C

import numpy as np
import pytest

import nullspace_ref as nr
import orc

pytestmark = pytest.mark.gpu

GRIDS = {120: (6, 5, 4), 4913: (17, 17, 17)}
PC_LEFT, PC_RIGHT = 0, 1


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def problems():
    """operator, Jacobi diagonal, one random right-hand side as it is and made consistent; computed once, left unchanged"""
    out = {}
    for n, g in GRIDS.items():
        csr = nr.neumann7(*g)
        b = np.random.default_rng(11).standard_normal(n)
        with orc.device_reduction_order():
            bc = nr.remove(b, True, ())
        out[n] = dict(csr=csr, dinv=nr.jacobi(*csr), raw=b, consistent=bc)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def V(P, a):
    return P.Vec.from_array(a, comm=P.lib().COMM_SELF)


def set_options(L, s):
    L.PetscOptionsClear()
    if s:
        L.PetscOptionsInsertString(s.encode())


def solve(P, csr, b, opts, nullsp="const", side=None, max_it=30, rtol=1e-30, defer=None, then_without=False):
    """one KSPSolve (zero guess); nullsp: 'const', None.  Returns x, history, its, reason (then_without: of a second solve on the same
    KSP after KSPSetNullSpace(ksp, NULL))"""
    L = P.lib()
    if defer is not None:
        L.raw("VecHIPMI355XSetDeferral")(defer)
    A = P.Mat.from_csr(*csr)
    vb, vx = V(P, b), V(P, np.zeros(b.size))
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    set_options(L, opts)
    k.set_tolerances(rtol=rtol, max_it=max_it)
    k.set_from_options()
    if side is not None:
        L.KSPSetPCSide(k.h, side)
    sp = P.NullSpace(True, comm=L.COMM_SELF) if nullsp else None
    if sp:
        k.set_null_space(sp)
    k.record_history()
    k.solve(vb, vx)
    if then_without:
        k.set_null_space(None)
        k.solve(vb, vx)
    res = vx.array(), k.history(), k.its, k.reason
    set_options(L, "")
    if defer is not None:
        L.raw("VecHIPMI355XSetDeferral")(-1)
    return res


# ------------------------------------------------------------------------------------------------------------- removal
@pytest.mark.parametrize("n", [120, 4913])
@pytest.mark.parametrize("has_cnst,nvec", [(True, 0), (False, 2), (True, 2)])
def test_removal_equals_the_reference_bit_for_bit(P, n, has_cnst, nvec):
    L = P.lib()
    v = np.random.default_rng(5).standard_normal(n) + 3.0
    basis = nr.orthonormal_pair(n)[:nvec]
    with orc.device_reduction_order():
        ref = nr.remove(v, has_cnst, basis)
    vecs = [V(P, a) for a in basis]
    sp = P.NullSpace(has_cnst, vecs, comm=L.COMM_SELF)
    x = V(P, v)
    sp.remove(x)
    assert np.array_equal(bits(x.array()), bits(ref))
    # the out form: the result in the null space's own vector, the argument untouched
    y = V(P, v)
    w = sp.remove(y, out=True)
    assert np.array_equal(bits(w.array()), bits(ref)) and np.array_equal(bits(y.array()), bits(v))
    sp.destroy()
    for a in vecs:
        assert np.array_equal(bits(a.array()), bits(basis[vecs.index(a)]))       # still alive: the null space only dropped its reference


@pytest.mark.parametrize("n", [120, 4913])
def test_sync_free_route_and_public_calls_give_the_same_bits(P, n):
    L = P.lib()
    v = np.random.default_rng(6).standard_normal(n) - 1.0
    a = V(P, v)
    P.NullSpace(True, comm=L.COMM_SELF).remove(a)                # "VecShiftByMean_C": one rank
    b = V(P, v)
    s = b.sum()
    s = s / (-1.0 * n)
    b.shift(s)                                                   # VecSum, then VecShift
    c = V(P, v)
    sp = P.NullSpace(False, comm=L.COMM_SELF)
    sp.set_device_constant()                                     # the callback route of a real PETSc tree
    sp.remove(c)
    assert np.array_equal(bits(a.array()), bits(b.array())) and np.array_equal(bits(a.array()), bits(c.array()))
    with orc.device_reduction_order():
        assert bits(np.array([s]))[0] == bits(np.array([nr.vec_sum(v) / (-1.0 * n)]))[0]
        assert np.array_equal(bits(a.array()), bits(nr.remove(v, True, ())))


def test_vec_max_min_through_the_type(P):
    x = np.random.default_rng(8).standard_normal(4913)
    x[100] = x[4000] = 7.0
    x[7] = x[4900] = -7.0
    v = V(P, x)
    assert v.max() == (100, 7.0) and v.min() == (7, -7.0)
    v.shift(1.0)
    assert v.max() == (100, 8.0)                                 # a writer: nothing stale is handed back
    assert abs(v.norm() - np.linalg.norm(x + 1.0)) <= 1e-12 * np.linalg.norm(x + 1.0)


def test_null_space_test(P, problems):
    L = P.lib()
    sp = P.NullSpace(True, comm=L.COMM_SELF)
    assert sp.test(P.Mat.from_csr(*problems[120]["csr"])) is True
    assert sp.test(P.Mat.from_csr(*P.gen_poisson7(6, 5, 4))) is False


# -------------------------------------------------------------------------------------------------------------- solves
@pytest.mark.parametrize("n", [120, 4913])
@pytest.mark.parametrize("rhs", ["raw", "consistent"])
@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_cg_with_a_null_space_walks_the_reference(P, problems, n, rhs, pc):
    p = problems[n]
    with orc.device_reduction_order():
        xo, ho, ito, ro = nr.pcg(*p["csr"], p[rhs], 1e-30, p["dinv"] if pc == "jacobi" else None, (True, ()), max_it=30)
    x, h, its, reason = solve(P, p["csr"], p[rhs], "-ksp_type cg -pc_type " + pc)
    assert (its, reason) == (ito, ro)
    assert np.array_equal(bits(h), bits(ho)), np.max(np.abs(h - ho) / ho)
    assert np.array_equal(bits(x), bits(xo))
    # one projection of an n = 4913 vector leaves about n eps |x| / n of mean behind
    assert abs(np.mean(x)) <= 1e-13 * np.max(np.abs(x))


@pytest.mark.parametrize("n", [120, 4913])
@pytest.mark.parametrize("rhs", ["raw", "consistent"])
def test_gmres_with_a_null_space_walks_the_reference(P, problems, n, rhs):
    """left-preconditioned GMRES(30) + Jacobi: the removal behind KSPInitialResidual's KSP_PCApply and behind every KSP_PCApplyBAorAB"""
    p = problems[n]
    with orc.device_reduction_order():
        xo, ho, ito, ro = nr.gmres(*p["csr"], p[rhs], 1e-30, p["dinv"], (True, ()), max_it=30)
    x, h, its, reason = solve(P, p["csr"], p[rhs], "-ksp_type gmres -pc_type jacobi", side=PC_LEFT)
    assert (its, reason) == (ito, ro)
    assert h.size == ho.size and np.array_equal(bits(h), bits(ho)), np.max(np.abs(h - ho) / ho)
    assert np.array_equal(bits(x), bits(xo))
    assert abs(np.mean(x)) <= 1e-13 * np.max(np.abs(x))


FUSED = [("cg", "-ksp_type cghipmi355x -ksp_cg_fused %d" % l) for l in range(5)] + [("gmres", "-ksp_type gmreshipmi355x"), ("bcgs", "-ksp_type bcgshipmi355x")]


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("plain,opts", FUSED)
def test_registered_solvers_give_the_bits_of_the_plain_types(P, problems, plain, opts, pc, defer):
    p = problems[4913]
    ref = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type %s" % (plain, pc), defer=defer)
    got = solve(P, p["csr"], p["consistent"], opts + " -pc_type " + pc, defer=defer)
    assert got[2:] == ref[2:]
    assert np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(bits(got[0]), bits(ref[0]))
    if plain != "bcgs":
        assert abs(np.mean(got[0])) <= 1e-13 * np.max(np.abs(got[0]))


def test_deferral_does_not_change_the_bits(P, problems):
    p = problems[4913]
    for t in ("cg", "gmres", "bcgs"):
        a = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, defer=0)
        b = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, defer=1)
        assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[0]), bits(b[0])), t


def test_right_preconditioning_does_not_apply_the_null_space(P, problems):
    p = problems[4913]
    for t in ("gmres", "gmreshipmi355x"):
        a = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, nullsp="const", side=PC_RIGHT)
        b = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, nullsp=None, side=PC_RIGHT)
        assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[0]), bits(b[0])), t


def test_taking_the_null_space_away_gives_the_bits_of_before(P, problems):
    p = problems[4913]
    for t in ("cg", "cghipmi355x", "gmreshipmi355x", "bcgshipmi355x"):
        a = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, nullsp="const", then_without=True)
        b = solve(P, p["csr"], p["consistent"], "-ksp_type %s -pc_type jacobi" % t, nullsp=None)
        assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[0]), bits(b[0])), t


def test_control_inconsistent_right_hand_side(P, problems):
    """b = random + 1 on the 17^3 operator, CG + Jacobi, rtol 1e-10, 200 iterations.  Chosen on the reference alone
    (tests/test_nullspace_cpu.py::test_reference_cg_on_an_inconsistent_right_hand_side): without a null space CG stops with DIVERGED_DTOL
    and an iterate that is all constant vector; with it the iterate is free of the constant and the residual falls, but the
    REFERENCE does not reach 1e-10 either (it stops with DIVERGED_INDEFINITE_PC after 18 iterations: the residual keeps its constant
    component and the Jacobi scaling mixes it back in), so convergence is asserted on the consistent right-hand side instead.  The
    device walks the reference in all three."""
    p = problems[4913]
    b = p["raw"] + 1.0
    with orc.device_reduction_order():
        ref0 = nr.pcg(*p["csr"], b, 1e-10, p["dinv"], None, max_it=200)
        ref1 = nr.pcg(*p["csr"], b, 1e-10, p["dinv"], (True, ()), max_it=200)
        refc = nr.pcg(*p["csr"], nr.remove(b, True, ()), 1e-10, p["dinv"], (True, ()), max_it=200)
    got0 = solve(P, p["csr"], b, "-ksp_type cg -pc_type jacobi", nullsp=None, max_it=200, rtol=1e-10)
    got1 = solve(P, p["csr"], b, "-ksp_type cg -pc_type jacobi", max_it=200, rtol=1e-10)
    with orc.device_reduction_order():
        gotc = solve(P, p["csr"], nr.remove(b, True, ()), "-ksp_type cg -pc_type jacobi", max_it=200, rtol=1e-10)
    for got, ref in ((got0, ref0), (got1, ref1), (gotc, refc)):
        print("its %d reason %d |z| %g -> %g (reference its %d reason %d)" % (got[2], got[3], got[1][0], got[1][-1], ref[2], ref[3]))
        assert got[2:] == ref[2:] and np.array_equal(bits(got[1]), bits(ref[1]))
    assert got0[3] < 0 and abs(np.mean(got0[0])) > 0.9 * np.max(np.abs(got0[0]))
    assert got1[3] != -4 and got1[1][-1] < got1[1][0] and abs(np.mean(got1[0])) <= 1e-13 * np.max(np.abs(got1[0]))
    assert gotc[3] == 2 and gotc[2] < 200


def test_control_inconsistent_right_hand_side_without_a_preconditioner(P, problems):
    """The same control with -pc_type none: z = P r, so z'r = |P r|^2 carries nothing of the residual's constant component beyond what
    rounding leaves of sum(z).  Without a null space CG stops with a divergence reason; with it the device walks the reference, the
    iterate stays free of the constant and |z| falls by many orders.  Whether rtol 1e-10 is reached within 200 iterations is what the
    reference says (printed): under the device summation order it is not -- z'r meets the rounding of sum(z) times the constant
    component first."""
    p = problems[4913]
    b = p["raw"] + 1.0
    with orc.device_reduction_order():
        ref0 = nr.pcg(*p["csr"], b, 1e-10, None, None, max_it=200)
        ref1 = nr.pcg(*p["csr"], b, 1e-10, None, (True, ()), max_it=200)
    got0 = solve(P, p["csr"], b, "-ksp_type cg -pc_type none", nullsp=None, max_it=200, rtol=1e-10)
    got1 = solve(P, p["csr"], b, "-ksp_type cg -pc_type none", max_it=200, rtol=1e-10)
    for got, ref in ((got0, ref0), (got1, ref1)):
        print("its %d reason %d |z| %g -> min %g (reference its %d reason %d)" % (got[2], got[3], got[1][0], got[1].min(), ref[2], ref[3]))
        assert got[2:] == ref[2:] and np.array_equal(bits(got[1]), bits(ref[1]))
    assert got0[3] == -4 and abs(np.mean(got0[0])) > 0.9 * np.max(np.abs(got0[0]))
    assert got1[3] != -4 and got1[1].min() < 1e-6 * got1[1][0]


def test_two_staged_ranks(built):
    """VecSum, VecMax / VecMin (with locations, the extremum on both ranks), MatNullSpaceRemove by both routes and one CG + Jacobi
    Neumann solve on two ranks sharing the GPU over the host-staged transport: tests/tools/nullspace_ranks.py compares with the
    one-rank reference (locations and extremal values exactly, sums and the solve to 1e-13 relative)"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29581",
           os.path.join(root, "tests", "tools", "nullspace_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
    for k in range(2):
        assert re.search(r"rank %d/2: null space on staged ranks ok=True" % k, out), out[-3000:]
