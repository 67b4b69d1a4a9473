"""BiCG and MatSolveTranspose on the device: the harness's bicg on HIPMI355X vectors against the host model (tests/bicg_ref.py) under the
device's reduction order -- x, residual history, iteration count and reason bit for bit -- with PCNONE, PCJACOBI, ILU(0) and ILU(1) and
both norm types; MatSolveTranspose of the ILU factor through the Mat interface against the reference's loop under each mode of the
forward application; what is refused; ICC(0); the life cycle of the transposed factor.  The operators are the upwinded 5-point
convection-diffusion stencil on 33 x 31 (1023 rows) and 41 x 25 (1025 rows) grids."""
import ctypes as C

import numpy as np
import pytest

import bicg_ref as br
import cheby_ref as cr
import orc
from test_ilu_device_factor_gpu import setup_again
from test_ilu_sweeps_gpu import V, ilu_pc

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP, PETSC_ERR_ARG_IDN = 56, 61
GRIDS = {1023: (33, 31), 1025: (41, 25)}
_cache = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def problem(n):
    if n not in _cache:
        csr = br.convdiff(*GRIDS[n])
        _cache[n] = (csr, np.cos(0.37 * np.arange(n)) + 0.25, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[n]


def model_factor(n, levels):
    key = ("factor", n, levels)
    if key not in _cache:
        csr = problem(n)[0]
        _cache[key] = br.iluk_factor(*csr, levels) if levels else orc.ilu0_factor(*csr)
    return _cache[key]


def model_pc(n, pc):
    csr = problem(n)[0]
    if pc == "none":
        return {}
    if pc == "jacobi":
        return dict(pc=cr.jacobi(*csr))
    f = model_factor(n, 1 if pc == "ilu1" else 0)
    return dict(pc=lambda r: orc.ilu0_solve(f, np.ascontiguousarray(r)), pct=lambda r: br.ilu_solve_transpose(f, r))


def solve(P, csr, b, pc, norm, x0=None, opts="", **tol):
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb = V(P, b)
    vx = V(P, np.zeros(b.size) if x0 is None else x0)
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    pcopt = "-pc_type ilu -pc_factor_levels 1" if pc == "ilu1" else "-pc_type %s" % pc
    L.PetscOptionsInsertString(("-ksp_type bicg %s -ksp_norm_type %s %s" % (pcopt, norm, opts)).encode())
    try:
        k.set_tolerances(**tol)
        k.set_from_options()
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    return vx.array(), k.history(), k.its, k.reason


def agree(got, want, what):
    x, h, its, reason = got
    xw, hw, itsw, reasonw = want
    assert (its, reason) == (itsw, reasonw), (what, its, reason, itsw, reasonw)
    assert h.size == hw.size and np.array_equal(bits(h), bits(hw)), (what, h, hw)
    assert np.array_equal(bits(x), bits(xw)), (what, float(np.max(np.abs(x - xw))))


@pytest.mark.parametrize("norm", [br.PRECONDITIONED, br.UNPRECONDITIONED])
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu", "ilu1"])
@pytest.mark.parametrize("n", [1023, 1025])
def test_harness_bicg_walks_with_the_model(P, n, pc, norm):
    csr, b, guess = problem(n)
    for x0 in (None, guess) if pc == "jacobi" else (None,):
        for kw in (dict(rtol=1e-8, max_it=400), dict(rtol=1e-30, max_it=3)):
            got = solve(P, csr, b, pc, norm, x0=x0, **kw)
            with orc.device_reduction_order():
                want = br.bicg(*csr, b, x0=x0, norm=norm, **model_pc(n, pc), **kw)
            agree(got, want, (n, pc, norm, x0 is not None, kw))
            if kw["max_it"] == 400:
                assert got[3] == cr.CONVERGED_RTOL and 0 < got[2] < 400


def test_exits(P):
    csr, b, _ = problem(1023)
    got = solve(P, csr, np.zeros(1023), "jacobi", br.PRECONDITIONED)
    assert got[2] == 0 and got[3] > 0 and not got[0].any()
    for kw in (dict(abstol=1e-3, rtol=1e-30), dict(dtol=1e-3, rtol=1e-30)):
        got = solve(P, csr, b, "jacobi", br.PRECONDITIONED, **kw)
        with orc.device_reduction_order():
            want = br.bicg(*csr, b, pc=cr.jacobi(*csr), **kw)
        agree(got, want, kw)
    assert want[3] == cr.DIVERGED_DTOL
    sw = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))     # dpi == 0 in the first iteration
    got = solve(P, sw, np.array([1.0, 0.0]), "none", br.PRECONDITIONED)
    assert (got[2], got[3], got[1].size) == (0, br.DIVERGED_BREAKDOWN, 1) and not got[0].any()
    neg = (np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, -1.0]))   # Jacobi of diag(1, -1): z = (1, -1), beta = z'r == 0
    got = solve(P, neg, np.array([1.0, 1.0]), "jacobi", br.PRECONDITIONED)
    assert (got[2], got[3], got[1].size) == (0, br.DIVERGED_BREAKDOWN, 1) and not got[0].any()
    for pc in ("bjacobi", "sor"):                                # no transposed application: the first PCApplyTranspose says so
        with pytest.raises(P.PetscError) as e:
            solve(P, csr, b, pc, br.PRECONDITIONED)
        assert e.value.code == PETSC_ERR_SUP, pc


# ------------------------------------------------------------------------------------------------ MatSolveTranspose
def factor_of(P, pc):
    F = C.c_void_p()
    P.lib().PCFactorGetMatrix(pc, C.byref(F))
    return F


def transpose_builds(P, pc):
    a, b = C.c_int(-1), C.c_int(-1)
    P.lib().PCILUGetTransposeBuilds_HIPMI355X(pc, C.byref(a), C.byref(b))
    return a.value, b.value


def solve_transpose(P, pc, b):
    vb, vx = V(P, b), V(P, np.full(b.size, 7.0))
    P.lib().MatSolveTranspose(factor_of(P, pc), vb.h, vx.h)
    return vx.array()


@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("mode", ["syncfree", "level"])
@pytest.mark.parametrize("n", [1023, 1025])
def test_mat_solve_transpose_is_the_reference_loop(P, n, mode, levels):
    csr, b, _ = problem(n)
    A = P.Mat.from_csr(*csr)
    opts = "-pc_factor_hipmi355x_trisolve %s" % mode
    ksp, pc, rc = ilu_pc(P, A, opts)
    assert rc == 0
    if levels:                                                    # (-pc_factor_levels is PCSetFromOptions' business: set directly, set up again)
        P.lib().PCFactorSetLevels(pc, levels)
        assert setup_again(P, ksp, pc, A, opts) == 0
    f = model_factor(n, levels)
    sf = C.c_int(-1); P.lib().PCILUGetSolver_HIPMI355X(pc, C.byref(sf), None)
    assert sf.value == (1 if mode == "syncfree" else 0)
    for k in range(2):
        r = np.random.default_rng(40 + k).standard_normal(n)
        assert np.array_equal(bits(solve_transpose(P, pc, r)), bits(br.ilu_solve_transpose(f, r))), (n, mode, levels, k)
    assert transpose_builds(P, pc) == (1, 0)
    vb, vx = V(P, b), V(P, np.zeros(n))                           # PCApplyTranspose is the same application; the forward one still its own
    P.lib().PCApplyTranspose(pc, vb.h, vx.h)
    assert np.array_equal(bits(vx.array()), bits(br.ilu_solve_transpose(f, b)))
    P.lib().PCApply(pc, vb.h, vx.h)
    assert np.array_equal(bits(vx.array()), bits(orc.ilu0_solve(f, b)))


def test_what_is_refused(P):
    csr, b, _ = problem(1023)
    A = P.Mat.from_csr(*csr)
    L = P.lib()
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:2")
    assert rc == 0
    vb, vx = V(P, b), V(P, np.full(1023, 7.0))
    assert L.raw("MatSolveTranspose")(factor_of(P, pc), vb.h, vx.h) == PETSC_ERR_SUP
    assert np.array_equal(vx.array(), np.full(1023, 7.0))
    ksp2, pc2, rc = ilu_pc(P, A, "")
    assert rc == 0
    assert L.raw("MatSolveTranspose")(factor_of(P, pc2), vb.h, vb.h) == PETSC_ERR_ARG_IDN
    assert np.array_equal(bits(vb.array()), bits(b))
    bs = 3                                                        # a block factor: said with the routine's name
    bi, bj, _ = P.gen_poisson7(4, 3, 2)
    rng = np.random.default_rng(5)
    ba = rng.standard_normal((bj.size, bs, bs)) * 0.1
    rows = np.repeat(np.arange(bi.size - 1), np.diff(bi))
    ba[rows == bj] += 8.0 * np.eye(bs)
    B = P.Mat.from_bsr(bs, bi, bj, ba.reshape(-1))
    ksp3, pc3, rc = ilu_pc(P, B, "")
    assert rc == 0
    nb = (bi.size - 1) * bs
    wb, wx = V(P, np.ones(nb)), V(P, np.zeros(nb))
    assert L.raw("MatSolveTranspose")(factor_of(P, pc3), wb.h, wx.h) == PETSC_ERR_SUP
    assert b"MatSolveTranspose" in L._h.PetscGetLastErrorMessage()


def test_icc_transpose_is_the_forward_application(P):
    csr = P.gen_poisson7(5, 4, 3)
    n = csr[0].size - 1
    A = P.Mat.from_csr(*csr)
    ksp, pc, rc = ilu_pc(P, A, "", pctype=b"icc")
    assert rc == 0
    r = np.random.default_rng(8).standard_normal(n)
    vb, vx, vy = V(P, r), V(P, np.zeros(n)), V(P, np.zeros(n))
    P.lib().PCApply(pc, vb.h, vx.h)
    P.lib().PCApplyTranspose(pc, vb.h, vy.h)
    assert vx.array().any() and np.array_equal(bits(vx.array()), bits(vy.array()))


@pytest.mark.parametrize("numeric", ["host", "device"])
def test_life_cycle_of_the_transposed_factor(P, numeric):
    """a factorisation on an unchanged pattern refills the values only; another pattern builds the form again; both routes of the
    numeric factorisation leave the same bits"""
    L = P.lib()
    csr, b, _ = problem(1023)
    opts = "-pc_factor_hipmi355x_numeric %s -pc_factor_hipmi355x_trisolve level" % numeric
    A = P.Mat.from_csr(*csr)
    ksp, pc, rc = ilu_pc(P, A, opts)
    assert rc == 0 and transpose_builds(P, pc) == (0, 0)
    f = model_factor(1023, 0)
    assert np.array_equal(bits(solve_transpose(P, pc, b)), bits(br.ilu_solve_transpose(f, b)))
    assert np.array_equal(bits(solve_transpose(P, pc, b)), bits(br.ilu_solve_transpose(f, b)))
    assert transpose_builds(P, pc) == (1, 0)
    L.MatScale(A.h, 0.5)
    assert setup_again(P, ksp, pc, A, opts) == 0
    f2 = orc.ilu0_factor(csr[0], csr[1], 0.5 * csr[2])
    got = solve_transpose(P, pc, b)
    assert transpose_builds(P, pc) == (1, 1)
    assert np.array_equal(bits(got), bits(br.ilu_solve_transpose(f2, b)))
    A2 = P.Mat.from_csr(*csr)                                     # a fresh build on the scaled values: the same bits
    L.MatScale(A2.h, 0.5)
    k2, pc2, rc = ilu_pc(P, A2, opts)
    assert rc == 0 and np.array_equal(bits(solve_transpose(P, pc2, b)), bits(got)) and transpose_builds(P, pc2) == (1, 0)
    other = br.convdiff(31, 33)                                   # the same size, another pattern
    A3 = P.Mat.from_csr(*other)
    assert setup_again(P, ksp, pc, A3, opts) == 0
    got3 = solve_transpose(P, pc, b)
    assert transpose_builds(P, pc)[0] == 2
    assert np.array_equal(bits(got3), bits(br.ilu_solve_transpose(orc.ilu0_factor(*other), b)))


def test_forward_and_transposed_applications_are_adjoint(P):
    """|x'(F y) - (F^T x)'y| / (|x| |F y|) on random x, y: allowed what tests/test_bicg_cpu.py allows the transposed solve against a dense
    one -- 100 x the forward solve's own error against a dense solve, measured here by the same function (8.7e-16 on this factor, so
    8.7e-14), with no factor of n"""
    from test_bicg_cpu import dense_errors
    csr, b, _ = problem(1023)
    A = P.Mat.from_csr(*csr)
    ksp, pc, rc = ilu_pc(P, A, "")
    assert rc == 0
    rng = np.random.default_rng(77)
    x, y = rng.standard_normal(1023), rng.standard_normal(1023)
    vy, vf = V(P, y), V(P, np.zeros(1023))
    P.lib().PCApply(pc, vy.h, vf.h)
    fy, ftx = vf.array(), solve_transpose(P, pc, x)
    gap = abs(float(x @ fy) - float(ftx @ y)) / (np.linalg.norm(x) * np.linalg.norm(fy))
    bound = 100.0 * dense_errors("ilu0")[0]
    print("adjoint gap", gap, "bound", bound)
    assert 0.0 < bound < 1e-12 and gap <= bound


@pytest.mark.parametrize("name", ["bidiagonal7", "diagonal300"])
def test_a_shallow_factor_takes_the_plain_launches(P, name):
    """14 levels and 2 levels in all: at most 16, so MatSolveTranspose launches level by level without a captured graph"""
    csr = br.bidiagonal(7) if name == "bidiagonal7" else br.diagonal(300)
    n = csr[0].size - 1
    A = P.Mat.from_csr(*csr)
    ksp, pc, rc = ilu_pc(P, A, "")
    assert rc == 0
    f = orc.ilu0_factor(*csr)
    r = np.random.default_rng(9).standard_normal(n)
    vb, vx = V(P, r), V(P, np.full(n, 7.0))
    for rep in range(2):
        ksp.get_pc().apply_transpose(vb, vx)
        assert np.array_equal(bits(vx.array()), bits(br.ilu_solve_transpose(f, r))), (name, rep)
    assert transpose_builds(P, pc) == (1, 0) and ksp.get_pc().apply_transpose_exists()


# ------------------------------------------------------------------------------------------------ bicghipmi355x
def solve_type(P, csr, b, ksp_type, pc, norm, x0=None, strip=False, opts="", **tol):
    """solve() for any KSP type -> (x, history, its, reason, (fused sweeps, op-by-op iterations)); strip: the vectors lose the table first"""
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb = V(P, b)
    vx = V(P, np.zeros(b.size) if x0 is None else x0)
    if strip:
        compose = L.raw("PetscObjectComposeFunction")
        compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        assert compose(vx.h, b"VecBicgFusedOps_C", b"", None) == 0 and compose(vb.h, b"VecBicgFusedOps_C", b"", None) == 0
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    pcopt = "-pc_type ilu -pc_factor_levels 1" if pc == "ilu1" else "-pc_type %s" % pc
    L.PetscOptionsInsertString(("-ksp_type %s %s -ksp_norm_type %s %s" % (ksp_type, pcopt, norm, opts)).encode())
    try:
        k.set_tolerances(**tol)
        k.set_from_options()
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    return vx.array(), k.history(), k.its, k.reason, k.fused_step_counts()


@pytest.mark.parametrize("norm", [br.PRECONDITIONED, br.UNPRECONDITIONED])
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu"])
@pytest.mark.parametrize("n", [1023, 1025])
def test_fused_type_is_the_plain_type_bit_for_bit(P, n, pc, norm):
    """fused, with -ksp_bicg_fused 0, and on vectors stripped of "VecBicgFusedOps_C"; the step counts as the solver's comment states
    them: bicg_dirs once per iteration entered and bicg_update once per iteration that gets past dpi -- 2 its sweeps here"""
    csr, b, guess = problem(n)
    for x0 in (None, guess) if pc == "jacobi" else (None,):
        for kw in (dict(rtol=1e-8, max_it=400), dict(rtol=1e-30, max_it=3)):
            what = (n, pc, norm, x0 is not None, kw)
            plain = solve_type(P, csr, b, "bicg", pc, norm, x0=x0, **kw)
            assert plain[4] == (0, 0)
            fused = solve_type(P, csr, b, "bicghipmi355x", pc, norm, x0=x0, **kw)
            agree(fused[:4], plain[:4], what + ("fused",))
            assert fused[4] == (2 * fused[2], 0) and fused[2] > 0, (what, fused[2:])
            off = solve_type(P, csr, b, "bicghipmi355x", pc, norm, x0=x0, opts="-ksp_bicg_fused 0", **kw)
            agree(off[:4], plain[:4], what + ("option off",))
            assert off[4] == (0, off[2]), (what, off[2:])
            stripped = solve_type(P, csr, b, "bicghipmi355x", pc, norm, x0=x0, strip=True, **kw)
            agree(stripped[:4], plain[:4], what + ("stripped",))
            assert stripped[4] == (0, stripped[2]), (what, stripped[2:])


def test_fused_type_exits(P):
    csr, b, _ = problem(1023)
    got = solve_type(P, csr, np.zeros(1023), "bicghipmi355x", "jacobi", br.PRECONDITIONED)
    assert got[2] == 0 and got[3] > 0 and got[4] == (0, 0)
    sw = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))     # dpi == 0: the first sweep ran, the second did not
    got = solve_type(P, sw, np.array([1.0, 0.0]), "bicghipmi355x", "none", br.PRECONDITIONED)
    assert (got[2], got[3], got[1].size, got[4]) == (0, br.DIVERGED_BREAKDOWN, 1, (1, 0)) and not got[0].any()
    neg = (np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, -1.0]))   # beta == 0: no sweep at all
    got = solve_type(P, neg, np.array([1.0, 1.0]), "bicghipmi355x", "jacobi", br.PRECONDITIONED)
    assert (got[2], got[3], got[4]) == (0, br.DIVERGED_BREAKDOWN, (0, 0))
    for kw in (dict(abstol=1e-3, rtol=1e-30), dict(dtol=1e-3, rtol=1e-30)):
        plain = solve_type(P, csr, b, "bicg", "jacobi", br.PRECONDITIONED, **kw)
        agree(solve_type(P, csr, b, "bicghipmi355x", "jacobi", br.PRECONDITIONED, **kw)[:4], plain[:4], kw)
    with pytest.raises(P.PetscError) as e:
        solve_type(P, csr, b, "bicghipmi355x", "sor", br.PRECONDITIONED)
    assert e.value.code == PETSC_ERR_SUP
