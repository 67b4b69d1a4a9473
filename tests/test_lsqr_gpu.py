"""LSQR on the device: the harness's lsqr on HIPMI355X vectors against the host model (tests/lsqr_ref.py) under the device's reduction
order, and lsqrhipmi355x against lsqr on the same objects -- x, residual history, iteration count, reason, arnorm and anorm bit for bit.
The operators are the 60 x 37 one of tests/test_lsqr_cpu.py and its transpose (the wide, minimum-norm case); a preconditioner is Jacobi or
ICC(0) on A^T A formed on the device with MatTranspose + MatMatMult."""
import ctypes as C

import numpy as np
import pytest

import cheby_ref as cr
import lsqr_ref as lr
from test_lsqr_cpu import ALPHA0, csr, operator

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP, PETSC_ERR_ARG_SIZ = 56, 60
_cache = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def problem(name):
    """(dense A, its CSR, b, a nonzero guess), made once"""
    if name not in _cache:
        A = operator()
        b = np.random.default_rng(5).standard_normal(60)
        if name == "wide":
            A, b = A.T.copy(), b[:37]
        n = A.shape[1]
        _cache[name] = (A, csr(A), b, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[name]


class Got:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def solve(P, a, n, b, ksp_type, pc="none", x0=None, normal_pmat=False, normal_tests=False, se=None, strip=False, norm_none=False, nullsp=False,
          side=None, x_size=None, **tol):
    """se: None, "option" (-ksp_lsqr_set_standard_error) or "vec" (KSPLSQRSetStandardErrorVec).  normal_pmat: the PC is built from A^T A."""
    L = P.lib()
    A = P.Mat.from_csr(*a, ncols=n)
    Pm = A.transpose().matmult(A) if normal_pmat else None
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array((np.zeros(n) if x0 is None else x0) if x_size is None else np.zeros(x_size), comm=L.COMM_SELF)
    if strip:
        compose = L.raw("PetscObjectComposeFunction")
        compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        assert compose(vx.h, b"VecLsqrFusedOps_C", b"", None) == 0 and compose(vb.h, b"VecLsqrFusedOps_C", b"", None) == 0
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A, Pm)
    L.PetscOptionsClear()
    opts = "-ksp_type %s" % ksp_type + (" -pc_type %s" % pc if pc else "") + (" -ksp_lsqr_set_standard_error" if se == "option" else "")
    L.PetscOptionsInsertString(opts.encode())
    try:
        if tol:
            k.set_tolerances(**tol)
        k.set_from_options()
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
        if normal_tests:
            k.set_convergence_test("KSPLSQRDefaultConverged")
        if norm_none:
            k.set_norm_type("none")
        if nullsp:
            k.set_null_space(P.NullSpace(True, comm=L.COMM_SELF))
        if side is not None:
            L.KSPSetPCSide(k.h, side)
        if se == "vec":
            k.lsqr_set_standard_error_vec(P.Vec.from_array(np.full(n, 7.0), comm=L.COMM_SELF))
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    arnorm, rhs_norm, anorm = k.lsqr_get_arnorm()
    sev = k.lsqr_get_standard_error_vec()
    d = cr.jacobi(*Pm.csr()) if normal_pmat else None
    return Got(x=vx.array(), hist=k.history(), its=k.its, reason=k.reason, counts=k.fused_step_counts(), arnorm=arnorm, rhs_norm=rhs_norm, anorm=anorm,
               se=sev.array() if sev is not None else None, jacobi=d)


def agree(got, want, what):
    assert (got.its, got.reason) == (want.its, want.reason), (what, got.its, got.reason, want.its, want.reason)
    assert got.hist.size == want.hist.size and np.array_equal(bits(got.hist), bits(want.hist)), (what, got.hist, want.hist)
    assert np.array_equal(bits(got.x), bits(want.x)), (what, float(np.max(np.abs(got.x - want.x))))
    for name in ("arnorm", "anorm", "rhs_norm"):
        assert bits(getattr(got, name)) == bits(getattr(want, name)), (what, name, getattr(got, name), getattr(want, name))
    assert (got.se is None) == (want.se is None), what
    if got.se is not None:
        assert np.array_equal(bits(got.se), bits(want.se)), (what, "standard-error sum")


def jacobi_of_normal(P, a, n):
    """the inverted diagonal PCJACOBI takes from the A^T A the device forms (its bits are the device product's)"""
    A = P.Mat.from_csr(*a, ncols=n)
    return cr.jacobi(*A.transpose().matmult(A).csr())


@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("mat", ["tall", "wide"])
def test_all_three_walk_together(P, mat, pc):
    """the harness's lsqr on HIP types is the model under the device's reduction order, and the plug-in's type is the harness's"""
    A, a, b, guess = problem(mat)
    n = A.shape[1]
    d = jacobi_of_normal(P, a, n) if pc == "jacobi" else None
    for x0 in (None, guess):
        for max_it, rtol, normal in ((200, 1e-10, True), (40, 1e-8, False), (3, 1e-30, False)):
            what = (mat, pc, "zero" if x0 is None else "nonzero", max_it, normal)
            model = lr.lsqr(*a, n, b, pc=d, x0=x0, max_it=max_it, rtol=rtol, normal_tests=normal, se=True, device_order=True)
            kw = dict(pc=pc, x0=x0, normal_pmat=pc == "jacobi", normal_tests=normal, se="option", rtol=rtol, max_it=max_it)
            plain = solve(P, a, n, b, "lsqr", **kw)
            agree(plain, model, what + ("lsqr against the model",))
            fused = solve(P, a, n, b, "lsqrhipmi355x", **kw)
            agree(fused, plain, what + ("lsqrhipmi355x against lsqr",))
            print(what, "its", fused.its, "reason", fused.reason, "counts", fused.counts, "arnorm", fused.arnorm, "anorm", fused.anorm)
            assert plain.counts == (0, 0) and fused.its > 0
            # PCNONE: the one-wait route, two bidiagonalisation sweeps and one update sweep per iteration; a PC: the row-space sweep alone
            assert fused.counts == ((2 * fused.its, fused.its) if pc == "none" else (fused.its, fused.its)), (what, fused.counts)
            if normal or (mat == "wide" and max_it == 40):                                 # the tall system is inconsistent: ||b - A x|| stays at 4.7
                assert fused.reason > 0, (what, fused.reason)                               # and only the tests on A^T r can end its solve
    if mat == "tall" and pc == "none":                                                  # the figures tests/test_lsqr_cpu.py holds the model to
        got = solve(P, a, n, b, "lsqrhipmi355x", normal_tests=True, rtol=1e-10)
        xs = np.linalg.lstsq(A, b, rcond=None)[0]
        res = b - A @ got.x
        assert (got.its, got.reason) == (24, lr.CONVERGED_RTOL_NORMAL)
        assert np.linalg.norm(got.x - xs) <= 1e-8 * np.linalg.norm(xs)
        assert abs(got.arnorm - np.linalg.norm(A.T @ res)) <= 1e-6 * np.linalg.norm(A.T @ res)
        assert abs(got.hist[-1] - np.linalg.norm(res)) <= 1e-12 * np.linalg.norm(res)


def test_a_non_trivial_preconditioner_takes_the_mixed_route(P):
    """ICC(0) on A^T A: KSP_PCApply forms Z1 and the update sweep takes it with its scaling"""
    A, a, b, guess = problem("tall")
    for x0 in (None, guess):
        for se in (None, "vec"):
            kw = dict(pc="icc", x0=x0, normal_pmat=True, normal_tests=True, se=se, rtol=1e-10, max_it=200)
            plain = solve(P, a, 37, b, "lsqr", **kw)
            fused = solve(P, a, 37, b, "lsqrhipmi355x", **kw)
            agree(fused, plain, ("icc", x0 is not None, se))
            assert fused.reason > 0 and fused.counts == (fused.its, fused.its) and (fused.se is None) == (se is None)
            xs = np.linalg.lstsq(A, b, rcond=None)[0]
            assert np.linalg.norm(fused.x - xs) <= 1e-8 * np.linalg.norm(xs)


def test_every_exit_on_both_types(P):
    A, a, b, guess = problem("tall")
    D = np.diag(np.arange(1.0, 6.0))
    Dt = np.vstack([D, np.zeros((2, 5))])
    e1 = np.zeros(5); e1[0] = 1.0
    xs = np.cos(0.3 * np.arange(37))
    cases = [("b = 0", a, 37, np.zeros(60), {}, {}, (0, lr.CONVERGED_ATOL)),
             ("A^T b = 0", csr(Dt), 5, np.array([0, 0, 0, 0, 0, 1.0, -2.0]), {}, {}, (0, lr.CONVERGED_ATOL_NORMAL)),
             ("consistent", a, 37, A @ xs, dict(rtol=1e-9), {}, (None, lr.CONVERGED_RTOL)),
             ("max_it 1", a, 37, b, dict(rtol=1e-30, max_it=1), {}, (1, lr.DIVERGED_ITS)),
             ("max_it 2", a, 37, b, dict(rtol=1e-30, max_it=2), {}, (2, lr.DIVERGED_ITS)),
             ("beta == 0, a test that leaves the reason unset", csr(D), 5, e1, {}, dict(norm_none=True), (1, lr.CONVERGED_HAPPY_BREAKDOWN)),
             ("beta == 0, the default test", csr(D), 5, e1, {}, {}, (1, lr.CONVERGED_ATOL)),
             ("alpha == 0", csr(ALPHA0[0]), 1, ALPHA0[1], {}, {}, (1, lr.CONVERGED_HAPPY_BREAKDOWN))]
    for what, aa_, n, rhs, tol, kw, (its, reason) in cases:
        model = lr.lsqr(*aa_, n, rhs, skip_test=bool(kw), device_order=True, **tol)
        plain = solve(P, aa_, n, rhs, "lsqr", **kw, **tol)
        fused = solve(P, aa_, n, rhs, "lsqrhipmi355x", **kw, **tol)
        print(what, "its", fused.its, "reason", fused.reason, "x", fused.x[:3])
        agree(plain, model, (what, "lsqr against the model"))
        agree(fused, plain, (what, "lsqrhipmi355x against lsqr"))
        assert fused.reason == reason and (its is None or fused.its == its), (what, fused.its, fused.reason)
    assert np.array_equal(fused.x, [1.0])                                               # the alpha == 0 exit kept the step that makes x exact


def test_vectors_without_the_table_are_refused_at_set_up(P):
    A, a, b, guess = problem("tall")
    with pytest.raises(P.PetscError) as e:
        solve(P, a, 37, b, "lsqrhipmi355x", strip=True)
    assert e.value.code == PETSC_ERR_SUP and "-ksp_type lsqr" in str(e.value)
    plain = solve(P, a, 37, b, "lsqr", strip=True, normal_tests=True, rtol=1e-10)       # the op-by-op type does not need it
    assert (plain.its, plain.reason) == (24, lr.CONVERGED_RTOL_NORMAL)


@pytest.mark.parametrize("ksp_type", ["lsqr", "lsqrhipmi355x"])
def test_what_is_refused(P, ksp_type):
    A, a, b, guess = problem("tall")
    for kw, code in ((dict(x_size=36), PETSC_ERR_ARG_SIZ), (dict(nullsp=True), PETSC_ERR_SUP), (dict(side=1), PETSC_ERR_SUP),
                     (dict(pc="jacobi"), PETSC_ERR_ARG_SIZ)):                           # side 1: PC_RIGHT; jacobi on the 60 x 37 matrix itself
        with pytest.raises(P.PetscError) as e:
            solve(P, a, 37, b, ksp_type, **kw)
        assert e.value.code == code, (kw, e.value.code, str(e.value)[:300])
    with pytest.raises(P.PetscError) as e:
        solve(P, a, 37, b[:59], ksp_type)
    assert e.value.code == PETSC_ERR_ARG_SIZ


def test_cg_cannot_and_lsqr_can(P):
    """no default PC is picked for the rectangular operator by the LSQR types (-pc_type is not given), and CG cannot run on it"""
    A, a, b, guess = problem("tall")
    with pytest.raises(P.PetscError):
        solve(P, a, 37, b, "cg", pc="none", rtol=1e-8, max_it=200)
    xs = np.linalg.lstsq(A, b, rcond=None)[0]
    for t in ("lsqr", "lsqrhipmi355x"):
        got = solve(P, a, 37, b, t, pc=None, normal_tests=True, rtol=1e-10)
        assert got.reason == lr.CONVERGED_RTOL_NORMAL and np.linalg.norm(got.x - xs) <= 1e-8 * np.linalg.norm(xs), (t, got.its, got.reason)
