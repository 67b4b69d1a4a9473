"""MINRES on the device: the harness's minres on HIPMI355X vectors against the host model (tests/minres_ref.py) under the device's
reduction order, and minreshipmi355x against minres on the same objects -- x, residual history, iteration count and reason bit for bit.
The indefinite operator is P7(5,4,3) - 3.1 I built on the device with MatShift; the SPD one plain P7(6,5,4)."""
import ctypes as C

import numpy as np
import pytest

import cheby_ref as cr
import minres_ref as mr
import nullspace_ref as nr
import orc

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP = 56
_cache = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def problem(name):
    """(csr of the unshifted operator, shift, b, a nonzero guess), made once"""
    if name not in _cache:
        dims, sigma = {"shifted": ((5, 4, 3), 3.1), "spd": ((6, 5, 4), 0.0)}[name]
        csr = orc.gen_p7(*dims)
        n = csr[0].size - 1
        _cache[name] = (csr, sigma, np.cos(0.37 * np.arange(n)) + 0.25, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[name]


def shifted_csr(csr, sigma):
    """what MatShift(A, -sigma) leaves: a(i,i) + (-sigma)"""
    ai, aj, aa = csr
    aa = aa.copy()
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    aa[rows == aj] += -sigma
    return ai, aj, aa


def solve(P, csr, sigma, b, ksp_type, pc, x0=None, nullsp=False, strip=False, pmat=None, **tol):
    """-> (x, history, its, reason, (fused, opbyop)); strip: the vectors lose "VecMinresFusedOps_C" first; pmat: csr the PC is built from"""
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    if sigma:
        A.shift(-sigma)
    Pm = P.Mat.from_csr(*pmat) if pmat is not None else None
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
    if strip:
        compose = L.raw("PetscObjectComposeFunction")
        compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        assert compose(vx.h, b"VecMinresFusedOps_C", b"", None) == 0
        assert compose(vb.h, b"VecMinresFusedOps_C", b"", None) == 0
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A, Pm)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type %s -pc_type %s" % (ksp_type, pc)).encode())
    try:
        if tol:
            k.set_tolerances(**tol)
        k.set_from_options()
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
        if nullsp:
            k.set_null_space(P.NullSpace(True, comm=L.COMM_SELF))
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    return vx.array(), k.history(), k.its, k.reason, k.fused_step_counts()


def agree(got, want, what):
    x, h, its, reason = got[:4]
    xw, hw, itsw, reasonw = want[:4]
    assert (its, reason) == (itsw, reasonw), (what, its, reason, itsw, reasonw)
    assert h.size == hw.size and np.array_equal(bits(h), bits(hw)), (what, h, hw)
    assert np.array_equal(bits(x), bits(xw)), (what, float(np.max(np.abs(x - xw))))


@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("mat", ["shifted", "spd"])
def test_all_three_walk_together(P, mat, pc):
    """the harness's minres on HIP types is the model under the device's reduction order, and the plug-in's type is the harness's"""
    csr, sigma, b, guess = problem(mat)
    A = shifted_csr(csr, sigma)
    d = cr.jacobi(*A) if pc == "jacobi" else None
    for x0 in (None, guess):
        for max_it, rtol in ((200, 1e-8), (3, 1e-30)):
            what = (mat, pc, "zero" if x0 is None else "nonzero", max_it)
            with orc.device_reduction_order():
                model = mr.minres(*A, b, pc=d, x0=x0, max_it=max_it, rtol=rtol)
            plain = solve(P, csr, sigma, b, "minres", pc, x0=x0, rtol=rtol, max_it=max_it)
            agree(plain, model, what + ("minres against the model",))
            fused = solve(P, csr, sigma, b, "minreshipmi355x", pc, x0=x0, rtol=rtol, max_it=max_it)
            agree(fused, plain, what + ("minreshipmi355x against minres",))
            assert plain[4] == (0, 0) and fused[4] == (fused[2], 0) and fused[2] > 0, (what, fused[2:])
            if max_it == 200:
                assert fused[3] == cr.CONVERGED_RTOL and fused[1][-1] <= 1e-8 * fused[1][0]
                assert np.all(np.diff(fused[1]) <= 0.0)


@pytest.mark.parametrize("pc", ["ilu", "sor"])
def test_a_general_preconditioner_on_the_spd_operator(P, pc):
    """KSP_PCApply forms z and the Lanczos sweep takes it as given"""
    csr, sigma, b, guess = problem("spd")
    for x0 in (None, guess):
        for max_it, rtol in ((200, 1e-8), (2, 1e-30)):
            plain = solve(P, csr, sigma, b, "minres", pc, x0=x0, rtol=rtol, max_it=max_it)
            fused = solve(P, csr, sigma, b, "minreshipmi355x", pc, x0=x0, rtol=rtol, max_it=max_it)
            agree(fused, plain, (pc, max_it))
            assert fused[4] == (fused[2], 0) and fused[2] > 0
            if max_it == 200:
                assert fused[3] == cr.CONVERGED_RTOL


def test_a_null_space_on_the_singular_neumann_operator(P):
    csr = nr.neumann7(6, 5, 4)
    n = csr[0].size - 1
    b = nr.remove(np.cos(0.37 * np.arange(n)) + 0.25, True, ())
    for max_it, rtol in ((1, 1e-30), (3, 1e-30), (200, 1e-8)):
        plain = solve(P, csr, 0.0, b, "minres", "jacobi", nullsp=True, rtol=rtol, max_it=max_it)
        fused = solve(P, csr, 0.0, b, "minreshipmi355x", "jacobi", nullsp=True, rtol=rtol, max_it=max_it)
        agree(fused, plain, ("null space", max_it))
        assert fused[4] == (fused[2], 0)
    assert fused[3] == cr.CONVERGED_RTOL


def test_every_exit_on_both_types(P):
    csr, sigma, b, guess = problem("shifted")
    A = shifted_csr(csr, sigma)
    zero = {t: solve(P, csr, sigma, np.zeros(b.size), t, "jacobi") for t in ("minres", "minreshipmi355x")}       # a zero right-hand side
    for t, got in zero.items():
        assert (got[2], got[3], got[1].size) == (0, mr.DIVERGED_INDEFINITE_MAT, 0) and not got[0].any() and got[4] == (0, 0), (t, got)
    ai, aj, aa = A                                                        # a Jacobi diagonal with one negative entry: the PC is built from pm
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    pa = aa.copy()
    pa[(rows == aj) & (rows == 7)] *= -1.0
    d = cr.jacobi(ai, aj, pa)
    assert np.sum(d < 0) == 1
    with orc.device_reduction_order():
        model = mr.minres(*A, b, pc=d, max_it=60, rtol=1e-8)
    assert model[3] == mr.DIVERGED_INDEFINITE_PC
    plain = solve(P, csr, sigma, b, "minres", "jacobi", pmat=(ai, aj, pa), rtol=1e-8, max_it=60)
    fused = solve(P, csr, sigma, b, "minreshipmi355x", "jacobi", pmat=(ai, aj, pa), rtol=1e-8, max_it=60)
    agree(plain, model, "indefinite PC: minres against the model")
    agree(fused, plain, "indefinite PC")
    assert fused[3] == mr.DIVERGED_INDEFINITE_PC and fused[4] == (fused[2], 0)
    for max_it in (1, 2):
        plain = solve(P, csr, sigma, b, "minres", "jacobi", rtol=1e-8, max_it=max_it)
        fused = solve(P, csr, sigma, b, "minreshipmi355x", "jacobi", rtol=1e-8, max_it=max_it)
        agree(fused, plain, ("out of iterations", max_it))
        assert (fused[2], fused[3], fused[4]) == (max_it, mr.DIVERGED_ITS, (max_it, 0))


def test_cg_fails_where_minres_converges(P):
    csr, sigma, b, guess = problem("shifted")
    cg = solve(P, csr, sigma, b, "cg", "jacobi", rtol=1e-8, max_it=200)
    assert cg[3] < 0, ("cg on an indefinite operator", cg[2:])
    for t in ("minres", "minreshipmi355x"):
        got = solve(P, csr, sigma, b, t, "jacobi", rtol=1e-8, max_it=200)
        assert got[3] == cr.CONVERGED_RTOL and got[1][-1] <= 1e-8 * got[1][0], (t, got[2:])
        A = shifted_csr(csr, sigma)
        res = b - orc.spmv(*A, got[0])
        true = np.linalg.norm(res * cr.jacobi(*A))
        print(t, "its", got[2], "estimate", got[1][-1], "true", true)
        assert abs(got[1][-1] - true) <= 1e-5 * true                       # the margin tests/test_minres_cpu.py holds the model to


def test_vectors_without_the_table_are_refused_at_set_up(P):
    csr, sigma, b, guess = problem("shifted")
    with pytest.raises(P.PetscError) as e:
        solve(P, csr, sigma, b, "minreshipmi355x", "jacobi", strip=True)
    assert e.value.code == PETSC_ERR_SUP and "minres" in str(e.value)
    plain = solve(P, csr, sigma, b, "minres", "jacobi", strip=True, rtol=1e-8, max_it=200)     # the op-by-op type does not need it
    assert plain[3] == cr.CONVERGED_RTOL
