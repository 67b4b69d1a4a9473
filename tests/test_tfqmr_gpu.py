"""TFQMR and CGS on the device: the harness's tfqmr / cgs on HIPMI355X vectors against the host model (tests/tfqmr_ref.py) under the
device's reduction order, and tfqmrhipmi355x / cgshipmi355x against the plain types on the same objects -- x, residual history,
iteration count and reason bit for bit -- fused, with -ksp_*_fused 0, and on vectors stripped of "VecTfqmrFusedOps_C".  The operators
are the upwinded 5-point convection-diffusion stencil on 33 x 31 (1023 rows) and 41 x 25 (1025 rows) grids."""
import ctypes as C

import numpy as np
import pytest

import cheby_ref as cr
import orc
import tfqmr_ref as tr

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP = 56
GRIDS = {1023: (33, 31), 1025: (41, 25)}
MODEL = {"tfqmr": tr.tfqmr, "cgs": tr.cgs}
_cache = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def problem(n):
    """(csr, b, a nonzero guess), made once"""
    if n not in _cache:
        csr = tr.convdiff(*GRIDS[n])
        assert csr[0].size - 1 == n
        _cache[n] = (csr, np.cos(0.37 * np.arange(n)) + 0.25, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[n]


def model_pc(csr, pc):
    if pc == "none":
        return None
    if pc == "jacobi":
        return cr.jacobi(*csr)
    f, shifts = orc.ilu0_factor_shift(*csr)
    assert shifts == 0
    return lambda r: orc.ilu0_solve(f, np.ascontiguousarray(r))


def solve(P, csr, b, ksp_type, pc, x0=None, strip=False, opts="", side=None, **tol):
    """-> (x, history, its, reason, (fused, opbyop)); strip: the vectors lose "VecTfqmrFusedOps_C" first"""
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
    if strip:
        compose = L.raw("PetscObjectComposeFunction")
        compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        assert compose(vx.h, b"VecTfqmrFusedOps_C", b"", None) == 0
        assert compose(vb.h, b"VecTfqmrFusedOps_C", b"", None) == 0
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type %s -pc_type %s %s" % (ksp_type, pc, opts)).encode())
    try:
        k.set_tolerances(**dict(dict(dtol=tr.DTOL), **tol))
        k.set_from_options()
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
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


def entered(which, got):
    """iterations whose sweeps ran: TFQMR leaves its at the iterations COMPLETED when a half step ends the solve"""
    its, hist = got[2], got[1]
    return hist.size // 2 if which == "tfqmr" else its            # one entry for iteration 0, then two per iteration entered


def three_routes(P, which, csr, b, pc, what, **kw):
    """the plain type, then the plug-in's type fused, with the option off, and on stripped vectors: all four the same bits"""
    plain = solve(P, csr, b, which, pc, **kw)
    assert plain[4] == (0, 0)
    hip = which + "hipmi355x"
    fused = solve(P, csr, b, hip, pc, **kw)
    agree(fused, plain, what + (hip, "fused"))
    n_it = entered(which, fused)
    # three sweeps per iteration entered; a checkpoint that ends CGS comes before the iteration's update sweep (TFQMR's exits inside
    # the half steps still run it, without the tail)
    n_sweeps = 3 * n_it - (1 if which == "cgs" and n_it and fused[3] != tr.DIVERGED_ITS else 0)
    assert fused[4] == (n_sweeps, 0), (what, fused[2:], n_it)
    off = solve(P, csr, b, hip, pc, opts="-ksp_%s_fused 0" % which, **kw)
    agree(off, plain, what + (hip, "option off"))
    assert off[4] == (0, n_it), (what, off[2:])
    stripped = solve(P, csr, b, hip, pc, strip=True, **kw)
    agree(stripped, plain, what + (hip, "stripped vectors"))
    assert stripped[4] == (0, n_it), (what, stripped[2:])
    return plain


@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu"])
@pytest.mark.parametrize("n", [1023, 1025])
@pytest.mark.parametrize("which", ["tfqmr", "cgs"])
def test_all_routes_walk_with_the_model(P, which, n, pc):
    csr, b, guess = problem(n)
    mpc = model_pc(csr, pc)
    for x0 in (None, guess) if pc == "jacobi" else (None,):
        for max_it, rtol in ((400, 1e-8), (3, 1e-30)):
            what = (which, n, pc, "zero" if x0 is None else "nonzero", max_it)
            with orc.device_reduction_order():
                model = MODEL[which](*csr, b, pc=mpc, x0=x0, max_it=max_it, rtol=rtol, dtol=tr.DTOL)
            plain = three_routes(P, which, csr, b, pc, what, x0=x0, rtol=rtol, max_it=max_it)
            agree(plain, model, what + ("the harness type against the model",))
            if max_it == 400:
                assert plain[3] == cr.CONVERGED_RTOL and plain[1][-1] <= 1e-8 * plain[1][0]
                print(what, "its", plain[2], "estimate", plain[1][-1], "|b - A x|", float(np.linalg.norm(b - orc.spmv(*csr, plain[0]))))
            else:
                assert (plain[2], plain[3]) == (3, tr.DIVERGED_ITS)


def half_step_tolerances(hist):
    """as tests/test_tfqmr_cpu.py: entry k >= 1 belongs to half (k - 1) % 2 of iteration (k - 1) // 2"""
    found = {}
    for k in range(3, hist.size):
        m = (k - 1) % 2
        before = float(np.min(hist[:k]))
        if m not in found and hist[k] < 0.9 * before:
            found[m] = (k, 0.5 * (hist[k] + before) / hist[0])
    return found


def test_every_exit_on_both_routes(P):
    csr, b, guess = problem(1023)
    n = b.size
    for which in ("tfqmr", "cgs"):
        zero = three_routes(P, which, csr, np.zeros(n), "jacobi", (which, "zero rhs"))          # iteration 0
        assert (zero[2], zero[1].size) == (0, 1) and zero[3] > 0 and not zero[0].any()
        sw = (np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([1.0, 1.0]))
        bd = three_routes(P, which, sw, np.array([1.0, 0.0]), "none", (which, "breakdown"))      # [[0,1],[1,0]], b = e1: s = 0 at once
        assert (bd[2], bd[3], bd[1].size) == (0, tr.DIVERGED_BREAKDOWN, 1) and not bd[0].any()
        for max_it in (1, 2):
            out = three_routes(P, which, csr, b, "jacobi", (which, "out of iterations", max_it), rtol=1e-30, max_it=max_it)
            assert (out[2], out[3]) == (max_it, tr.DIVERGED_ITS)
    with orc.device_reduction_order():
        full = tr.tfqmr(*csr, b, pc=cr.jacobi(*csr), max_it=400, rtol=1e-8)[1]
    found = half_step_tolerances(full)
    assert set(found) == {0, 1}, found
    for m, (k, rtol) in found.items():
        got = three_routes(P, "tfqmr", csr, b, "jacobi", ("tfqmr", "half", m), rtol=rtol, max_it=400)
        assert got[3] == cr.CONVERGED_RTOL and got[1].size == k + 1 and got[2] == (k - 1) // 2, (m, k, got[2:])
        assert np.array_equal(bits(got[1]), bits(full[:k + 1]))


def test_right_preconditioning_is_refused(P):
    csr, b, guess = problem(1023)
    for t in ("tfqmr", "cgs", "tfqmrhipmi355x", "cgshipmi355x"):
        with pytest.raises(P.PetscError) as e:
            solve(P, csr, b, t, "jacobi", opts="-ksp_pc_side right")
        assert e.value.code == PETSC_ERR_SUP, (t, e.value)
