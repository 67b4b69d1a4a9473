"""pipecghipmi355x against the harness's pipecg on the same objects: x, residual history, iteration count and reason bit for bit --
every norm type, PCNONE / PCJACOBI (the preconditioner rides in the sweep) and PCILU (the general route), a nonzero guess, every
exit, a null space, and the three ways back to the public calls (option, vectors without the table, a general PC's m)."""
import ctypes as C

import numpy as np
import pytest

import nullspace_ref as nr
import orc

pytestmark = pytest.mark.gpu
NORMS = ["preconditioned", "unpreconditioned", "natural", "none"]
DIVERGED_ITS = -3
# 5 x 4 x 3: one workgroup; 17 x 16 x 16: 4352 rows, the reduction spans two workgroups
MATRICES = {"p7_5x4x3": (5, 4, 3), "p7_17x16x16": (17, 16, 16)}
_cache = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def problem(name):
    """(csr, b, a nonzero guess), made once"""
    if name not in _cache:
        csr = orc.gen_p7(*MATRICES[name])
        n = csr[0].size - 1
        _cache[name] = (csr, np.cos(0.37 * np.arange(n)) + 0.25, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[name]


def solve(P, csr, b, opts, x0=None, nullsp=False, strip=False, after=None, **tol):
    """-> (x, history, its, reason, (fused, opbyop)); strip: the solution vector loses "VecPipelinedCGFusedOps_C" first"""
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
    if strip:
        compose = L.raw("PetscObjectComposeFunction")
        compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        assert compose(vx.h, b"VecPipelinedCGFusedOps_C", b"", None) == 0
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(opts.encode())
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
    if after:
        after(L, vb, vx)
    return vx.array(), k.history(), k.its, k.reason, k.fused_step_counts()


def agree(got, want, what):
    x, h, its, reason = got[:4]
    xw, hw, itsw, reasonw = want[:4]
    assert (its, reason) == (itsw, reasonw), (what, its, reason, itsw, reasonw)
    assert h.size == hw.size and np.array_equal(bits(h), bits(hw)), (what, h, hw)
    assert np.array_equal(bits(x), bits(xw)), (what, float(np.max(np.abs(x - xw))))


def options(t, pc, norm, extra=""):
    return "-ksp_type %s -pc_type %s -ksp_norm_type %s %s" % (t, pc, norm, extra)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu"])
@pytest.mark.parametrize("mat", list(MATRICES))
def test_plugin_type_walks_the_harness_type(P, mat, pc, norm):
    """max_it 25: with the preconditioned or the unpreconditioned norm this is the branch of the snapshot that does not converge
    (res'u reduced in iteration 0 only); rtol 1e-6 ends the other two norms on the small operator by a tolerance"""
    csr, b, guess = problem(mat)
    for x0 in (None, guess):
        for max_it, rtol in ((25, 1e-6), (3, 1e-30)):
            what = (mat, pc, norm, "zero" if x0 is None else "nonzero", max_it)
            plain = solve(P, csr, b, options("pipecg", pc, norm), x0=x0, rtol=rtol, max_it=max_it)
            fused = solve(P, csr, b, options("pipecghipmi355x", pc, norm), x0=x0, rtol=rtol, max_it=max_it)
            agree(fused, plain, what)
            assert plain[4] == (0, 0)
            nf, no = fused[4]
            assert no == 0 and nf == fused[2] and nf > 0, (what, fused[2:], "every update step in one sweep")


@pytest.mark.parametrize("norm", NORMS)
def test_every_way_back_to_the_public_calls_gives_the_same_bits(P, norm):
    csr, b, guess = problem("p7_17x16x16")
    kw = dict(x0=guess, rtol=1e-30, max_it=12)
    plain = solve(P, csr, b, options("pipecg", "jacobi", norm), **kw)
    fused = solve(P, csr, b, options("pipecghipmi355x", "jacobi", norm), **kw)
    agree(fused, plain, (norm, "fused"))
    assert fused[4] == (12, 0)
    off = solve(P, csr, b, options("pipecghipmi355x", "jacobi", norm, "-ksp_pipecg_fused false"), **kw)
    agree(off, plain, (norm, "-ksp_pipecg_fused false"))
    assert off[4] == (0, 12)
    stripped = solve(P, csr, b, options("pipecghipmi355x", "jacobi", norm), strip=True, **kw)
    agree(stripped, plain, (norm, "vectors without the table"))
    assert stripped[4] == (0, 12)


@pytest.mark.parametrize("norm", ["preconditioned", "unpreconditioned", "natural"])
def test_a_solve_that_ends_at_iteration_zero(P, norm):
    csr, b, guess = problem("p7_5x4x3")
    plain = solve(P, csr, np.zeros(b.size), options("pipecg", "jacobi", norm))               # a zero right-hand side: the first norm is 0
    fused = solve(P, csr, np.zeros(b.size), options("pipecghipmi355x", "jacobi", norm))
    agree(fused, plain, norm)
    assert fused[2] == 0 and fused[3] > 0 and fused[1].size == 1 and not fused[0].any() and fused[4] == (0, 0), fused


@pytest.mark.parametrize("max_it", [1, 2, 5])
@pytest.mark.parametrize("norm", NORMS)
def test_out_of_iterations_leaves_no_split_phase_pending(P, norm, max_it):
    """KSP_DIVERGED_ITS: the sweep of the last permitted iteration queued no sums -- a VecDotBegin / VecDotEnd pair on the same vectors
    right after the solve succeeds and returns their dot"""
    csr, b, guess = problem("p7_17x16x16")
    seen = []

    def pair(L, vb, vx):
        r = C.c_double()
        L.VecDotBegin(vb.h, vx.h, C.byref(r))
        L.PetscCommSplitReductionBegin(L.COMM_SELF)
        L.VecDotEnd(vb.h, vx.h, C.byref(r))
        seen.append((r.value, vb.dot(vx)))

    plain = solve(P, csr, b, options("pipecg", "jacobi", norm), rtol=1e-30, max_it=max_it)
    fused = solve(P, csr, b, options("pipecghipmi355x", "jacobi", norm), rtol=1e-30, max_it=max_it, after=pair)
    agree(fused, plain, (norm, max_it))
    assert fused[2] == max_it and fused[3] == DIVERGED_ITS and fused[4] == (max_it, 0)
    assert len(seen) == 1 and seen[0][0] == seen[0][1]


@pytest.mark.parametrize("norm", NORMS)
def test_an_exit_at_a_checkpoint_leaves_nothing_pending(P, norm):
    """an exit the convergence test decides (a tolerance with the natural norm; with the other norms whatever the plain type meets)
    comes right after the End calls: a later split phase works"""
    csr, b, guess = problem("p7_5x4x3")
    done = []

    def pair(L, vb, vx):
        r = C.c_double()
        L.VecDotBegin(vb.h, vx.h, C.byref(r)); L.VecDotEnd(vb.h, vx.h, C.byref(r))
        done.append(r.value == vb.dot(vx))

    plain = solve(P, csr, b, options("pipecg", "none", norm), rtol=1e-4, max_it=60)
    fused = solve(P, csr, b, options("pipecghipmi355x", "none", norm), rtol=1e-4, max_it=60, after=pair)
    agree(fused, plain, norm)
    assert done == [True]


@pytest.mark.parametrize("norm", NORMS)
def test_general_route_null_space(P, norm):
    """a null space attached (the 6 x 5 x 4 Neumann operator, Jacobi): every m goes through KSP_PCApply and its projection; the rest of
    the update is still one sweep"""
    csr = nr.neumann7(6, 5, 4)
    n = csr[0].size - 1
    b = nr.remove(np.cos(0.37 * np.arange(n)) + 0.25, True, ())
    for max_it in (1, 3, 8):
        plain = solve(P, csr, b, options("pipecg", "jacobi", norm), nullsp=True, rtol=1e-30, max_it=max_it)
        fused = solve(P, csr, b, options("pipecghipmi355x", "jacobi", norm), nullsp=True, rtol=1e-30, max_it=max_it)
        agree(fused, plain, (norm, max_it))
        assert fused[4] == (max_it, 0)
