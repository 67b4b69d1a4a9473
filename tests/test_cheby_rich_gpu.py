"""KSPCHEBYCHEV / KSPRICHARDSON through the harness on the GPU: the harness types against the host model (tests/cheby_ref.py) and the
plug-in's chebychevhipmi355x / richardsonhipmi355x against the harness types -- x, residual history (device reduction order), iteration
count and reason bit for bit; the general-preconditioner route (PCSOR, a null space); PCApplyRichardson's one-MatSOR shortcut."""
import ctypes as C

import numpy as np
import pytest

import cheby_ref as cr
import nullspace_ref as nr
import orc
import sor_ref as sr

pytestmark = pytest.mark.gpu
EMIN, EMAX = 0.1, 2.0
MONITOR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p)


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def laplace1d(n=1025):
    return sr.from_rows([{c: 2.0 if c == i else -1.0 for c in (i - 1, i, i + 1) if 0 <= c < n} for i in range(n)])


MATRICES = {"p7_6x5x4": lambda: orc.gen_p7(6, 5, 4), "laplace1d_1025": laplace1d}
_cache = {}


def problem(name):
    """(csr, b, a nonzero guess), made once"""
    if name not in _cache:
        csr = MATRICES[name]()
        n = csr[0].size - 1
        _cache[name] = (csr, np.cos(0.37 * np.arange(n)) + 0.25, 0.1 * np.sin(0.61 * np.arange(n)) - 0.05)
    return _cache[name]


def solve(P, csr, b, opts, x0=None, nullsp=False, monitor=None, **tol):
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
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
            sp = P.NullSpace(True, comm=L.COMM_SELF)
            k.set_null_space(sp)
        seen = []
        if monitor is not None:
            cb = MONITOR(lambda ksp, it, rn, ctx: seen.append((it, rn)) or 0)
            L.KSPMonitorSet(k.h, C.cast(cb, C.c_void_p), None, None)
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    out = (vx.array(), k.history(), k.its, k.reason)
    return out + (seen, A) if monitor is not None else out


def agree(got, want, what):
    x, h, its, reason = got[:4]
    xw, hw, itsw, reasonw = want[:4]
    assert (its, reason) == (itsw, reasonw), (what, its, reason, itsw, reasonw)
    assert h.size == hw.size and np.array_equal(bits(h), bits(hw)), (what, h, hw)
    assert np.array_equal(bits(x), bits(xw)), (what, float(np.max(np.abs(x - xw))))


def type_options(kind, t, pc, norm, scale):
    o = "-ksp_type %s -pc_type %s -ksp_norm_type %s" % (t, pc, norm)
    return o + (" -ksp_chebychev_eigenvalues %g,%g" % (EMIN, EMAX) if kind == "chebychev" else " -ksp_richardson_scale %g" % scale)


@pytest.mark.parametrize("norm", ["none", "preconditioned", "unpreconditioned"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("mat", list(MATRICES))
@pytest.mark.parametrize("kind", ["chebychev", "richardson"])
def test_harness_type_walks_the_model_and_the_plugin_type_walks_the_harness_type(P, kind, mat, pc, norm):
    csr, b, guess = problem(mat)
    dinv = cr.jacobi(*csr) if pc == "jacobi" else None
    scale = 0.8 if pc == "jacobi" else 0.2
    for x0 in (None, guess):
        for max_it in (1, 2, 3, 8):
            kw = dict(pc=dinv, norm=norm, x0=x0, max_it=max_it, rtol=1e-30)
            with orc.device_reduction_order():
                model = cr.chebychev(*csr, b, EMIN, EMAX, **kw) if kind == "chebychev" else cr.richardson(*csr, b, scale=scale, **kw)
            what = (kind, mat, pc, norm, "zero" if x0 is None else "nonzero", max_it)
            harness = solve(P, csr, b, type_options(kind, kind, pc, norm, scale), x0=x0, rtol=1e-30, max_it=max_it)
            agree(harness, model, what + ("harness against the model",))
            if harness[3] != cr.DIVERGED_DTOL:          # (without a preconditioner the bounds 0.1, 2.0 do not hold the spectrum: the norm grows)
                assert harness[2] == max_it and harness[3] == (cr.CONVERGED_ITS if norm == "none" else cr.DIVERGED_ITS)
            plugin = solve(P, csr, b, type_options(kind, kind + "hipmi355x", pc, norm, scale), x0=x0, rtol=1e-30, max_it=max_it)
            agree(plugin, harness, what + ("plug-in against the harness",))


@pytest.mark.parametrize("norm", ["preconditioned", "unpreconditioned"])
@pytest.mark.parametrize("kind", ["chebychev", "richardson"])
def test_a_tolerance_stops_the_solve_mid_way(P, kind, norm):
    """rtol 1e-3 on P7 + Jacobi: the convergence test ends the solve before the budget is spent (for Chebyshev: at the checkpoint behind
    which the fused step has already written p[kp1], a work vector) -- same iterate, history, count and reason on all three"""
    csr, b, guess = problem("p7_6x5x4")
    dinv = cr.jacobi(*csr)
    for x0 in (None, guess):
        with orc.device_reduction_order():
            kw = dict(pc=dinv, norm=norm, x0=x0, max_it=200, rtol=1e-3)
            model = cr.chebychev(*csr, b, EMIN, EMAX, **kw) if kind == "chebychev" else cr.richardson(*csr, b, scale=0.8, **kw)
        assert model[3] == cr.CONVERGED_RTOL and 2 < model[2] < 200
        harness = solve(P, csr, b, type_options(kind, kind, "jacobi", norm, 0.8), x0=x0, rtol=1e-3, max_it=200)
        agree(harness, model, (kind, norm, "harness against the model"))
        plugin = solve(P, csr, b, type_options(kind, kind + "hipmi355x", "jacobi", norm, 0.8), x0=x0, rtol=1e-3, max_it=200)
        agree(plugin, harness, (kind, norm, "plug-in against the harness"))


@pytest.mark.parametrize("norm", ["none", "preconditioned", "unpreconditioned"])
@pytest.mark.parametrize("kind", ["chebychev", "richardson"])
def test_general_preconditioner_route_sor(P, kind, norm):
    """-pc_type sor: nothing of the preconditioner can ride in the sweep; a monitor keeps the harness Richardson off PCApplyRichardson,
    which the plug-in type never takes.  The harness type itself is held to the model with sor_ref as the preconditioner."""
    csr, b, guess = problem("p7_6x5x4")
    n = b.size

    def ssor(r):
        return sr.sor_ref(*csr, r, np.zeros(n), 1.0, sr.LOCAL_SYMMETRIC | sr.ZERO_INITIAL_GUESS, 0.0, 1, 1)

    for x0 in (None, guess):
        for max_it, rtol in ((3, 1e-30), (40, 1e-3)):
            opts = lambda t: type_options(kind, t, "sor", norm, 0.9)
            harness = solve(P, csr, b, opts(kind), x0=x0, monitor=True, rtol=rtol, max_it=max_it)
            plugin = solve(P, csr, b, opts(kind + "hipmi355x"), x0=x0, monitor=True, rtol=rtol, max_it=max_it)
            agree(plugin, harness, (kind, norm, max_it))
            assert plugin[4] == harness[4] and (norm == "none" or len(harness[4]) == harness[1].size)      # what the monitors saw
            with orc.device_reduction_order():
                kw = dict(pc=ssor, norm=norm, x0=x0, max_it=max_it, rtol=rtol)
                model = cr.chebychev(*csr, b, EMIN, EMAX, **kw) if kind == "chebychev" else cr.richardson(*csr, b, scale=0.9, **kw)
            agree(harness, model, (kind, norm, max_it, "harness against the model"))


@pytest.mark.parametrize("norm", ["none", "preconditioned"])
@pytest.mark.parametrize("kind", ["chebychev", "richardson"])
def test_general_preconditioner_route_null_space(P, kind, norm):
    """a null space attached (the 6 x 5 x 4 Neumann operator, Jacobi): every z goes through KSP_PCApply and its projection"""
    csr = nr.neumann7(6, 5, 4)
    n = csr[0].size - 1
    b = nr.remove(np.cos(0.37 * np.arange(n)) + 0.25, True, ())
    for max_it in (1, 3, 8):
        harness = solve(P, csr, b, type_options(kind, kind, "jacobi", norm, 0.8), nullsp=True, rtol=1e-30, max_it=max_it)
        plugin = solve(P, csr, b, type_options(kind, kind + "hipmi355x", "jacobi", norm, 0.8), nullsp=True, rtol=1e-30, max_it=max_it)
        agree(plugin, harness, (kind, norm, max_it))
        assert abs(np.mean(harness[0])) <= 1e-13 * np.max(np.abs(harness[0]))
        free = solve(P, csr, b, type_options(kind, kind + "hipmi355x", "jacobi", norm, 0.8), rtol=1e-30, max_it=max_it)
        assert free[2] == max_it and np.all(np.isfinite(free[0]))


@pytest.mark.parametrize("nonzero", [False, True])
def test_richardson_with_sor_is_one_matsor_call(P, nonzero):
    """-ksp_type richardson -pc_type sor, max_it 3, no monitor: PCApplyRichardson_SOR -- x has the bits of ONE MatSOR of 3 sweeps with
    the PC's flags, and the matrix counted exactly one device application"""
    L = P.lib()
    csr, b, guess = problem("p7_6x5x4")
    x0 = guess if nonzero else None
    A = P.Mat.from_csr(*csr)
    vb = P.Vec.from_array(b, comm=L.COMM_SELF)
    vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
    flag = P.SOR_LOCAL_SYMMETRIC_SWEEP | (0 if nonzero else P.SOR_ZERO_INITIAL_GUESS)
    A.sor(vb, vx, omega=1.0, flag=flag, its=3, lits=1)
    ref = vx.array().copy()
    assert np.array_equal(bits(ref), bits(sr.sor_ref(*csr, b, np.zeros(b.size) if x0 is None else x0, 1.0, sr.LOCAL_SYMMETRIC | (0 if nonzero else sr.ZERO_INITIAL_GUESS), 0.0, 3, 1)))
    vx.set_array(np.zeros(b.size) if x0 is None else x0)
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(b"-ksp_type richardson -pc_type sor -ksp_max_it 3")
    try:
        k.set_from_options()
        if nonzero:
            k.set_initial_guess_nonzero(True)
        before = A.sor_info()[4]
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    assert A.sor_info()[4] == before + 1
    assert k.its == 3 and k.reason == cr.CONVERGED_ITS
    assert np.array_equal(bits(vx.array()), bits(ref))
    # the plug-in's type never takes the shortcut: three applications, Richardson's own arithmetic
    vx.set_array(np.zeros(b.size) if x0 is None else x0)
    L.PetscOptionsInsertString(b"-ksp_type richardsonhipmi355x -pc_type sor -ksp_max_it 3 -ksp_norm_type none")
    try:
        k2 = P.KSP(comm=L.COMM_SELF)
        k2.set_operators(A)
        k2.set_from_options()
        if nonzero:
            k2.set_initial_guess_nonzero(True)
        before = A.sor_info()[4]
        k2.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    assert A.sor_info()[4] == before + 3 and k2.its == 3
    # x + B (b - A x) with B one symmetric sweep from zero IS the symmetric sweep from x, in another association: three contracting steps
    # on 120 unknowns with entries of size 1 differ by a few hundred roundings at most
    assert np.max(np.abs(vx.array() - ref)) <= 1e-12 * np.max(np.abs(ref))
