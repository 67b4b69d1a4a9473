"""Flexible GMRES and PCKSP on the device: the harness's fgmres on HIPMI355X vectors and the plug-in's fgmreshipmi355x, with
-ksp_fgmres_fused on, off and left at its default (off), against the host model (tests/fgmres_ref.py) under the device's reduction order -- x, residual history,
iteration count and reason bit for bit.  PCNONE, PCJACOBI and ILU(0), restarts 5 and 20, zero and nonzero guesses, the fall-backs of the
fused step and their counts, PCKSP with a fixed and with a truly variable inner solver, KSPFGMRESSetModifyPC, every way out of the cycle,
a second solve after MatScale.  The operators are the upwinded 5-point convection-diffusion stencil on 33 x 31 (1023 rows) and 41 x 25
(1025 rows) grids; the exits run on 8- to 40-row matrices."""
import numpy as np
import pytest

import bicg_ref as br
import cheby_ref as cr
import fgmres_ref as fr
import nullspace_ref as nr
import orc
from test_ilu_sweeps_gpu import V

pytestmark = pytest.mark.gpu
PETSC_ERR_PLIB = 77
EPS = np.finfo(np.float64).eps
GRIDS = {1023: (33, 31), 1025: (41, 25)}
VARIANTS = (("fgmres", ""), ("fgmreshipmi355x", "-ksp_fgmres_fused 1"), ("fgmreshipmi355x", "-ksp_fgmres_fused 0"), ("fgmreshipmi355x", ""))   # the default is off
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


def model_pc(csr, pc):
    if pc == "none":
        return None
    if pc == "jacobi":
        return cr.jacobi(*csr)
    key = ("ilu", csr[0].size)
    if key not in _cache:
        _cache[key] = orc.ilu0_factor(*csr)
    f = _cache[key]
    return lambda r: orc.ilu0_solve(f, np.ascontiguousarray(r))


def model(csr, b, pc, key=None, **kw):
    """the model's run under the device's reduction order, made once per key"""
    if key is not None and key in _cache:
        return _cache[key]
    with orc.device_reduction_order():
        R = fr.fgmres(*csr, b, pc=model_pc(csr, pc) if isinstance(pc, str) else pc, **kw)
    if key is not None:
        _cache[key] = R
    return R


class Run:
    pass


def solve(P, csr, b, ksp_type, pcopts, x0=None, opts="", restart=30, nullsp=None, modify=None, A=None, ksp=None, **tol):
    """one KSPSolve -> Run with x, hist, its, reason, counts, the KSP and the matrix (for a second solve)"""
    L = P.lib()
    A = A if A is not None else P.Mat.from_csr(*csr)
    vb = V(P, b)
    vx = V(P, np.zeros(b.size) if x0 is None else x0)
    k = ksp if ksp is not None else P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    if "-pc_type" not in pcopts:
        pcopts = "-pc_type " + pcopts
    L.PetscOptionsInsertString(("-ksp_type %s %s -ksp_gmres_restart %d %s" % (ksp_type, pcopts, restart, opts)).encode())
    try:
        k.set_tolerances(**tol)
        if ksp is None:
            k.set_from_options()
        if nullsp is not None:
            k.set_null_space(nullsp)
        if modify is not None:
            k.fgmres_set_modify_pc(modify)
        if x0 is not None:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    r = Run()
    r.x, r.hist, r.its, r.reason, r.counts, r.ksp, r.A = vx.array(), k.history(), k.its, k.reason, k.fused_step_counts(), k, A
    return r


def agree(got, R, what):
    xw, hw, itsw, reasonw = R
    assert (got.its, got.reason) == (itsw, reasonw), (what, got.its, got.reason, itsw, reasonw)
    assert got.hist.size == hw.size and np.array_equal(bits(got.hist), bits(hw)), (what, got.hist, hw)
    assert np.array_equal(bits(got.x), bits(xw)), (what, float(np.max(np.abs(got.x - xw))))


def check_counts(got, R, ksp_type, opts, restart, fusible, what):
    if ksp_type == "fgmres":
        assert got.counts == (0, 0), what
    elif "fused 1" not in opts or not fusible:
        assert got.counts == (0, got.its), (what, got.counts)
    else:
        assert got.counts == fr.expected_step_counts(R, restart), (what, got.counts)


@pytest.mark.parametrize("restart", [5, 20])
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu"])
@pytest.mark.parametrize("n", [1023, 1025])
def test_the_three_drivers_walk_with_the_model(P, n, pc, restart):
    """restart 5: several cycles; restart 20: the basis crosses the MDot width of 16.  ILU(0) is no diagonal: the plug-in takes KSP_PCApply
    and the plain normalising call, still one wait per step, and counts no fused step"""
    csr, b, guess = problem(n)
    for x0 in (None, guess):
        kw = dict(rtol=1e-10, max_it=400, restart=restart)
        R = model(csr, b, pc, key=("walk", n, pc, restart, x0 is not None), x0=x0, **kw)
        assert R.reason == fr.CONVERGED_RTOL and R.its > restart
        for ksp_type, opts in VARIANTS:
            what = (n, pc, restart, x0 is not None, ksp_type, opts)
            got = solve(P, csr, b, ksp_type, pc, x0=x0, opts=opts, **kw)
            agree(got, R, what)
            check_counts(got, R, ksp_type, opts, restart, pc != "ilu", what)


def test_steps_past_32_basis_vectors_take_the_plain_call(P):
    csr, b, _ = problem(1023)
    kw = dict(rtol=1e-30, max_it=36, restart=40)
    R = model(csr, b, "jacobi", **kw)
    assert (R.its, R.reason, R.nv[-1]) == (36, fr.DIVERGED_ITS, 36)
    for ksp_type, opts in VARIANTS[1:]:
        got = solve(P, csr, b, ksp_type, "jacobi", opts=opts, **kw)
        agree(got, R, opts)
        assert got.counts == ((32, 4) if "fused 1" in opts else (0, 36)), got.counts


@pytest.mark.parametrize("refine", [fr.ALWAYS, fr.IFNEEDED])
def test_refinement_takes_the_unfused_step(P, refine):
    csr, b, _ = problem(1025)
    kw = dict(rtol=1e-10, max_it=400, restart=20)
    R = model(csr, b, "jacobi", refine=refine, **kw)
    assert R.reason == fr.CONVERGED_RTOL
    for ksp_type, opts in VARIANTS:
        got = solve(P, csr, b, ksp_type, "jacobi", opts=opts + " -ksp_gmres_cgs_refinement_type " + refine, **kw)
        agree(got, R, (refine, ksp_type, opts))
        assert got.counts == ((0, 0) if ksp_type == "fgmres" else (0, got.its))


def test_a_null_space_refuses_the_fused_step(P):
    """on the right side nothing is projected (KSP_RemoveNullSpace acts on the left only), so the model is the plain one; the plug-in
    must not fold the preconditioner into its sweep once a null space is attached"""
    csr = nr.neumann7(7, 6, 5)
    n = csr[0].size - 1
    u = np.sin(0.4 * np.arange(n))
    b = orc.spmv(*csr, u - np.mean(u))
    kw = dict(rtol=1e-8, max_it=300, restart=20)
    R = model(csr, b, "jacobi", **kw)
    assert R.reason == fr.CONVERGED_RTOL
    for ksp_type, opts in VARIANTS:
        ns = P.NullSpace(constant=True, comm=P.lib().COMM_SELF)
        got = solve(P, csr, b, ksp_type, "jacobi", opts=opts, nullsp=ns, **kw)
        agree(got, R, (ksp_type, opts))
        assert got.counts == ((0, 0) if ksp_type == "fgmres" else (0, got.its))
        got.ksp.set_null_space(None)


# ------------------------------------------------------------------------------------------------ PCKSP
def inner_richardson(csr):
    d = cr.jacobi(*csr)

    def run(r):
        x, hist, its, reason, _ = cr.richardson(*csr, r, pc=d, norm=cr.PRECONDITIONED, max_it=3)
        return x, its
    return run


def inner_bcgs(csr):
    def run(r):
        x, hist, its, reason = orc.ksp_solve(*csr, r, ksp="bcgs", pc="jacobi", rtol=1e-2)
        return x, its
    return run


RICH = "ksp -ksp_ksp_type richardson -ksp_pc_type jacobi -ksp_ksp_max_it 3"
BCGS = "ksp -ksp_ksp_type bcgs -ksp_pc_type jacobi -ksp_ksp_rtol 1e-2"


@pytest.mark.parametrize("inner", ["richardson", "bcgs"])
@pytest.mark.parametrize("n", [1023, 1025])
def test_an_iteration_as_the_preconditioner(P, n, inner):
    """inner Richardson + Jacobi, 3 steps: a fixed polynomial; inner BiCGStab + Jacobi to rtol 1e-2: another operator at every call.
    Bits of the model with the same inner model solver; PCKSPGetTotalIterations is the model's sum"""
    csr, b, _ = problem(n)
    B = fr.PCKSP(inner_richardson(csr) if inner == "richardson" else inner_bcgs(csr))
    kw = dict(rtol=1e-10, max_it=300, restart=20)
    R = model(csr, b, B, **kw)
    assert R.reason == fr.CONVERGED_RTOL and B.applications == R.its
    for ksp_type, opts in VARIANTS[:2]:
        got = solve(P, csr, b, ksp_type, RICH if inner == "richardson" else BCGS, opts=opts, **kw)
        agree(got, R, (n, inner, ksp_type))
        assert got.ksp.get_pc().ksp_total_iterations() == B.total, (ksp_type, B.total)
        assert got.counts == ((0, 0) if ksp_type == "fgmres" else (0, got.its))
        assert got.ksp.get_pc().ksp_get_ksp().get_type() == inner


def test_gmres_with_a_fixed_chebyshev_inner_solver_converges(P):
    """4 Chebyshev steps without a norm are one fixed polynomial in D^-1 A: a linear preconditioner, which plain left-preconditioned
    GMRES may use.  The bounds are taken from the spectrum of the dense D^-1 A."""
    csr, b, _ = problem(1023)
    ev = np.linalg.eigvals(np.diag(cr.jacobi(*csr)) @ br.dense(*csr)).real
    emax, emin = 1.05 * float(ev.max()), 0.1 * float(ev.max())
    pcopts = ("ksp -ksp_ksp_type chebychevhipmi355x -ksp_ksp_max_it 4 -ksp_ksp_norm_type none -ksp_pc_type jacobi "
              "-ksp_ksp_chebychev_eigenvalues %.17g,%.17g" % (emin, emax))
    got = solve(P, csr, b, "gmres", pcopts, opts="-ksp_pc_side left", rtol=1e-8, max_it=300)
    assert got.reason == fr.CONVERGED_RTOL and 0 < got.its < 300, (got.its, got.reason)
    total = got.ksp.get_pc().ksp_total_iterations()                               # one application per step and one per cycle start
    assert total % 4 == 0 and total >= 4 * (got.its + 1), total
    assert got.hist[-1] <= 1e-8 * got.hist[0]


def test_fgmres_history_is_the_true_residual_with_a_variable_pc(P):
    """with the BiCGStab inner solver the last history entry of fgmreshipmi355x is the norm of b - A x: |true - history| <=
    100 eps cond(A) |b| (the update x += Z y is exact up to rounding whatever the Z_k were; eps cond(A) |b| is the size of a backward-stable
    residual, 100 covers the steps).  The contrast: left-preconditioned gmres with the same inner solver stops with CONVERGED_RTOL on its
    recurrence's estimate while the true relative residual is above cond(A) * rtol, more than any ONE linear preconditioner could hide
    (the reasoning and the CPU model's numbers -- 5.2e-09 claimed, 4.8e-03 true against 2.2e-06 -- are in
    tests/test_fgmres_cpu.py::test_gmres_claims_a_residual_it_does_not_have_fgmres_does_not, where the mismatch shows first)."""
    csr, b, _ = problem(1023)
    M = br.dense(*csr)
    cond, nb = float(np.linalg.cond(M)), float(np.linalg.norm(b))
    got = solve(P, csr, b, "fgmreshipmi355x", BCGS, rtol=1e-8, max_it=300, restart=20)
    true = float(np.linalg.norm(b - M @ got.x))
    bound = 100.0 * EPS * cond * nb
    print("true residual %.6e history %.6e difference %.3e bound %.3e" % (true, got.hist[-1], abs(true - got.hist[-1]), bound))
    assert got.reason == fr.CONVERGED_RTOL and abs(true - got.hist[-1]) <= bound
    plain = solve(P, csr, b, "gmres", BCGS, opts="-ksp_pc_side left", rtol=1e-8, max_it=300)
    claimed, true = plain.hist[-1] / plain.hist[0], float(np.linalg.norm(b - M @ plain.x)) / nb
    print("gmres its %d reason %d claimed %.3e true %.3e cond * rtol %.3e" % (plain.its, plain.reason, claimed, true, cond * 1e-8))
    assert plain.reason == fr.CONVERGED_RTOL and claimed <= 1e-8 and true > cond * 1e-8


def test_modify_pc_sees_the_models_arguments(P):
    csr, b, _ = problem(1025)
    kw = dict(rtol=1e-10, max_it=400, restart=5)
    R = model(csr, b, "jacobi", **kw)
    for ksp_type, opts in VARIANTS[:2]:
        seen = []
        got = solve(P, csr, b, ksp_type, "jacobi", modify=lambda its, k, rn: seen.append((its, k, rn)), **kw)
        agree(got, R, ksp_type)
        assert len(seen) == len(R.modify) == R.its
        assert [s[:2] for s in seen] == [m[:2] for m in R.modify]
        assert np.array_equal(bits([s[2] for s in seen]), bits([m[2] for m in R.modify]))
        assert got.counts == ((0, 0) if ksp_type == "fgmres" else (0, got.its))     # a routine that may change the PC: nothing is folded in


# ------------------------------------------------------------------------------------------------ every way out
def csr_of(rows):
    rows = np.asarray(rows, dtype=np.float64)
    ai, aj, aa = [0], [], []
    for r in rows:
        for c in np.flatnonzero(r):
            aj.append(c); aa.append(r[c])
        ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64)


def tridiag(n):
    return csr_of(np.diag(np.full(n, 4.0)) + np.diag(np.full(n - 1, -1.0), 1) + np.diag(np.full(n - 1, -2.0), -1))


def _shift8():
    rows = np.eye(8); rows[0, 0] = 0.0; rows[0, 1] = 1.0                          # A e1 = 0
    return csr_of(rows)


def _e(n, j, v):
    e = np.zeros(n); e[j] = v
    return e


def _nan_b(n):
    b = np.ones(n); b[3] = np.nan
    return b


T40, B40 = tridiag(40), np.cos(0.3 * np.arange(40)) + 2.0
# name -> (csr, b, pc, model / solver keywords, (its, reason) the case is there for; None: whatever the model says)
EXITS = {
    "zero_rhs": (T40, np.zeros(40), "jacobi", {}, (0, fr.CONVERGED_ATOL)),
    "dtol_at_start": (T40, B40, "jacobi", dict(dtol=1e-3, rtol=1e-30), (0, fr.DIVERGED_DTOL)),
    "nan_norm": (T40, _nan_b(40), "jacobi", {}, (0, fr.DIVERGED_NAN)),
    "happy_breakdown": (csr_of(np.diag(np.arange(1.0, 9.0))), _e(8, 2, 2.0), "none", {}, (1, fr.CONVERGED_ATOL)),
    "zero_pivot_in_update": (_shift8(), _e(8, 0, 1.0), "none", {}, (1, fr.CONVERGED_ATOL)),
    "restart": (T40, B40, "jacobi", dict(restart=5, rtol=1e-12), None),
    "max_it_inside_cycle": (T40, B40, "jacobi", dict(restart=5, rtol=1e-30, max_it=7), (7, fr.DIVERGED_ITS)),
    "max_it_at_boundary": (T40, B40, "jacobi", dict(restart=5, rtol=1e-30, max_it=10), (10, fr.DIVERGED_ITS)),
    "atol": (T40, B40, "jacobi", dict(abstol=1e-3, rtol=1e-30), None),
    "norm_none": (T40, B40, "jacobi", dict(restart=5, max_it=6, norm=fr.NONE), (6, fr.CONVERGED_ITS)),
}


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_way_out_through_the_plug_in(P, name):
    """a rotation of length 0 is not in the table: no input reaches it (tests/test_fgmres_cpu.py::test_model_exits says why)"""
    csr, b, pc, kw, expect = EXITS[name]
    kw = dict(kw)
    norm = kw.pop("norm", None)
    R = model(csr, b, pc, norm=norm or fr.UNPRECONDITIONED, **kw)
    if expect is not None:
        assert (R.its, R.reason) == expect
    else:
        assert R.reason > 0 and R.its > kw.get("restart", 0)
    for ksp_type, opts in VARIANTS:
        got = solve(P, csr, b, ksp_type, pc, opts=opts + (" -ksp_norm_type none" if norm else ""), **kw)
        agree(got, R, (name, ksp_type, opts))


def test_happy_breakdown_nobody_notices_is_an_error(P):
    csr, b = csr_of(np.diag(np.arange(1.0, 9.0))), _e(8, 2, 2.0)
    for ksp_type, opts in VARIANTS:
        with pytest.raises(P.PetscError) as e:
            solve(P, csr, b, ksp_type, "none", opts=opts + " -ksp_norm_type none", max_it=5)
        assert e.value.code == PETSC_ERR_PLIB, (ksp_type, e.value)


def test_second_solve_after_matscale_equals_a_fresh_solver(P):
    csr, b, _ = problem(1023)
    kw = dict(rtol=1e-10, max_it=400, restart=20)
    scaled = (csr[0], csr[1], 2.0 * csr[2])
    R = model(scaled, b, "jacobi", **kw)
    for ksp_type, opts in VARIANTS[1:]:
        first = solve(P, csr, b, ksp_type, "jacobi", opts=opts, **kw)
        P.lib().MatScale(first.A.h, 2.0)
        again = solve(P, csr, b, ksp_type, "jacobi", A=first.A, ksp=first.ksp, **kw)
        fresh = solve(P, scaled, b, ksp_type, "jacobi", opts=opts, **kw)
        agree(again, R, ("again", opts))
        agree(fresh, R, ("fresh", opts))
