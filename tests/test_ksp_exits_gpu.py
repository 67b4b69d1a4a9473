"""Every way out of the registered Krylov types (cghipmi355x at -ksp_cg_fused 0..4, gmreshipmi355x and bcgshipmi355x at
-ksp_*_fused 0/1, and the eight registered since: tfqmr-, cgs-, bicg-, pipecghipmi355x at -ksp_*_fused 0/1, minres-, chebychev-,
richardson- and lsqrhipmi355x, which read no level) against the plain harness types over the same device Vec / Mat types, on the
table of tests/kspexits.py, tiny (the one-lane tail) and replicated block-diagonally to >= 4096 rows (several workgroups).

Per case, solver, preconditioner, size and level:
  * error or reason: both return, or both raise the same PETSc error code (the plain type decides which);
  * where both return: x, the residual history, its and reason carry the plain type's bits (NaN compared as bits, tests/specials.py);
    the oracle replayed in the device's reduction order agrees where it returns the same kind of exit;
  * after an error or a refused step (INDEFINITE_MAT / _PC, BREAKDOWN, NULL, DIVERGED_NAN) x is the plain type's, bit for bit;
  * a second solve on the same KSP (a benign system of the same size) carries the bits of a fresh KSP;
  * the eight: (its, reason) are the table's and the host model's (kspexits.model); every quantity is held to the plain type's bits
    (none of their DESIGN.md sections takes a sum from another tree); KSPHIPMI355XGetFusedStepCounts reports what the solver's own
    GPU test derives from its, and no op-by-op step at a fused level;
  * what the types refuse at set-up they refuse with the plain type's code.
Shapes: n = 2, 3, 8, 12 and 4^k copies of them.  Cost is launches, not bytes: about 0.1 - 2 s per test."""
import numpy as np
import pytest

import kspexits as kx
import vecspecials as vs
from gpu import PRODUCT_KSP

pytestmark = pytest.mark.gpu

LEVELS = {"cg": ["-ksp_cg_fused %d" % k for k in range(5)] + [""], "gmres": ["-ksp_gmres_fused 0", "-ksp_gmres_fused 1", ""],
          "bcgs": ["-ksp_bcgs_fused 0", "-ksp_bcgs_fused 1", ""],
          # what KSPSetFromOptions_* of host/kspfused.c reads: a level for four of the eight, none for the others
          "tfqmr": ["-ksp_tfqmr_fused 0", "-ksp_tfqmr_fused 1", ""], "cgs": ["-ksp_cgs_fused 0", "-ksp_cgs_fused 1", ""],
          "bicg": ["-ksp_bicg_fused 0", "-ksp_bicg_fused 1", ""], "pipecg": ["-ksp_pipecg_fused 0", "-ksp_pipecg_fused 1", ""],
          "minres": [""], "chebychev": [""], "richardson": [""], "lsqr": [""]}
PRODUCT = dict(PRODUCT_KSP, **{k: k + "hipmi355x" for k in ("tfqmr", "cgs", "bicg", "pipecg", "minres", "chebychev", "richardson", "lsqr")})
PAIRS = [(c.name, s) for c in kx.CASES for s in kx.solvers_of(c) if s in kx.SOLVERS]
MORE_PAIRS = [(c.name, s) for c in kx.CASES for s in kx.solvers_of(c) if s in kx.MORE_SOLVERS]


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


class Run:
    """one KSP on one system; solve() returns ("ok", x, hist, its, reason) or ("error", code, x)"""

    def __init__(self, P, c, ksp_type, pc, opts, system, label=None):
        """label: the table's solver label where it carries a variant or the case settings (kspexits.MORE_SOLVERS)"""
        self.P, L = P, P.lib()
        ai, aj, aa, b, x0 = system
        self.n = b.size
        self.pc, self.label = pc, label
        self.kind, self.variant = (kx.kind_of(label), kx.variant_of(label)) if label else (None, None)
        self.ncols = None if c.ncols is None else c.ncols * (b.size // (kx.matrix_of(c)[0].size - 1))
        self.k = P.KSP(comm=L.COMM_SELF)
        self.operators(ai, aj, aa)
        text = "-ksp_type %s -pc_type %s -ksp_gmres_restart %d %s %s" % (ksp_type, pc, c.restart, "-ksp_pc_side right" if c.pc_right else "", opts)
        if self.variant in ("preconditioned", "unpreconditioned", "natural", "none"):
            text += " -ksp_norm_type " + self.variant
        if self.kind == "chebychev":
            text += " -ksp_chebychev_eigenvalues %r,%r" % tuple(float(v) for v in c.eig[pc])
        if self.kind == "richardson":
            text += " -ksp_richardson_scale %r" % float(c.scale[pc])
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(text.encode())
        try:
            self.k.set_tolerances(**c.tol)
            self.k.set_from_options()
        finally:
            L.PetscOptionsClear()
        if self.variant == "normal":
            self.k.set_convergence_test("KSPLSQRDefaultConverged")
        self.k.record_history()

    def operators(self, ai, aj, aa):
        """KSPLSQR with a preconditioner: its matrix is A'A, formed on the device"""
        L = self.P.lib()
        self.keep = getattr(self, "keep", []) + [getattr(self, "A", None), getattr(self, "Pm", None)]     # the KSP may still hold them
        self.A = self.P.Mat.from_csr(ai, aj, aa, ncols=self.ncols, comm=L.COMM_SELF) if self.ncols is not None else self.P.Mat.from_csr(ai, aj, aa, comm=L.COMM_SELF)
        self.Pm = self.A.transpose().matmult(self.A) if (self.kind == "lsqr" and self.pc != "none") else None
        if self.Pm is not None:
            self.k.set_operators(self.A, self.Pm)
        else:
            self.k.set_operators(self.A)

    def solve(self, b, x0=None):
        P, L = self.P, self.P.lib()
        vb = P.Vec.from_array(b, comm=L.COMM_SELF)
        vx = P.Vec.from_array(np.zeros(b.size if self.ncols is None else self.ncols) if x0 is None else x0, comm=L.COMM_SELF)
        L.KSPSetInitialGuessNonzero(self.k.h, 0 if x0 is None else 1)
        before = self.k.fused_step_counts()
        try:
            self.k.solve(vb, vx)
        except P.PetscError as e:
            return ("error", e.code, vx.array())
        after = self.k.fused_step_counts()
        return ("ok", vx.array(), self.k.history(), self.k.its, self.k.reason, (after[0] - before[0], after[1] - before[1]))

    def second(self, Ab, b):
        """the same KSP on another matrix of the same size with the default tolerances"""
        self.operators(*Ab)
        self.k.set_tolerances(rtol=1e-5, abstol=1e-50, dtol=1e4, max_it=60)
        return self.solve(b)


def same(a, b):
    """tests/vecspecials.py's rule: any NaN equals any NaN (sign and payload of a NaN are not part of the contract), every other
    value bit for bit"""
    return a.shape == b.shape and not vs.differing(a, b).any()


def close_level4(a, b, h0, its, n):
    """-ksp_cg_fused 4 (the default) takes p'w from the SpMV pass, another summation tree (DESIGN, kspfused.c: "agrees with the other
    levels to rounding, not bit for bit"): where iterations were completed its history and x are compared to rounding -- a dot over
    n terms differs by at most n eps relative between two trees, the step length with it, over `its` iterations, times 8 for the
    growth through the recurrences of these well-conditioned systems -- and to 1e-9 relative, the bound of
    test_ksp_cg_fused_forms_are_bit_identical.  Non-finite entries by class."""
    if a.shape != b.shape:
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]):
        return False
    tol = 1e-9 * np.abs(b[fin]) + 8.0 * max(its, 1) * n * 2.220446049250313e-16 * h0
    return bool(np.all(np.abs(a[fin] - b[fin]) <= tol))


def describe(r):
    return r[:2] if r[0] == "error" else ("ok", r[3], r[4], r[2][-3:])


@pytest.fixture(scope="module")
def systems():
    memo = {}

    def get(name, size):
        if (name, size) not in memo:
            memo[name, size] = kx.system(kx.BY_NAME[name], size)
        return memo[name, size]
    return get


@pytest.mark.parametrize("name,solver", PAIRS)
def test_registered_type_leaves_like_the_plain_type(P, systems, name, solver):
    c = kx.BY_NAME[name]
    for pc in kx.pcs_of(c):
        e = kx.expected(c, solver, pc)
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            b, x0 = sysm[3], sysm[4]
            where = "%s %s %s %s" % (name, solver, pc, size)
            plain = Run(P, c, solver, pc, "", sysm).solve(b, x0)
            # the table: an error where it names one, with the code it names; a reason otherwise
            if e.error is not None:
                assert plain[0] == "error" and plain[1] == e.error, (where, describe(plain))
            else:
                assert plain[0] == "ok", (where, describe(plain))
                xo, ho, itso, ro = kx.oracle(c, solver, pc, size, device_order=True)
                if (name, solver) in kx.ROUNDING:
                    assert (plain[3], plain[4]) in kx.ROUNDING[name, solver], (where, describe(plain))
                else:
                    assert (plain[3], plain[4]) == (itso, ro) == (e.its, e.reason), (where, describe(plain), itso, ro)
                    keep = -1 if "bcgs_tt_zero_s_zero" in e.exits else None      # the oracle logs 0.0 there, the reference the old norm
                    assert np.array_equal(plain[2][:keep], ho[:keep], equal_nan=True), (where, plain[2], ho)     # NaN by position: the host's NaN has its own payload
                    assert np.array_equal(plain[1], xo, equal_nan=True), (where, plain[1][:8], xo[:8])
            for opts in LEVELS[solver]:
                got = Run(P, c, PRODUCT_KSP[solver], pc, opts, sysm).solve(b, x0)
                at = where + " [" + (opts or "default") + "]"
                assert got[0] == plain[0], (at, describe(got), describe(plain))
                if plain[0] == "error":
                    assert got[1] == plain[1], (at, describe(got), describe(plain))
                    if solver == "cg" and opts in ("-ksp_cg_fused 4", "") and e.its > 1 and not same(got[2], plain[2]):
                        # level 4 completed iterations in its own summation tree before the refused one: the iterate to rounding
                        fin = plain[2][np.isfinite(plain[2])]
                        assert close_level4(got[2], plain[2], float(np.max(np.abs(fin), initial=0.0)), e.its, b.size), (at, got[2][:8], plain[2][:8])
                        continue
                    assert same(got[2], plain[2]), (at, got[2][:8], plain[2][:8])        # x after the refused step
                    continue
                assert (got[3], got[4]) == (plain[3], plain[4]), (at, describe(got), describe(plain))
                stepped = solver == "cg" and opts in ("-ksp_cg_fused 4", "") and len(plain[2]) > 1       # level 4 and an update was made
                if stepped and not same(got[2], plain[2]):
                    xscale = float(np.max(np.abs(plain[1][np.isfinite(plain[1])]), initial=0.0))
                    assert close_level4(got[2], plain[2], plain[2][0], plain[3], b.size), (at, got[2], plain[2])
                    assert close_level4(got[1], plain[1], xscale, plain[3], b.size), (at, got[1][:8], plain[1][:8])
                    continue
                assert same(got[2], plain[2]), (at, got[2], plain[2])                     # history
                assert same(got[1], plain[1]), (at, got[1][:8], plain[1][:8])             # x: after a refused step as after any other


@pytest.mark.parametrize("name,solver", PAIRS)
def test_second_solve_on_the_same_ksp_carries_the_bits_of_a_fresh_one(P, systems, name, solver):
    c = kx.BY_NAME[name]
    for pc in kx.pcs_of(c):
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            n = sysm[3].size
            nb = kx.matrix_of(c)[0].size - 1
            rows = kx.tridiag(nb, 1.0, 4.0, 1.0)
            benign = kx.Case("b", rows, np.arange(1.0, nb + 1), None, kx.DEFAULT_TOL, c.restart, c.pc_right, c.pcs, {}, False)
            Ab = kx.system(benign, size)
            assert Ab[3].size == n
            used = Run(P, c, PRODUCT_KSP[solver], pc, "", sysm)
            used.solve(sysm[3], sysm[4])
            again = used.second(Ab[:3], Ab[3])
            fresh = Run(P, c, PRODUCT_KSP[solver], pc, "", sysm).second(Ab[:3], Ab[3])
            where = "%s %s %s %s" % (name, solver, pc, size)
            assert again[0] == fresh[0] == "ok", (where, describe(again), describe(fresh))
            assert again[4] == fresh[4] and fresh[4] in (kx.RTOL, kx.ATOL) and again[3] == fresh[3] > 0, (where, describe(again), describe(fresh))
            assert same(again[2], fresh[2]) and same(again[1], fresh[1]), (where, again[2], fresh[2])


# ------------------------------------------------------------------------------------------------ the eight types registered since
def expected_counts(kind, opts, pc, e, got):
    """KSPHIPMI355XGetFusedStepCounts after one solve, by the expressions of the solvers' own GPU tests (test_tfqmr_gpu.py: three
    sweeps per iteration entered, one fewer where a checkpoint ends CGS; test_bicg_gpu.py and the solver's comment: 2 its, 2 its + 1
    after dpi == 0; test_pipelined_cg_gpu.py: its; test_minres_gpu.py: (its, 0); test_lsqr_gpu.py: (2 its, its) with PCNONE, (its, its)
    with a PC, the second slot being update sweeps), and with -ksp_*_fused 0 the same iterations op by op"""
    hist, its, reason = got[2], got[3], got[4]
    off = opts.endswith("fused 0")
    if kind == "tfqmr":
        entered = hist.size // 2
        return (0, entered) if off else (3 * entered, 0)
    if kind == "cgs":
        return (0, its) if off else (3 * its - (1 if its and reason not in (kx.ITS, kx.BREAKDOWN) else 0), 0)
    if kind == "bicg":
        extra = 1 if reason == kx.BREAKDOWN and "bicg_beta_zero" not in e.exits else 0
        return (0, its + extra) if off else (2 * its + extra, 0)
    if kind == "pipecg":
        return (0, its) if off else (its, 0)
    if kind == "minres":
        return (its, 0)
    if kind == "lsqr":
        return (2 * its, its) if pc == "none" else (its, its)
    return (0, 0)


@pytest.mark.parametrize("name,solver", MORE_PAIRS)
def test_registered_type_of_the_eight_leaves_like_the_plain_type(P, systems, name, solver):
    c = kx.BY_NAME[name]
    kind = kx.kind_of(solver)
    for pc in kx.pcs_of(c, solver):
        e = kx.expected(c, solver, pc)
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            b, x0 = sysm[3], sysm[4]
            where = "%s %s %s %s" % (name, solver, pc, size)
            plain = Run(P, c, kind, pc, "", sysm, solver).solve(b, x0)
            if e.error is not None:
                assert plain[0] == "error" and plain[1] == e.error, (where, describe(plain))
            else:
                assert plain[0] == "ok", (where, describe(plain))
                assert plain[5] == (0, 0), (where, plain[5])
                xm, hm, itsm, rm = kx.model(c, solver, pc, size, device_order=True)
                print(where, "plain", plain[3], plain[4], "model", itsm, rm, "table", e.its, e.reason)
                if (name, solver) in kx.ROUNDING:
                    assert (plain[3], plain[4]) in kx.ROUNDING[name, solver], (where, describe(plain))
                else:
                    assert (plain[3], plain[4]) == (itsm, rm) == (e.its, e.reason), (where, describe(plain), itsm, rm)
                if plain[3] == 0 and not (kind == "tfqmr" and plain[2].size > 1):      # nothing was done: x is the guess
                    guess = np.zeros(plain[1].size) if x0 is None else x0
                    assert same(plain[1], guess), (where, plain[1][:8])
            for opts in LEVELS[kind]:
                got = Run(P, c, PRODUCT[kind], pc, opts, sysm, solver).solve(b, x0)
                at = where + " [" + (opts or "default") + "]"
                assert got[0] == plain[0], (at, describe(got), describe(plain))
                if plain[0] == "error":
                    assert got[1] == plain[1], (at, describe(got), describe(plain))
                    assert same(got[2], plain[2]), (at, got[2][:8], plain[2][:8])        # x after the refused solve
                    continue
                assert (got[3], got[4]) == (plain[3], plain[4]), (at, describe(got), describe(plain))
                assert same(got[2], plain[2]), (at, got[2], plain[2])                     # history
                assert same(got[1], plain[1]), (at, got[1][:8], plain[1][:8])             # x: after a refused step as after any other
                assert got[5] == expected_counts(kind, opts, pc, e, got), (at, got[5], describe(got))
                if not opts.endswith("fused 0") and kind != "lsqr":                       # no exit falls back to the public calls
                    assert got[5][1] == 0, (at, got[5])


def benign_like(c, solver, size):
    """(ai, aj, aa, b) of a benign full-rank system of the case's shape: 4 on the diagonal, 1 beside it, and a 1 per row or column
    beyond the square part; b = A (1, 2, ...), so a rectangular system is consistent"""
    ai0 = kx.matrix_of(c)[0]
    m = ai0.size - 1
    n = m if c.ncols is None else c.ncols
    rows = [{j: (4.0 if j == i else 1.0) for j in (i - 1, i, i + 1) if 0 <= j < n} for i in range(m)]
    for i in range(n, m):
        rows[i] = {i % n: 1.0}
    for j in range(m, n):
        rows[j % m][j] = 1.0
    xs = np.arange(1.0, n + 1)
    bb = np.array([sum(v * xs[j] for j, v in r.items()) for r in rows])
    benign = kx.Case("b", rows, bb, None, kx.DEFAULT_TOL, c.restart, c.pc_right, c.pcs, {}, False, c.ncols)
    return kx.system(benign, size)


BENIGN_EIG = {"none": (2.0, 6.0), "jacobi": (0.5, 1.5)}       # 4 + 2 cos lies inside (2, 6); B = 1 / 4
BENIGN_SCALE = {"none": 0.25, "jacobi": 1.0}


@pytest.mark.parametrize("name,solver", MORE_PAIRS)
def test_second_solve_of_the_eight_carries_the_bits_of_a_fresh_ksp(P, systems, name, solver):
    c = kx.BY_NAME[name]
    kind, variant = kx.kind_of(solver), kx.variant_of(solver)

    def second(run, Ab):
        if kind == "chebychev":
            run.k.set_chebychev_eigenvalues(BENIGN_EIG[run.pc][1], BENIGN_EIG[run.pc][0])
        if kind == "richardson":
            run.k.set_richardson_scale(BENIGN_SCALE[run.pc])
        return run.second(Ab[:3], Ab[3])
    for pc in kx.pcs_of(c, solver):
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            Ab = benign_like(c, solver, size)
            assert Ab[3].size == sysm[3].size
            used = Run(P, c, PRODUCT[kind], pc, "", sysm, solver)
            used.solve(sysm[3], sysm[4])
            again = second(used, Ab)
            fresh = second(Run(P, c, PRODUCT[kind], pc, "", sysm, solver), Ab)
            where = "%s %s %s %s" % (name, solver, pc, size)
            assert again[0] == fresh[0] == "ok", (where, describe(again), describe(fresh))
            assert (again[3], again[4]) == (fresh[3], fresh[4]) and fresh[3] > 0, (where, describe(again), describe(fresh))
            block = kx.matrix_of(c)[0].size - 1
            if kind == "minres" and fresh[4] == kx.INDEF_PC:          # the lucky breakdown: the Krylov space of a block is exhausted, x is exact
                assert fresh[3] <= block, (where, describe(fresh))     # (r'z < 1e-18 is taken there too, as in the reference)
            elif not (kind == "pipecg" and variant != "natural"):     # those forms of the snapshot do not converge like CG (harness/krylov.c)
                assert fresh[4] > 0, (where, describe(fresh))
            assert same(again[2], fresh[2]) and same(again[1], fresh[1]), (where, again[2], fresh[2])
            assert again[5] == fresh[5], (where, again[5], fresh[5])  # nothing of the first solve is counted or queued into the second


def attempt(P, c, ksp_type, pc, opts, sysm, label, nullsp=False):
    try:
        run = Run(P, c, ksp_type, pc, opts, sysm, label)
        if nullsp:
            run.k.set_null_space(P.NullSpace(True, comm=P.lib().COMM_SELF))
        got = run.solve(sysm[3], sysm[4])
    except P.PetscError as err:                                      # refused before the solve
        return ("error", err.code)
    return got[:2] if got[0] == "error" else ("ok",)


def test_refusals_at_set_up(P, systems):
    """a side the type does not support, Chebychev bounds of the wrong order or of mixed sign, BiCG and LSQR with a null space, an
    LSQR preconditioner matrix that is not n x n: the registered type answers as the plain type does, with its code"""
    c = kx.BY_NAME["benign"]
    sysm = systems("benign", "tiny")
    for solver in ("tfqmr", "cgs", "bicg", "minres", "pipecg", "chebychev", "richardson", "lsqr"):
        for side in ("right", "symmetric"):
            plain = attempt(P, c, solver, "jacobi", "-ksp_pc_side " + side, sysm, solver)
            got = attempt(P, c, PRODUCT[solver], "jacobi", "-ksp_pc_side " + side, sysm, solver)
            print(solver, side, plain, got)
            assert got == plain, (solver, side, got, plain)
            if solver in ("tfqmr", "cgs", "bicg", "lsqr") and side == "right":
                assert plain == ("error", kx.ERR_SUP), (solver, side, plain)
    for bounds in ((3, 1), (-1, 1)):                                 # (emin, emax): wrong order, mixed sign
        bad = c._replace(eig={"none": bounds})
        for t in ("chebychev", PRODUCT["chebychev"]):
            assert attempt(P, bad, t, "none", "", sysm, "chebychev") == ("error", kx.ERR_ARG_INCOMP), (t, bounds)
    for solver in ("bicg", "lsqr"):
        for t in (solver, PRODUCT[solver]):
            assert attempt(P, c, t, "none", "", sysm, solver, nullsp=True) == ("error", kx.ERR_SUP), t
    tall = kx.BY_NAME["ls_tall"]
    for t in ("lsqr", PRODUCT["lsqr"]):                              # Jacobi on the 3 x 2 matrix itself (no label: no A'A is formed)
        assert attempt(P, tall, t, "jacobi", "", systems("ls_tall", "tiny"), None) == ("error", kx.ERR_ARG_SIZ), t
