"""The ways out of a Krylov solve (test_ksp_exits_cpu.py, test_ksp_exits_gpu.py): a table of tiny systems, each NAMED for the exit
line of KSPSolve_CG / _GMRES / _BCGS (oracle/ksp_oracle.c, harness/krylov.c, host/kspfused.c) or of KSPDefaultConverged it leaves
through.  Pure numpy + the oracle; imports without a GPU.

The systems are a few rows of small integers or powers of two, so the zeros the exits hang on ARE zeros: a dot that vanishes does
so in any summation order, on one lane or over sixty-four workgroups.  Every case also exists replicated block-diagonally
(replicated()) with a power-of-two number of copies to >= 4096 rows: the same exact zeros, the same exits, reductions over several
wavefronts and workgroups; the tiny form runs the one-lane tail.

What a case says per solver is (its, reason, exit) with pc none, and the same under "jacobi" where Jacobi applies (no zero on the
diagonal).  ERROR cases: the reference, the harness and the registered types raise a PETSc error there; the oracle never raises,
so `its, reason` is then the oracle's stand-in and `error` the PETSc code the plain harness type must raise (the GPU test takes
the plain type as the reference for error-versus-reason).

Exits nothing here reaches, with the reason:
  * gmres_breakdown_inner  H(k,k) == 0 for a k BELOW the last column (gmres.c:330-336's loop; the second test in
    gmres_build_soln).  A column below the last one was rotated, and the rotation writes H(k,k) = sqrt(h_k^2 + h_k+1^2), which is
    the tt the DIVERGED_NULL test has just found non-zero; only the last column of a cycle that ended in the happy branch is
    unrotated.  The line is dead code in the reference; the harness and the registered type have one loop for both.
  * "happy breakdown but convergence not indicated" (PETSC_ERR_PLIB): the happy branch sets the norm to 0.0, which
    KSPDefaultConverged accepts whatever the tolerances (0 <= ttol); only a replaced convergence test could refuse it.
  * a stored Inf that waits for the Krylov space: 0 * Inf is NaN in the first product, so inf_in_A has its NaN at iteration 1
    (p'w = NaN for CG).  The late arrivals are entries of 2^1023 (overflow_norm: the norm overflows first, CG included;
    overflow_pw: p'w = Inf first); see the comment at those cases.
  * dtol = 0.5 at iteration 1: KSPDefaultConverged tests rnorm >= dtol * rnorm0 at iteration 0 too; dtol is 1.5 (cases dtol, dtol_both).
  * DIVERGED_NULL as the reason returned: see zero_matrix.
Rows where rounding decides what follows the named exit are listed in ROUNDING with every outcome an exact run could take.
rho_zero: see RHO_ZERO_SEARCH below.
"""
import collections

import numpy as np

import orc

NAN, INF = float("nan"), float("inf")
RTOL, ATOL, ITS_OK = 2, 3, 4
NULL, ITS, DTOL, BREAKDOWN, INDEF_PC, DNAN, INDEF_MAT = -2, -3, -4, -5, -8, -9, -10
ERR_FP, ERR_PLIB = 72, 77             # PETSC_ERR_FP, PETSC_ERR_PLIB (include/petscmini.h)
SOLVERS = ("cg", "gmres", "bcgs")
# (case, solver) whose way past the named exit is decided by rounding, with every outcome an exact run could take: GMRES on
# `singular` has spanned the space after two steps; what is left of the third vector is rounding (the oracle's own order: walks on
# to max_it, the row of the issue) or an exact zero (replicated: the happy branch on a singular H, BREAKDOWN at 2)
ROUNDING = {("singular", "gmres"): ((10, -3), (2, -5))}
LEFT_OUT = {}                        # exit -> why no case reaches it; at most bcgs_rho_zero may stand here.  The search found one: empty.


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

# every exit line; the table must claim each one (test_ksp_exits_cpu.py)
EXITS = (
    # KSPDefaultConverged (iterativ.c:702-780)
    "conv_nan", "conv_rtol", "conv_atol", "conv_dtol",
    # KSPSolve_CG (cg.c:92-286)
    "cg_start_reason",        # the test at iteration 0 already has a reason
    "cg_beta_zero",           # z'r == 0: CONVERGED_ATOL
    "cg_indefinite_pc",       # z'r changed sign
    "cg_indefinite_mat",      # p'w == 0, or changed sign
    "cg_dot_not_finite",      # p'w NaN or Inf: PETSC_ERR_FP (the oracle goes on to DIVERGED_NAN)
    "cg_test_reason",         # the test after an update has a reason
    "cg_max_it",
    # KSPSolve_GMRES (gmres.c:118-409)
    "gmres_res_zero",         # !res at the start of a cycle
    "gmres_start_reason",     # the test at the start of a cycle has a reason
    "gmres_null",             # update_hessenberg: tt == 0
    "gmres_test_reason",      # the test after a step has a reason
    "gmres_happy",            # the happy branch ended the cycle
    "gmres_breakdown",        # H(it,it) == 0 in the triangular solve
    "gmres_cycle_full",       # restart columns done: another cycle
    "gmres_max_it_in_cycle",  # ksp->its reached max_it inside a cycle
    "gmres_max_it",           # total >= max_it after a cycle: DIVERGED_ITS
    # KSPSolve_BCGS (bcgs.c:43-160)
    "bcgs_start_reason",
    "bcgs_sv_zero",           # (v, r~) == 0: PETSC_ERR_PLIB "Divide by zero" (the oracle: -5 without counting the iteration)
    "bcgs_tt_zero_s_zero",    # t = 0 and s = 0: x + alpha p, CONVERGED_RTOL, the OLD norm logged
    "bcgs_tt_zero_s_nonzero", # t = 0, s != 0: DIVERGED_BREAKDOWN
    "bcgs_test_reason",
    "bcgs_rho_zero",          # the rho this iteration used was 0
    "bcgs_max_it",
)

Expect = collections.namedtuple("Expect", "its reason exits error")
Case = collections.namedtuple("Case", "name rows b x0 tol restart pc_right pcs expect cg_anyway")


def E(its, reason, exits, error=None):
    return Expect(its, reason, tuple(exits.split()), error)


def dense(rows):
    """every entry stored, zeros too"""
    return [{j: float(v) for j, v in enumerate(r)} for r in rows]


def tridiag(n, lo=-1.0, d=2.0, up=-1.0):
    return [{c: (d if c == i else lo if c < i else up) for c in (i - 1, i, i + 1) if 0 <= c < n} for i in range(n)]


def csr(rows):
    ai = np.zeros(len(rows) + 1, dtype=np.int32)
    aj, aa = [], []
    for i, r in enumerate(rows):
        for c in sorted(r):
            aj.append(c); aa.append(float(r[c]))
        ai[i + 1] = len(aj)
    return ai, np.array(aj, dtype=np.int32), np.array(aa, dtype=np.float64)


def _inf_tridiag(both, v=INF):
    rows = tridiag(8)
    rows[5][6] = v
    if both:
        rows[6][5] = v
    return rows


def maxit_matrix():
    import sor_ref
    return sor_ref.nonsym200(12, dominant=True)


SPD2 = dense([[2, 1], [1, 2]])
DEFAULT_TOL = dict(rtol=1e-5, abstol=1e-50, dtol=1e4, max_it=10)

# RHO_ZERO_SEARCH.  KSPSolve_BCGS leaves through `rho == 0` (bcgs.c:146) when (r_k, r~) vanishes exactly for a k >= 1 although the
# residual has not met the tolerance.  A numpy restatement of the recurrence that names its exit line (bcgs_exit below) was run on
# every matrix of 2 rows with entries in {-2..2} against every right-hand side in {-2..2}^2 (15625 systems: none leaves there) and
# on random draws of 3 and of 4 rows from the same set: 5 hits in the first 218 draws of 3 rows, 5 in the first 882 of 4 rows.
# The upper triangular hit is the case rho_zero (default tolerances, nothing forced); the oracle agrees, with Jacobi as well.
CASES = []


def case(name, rows, b, expect, x0=None, tol=None, restart=30, pc_right=False, pcs=("none", "jacobi"), cg_anyway=False):
    t = dict(DEFAULT_TOL)
    t.update(tol or {})
    CASES.append(Case(name, rows, np.array(b, dtype=np.float64), None if x0 is None else np.array(x0, dtype=np.float64), t, restart, pc_right,
                      tuple(pcs), expect, cg_anyway))


def matrix_of(c):
    return c.rows if isinstance(c.rows, tuple) else csr(c.rows)


def is_symmetric(c):
    ai, aj, aa = matrix_of(c)
    d = {}
    for i in range(ai.size - 1):
        for q in range(ai[i], ai[i + 1]):
            d[i, int(aj[q])] = aa[q]
    return all(d.get((j, i), 0.0) == v or (v != v) for (i, j), v in d.items())


def jacobi_applies(c):
    ai, aj, aa = matrix_of(c)
    dg = orc.get_diagonal(ai, aj, aa)
    return bool(np.all(dg != 0.0))


def solvers_of(c):
    """CG is left out where the matrix is not symmetric and the case is not about that"""
    return [s for s in SOLVERS if s in c.expect and (s != "cg" or c.cg_anyway or is_symmetric(c))]


def pcs_of(c):
    return [p for p in c.pcs if p == "none" or jacobi_applies(c)]


def copies_for(n):
    """a power of FOUR: the norm of the replicated right-hand side is then the tiny one's times a power of two, exactly"""
    k = 1
    while k * n < 4096:
        k *= 4
    return k


def replicated(c):
    """(ai, aj, aa, b, x0) of the block-diagonal matrix of copies_for(n) copies"""
    ai, aj, aa = matrix_of(c)
    n = ai.size - 1
    k = copies_for(n)
    nz = int(ai[-1])
    Ai = np.concatenate([[0], (ai[1:][None, :] + nz * np.arange(k)[:, None]).ravel()]).astype(np.int32)
    Aj = (aj[None, :] + n * np.arange(k)[:, None]).ravel().astype(np.int32)
    Aa = np.tile(aa, k)
    return Ai, Aj, Aa, np.tile(c.b, k), None if c.x0 is None else np.tile(c.x0, k)


def system(c, size):
    if size == "tiny":
        ai, aj, aa = matrix_of(c)
        return ai, aj, aa, c.b.copy(), None if c.x0 is None else c.x0.copy()
    return replicated(c)


def oracle(c, solver, pc, size="tiny", device_order=False):
    ai, aj, aa, b, x0 = system(c, size)
    kw = dict(ksp=solver, pc=pc, x0=x0, restart=c.restart, pc_right=1 if c.pc_right else 0, **c.tol)
    if device_order:
        with orc.device_reduction_order():
            return orc.ksp_solve(ai, aj, aa, b, **kw)
    return orc.ksp_solve(ai, aj, aa, b, **kw)


def expected(c, solver, pc):
    e = c.expect[solver]
    if isinstance(e, dict):
        e = e[pc]
    return e


def bcgs_exit(ai, aj, aa, b, tol, jacobi=False):
    """numpy restatement of KSPSolve_BCGS from a zero guess (left PC none / Jacobi) that NAMES the line it leaves through:
    (exit, its, reason).  Independent of the oracle's C; used to check the BiCGStab claims of the table and for the rho_zero search."""
    n = ai.size - 1
    A = np.zeros((n, n))
    for i in range(n):
        for q in range(ai[i], ai[i + 1]):
            A[i, aj[q]] = aa[q]
    d = np.ones(n)
    if jacobi:
        dg = np.diag(A).copy()
        d = np.where(dg == 0.0, 1.0, 1.0 / np.where(dg == 0.0, 1.0, dg))
    K = lambda v: d * np.array([sum(A[i, j] * v[j] for j in range(n)) for i in range(n)])

    def test(rn, r0, ttol):
        if not np.isfinite(rn):
            return DNAN
        if rn <= ttol:
            return ATOL if rn < tol["abstol"] else RTOL
        if rn >= tol["dtol"] * r0:
            return DTOL
        return 0
    with np.errstate(all="ignore"):
        r = d * b
        rn0 = float(np.sqrt(np.sum(r * r)))
        ttol = max(tol["rtol"] * rn0, tol["abstol"])
        why = test(rn0, rn0, ttol)
        if why:
            return "bcgs_start_reason", 0, why
        rs = r.copy(); p = np.zeros(n); v = np.zeros(n); x = np.zeros(n)
        rho_old = alpha = omega_old = np.float64(1.0)
        its = 0
        for i in range(tol["max_it"]):
            rho = np.float64(np.sum(r * rs))
            beta = (rho / rho_old) * (alpha / omega_old)
            p = r + (-omega_old * beta) * v + beta * p
            v = K(p)
            d1 = np.float64(np.sum(v * rs))
            if d1 == 0.0:
                return "bcgs_sv_zero", its, BREAKDOWN
            alpha = rho / d1
            s = r - alpha * v
            t = K(s)
            d1, d2 = np.float64(np.sum(s * t)), np.float64(np.sum(t * t))
            if d2 == 0.0:
                if float(np.sum(s * s)) != 0.0:
                    return "bcgs_tt_zero_s_nonzero", its, BREAKDOWN
                return "bcgs_tt_zero_s_zero", its + 1, RTOL
            omega = d1 / d2
            x = x + alpha * p + omega * s
            r = s - omega * t
            rho_old, omega_old = rho, omega
            its += 1
            why = test(float(np.sqrt(np.sum(r * r))), rn0, ttol)
            if why:
                return "bcgs_test_reason", its, why
            if rho == 0.0:
                return "bcgs_rho_zero", its, BREAKDOWN
        return "bcgs_max_it", its, ITS


def cg_exit(ai, aj, aa, b, tol, jacobi=False):
    """the same for KSPSolve_CG (preconditioned norm, zero guess, the FINITE checks of the harness included): (exit, its, reason or
    None where PETSC_ERR_FP is raised)"""
    n = ai.size - 1
    A = np.zeros((n, n))
    for i in range(n):
        for q in range(ai[i], ai[i + 1]):
            A[i, aj[q]] = aa[q]
    d = np.ones(n)
    if jacobi:
        dg = np.diag(A).copy()
        d = np.where(dg == 0.0, 1.0, 1.0 / np.where(dg == 0.0, 1.0, dg))
    mult = lambda v: np.array([sum(A[i, j] * v[j] for j in range(n)) for i in range(n)])
    with np.errstate(all="ignore"):
        r = np.array(b, dtype=np.float64)
        z = d * r
        rn0 = np.sqrt(np.sum(z * z))
        ttol = max(tol["rtol"] * rn0, tol["abstol"])

        def test(rn):
            if not np.isfinite(rn):
                return DNAN
            if rn <= ttol:
                return ATOL if rn < tol["abstol"] else RTOL
            if rn >= tol["dtol"] * rn0:
                return DTOL
            return 0
        why = test(rn0)
        if why:
            return "cg_start_reason", 0, why
        rz = np.float64(np.sum(z * r))
        if not np.isfinite(rz):
            return "cg_dot_not_finite", 0, None
        rz_last, pw = np.float64(1.0), np.float64(0.0)
        p = np.zeros(n)
        for k in range(tol["max_it"]):
            if rz == 0.0:
                return "cg_beta_zero", k + 1, ATOL
            if k > 0 and rz * rz_last < 0.0:
                return "cg_indefinite_pc", k + 1, INDEF_PC
            p = z.copy() if k == 0 else z + (rz / rz_last) * p
            pw_last = pw
            w = mult(p)
            pw = np.float64(np.sum(p * w))
            rz_last = rz
            if not np.isfinite(pw):
                return "cg_dot_not_finite", k + 1, None
            if pw == 0.0 or (k > 0 and pw * pw_last <= 0.0):
                return "cg_indefinite_mat", k + 1, INDEF_MAT
            a = rz / pw
            r = r - a * w
            z = d * r
            why = test(np.sqrt(np.sum(z * z)))
            if why:
                return "cg_test_reason", k + 1, why
            rz = np.float64(np.sum(z * r))
            if not np.isfinite(rz):
                return "cg_dot_not_finite", k + 1, None
        return "cg_max_it", tol["max_it"], ITS


def _start(s, reason, conv):
    return E(0, reason, "%s_start_reason %s" % (s, conv))


def _all_start(reason, conv, gmres_exit=None):
    return {"cg": _start("cg", reason, conv), "gmres": E(0, reason, gmres_exit) if gmres_exit else _start("gmres", reason, conv), "bcgs": _start("bcgs", reason, conv)}


SV_ZERO0 = E(0, BREAKDOWN, "bcgs_sv_zero", ERR_PLIB)        # the oracle's stand-in for PETSC_ERR_PLIB "Divide by zero"
CG_INDEF1 = E(1, INDEF_MAT, "cg_indefinite_mat")

case("zero_rhs", SPD2, [0, 0], _all_start(ATOL, "conv_atol", "gmres_res_zero"))
case("twoI", dense([[2, 0, 0], [0, 2, 0], [0, 0, 2]]), [1, 2, 3],
     {"cg": E(1, ATOL, "cg_test_reason conv_atol"), "gmres": E(1, ATOL, "gmres_test_reason conv_atol"), "bcgs": E(1, RTOL, "bcgs_tt_zero_s_zero")})
# GMRES on `singular` spans the whole space after two steps; what is left of the third vector is rounding, and the oracle in its own
# summation order walks on it to max_it (the row of the issue).  In another order the remainder can be an exact zero (BREAKDOWN at 2).
case("singular", dense([[1, 0], [0, 0]]), [1, 1],
     {"cg": E(2, INDEF_MAT, "cg_indefinite_mat"), "gmres": E(10, ITS, "gmres_max_it"), "bcgs": E(1, BREAKDOWN, "bcgs_sv_zero", ERR_PLIB)})
case("nilpotent", dense([[0, 1], [0, 0]]), [0, 1], {"cg": CG_INDEF1, "gmres": E(2, BREAKDOWN, "gmres_null gmres_breakdown"), "bcgs": SV_ZERO0}, cg_anyway=True)
case("skew", dense([[0, 1], [-1, 0]]), [1, 0], {"cg": CG_INDEF1, "gmres": E(2, ATOL, "gmres_test_reason conv_atol"), "bcgs": SV_ZERO0}, cg_anyway=True)
case("indefinite", dense([[1, 0], [0, -1]]), [1, 1],
     {"cg": {"none": CG_INDEF1, "jacobi": E(1, ATOL, "cg_beta_zero")},
      "gmres": {"none": E(2, RTOL, "gmres_test_reason conv_rtol"), "jacobi": E(1, RTOL, "gmres_test_reason conv_rtol")},
      "bcgs": {"none": SV_ZERO0, "jacobi": E(1, RTOL, "bcgs_tt_zero_s_zero")}})
case("nan_b", SPD2, [NAN, 1], _all_start(DNAN, "conv_nan"))
case("inf_b", SPD2, [INF, 1], _all_start(DNAN, "conv_nan"))
case("exact_guess", SPD2, [4, 5], _all_start(ATOL, "conv_atol", "gmres_res_zero"), x0=[1, 2])
# the tt == 0.0 line of update_hessenberg sets DIVERGED_NULL, and the triangular solve that follows finds H(it,it) == 0 (both
# entries of the column are zero, or tt would not be) and overwrites it with DIVERGED_BREAKDOWN: in the reference as here, NULL is
# never the reason a solve returns.
case("zero_matrix", dense([[0, 0], [0, 0]]), [1, 2], {"cg": CG_INDEF1, "gmres": E(1, BREAKDOWN, "gmres_null gmres_breakdown"), "bcgs": SV_ZERO0})
case("nan_x0", SPD2, [1, 1], _all_start(DNAN, "conv_nan"), x0=[NAN, 0])
# A stored Inf does not wait for the Krylov space to reach it: 0 * Inf is NaN in the FIRST product.  inf_in_A keeps the literal
# entry (NaN mid-solve at iteration 1; p'w = NaN for CG).  The late arrivals are entries of 2^1023, which are harmless against a
# zero and overflow once the vectors have grown to column 6: symmetric, b = e0: CG's p'w stays finite (p_6 = 0) and the norm
# overflows first; a(5,6) alone with b = 2^40 e0: p_5 w_5 overflows, p'w = Inf first.
_FP = dict(cg_anyway=True)
case("inf_in_A", _inf_tridiag(True), [1, 0, 0, 0, 0, 0, 0, 0],
     {"cg": E(1, DNAN, "cg_dot_not_finite", ERR_FP), "gmres": E(1, DNAN, "gmres_test_reason conv_nan"), "bcgs": E(1, DNAN, "bcgs_test_reason conv_nan")},
     tol=dict(max_it=20), **_FP)
_OVF = dict(max_it=20, rtol=1e-30, dtol=1e300)
case("overflow_norm", _inf_tridiag(True, 2.0 ** 1023), [1, 0, 0, 0, 0, 0, 0, 0],
     {"cg": E(6, DNAN, "cg_test_reason conv_nan"), "gmres": E(6, DNAN, "gmres_test_reason conv_nan"), "bcgs": E(4, DNAN, "bcgs_test_reason conv_nan")}, tol=_OVF, **_FP)
case("overflow_pw", _inf_tridiag(False, 2.0 ** 1023), [2.0 ** 40, 0, 0, 0, 0, 0, 0, 0],
     {"cg": E(20, ITS, "cg_dot_not_finite", ERR_FP), "gmres": E(7, BREAKDOWN, "gmres_breakdown"), "bcgs": E(4, DNAN, "bcgs_test_reason conv_nan")}, tol=_OVF, **_FP)
# KSPDefaultConverged tests rnorm >= dtol * rnorm0 at iteration 0 as well, so a dtol below 1 ends every solve there; 1.5 it is.
# BiCGStab's second half-step minimises the residual, and on SPD tridiagonals no right-hand side in {-2..2}^n made it grow by
# 1.5 in one iteration: dtol is the SPD system (CG), dtol_both a symmetric indefinite one found by search (CG and BiCGStab).
case("dtol", tridiag(8), [1] * 8,
     {"cg": E(1, DTOL, "cg_test_reason conv_dtol"), "gmres": E(4, RTOL, "gmres_test_reason conv_rtol"), "bcgs": E(4, RTOL, "bcgs_test_reason conv_rtol")}, tol=dict(dtol=1.5))
case("dtol_both", dense([[2, -1, -1], [-1, -2, 2], [-1, 2, -1]]), [0, -1, -2],
     {"cg": E(1, DTOL, "cg_test_reason conv_dtol"), "gmres": E(3, RTOL, "gmres_test_reason conv_rtol"), "bcgs": E(1, DTOL, "bcgs_test_reason conv_dtol")}, tol=dict(dtol=1.5))
case("indefinite_pc", dense([[2, 1], [1, -2]]), [1, 0],
     {"cg": {"none": E(2, INDEF_MAT, "cg_indefinite_mat"), "jacobi": E(2, INDEF_PC, "cg_indefinite_pc")},
      "gmres": E(2, ATOL, "gmres_test_reason conv_atol"), "bcgs": E(2, RTOL, "bcgs_tt_zero_s_zero")})
# the happy bound is relative to the residual norm (tt < |tt / rnorm|, capped at 1e-30): the right-hand side is small enough that the
# replicated norm (64 times the tiny one) stays below 1 as well
case("happy", dense([[1, 0], [2.0 ** -110, 1]]), [2.0 ** -20, 0], {"gmres": E(1, ATOL, "gmres_happy conv_atol"), "bcgs": E(1, ATOL, "bcgs_test_reason conv_atol")})
case("s_in_null", dense([[-2, -2], [0, 0]]), [1, 1], {"bcgs": E(0, BREAKDOWN, "bcgs_tt_zero_s_nonzero")})      # alpha = -1/2, s = (-1, 1), A s = 0
case("rho_zero", dense([[2, 2, 2], [0, 2, -1], [0, 0, 2]]), [-1, 0, 1], {"gmres": E(3, RTOL, "gmres_test_reason conv_rtol"), "bcgs": E(2, BREAKDOWN, "bcgs_rho_zero")})
BENIGN = dict(rows=dense([[4, 1, 0], [1, 4, 1], [0, 1, 4]]), b=[1, 2, 3])     # also the second solve on a KSP that has left early
case("benign", BENIGN["rows"], BENIGN["b"],
     {"cg": E(3, RTOL, "cg_test_reason conv_rtol"), "gmres": E(3, RTOL, "gmres_test_reason conv_rtol"), "bcgs": E(3, RTOL, "bcgs_test_reason conv_rtol")})
case("maxit3", tridiag(8), [1, 0, 0, 0, 0, 0, 0, 0],
     {"cg": E(3, ITS, "cg_max_it"), "gmres": E(3, ITS, "gmres_max_it gmres_max_it_in_cycle"), "bcgs": E(3, ITS, "bcgs_max_it")}, tol=dict(max_it=3, rtol=1e-12))


def _maxit_cases():
    A = maxit_matrix()
    b = [1, -2, 3, -4, 5, -6, 7, -8, 9, -10, 11, -12]
    for r in (1, 2, 5):
        for m in sorted({r - 1, r, r + 1, 2 * r, 2 * r + 1, 1}):
            ex = "gmres_max_it" + (" gmres_cycle_full" if m > r else "") + (" gmres_max_it_in_cycle" if m % r else "")
            case("maxit_r%d_m%d" % (r, m), A, b, {"gmres": E(m, ITS, ex)}, tol=dict(rtol=0.0, max_it=m), restart=r, pcs=("jacobi",))
    case("maxit_r2_m3_right", A, b, {"gmres": E(3, ITS, "gmres_max_it gmres_cycle_full gmres_max_it_in_cycle")}, tol=dict(rtol=0.0, max_it=3), restart=2,
         pc_right=True, pcs=("jacobi",))


_maxit_cases()
BY_NAME = {c.name: c for c in CASES}
