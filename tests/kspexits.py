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

The eight types registered since (TFQMR, CGS, BiCG, MINRES, pipelined CG, Chebychev, Richardson, LSQR: MORE_SOLVERS) have their
rows in MORE, merged into the cases at the end of the module; their (its, reason) come from the host models (model()), the line
from the restatements tfqmr_exit / cgs_exit / bicg_exit / minres_exit.  The exit lines were read off harness/krylov.c and
host/kspfused.c, which have the same set for the preconditioners used here (none, Jacobi); one difference outside it: the harness's
KSPSolve_Richardson hands the whole iteration to PCApplyRichardson (PCSOR, rich.c:47-56), richardsonhipmi355x has no such route.
LATE_ZERO_SEARCH: over the search space of RHO_ZERO_SEARCH -- all 15625 systems of 2 rows with entries and right-hand sides in
{-2..2}, 2000 random draws of 3 rows and 2000 of 4 rows (numpy default_rng(1)) -- the restatements leave through
  tfqmr_s_zero_late        2352 / 200 / 49 times (2, 3, 4 rows),
  cgs_s_zero_late          2192 / 158 / 33,
  bicg_dpi_zero_late       2432 / 190 / 40,
  tfqmr_test_reason_half1  10528 / 1480 / 1622 (every exact convergence: dp = 0 makes the FIRST half step's estimate zero),
and bicg_beta_zero needs no search (`indefinite` under Jacobi: zr'rl = 1 - 1).  LEFT_OUT stays empty.
Not in the table: `rho_zero` for TFQMR / CGS / BiCG (rho == 0 makes the next rhoold zero; the models divide Python floats there and
raise where C gives Inf), and the LSQR rows whose reason hangs on the rounding of a square root (singular, s_in_null, a tall
inconsistent system): KSPLSQR's *_NORMAL reasons are claimed where Inf or an exact zero decides them (overflow_pw, ls_alpha_zero).
"""
import collections

import numpy as np

import orc

NAN, INF = float("nan"), float("inf")
RTOL, ATOL, ITS_OK = 2, 3, 4
NULL, ITS, DTOL, BREAKDOWN, INDEF_PC, DNAN, INDEF_MAT = -2, -3, -4, -5, -8, -9, -10
ERR_FP, ERR_PLIB = 72, 77             # PETSC_ERR_FP, PETSC_ERR_PLIB (include/petscmini.h)
HAPPY, ATOL_NORMAL, RTOL_NORMAL = 8, 9, 1             # KSP_CONVERGED_HAPPY_BREAKDOWN, _ATOL_NORMAL, _RTOL_NORMAL (KSPLSQR)
ERR_SUP, ERR_ARG_SIZ, ERR_ARG_INCOMP = 56, 60, 75     # PETSC_ERR_SUP, PETSC_ERR_ARG_SIZ, PETSC_ERR_ARG_INCOMP
SOLVERS = ("cg", "gmres", "bcgs")
# the eight types registered since; a label is "kind" or "kind:variant" -- the variant a norm type (-ksp_norm_type) where the kind
# accepts several and the exits differ, or "normal" for KSPLSQR under KSPLSQRDefaultConverged ("lsqr:none": KSPSkipConverged).  No variant: the preconditioned
# norm (KSPLSQR: the unpreconditioned one, its only one).
MORE_SOLVERS = ("tfqmr", "cgs", "bicg", "bicg:unpreconditioned", "minres", "pipecg", "pipecg:unpreconditioned", "pipecg:natural", "pipecg:none",
                "chebychev", "chebychev:unpreconditioned", "chebychev:none", "richardson", "richardson:unpreconditioned", "richardson:none",
                "lsqr", "lsqr:normal", "lsqr:none")
SYMMETRIC_ONLY = ("cg", "minres", "pipecg")
# (case, solver) whose way past the named exit is decided by rounding, with every outcome an exact run could take: GMRES on
# `singular` has spanned the space after two steps; what is left of the third vector is rounding (the oracle's own order: walks on
# to max_it, the row of the issue) or an exact zero (replicated: the happy branch on a singular H, BREAKDOWN at 2)
ROUNDING = {("singular", "gmres"): ((10, -3), (2, -5)),
            # pipelined CG, natural norm, on overflow_pw: whether res'u overflows in iteration 7 or 8 hangs on the last bits of a sum near 2^1024
            ("overflow_pw", "pipecg:natural"): ((8, -9), (7, -9))}
LEFT_OUT = {}                        # exit -> why no case reaches it; only the searched-for exits may stand here (test_ksp_exits_cpu.py).  Every search found one: empty.


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
    # KSPSolve_TFQMR (tfqmr.c) and KSPSolve_CGS (cgs.c)
    "tfqmr_start_reason",
    "tfqmr_s_zero_first",     # s = v'rp == 0 in iteration 0: DIVERGED_BREAKDOWN where the reference divides
    "tfqmr_s_zero_late",      # ... in an iteration >= 1
    "tfqmr_test_reason_half1",  # the test after the first half step has a reason: the update sweep runs ONE half step, its stays
    "tfqmr_test_reason_half2",  # ... after the second
    "tfqmr_max_it",
    "cgs_start_reason", "cgs_s_zero_first", "cgs_s_zero_late",
    "cgs_test_reason",        # x += a t was made BEFORE the test, the u, q, p update is not
    "cgs_max_it",
    # KSPSolve_BiCG (bicg.c)
    "bicg_start_reason",
    "bicg_beta_zero",         # zr'rl == 0 in iteration 0: the return inside the loop
    "bicg_dpi_zero_first",    # zr'pl == 0 in iteration 0
    "bicg_dpi_zero_late",
    "bicg_test_reason", "bicg_max_it",
    # KSPSolve_MINRES (minres.c)
    "minres_start_reason",
    "minres_indefinite_mat",  # r'z < 1e-18 before the loop (no history entry)
    "minres_indefinite_pc",   # ... inside it, before x is updated: also the lucky breakdown
    "minres_test_reason", "minres_max_it",
    # KSPSolve_PIPECG (pipecg.c): no breakdown test of its own; a zero gamma or delta ends in conv_nan
    "pipecg_start_reason",
    "pipecg_dot_not_finite",  # natural norm: res'u NaN or Inf at the start: PETSC_ERR_FP (the model goes on to DIVERGED_NAN at 0)
    "pipecg_test_reason", "pipecg_max_it",
    # KSPSolve_Chebychev (cheby.c), KSPSolve_Richardson (rich.c)
    "chebychev_start_reason", "chebychev_test_reason",
    "chebychev_converged_its",  # KSP_NORM_NONE: the budget spent is CONVERGED_ITS
    "chebychev_max_it",
    "richardson_start_reason", "richardson_test_reason", "richardson_converged_its",
    "richardson_final_reason",  # the test after the loop, on the norm of the last iterate, has a reason
    "richardson_max_it",
    # KSPSolve_LSQR (lsqr.c as DESIGN.md section 4 states it), KSPLSQRDefaultConverged
    "lsqr_start_reason",
    "lsqr_atol_normal_start", # A'r0 == 0
    "lsqr_happy_beta",        # beta == 0 in the loop and a test that leaves the reason unset: CONVERGED_HAPPY_BREAKDOWN
    "lsqr_happy_alpha",       # alpha == 0 in the loop
    "lsqr_test_reason", "lsqr_conv_atol_normal", "lsqr_conv_rtol_normal",
    "lsqr_max_it",
)

Expect = collections.namedtuple("Expect", "its reason exits error")
# ncols: the columns of a rectangular operator (KSPLSQR only); eig: {pc: (emin, emax)} for Chebychev; scale: {pc: s} for Richardson
Case = collections.namedtuple("Case", "name rows b x0 tol restart pc_right pcs expect cg_anyway ncols eig scale", defaults=(None, None, None))


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


def case(name, rows, b, expect, x0=None, tol=None, restart=30, pc_right=False, pcs=("none", "jacobi"), cg_anyway=False, ncols=None, eig=None, scale=None):
    t = dict(DEFAULT_TOL)
    t.update(tol or {})
    CASES.append(Case(name, rows, np.array(b, dtype=np.float64), None if x0 is None else np.array(x0, dtype=np.float64), t, restart, pc_right,
                      tuple(pcs), expect, cg_anyway, ncols, eig, scale))


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
    if c.ncols is not None:                                # KSPLSQR preconditions the normal equations: the diagonal of A'A
        dg = normal_diagonal(ai, aj, aa, c.ncols)
        return bool(np.all(np.isfinite(dg) & (dg != 0.0)))
    dg = orc.get_diagonal(ai, aj, aa)
    return bool(np.all(dg != 0.0))


def kind_of(label):
    return label.split(":")[0]


def variant_of(label):
    return label.split(":")[1] if ":" in label else None


def solvers_of(c):
    """CG (MINRES, pipelined CG) is left out where the matrix is not symmetric and the case is not about that; the table decides the
    rest: a solver has a row where the case applies to it"""
    return [s for s in SOLVERS + MORE_SOLVERS if s in c.expect and (kind_of(s) not in SYMMETRIC_ONLY or c.cg_anyway or is_symmetric(c))]


def pcs_of(c, solver=None):
    """Jacobi where no diagonal entry is zero; for KSPLSQR on a square case the diagonal is that of A'A (finite and non-zero)"""
    if solver is not None and kind_of(solver) == "lsqr" and c.ncols is None:
        ai, aj, aa = matrix_of(c)
        dg = normal_diagonal(ai, aj, aa, ai.size - 1)
        return [p for p in c.pcs if p == "none" or bool(np.all(np.isfinite(dg) & (dg != 0.0)))]
    return [p for p in c.pcs if p == "none" or jacobi_applies(c)]


def normal_diagonal(ai, aj, aa, ncols):
    """the diagonal of A'A, column by column in row order (small integers and powers of two: exact in any order)"""
    dg = np.zeros(ncols)
    with np.errstate(all="ignore"):
        for q in range(int(ai[-1])):
            dg[aj[q]] += aa[q] * aa[q]
    return dg


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
    Aj = (aj[None, :] + (n if c.ncols is None else c.ncols) * np.arange(k)[:, None]).ravel().astype(np.int32)     # rows and columns replicated separately
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


def ncols_of(c, size="tiny"):
    ai = matrix_of(c)[0]
    n = ai.size - 1
    return (n if c.ncols is None else c.ncols) * (1 if size == "tiny" else copies_for(n))


def model(c, solver, pc, size="tiny", device_order=False):
    """(x, history, its, reason) of the reference model of one of MORE_SOLVERS (tests/*_ref.py: the reference's loops in its order,
    every Vec call through the oracle).  The models never raise; what stands in for an error is stated at the rows that name one."""
    import bicg_ref, cheby_ref, lsqr_ref, minres_ref, pipecg_ref, tfqmr_ref
    kind, variant = kind_of(solver), variant_of(solver)
    ai, aj, aa, b, x0 = system(c, size)
    d = None
    if pc == "jacobi":
        if kind == "lsqr":
            dg = normal_diagonal(ai, aj, aa, ncols_of(c, size))
            d = np.where(dg == 0.0, 1.0, 1.0 / np.where(dg == 0.0, 1.0, dg))
        else:
            d = cheby_ref.jacobi(ai, aj, aa)
    norm = variant or "preconditioned"

    def run():
        if kind == "tfqmr":
            return tfqmr_ref.tfqmr(ai, aj, aa, b, pc=d, x0=x0, **c.tol)
        if kind == "cgs":
            return tfqmr_ref.cgs(ai, aj, aa, b, pc=d, x0=x0, **c.tol)
        if kind == "bicg":
            return bicg_ref.bicg(ai, aj, aa, b, x0=x0, pc=d, norm=norm, **c.tol)
        if kind == "minres":
            return minres_ref.minres(ai, aj, aa, b, pc=d, x0=x0, **c.tol)
        if kind == "pipecg":
            assert x0 is None
            return pipecg_ref.pipecg(ai, aj, aa, b, pc=d, norm=norm, **c.tol)
        if kind == "chebychev":
            emin, emax = c.eig[pc]
            return cheby_ref.chebychev(ai, aj, aa, b, emin, emax, pc=d, norm=norm, x0=x0, **c.tol)[:4]
        if kind == "richardson":
            return cheby_ref.richardson(ai, aj, aa, b, scale=c.scale[pc], pc=d, norm=norm, x0=x0, **c.tol)[:4]
        assert kind == "lsqr"
        return tuple(lsqr_ref.lsqr(ai, aj, aa, ncols_of(c, size), b, pc=d, x0=x0, normal_tests=variant == "normal", skip_test=variant == "none", **c.tol))
    with np.errstate(all="ignore"):
        if device_order:
            with orc.device_reduction_order():
                return run()
        return run()


def _dense_operator(ai, aj, aa, jacobi):
    n = ai.size - 1
    A = np.zeros((n, n))
    for i in range(n):
        for q in range(ai[i], ai[i + 1]):
            A[i, aj[q]] = aa[q]
    d = np.ones(n)
    if jacobi:
        dg = np.diag(A).copy()
        d = np.where(dg == 0.0, 1.0, 1.0 / np.where(dg == 0.0, 1.0, dg))
    mult = lambda M, v: np.array([sum(M[i, j] * v[j] for j in range(n)) for i in range(n)])
    return A, d, mult


def _default_test(tol, rn0):
    ttol = max(tol["rtol"] * rn0, tol["abstol"])

    def test(rn):
        if not np.isfinite(rn):
            return DNAN
        if rn <= ttol:
            return ATOL if rn < tol["abstol"] else RTOL
        if rn >= tol["dtol"] * rn0:
            return DTOL
        return 0
    return test


def _dot(x, y):
    return np.float64(np.sum(x * y))


def _nrm(x):
    return np.float64(np.sqrt(np.sum(x * x)))


def _cgs_family_exit(cgs, ai, aj, aa, b, tol, jacobi):
    s_ = "cgs" if cgs else "tfqmr"
    A, d, mult = _dense_operator(ai, aj, aa, jacobi)
    K = lambda v: d * mult(A, v)
    n = A.shape[0]
    with np.errstate(all="ignore"):
        r = d * np.array(b, dtype=np.float64)
        dp = _nrm(r)
        test = _default_test(tol, dp)
        why = test(dp)
        if why:
            return s_ + "_start_reason", 0, why
        rp = r.copy()
        rhoold = _dot(r, rp)
        u, p = r.copy(), r.copy()
        v = K(p)
        D, x, q = np.zeros(n), np.zeros(n), np.zeros(n)
        tau = dpold = dp
        etaold = psiold = np.float64(0.0)
        for i in range(tol["max_it"]):
            s = _dot(v, rp)
            if s == 0.0:
                return s_ + ("_s_zero_late" if i else "_s_zero_first"), i, BREAKDOWN
            a = rhoold / s
            q = u - a * v
            t = u + q
            if cgs:
                x = x + a * t
            r = r - a * K(t)
            dp = _nrm(r)
            if cgs:
                rho = _dot(r, rp)
                why = test(dp)
                if why:
                    return "cgs_test_reason", i + 1, why
            else:
                for m in range(2):
                    w = dp if m else np.sqrt(dp * dpold)
                    psi = w / tau
                    cm = 1.0 / np.sqrt(1.0 + psi * psi)
                    tau = tau * psi * cm
                    eta = cm * cm * a
                    D = (q if m else u) + (psiold * psiold * etaold / a) * D
                    x = x + eta * D
                    why = test(np.sqrt(m + 1.0) * tau)
                    if why:
                        return "tfqmr_test_reason_half%d" % (m + 1), i, why      # its counts the iterations completed
                    etaold, psiold = eta, psi
                rho = _dot(r, rp)
            bb = rho / rhoold
            u = r + bb * q
            q = q + bb * p
            p = u + bb * q
            v = K(p)
            rhoold, dpold = rho, dp
        return s_ + "_max_it", tol["max_it"], ITS


def tfqmr_exit(ai, aj, aa, b, tol, jacobi=False):
    """numpy restatement of KSPSolve_TFQMR from a zero guess (left PC none / Jacobi) that names the line it leaves through:
    (exit, its, reason).  Independent of tests/tfqmr_ref.py; also the search function for the late s == 0 and for the first half step."""
    return _cgs_family_exit(False, ai, aj, aa, b, tol, jacobi)


def cgs_exit(ai, aj, aa, b, tol, jacobi=False):
    """the same for KSPSolve_CGS"""
    return _cgs_family_exit(True, ai, aj, aa, b, tol, jacobi)


def bicg_exit(ai, aj, aa, b, tol, jacobi=False):
    """the same for KSPSolve_BiCG (preconditioned norm); independent of tests/bicg_ref.py"""
    A, d, mult = _dense_operator(ai, aj, aa, jacobi)
    At = A.T.copy()
    with np.errstate(all="ignore"):
        rr = np.array(b, dtype=np.float64)
        rl = rr.copy()
        zr, zl = d * rr, d * rl
        dp = _nrm(zr)
        test = _default_test(tol, dp)
        why = test(dp)
        if why:
            return "bicg_start_reason", 0, why
        pr = pl = None
        betaold = np.float64(1.0)
        for i in range(tol["max_it"]):
            beta = _dot(zr, rl)
            if i == 0:
                if beta == 0.0:
                    return "bicg_beta_zero", 0, BREAKDOWN
                pr, pl = zr.copy(), zl.copy()
            else:
                pr, pl = zr + (beta / betaold) * pr, zl + (beta / betaold) * pl
            betaold = beta
            zr, zl = mult(A, pr), mult(At, pl)
            dpi = _dot(zr, pl)
            if dpi == 0.0:
                return "bicg_dpi_zero_late" if i else "bicg_dpi_zero_first", i, BREAKDOWN
            a = beta / dpi
            rr, rl = rr - a * zr, rl - a * zl
            zr, zl = d * rr, d * rl
            why = test(_nrm(zr))
            if why:
                return "bicg_test_reason", i + 1, why
        return "bicg_max_it", tol["max_it"], ITS


def minres_exit(ai, aj, aa, b, tol, jacobi=False):
    """the same for KSPSolve_MINRES; independent of tests/minres_ref.py"""
    A, d, mult = _dense_operator(ai, aj, aa, jacobi)
    n = A.shape[0]
    with np.errstate(all="ignore"):
        r = np.array(b, dtype=np.float64)
        z = d * r
        nrm = _nrm(z)
        dp = _dot(r, z)
        if dp < 1e-18:
            return "minres_indefinite_mat", 0, INDEF_MAT
        beta = np.sqrt(np.abs(dp))
        v, u = r / beta, z / beta
        vold, uold = np.zeros(n), np.zeros(n)
        test = _default_test(tol, nrm)
        why = test(nrm)
        if why:
            return "minres_start_reason", 0, why
        c = cold = np.float64(1.0)
        s = sold = np.float64(0.0)
        rnorm = nrm
        for i in range(tol["max_it"]):
            r = mult(A, u)
            alpha = _dot(u, r)
            z = d * r
            r = r - alpha * v - beta * vold
            z = z - alpha * u - beta * uold
            betaold = beta
            dp = _dot(r, z)
            if dp < 1e-18:
                return "minres_indefinite_pc", i + 1, INDEF_PC
            beta = np.sqrt(np.abs(dp))
            coold, cold, sold = cold, c, s
            rho0 = cold * alpha - coold * sold * betaold
            rho1 = np.sqrt(rho0 * rho0 + beta * beta)
            c, s = rho0 / rho1, beta / rho1
            vold, uold, v, u = v, u, r / beta, z / beta
            rnorm = rnorm * np.abs(s)
            why = test(rnorm)
            if why:
                return "minres_test_reason", i + 1, why
        return "minres_max_it", tol["max_it"], ITS


EXIT_OF = {"cg": cg_exit, "bcgs": bcgs_exit, "tfqmr": tfqmr_exit, "cgs": cgs_exit, "bicg": bicg_exit, "minres": minres_exit}


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

# ------------------------------------------------------------------------------------------------ the eight types registered since
# Cases of their own.  LATE_ZERO_SEARCH: the restatements tfqmr_exit / cgs_exit / bicg_exit were run over the search space of
# RHO_ZERO_SEARCH (module docstring: the counts); late_zero is the first draw of 3 rows that leaves all three through the late
# zero at iteration 1, half1_late the first whose TFQMR residual vanishes exactly in iteration 2 (the estimate of the FIRST half
# step is then zero: sqrt(dp dpold) with dp = 0).
_SPD2_SET = dict(eig={"none": (1, 3), "jacobi": (0.5, 1.5)}, scale={"none": 0.5, "jacobi": 1.0})          # the spectrum of SPD2 is {1, 3}, of B A {1/2, 3/2}
_TRI8_SET = dict(eig={"none": (0.125, 4), "jacobi": (0.0625, 2)}, scale={"none": 0.5, "jacobi": 1.0})    # tridiag(8) lies inside (0, 4), B A inside (0, 2)
SETTINGS = {"zero_rhs": _SPD2_SET, "nan_b": _SPD2_SET, "inf_b": _SPD2_SET, "exact_guess": _SPD2_SET, "nan_x0": _SPD2_SET,
            "twoI": dict(eig={"none": (1, 4), "jacobi": (0.5, 2)}, scale={"none": 0.25, "jacobi": 0.5}),          # the spectrum is {2}; neither setting is exact in one step
            "benign": dict(eig={"none": (2, 6), "jacobi": (0.5, 1.5)}, scale={"none": 0.25, "jacobi": 0.75}),     # 4 + 2 cos: inside (2, 6)
            "inf_in_A": _TRI8_SET, "overflow_norm": _TRI8_SET, "overflow_pw": _TRI8_SET, "dtol": _TRI8_SET, "maxit3": _TRI8_SET}
case("late_zero", dense([[-1, 0, 0], [2, 1, 1], [0, -1, -1]]), [0, 0, -1], {}, pcs=("none",))
case("half1_late", dense([[2, -1, 0], [-1, -2, 1], [-2, -1, 0]]), [0, -2, 2], {}, pcs=("none",))
# bounds and a scale that miss the spectrum {1, 3} (B A: {1/2, 3/2}): Richardson's residual along (1, 1) doubles per step
case("diverging", SPD2, [1, 1], {}, tol=dict(dtol=1.5), eig={"none": (0.25, 0.75), "jacobi": (0.125, 0.375)}, scale={"none": 1.0, "jacobi": 2.0})
# the budget of ONE iteration is spent and the iterate is exact: the test after the loop has the reason (cheby.c, rich.c)
case("final_exact", dense([[2, 0, 0], [0, 2, 0], [0, 0, 2]]), [1, 2, 3], {}, tol=dict(max_it=1), eig={"none": (1, 3), "jacobi": (0.5, 1.5)}, scale={"none": 0.5, "jacobi": 1.0})
# rectangular systems (KSPLSQR only); Jacobi is PCJACOBI on A'A
_TALL = dense([[1, 0], [0, 1], [1, 1]])
case("ls_tall", _TALL, [1, 2, 3], {}, ncols=2)                                   # consistent: x = (1, 2)
case("ls_tall_inconsistent", _TALL, [1, 1, 0], {}, ncols=2)                      # ||b - A x|| stays at 2 / sqrt(3): only A'r can end it
case("ls_wide", dense([[1, 0, 1], [0, 2, 0]]), [2, 2], {}, ncols=3)              # the minimum-norm solution (1, 1, 1)
case("ls_atb_zero", dense([[1, 0], [0, 2], [0, 0]]), [0, 0, 1], {}, ncols=2)     # A'b = 0: x = 0 is a least-squares solution already
case("ls_alpha_zero", dense([[2], [0]]), [2, 2], {}, ncols=1)                    # after one step x = 1 and what is left of b is outside the range of A
case("ls_beta_zero", dense([[1, 0, 0], [0, 2, 0], [0, 0, 4]]), [1, 0, 0], {})    # b is an eigenvector: u1 = A v - alpha u = 0
case("ls_maxit2", dense([[1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]]), [1, 0, 0, 2], {}, ncols=3, tol=dict(max_it=2, rtol=1e-12))

# (its, reason) from the reference models (model() above: tfqmr_ref.tfqmr / .cgs, bicg_ref.bicg, minres_ref.minres, pipecg_ref.pipecg,
# cheby_ref.chebychev / .richardson, lsqr_ref.lsqr), run on the host; the line from the *_exit restatements where there is one
MORE = {
    "zero_rhs": {
        "tfqmr": E(0, ATOL, "tfqmr_start_reason conv_atol"),
        "cgs": E(0, ATOL, "cgs_start_reason conv_atol"),
        "bicg": E(0, ATOL, "bicg_start_reason conv_atol"),
        "bicg:unpreconditioned": E(0, ATOL, "bicg_start_reason conv_atol"),
        "minres": E(0, INDEF_MAT, "minres_indefinite_mat"),
        "pipecg": E(0, ATOL, "pipecg_start_reason conv_atol"),
        "pipecg:unpreconditioned": E(0, ATOL, "pipecg_start_reason conv_atol"),
        "pipecg:natural": E(0, ATOL, "pipecg_start_reason conv_atol"),
        "chebychev": E(1, ATOL, "chebychev_start_reason conv_atol"),
        "chebychev:unpreconditioned": E(1, ATOL, "chebychev_start_reason conv_atol"),
        "richardson": E(0, ATOL, "richardson_start_reason conv_atol"),
        "richardson:unpreconditioned": E(0, ATOL, "richardson_start_reason conv_atol"),
        "lsqr": E(0, ATOL, "lsqr_start_reason conv_atol"),
        "lsqr:normal": E(0, ATOL, "lsqr_start_reason conv_atol")},
    "twoI": {
        "tfqmr": E(0, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(1, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(1, ATOL, "bicg_test_reason conv_atol"),
        "bicg:unpreconditioned": E(1, ATOL, "bicg_test_reason conv_atol"),
        "minres": E(1, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "pipecg:unpreconditioned": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "pipecg:natural": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "chebychev": E(10, ITS, "chebychev_max_it"),
        "chebychev:unpreconditioned": E(10, ITS, "chebychev_max_it"),
        "richardson": E(10, ITS, "richardson_max_it"),
        "richardson:unpreconditioned": E(10, ITS, "richardson_max_it"),
        "lsqr": E(1, ATOL, "lsqr_test_reason conv_atol")},
    "singular": {
        "tfqmr": E(1, BREAKDOWN, "tfqmr_s_zero_late"),
        "cgs": E(1, BREAKDOWN, "cgs_s_zero_late"),
        "bicg": E(1, BREAKDOWN, "bicg_dpi_zero_late"),
        "minres": E(2, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(2, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(2, DNAN, "pipecg_test_reason conv_nan")},
    "nilpotent": {
        "tfqmr": E(0, BREAKDOWN, "tfqmr_s_zero_first"),
        "cgs": E(0, BREAKDOWN, "cgs_s_zero_first"),
        "bicg": E(0, BREAKDOWN, "bicg_dpi_zero_first"),
        "minres": E(10, ITS, "minres_max_it"),
        "pipecg": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "lsqr": E(0, ATOL_NORMAL, "lsqr_atol_normal_start")},
    "skew": {
        "tfqmr": E(0, BREAKDOWN, "tfqmr_s_zero_first"),
        "cgs": E(0, BREAKDOWN, "cgs_s_zero_first"),
        "bicg": E(0, BREAKDOWN, "bicg_dpi_zero_first"),
        "minres": E(10, ITS, "minres_max_it"),
        "pipecg": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "lsqr": E(1, ATOL, "lsqr_test_reason conv_atol")},
    "indefinite": {
        "tfqmr": {"none": E(0, BREAKDOWN, "tfqmr_s_zero_first"), "jacobi": E(0, ATOL, "tfqmr_test_reason_half1 conv_atol")},
        "cgs": {"none": E(0, BREAKDOWN, "cgs_s_zero_first"), "jacobi": E(1, ATOL, "cgs_test_reason conv_atol")},
        "bicg": {"none": E(0, BREAKDOWN, "bicg_dpi_zero_first"), "jacobi": E(0, BREAKDOWN, "bicg_beta_zero")},
        "bicg:unpreconditioned": {"none": E(0, BREAKDOWN, "bicg_dpi_zero_first"), "jacobi": E(0, BREAKDOWN, "bicg_beta_zero")},
        "minres": {"none": E(2, INDEF_PC, "minres_indefinite_pc"), "jacobi": E(0, INDEF_MAT, "minres_indefinite_mat")},
        "pipecg": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": {"none": E(1, DNAN, "pipecg_test_reason conv_nan"), "jacobi": E(0, ATOL, "pipecg_start_reason conv_atol")}},
    "nan_b": {
        "tfqmr": E(0, DNAN, "tfqmr_start_reason conv_nan"),
        "cgs": E(0, DNAN, "cgs_start_reason conv_nan"),
        "bicg": E(0, DNAN, "bicg_start_reason conv_nan"),
        "bicg:unpreconditioned": E(0, DNAN, "bicg_start_reason conv_nan"),
        "minres": E(0, DNAN, "minres_start_reason conv_nan"),
        "pipecg": E(0, DNAN, "pipecg_start_reason conv_nan"),
        "pipecg:unpreconditioned": E(0, DNAN, "pipecg_start_reason conv_nan"),
        "pipecg:natural": E(0, DNAN, "pipecg_dot_not_finite", ERR_FP),
        "pipecg:none": E(10, ITS, "pipecg_max_it"),
        "chebychev": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "chebychev:unpreconditioned": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "chebychev:none": E(10, ITS_OK, "chebychev_converged_its"),
        "richardson": E(0, DNAN, "richardson_start_reason conv_nan"),
        "richardson:unpreconditioned": E(0, DNAN, "richardson_start_reason conv_nan"),
        "richardson:none": E(10, ITS_OK, "richardson_converged_its"),
        "lsqr": E(0, DNAN, "lsqr_start_reason conv_nan"),
        "lsqr:normal": E(0, DNAN, "lsqr_start_reason conv_nan")},
    "inf_b": {
        "tfqmr": E(0, DNAN, "tfqmr_start_reason conv_nan"),
        "cgs": E(0, DNAN, "cgs_start_reason conv_nan"),
        "bicg": E(0, DNAN, "bicg_start_reason conv_nan"),
        "minres": E(0, DNAN, "minres_start_reason conv_nan"),
        "pipecg": E(0, DNAN, "pipecg_start_reason conv_nan"),
        "pipecg:natural": E(0, DNAN, "pipecg_dot_not_finite", ERR_FP),
        "chebychev": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "richardson": E(0, DNAN, "richardson_start_reason conv_nan"),
        "lsqr": E(0, DNAN, "lsqr_start_reason conv_nan")},
    "exact_guess": {
        "tfqmr": E(0, ATOL, "tfqmr_start_reason conv_atol"),
        "cgs": E(0, ATOL, "cgs_start_reason conv_atol"),
        "bicg": E(0, ATOL, "bicg_start_reason conv_atol"),
        "minres": E(0, INDEF_MAT, "minres_indefinite_mat"),
        "chebychev": E(1, ATOL, "chebychev_start_reason conv_atol"),
        "richardson": E(0, ATOL, "richardson_start_reason conv_atol"),
        "lsqr": E(0, ATOL, "lsqr_start_reason conv_atol")},
    "zero_matrix": {
        "tfqmr": E(0, BREAKDOWN, "tfqmr_s_zero_first"),
        "cgs": E(0, BREAKDOWN, "cgs_s_zero_first"),
        "bicg": E(0, BREAKDOWN, "bicg_dpi_zero_first"),
        "minres": E(1, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:unpreconditioned": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "lsqr": E(0, ATOL_NORMAL, "lsqr_atol_normal_start")},
    "nan_x0": {
        "tfqmr": E(0, DNAN, "tfqmr_start_reason conv_nan"),
        "cgs": E(0, DNAN, "cgs_start_reason conv_nan"),
        "bicg": E(0, DNAN, "bicg_start_reason conv_nan"),
        "minres": E(0, DNAN, "minres_start_reason conv_nan"),
        "chebychev": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "richardson": E(0, DNAN, "richardson_start_reason conv_nan"),
        "lsqr": E(0, DNAN, "lsqr_start_reason conv_nan")},
    "inf_in_A": {
        "tfqmr": E(0, DNAN, "tfqmr_test_reason_half1 conv_nan"),
        "cgs": E(1, DNAN, "cgs_test_reason conv_nan"),
        "bicg": E(1, DNAN, "bicg_test_reason conv_nan"),
        "bicg:unpreconditioned": E(1, DNAN, "bicg_test_reason conv_nan"),
        "minres": E(1, DNAN, "minres_test_reason conv_nan"),
        "pipecg": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:unpreconditioned": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(1, DNAN, "pipecg_test_reason conv_nan"),
        "chebychev": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "chebychev:unpreconditioned": E(1, DNAN, "chebychev_start_reason conv_nan"),
        "richardson": E(1, DNAN, "richardson_test_reason conv_nan"),
        "richardson:unpreconditioned": E(1, DNAN, "richardson_test_reason conv_nan"),
        "lsqr": E(1, DNAN, "lsqr_test_reason conv_nan")},
    "overflow_norm": {
        "tfqmr": E(2, DNAN, "tfqmr_test_reason_half1 conv_nan"),
        "cgs": E(3, DNAN, "cgs_test_reason conv_nan"),
        "bicg": E(6, DNAN, "bicg_test_reason conv_nan"),
        "bicg:unpreconditioned": E(6, DNAN, "bicg_test_reason conv_nan"),
        "minres": E(6, DNAN, "minres_test_reason conv_nan"),
        "pipecg": E(6, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:unpreconditioned": E(6, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(6, DNAN, "pipecg_test_reason conv_nan"),
        "chebychev": E(6, DNAN, "chebychev_test_reason conv_nan"),
        "chebychev:unpreconditioned": E(6, DNAN, "chebychev_test_reason conv_nan"),
        "richardson": E(6, DNAN, "richardson_test_reason conv_nan"),
        "richardson:unpreconditioned": E(6, DNAN, "richardson_test_reason conv_nan"),
        "lsqr": E(3, DNAN, "lsqr_test_reason conv_nan")},
    "overflow_pw": {
        "tfqmr": E(3, DNAN, "tfqmr_test_reason_half1 conv_nan"),
        "cgs": E(4, DNAN, "cgs_test_reason conv_nan"),
        "bicg": E(7, DNAN, "bicg_test_reason conv_nan"),
        "minres": E(7, DNAN, "minres_test_reason conv_nan"),
        "pipecg": E(8, DNAN, "pipecg_test_reason conv_nan"),
        "pipecg:natural": E(8, DNAN, "pipecg_test_reason conv_nan"),
        "chebychev": E(7, DNAN, "chebychev_test_reason conv_nan"),
        "richardson": E(7, DNAN, "richardson_test_reason conv_nan"),
        "lsqr": E(4, DNAN, "lsqr_test_reason conv_nan"),
        "lsqr:normal": E(3, RTOL_NORMAL, "lsqr_test_reason lsqr_conv_rtol_normal")},
    "dtol": {
        "tfqmr": E(3, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(1, DTOL, "cgs_test_reason conv_dtol"),
        "bicg": E(1, DTOL, "bicg_test_reason conv_dtol"),
        "bicg:unpreconditioned": E(1, DTOL, "bicg_test_reason conv_dtol"),
        "minres": E(4, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(1, DTOL, "pipecg_test_reason conv_dtol"),
        "pipecg:unpreconditioned": E(1, DTOL, "pipecg_test_reason conv_dtol"),
        "pipecg:natural": E(1, DTOL, "pipecg_test_reason conv_dtol"),
        "chebychev": E(10, ITS, "chebychev_max_it"),
        "chebychev:unpreconditioned": E(10, ITS, "chebychev_max_it"),
        "richardson": E(10, ITS, "richardson_max_it"),
        "richardson:unpreconditioned": E(10, ITS, "richardson_max_it")},
    "dtol_both": {
        "tfqmr": {"none": E(2, RTOL, "tfqmr_test_reason_half1 conv_rtol"), "jacobi": E(2, RTOL, "tfqmr_test_reason_half2 conv_rtol")},
        "cgs": E(1, DTOL, "cgs_test_reason conv_dtol"),
        "bicg": E(1, DTOL, "bicg_test_reason conv_dtol"),
        "minres": {"none": E(3, INDEF_PC, "minres_indefinite_pc"), "jacobi": E(0, INDEF_MAT, "minres_indefinite_mat")},
        "pipecg": E(1, DTOL, "pipecg_test_reason conv_dtol"),
        "pipecg:natural": E(1, DTOL, "pipecg_test_reason conv_dtol")},
    "indefinite_pc": {
        "tfqmr": E(1, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(2, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(2, ATOL, "bicg_test_reason conv_atol"),
        "minres": {"none": E(2, INDEF_PC, "minres_indefinite_pc"), "jacobi": E(1, INDEF_PC, "minres_indefinite_pc")},
        "pipecg": E(10, ITS, "pipecg_max_it"),
        "pipecg:natural": E(2, ATOL, "pipecg_test_reason conv_atol"),
        "lsqr": E(1, ATOL, "lsqr_test_reason conv_atol")},
    "happy": {
        "tfqmr": E(0, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(1, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(1, RTOL, "bicg_test_reason conv_rtol")},
    "s_in_null": {
        "tfqmr": E(1, BREAKDOWN, "tfqmr_s_zero_late"),
        "cgs": E(1, BREAKDOWN, "cgs_s_zero_late"),
        "bicg": E(1, BREAKDOWN, "bicg_dpi_zero_late")},
    "benign": {
        "tfqmr": E(2, RTOL, "tfqmr_test_reason_half1 conv_rtol"),
        "cgs": E(3, RTOL, "cgs_test_reason conv_rtol"),
        "bicg": E(3, RTOL, "bicg_test_reason conv_rtol"),
        "bicg:unpreconditioned": E(3, RTOL, "bicg_test_reason conv_rtol"),
        "minres": E(3, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(10, ITS, "pipecg_max_it"),
        "pipecg:unpreconditioned": E(10, ITS, "pipecg_max_it"),
        "pipecg:natural": E(3, RTOL, "pipecg_test_reason conv_rtol"),
        "pipecg:none": E(10, ITS, "pipecg_max_it"),
        "chebychev": E(10, RTOL, "chebychev_test_reason conv_rtol"),
        "chebychev:unpreconditioned": E(10, RTOL, "chebychev_test_reason conv_rtol"),
        "chebychev:none": E(10, ITS_OK, "chebychev_converged_its"),
        "richardson": E(10, ITS, "richardson_max_it"),
        "richardson:unpreconditioned": E(10, ITS, "richardson_max_it"),
        "richardson:none": E(10, ITS_OK, "richardson_converged_its"),
        "lsqr": E(3, RTOL, "lsqr_test_reason conv_rtol"),
        "lsqr:normal": E(3, RTOL, "lsqr_test_reason conv_rtol")},
    "maxit3": {
        "tfqmr": E(3, ITS, "tfqmr_max_it"),
        "cgs": E(3, ITS, "cgs_max_it"),
        "bicg": E(3, ITS, "bicg_max_it"),
        "bicg:unpreconditioned": E(3, ITS, "bicg_max_it"),
        "minres": E(3, ITS, "minres_max_it"),
        "pipecg": E(3, ITS, "pipecg_max_it"),
        "pipecg:unpreconditioned": E(3, ITS, "pipecg_max_it"),
        "pipecg:natural": E(3, ITS, "pipecg_max_it"),
        "pipecg:none": E(3, ITS, "pipecg_max_it"),
        "chebychev": E(3, ITS, "chebychev_max_it"),
        "chebychev:unpreconditioned": E(3, ITS, "chebychev_max_it"),
        "chebychev:none": E(3, ITS_OK, "chebychev_converged_its"),
        "richardson": E(3, ITS, "richardson_max_it"),
        "richardson:unpreconditioned": E(3, ITS, "richardson_max_it"),
        "richardson:none": E(3, ITS_OK, "richardson_converged_its"),
        "lsqr": E(3, ITS, "lsqr_max_it"),
        "lsqr:normal": E(3, ITS, "lsqr_max_it")},
    "late_zero": {
        "tfqmr": E(1, BREAKDOWN, "tfqmr_s_zero_late"),
        "cgs": E(1, BREAKDOWN, "cgs_s_zero_late"),
        "bicg": E(1, BREAKDOWN, "bicg_dpi_zero_late"),
        "bicg:unpreconditioned": E(1, BREAKDOWN, "bicg_dpi_zero_late")},
    "half1_late": {
        "tfqmr": E(2, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(3, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(3, ATOL, "bicg_test_reason conv_atol")},
    "diverging": {
        "tfqmr": E(0, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(1, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(1, ATOL, "bicg_test_reason conv_atol"),
        "minres": E(1, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "pipecg:unpreconditioned": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "pipecg:natural": E(1, ATOL, "pipecg_test_reason conv_atol"),
        "chebychev": E(2, DTOL, "chebychev_test_reason conv_dtol"),
        "chebychev:unpreconditioned": E(2, DTOL, "chebychev_test_reason conv_dtol"),
        "richardson": E(1, DTOL, "richardson_test_reason conv_dtol"),
        "richardson:unpreconditioned": E(1, DTOL, "richardson_test_reason conv_dtol")},
    "final_exact": {
        "tfqmr": E(0, ATOL, "tfqmr_test_reason_half1 conv_atol"),
        "cgs": E(1, ATOL, "cgs_test_reason conv_atol"),
        "bicg": E(1, ATOL, "bicg_test_reason conv_atol"),
        "minres": E(1, INDEF_PC, "minres_indefinite_pc"),
        "pipecg": E(1, ITS, "pipecg_max_it"),
        "pipecg:unpreconditioned": E(1, ITS, "pipecg_max_it"),
        "pipecg:natural": E(1, ITS, "pipecg_max_it"),
        "pipecg:none": E(1, ITS, "pipecg_max_it"),
        "chebychev": E(1, ATOL, "chebychev_start_reason conv_atol"),
        "chebychev:unpreconditioned": E(1, ATOL, "chebychev_start_reason conv_atol"),
        "chebychev:none": E(1, ITS_OK, "chebychev_converged_its"),
        "richardson": E(1, ATOL, "richardson_final_reason conv_atol"),
        "richardson:unpreconditioned": E(1, ATOL, "richardson_final_reason conv_atol"),
        "richardson:none": E(1, ITS_OK, "richardson_converged_its")},
    "ls_tall": {
        "lsqr": E(2, RTOL, "lsqr_test_reason conv_rtol"),
        "lsqr:normal": E(2, RTOL, "lsqr_test_reason conv_rtol")},
    "ls_wide": {
        "lsqr": E(2, RTOL, "lsqr_test_reason conv_rtol"),
        "lsqr:normal": E(2, RTOL, "lsqr_test_reason conv_rtol")},
    "ls_atb_zero": {
        "lsqr": E(0, ATOL_NORMAL, "lsqr_atol_normal_start"),
        "lsqr:normal": E(0, ATOL_NORMAL, "lsqr_atol_normal_start")},
    "ls_alpha_zero": {
        "lsqr": E(1, HAPPY, "lsqr_happy_alpha"),
        "lsqr:normal": E(1, ATOL_NORMAL, "lsqr_test_reason lsqr_conv_atol_normal"),
        "lsqr:none": E(1, HAPPY, "lsqr_happy_alpha")},
    "ls_beta_zero": {
        "lsqr": E(1, ATOL, "lsqr_test_reason conv_atol"),
        "lsqr:normal": E(1, ATOL, "lsqr_test_reason conv_atol"),
        "lsqr:none": E(1, HAPPY, "lsqr_happy_beta")},
    "ls_maxit2": {
        "lsqr": E(2, ITS, "lsqr_max_it")},
}


def _merge():
    for i, c in enumerate(CASES):
        c.expect.update(MORE.get(c.name, {}))
        if c.name in SETTINGS:
            CASES[i] = c._replace(**SETTINGS[c.name])


_merge()
BY_NAME = {c.name: c for c in CASES}
