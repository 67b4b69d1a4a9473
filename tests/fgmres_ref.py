"""Host model of flexible GMRES for tests/test_fgmres_*: the call sequence of the harness driver (petsc-dev_amd/harness/krylov.c,
KSPSolve_FGMRES; the contract is the sequence DESIGN.md section 4 states, restated without the reference's fgmres.c at hand), every Vec /
Mat call through the oracle (tests/orc.py: matmult, vec_mdot, vec_maxpy, vec_norm, ... -- under orc.device_reduction_order() the sums
carry the device's bits).  Right preconditioning, the norm of the true residual (or none), classical Gram-Schmidt with the three
refinement types.  The preconditioner is None (PCNONE), an inverted diagonal (PCJACOBI) or any callable r -> z, which may answer
differently from call to call; PCKSP below is such a callable around an inner model solver.  Nothing here calls the code under test."""
import numpy as np

import orc

NONE, UNPRECONDITIONED = "none", "unpreconditioned"
NEVER, IFNEEDED, ALWAYS = "refine_never", "refine_ifneeded", "refine_always"
CONVERGED_RTOL, CONVERGED_ATOL, CONVERGED_ITS = 2, 3, 4
DIVERGED_NULL, DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_NAN = -2, -3, -4, -9


class HappyBreakdownWithoutConvergence(RuntimeError):
    """the PETSC_ERR_PLIB exit: the new basis vector vanished and the convergence test did not stop the solve"""


class Result:
    def __init__(self):
        self.x, self.hist, self.its, self.reason = None, [], 0, 0
        self.monitor = []            # (its, rn) of every monitor call
        self.modify = []             # (its, k, rn) of every modifypc call
        self.cycles = []             # steps of every cycle
        self.nv = []                 # basis vectors orthogonalised against, per step

    def __iter__(self):              # x, history, its, reason = fgmres(...)
        return iter((self.x, np.array(self.hist), self.its, self.reason))


def fgmres(ai, aj, aa, b, pc=None, x0=None, restart=30, refine=NEVER, norm=UNPRECONDITIONED, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4,
           haptol=1.0e-30, modify=None):
    b = np.ascontiguousarray(b, dtype=np.float64)
    n, m = b.size, restart
    R = Result()
    guess_zero = x0 is None
    x = np.zeros(n) if guess_zero else np.array(x0, dtype=np.float64)
    R.x = x
    state = dict(rn0=None, ttol=None)

    def mult(v):
        return orc.matmult(ai, aj, aa, np.ascontiguousarray(v))[0]

    def apply(r):                                        # KSP_PCApply; no null space is removed on the right
        if callable(pc):
            return np.ascontiguousarray(pc(r.copy()), dtype=np.float64)
        z = np.zeros(n)
        if pc is None:
            orc.vec_copy(r, z)
        else:
            orc.vec_pointwise_mult(z, r, np.ascontiguousarray(pc))
        return z

    def converged(it, rn):                               # KSPSkipConverged / KSPDefaultConverged (iterativ.c:536, 702-783)
        if norm == NONE:
            return CONVERGED_ITS if it >= max_it else 0
        if it == 0:
            if guess_zero:
                state["rn0"] = rn
            else:
                s = float(orc.vec_norm(b, 1))
                state["rn0"] = s if s else rn
            state["ttol"] = max(rtol * state["rn0"], abstol)
        if np.isnan(rn) or np.isinf(rn):
            return DIVERGED_NAN
        if rn <= state["ttol"]:
            return CONVERGED_ATOL if rn < abstol else CONVERGED_RTOL
        if rn >= dtol * state["rn0"]:
            return DIVERGED_DTOL
        return 0

    def residual():                                      # V[0] = A x; VecAYPX(V[0], -1, b)
        r = mult(x)
        orc.vec_aypx(r, -1.0, b)
        return r

    def orthogonalize(w, V, h, k):                       # borthog2.c:35-119
        again = refine == ALWAYS
        h[:k + 1] = 0.0
        for p in range(2):
            coef = orc.vec_mdot(w, V[:k + 1])
            coef = -coef
            orc.vec_maxpy(w, coef, V[:k + 1])
            for j in range(k + 1):
                h[j] -= coef[j]
            if p == 0 and refine == IFNEEDED:
                removed = 0.0
                for j in range(k + 1):
                    removed += coef[j] * coef[j]
                removed = float(np.sqrt(removed))
                if float(orc.vec_norm(w, 1)) < 1.0286 * removed:
                    again = True
            if not again:
                break

    def cycle(v0):
        V, Z = [v0], []
        H = np.zeros((m + 2, m + 1))                     # H[i, k]: row i of column k
        c, s, rhs, k, hapend = np.zeros(m + 2), np.zeros(m + 2), np.zeros(m + 2), 0, False
        with np.errstate(all="ignore"):
            rn = float(orc.vec_norm(V[0], 1))
            rhs[0] = rn
            R.hist.append(rn)
            R.reason = converged(R.its, rn)
            if R.reason:
                R.cycles.append(0)
                return
            orc.vec_scale(V[0], 1.0 / rn)
            while not R.reason and k < m and R.its < max_it:
                if k:
                    R.hist.append(rn)
                R.monitor.append((R.its, rn))
                R.modify.append((R.its, k, rn))
                if modify is not None:
                    modify(R.its, k, rn)
                Z.append(apply(V[k]))
                w = mult(Z[k])
                R.nv.append(k + 1)
                orthogonalize(w, V, H[:, k], k)
                V.append(w)
                tt = float(orc.vec_norm(w, 1))
                H[k + 1, k] = tt
                hapbnd = abs(tt / rhs[k])
                if hapbnd > haptol:
                    hapbnd = haptol
                if tt > hapbnd:
                    orc.vec_scale(w, 1.0 / tt)
                else:
                    hapend = True
                for j in range(k):                       # the earlier rotations, then the new one
                    upper = H[j, k]
                    H[j, k] = c[j] * upper + s[j] * H[j + 1, k]
                    H[j + 1, k] = c[j] * H[j + 1, k] - (s[j] * upper)
                if hapend:
                    rn = 0.0
                else:
                    ln = float(np.sqrt(H[k, k] * H[k, k] + H[k + 1, k] * H[k + 1, k]))
                    if ln == 0.0:
                        R.reason = DIVERGED_NULL
                        break
                    c[k] = H[k, k] / ln
                    s[k] = H[k + 1, k] / ln
                    rhs[k + 1] = -(s[k] * rhs[k])
                    rhs[k] = c[k] * rhs[k]
                    H[k, k] = c[k] * H[k, k] + s[k] * H[k + 1, k]
                    rn = abs(rhs[k + 1])
                k += 1
                R.its += 1
                R.reason = converged(R.its, rn)
                if hapend:
                    if not R.reason:
                        raise HappyBreakdownWithoutConvergence(rn)
                    break
            R.hist.append(rn)
            if R.reason or R.its >= max_it:
                R.monitor.append((R.its, rn))
            R.cycles.append(k)
            if k:                                        # x += Z y, R y = rhs over k columns; a zero last pivot: y[k-1] = 0
                y = np.zeros(k)
                y[k - 1] = rhs[k - 1] / H[k - 1, k - 1] if H[k - 1, k - 1] != 0.0 else 0.0
                for r in range(k - 2, -1, -1):
                    acc = rhs[r]
                    for j in range(r + 1, k):
                        acc = acc - H[r, j] * y[j]
                    y[r] = acc / H[r, r]
                upd = np.zeros(n)
                orc.vec_maxpy(upd, y, Z[:k])
                orc.vec_axpy(x, 1.0, upd)

    cycle(b.copy() if guess_zero else residual())
    while not R.reason:
        v0 = residual()
        if R.its >= max_it:
            break
        cycle(v0)
    if R.its >= max_it and not R.reason:
        R.reason = DIVERGED_ITS
    return R


def expected_step_counts(R, restart, fusible=True):
    """(fused, unfused) steps of fgmreshipmi355x for the run the model made: a step writes the next preconditioned direction in its own
    sweep when the preconditioner is fusible, at most 32 vectors are orthogonalised against and the cycle has a next direction to write"""
    fused = sum(1 for nv in R.nv if fusible and nv <= 32 and nv < restart)
    return fused, len(R.nv) - fused


class PCKSP:
    """the model of PCKSP: every application is the inner model solver from a zero guess, with its own tolerances; solve(r) -> (x, its).
    The inner iteration counts accumulate (PCKSPGetTotalIterations)."""

    def __init__(self, solve):
        self.solve, self.total, self.applications = solve, 0, 0

    def __call__(self, r):
        x, its = self.solve(np.ascontiguousarray(r, dtype=np.float64))
        self.total += its
        self.applications += 1
        return x


def gmres_left(ai, aj, aa, b, pc, restart=30, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4):
    """KSPSolve_GMRES as the harness runs it (gmres.c:118-409; left preconditioning, the preconditioned norm, zero guess, no refinement,
    KSPDefaultConverged) with the preconditioner a callable r -> z, which plain GMRES takes for ONE linear operator: the sequence of
    nullspace_ref.gmres without a null space.  With a callable that answers differently from call to call the history is the recurrence's
    estimate of a "preconditioned residual" no operator defines.  Returns x, the residual history, its, reason."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    n, m = b.size, restart

    def apply(r):
        return np.ascontiguousarray(pc(np.ascontiguousarray(r).copy()), dtype=np.float64)

    def normalize(v):                                    # VecNormalize (rvector.c:299)
        nrm = float(orc.vec_norm(v, 1))
        if nrm != 0.0 and nrm != 1.0:
            orc.vec_scale(v, 1.0 / nrm)
        return nrm

    state = dict(rn0=None, ttol=None)

    def converged(it, rn):
        if it == 0:
            state["rn0"] = rn
            state["ttol"] = max(rtol * rn, abstol)
        if np.isnan(rn) or np.isinf(rn):
            return DIVERGED_NAN
        if rn <= state["ttol"]:
            return CONVERGED_ATOL if rn < abstol else CONVERGED_RTOL
        return DIVERGED_DTOL if rn >= dtol * state["rn0"] else 0

    x, hist, its, total, reason, guess_zero = np.zeros(n), [], 0, 0, 0, True
    while not reason:
        if guess_zero:                                   # KSPInitialResidual (itres.c:39-73)
            v0 = apply(b)
        else:
            t2 = b.copy()
            orc.vec_axpy(t2, -1.0, orc.matmult(ai, aj, aa, x)[0])
            v0 = apply(t2)
        V = [v0]
        H = np.zeros((m + 2, m + 1))
        c, s, rhs = np.zeros(m + 2), np.zeros(m + 2), np.zeros(m + 2)
        rn = normalize(V[0])
        rhs[0] = rn
        hist.append(rn)
        k, happy = 0, False
        if not rn:
            reason = CONVERGED_ATOL
            break
        reason = converged(its, rn)
        while not reason and k < m and its < max_it:
            if k:
                hist.append(rn)
            w = apply(orc.matmult(ai, aj, aa, V[k])[0])
            coef = orc.vec_mdot(w, V[:k + 1])
            coef = -coef
            orc.vec_maxpy(w, coef, V[:k + 1])
            for j in range(k + 1):
                H[j, k] = 0.0
                H[j, k] -= coef[j]
            hnext = normalize(w)
            V.append(w)
            H[k + 1, k] = hnext
            bound = abs(hnext / rhs[k])
            if bound > 1.0e-30:
                bound = 1.0e-30
            if hnext < bound:
                happy = True
            for j in range(k):
                upper = H[j, k]
                H[j, k] = c[j] * upper + s[j] * H[j + 1, k]
                H[j + 1, k] = c[j] * H[j + 1, k] - (s[j] * upper)
            if happy:
                rn = 0.0
            else:
                ln = float(np.sqrt(H[k, k] * H[k, k] + H[k + 1, k] * H[k + 1, k]))
                if ln == 0.0:
                    reason = DIVERGED_NULL
                else:
                    c[k] = H[k, k] / ln
                    s[k] = H[k + 1, k] / ln
                    rhs[k + 1] = -(s[k] * rhs[k])
                    rhs[k] = c[k] * rhs[k]
                    H[k, k] = c[k] * H[k, k] + s[k] * H[k + 1, k]
                    rn = abs(rhs[k + 1])
            k += 1
            its += 1
            if reason:
                break
            reason = converged(its, rn)
            if happy:
                break
        if k and (reason or its >= max_it):
            hist.append(rn)
        if k:                                            # KSPGMRESBuildSoln (gmres.c:309-354)
            y, broke = np.zeros(k), False
            for r in range(k - 1, -1, -1):
                acc = rhs[r]
                for j in range(r + 1, k):
                    acc = acc - H[r, j] * y[j]
                if H[r, r] == 0.0:
                    reason, broke = -5, True
                    break
                y[r] = acc / H[r, r]
            if not broke:
                upd = np.zeros(n)
                orc.vec_maxpy(upd, y, V[:k])
                orc.vec_axpy(x, 1.0, upd)
        total += k
        if total >= max_it:
            if not reason:
                reason = DIVERGED_ITS
            break
        guess_zero = False
    return x, np.array(hist), its, reason
