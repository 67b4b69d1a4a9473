"""Host model of KSPSolve_Chebychev (src/ksp/ksp/impls/cheby/cheby.c) and KSPSolve_Richardson (src/ksp/ksp/impls/rich/rich.c) of PETSc 3.3
for tests/test_cheby_*: the call sequences of the harness drivers (petsc-dev_amd/harness/krylov.c), every Vec / Mat call through the
oracle (tests/orc.py: spmv, vec_*, vec_norm -- under orc.device_reduction_order() the norms carry the device's bits), the
preconditioner an inverted diagonal (PCJACOBI), None (PCNONE) or any callable r -> z.  Left preconditioning, KSPDefaultConverged /
KSPSkipConverged.  Both return (x, history, its, reason, number of preconditioner applications)."""
import numpy as np

import orc

NONE, PRECONDITIONED, UNPRECONDITIONED = "none", "preconditioned", "unpreconditioned"
CONVERGED_RTOL, CONVERGED_ATOL, CONVERGED_ITS, DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_NAN = 2, 3, 4, -3, -4, -9


def jacobi(ai, aj, aa):
    """PCSetUp_Jacobi's inverted diagonal (jacobi.c: 1/d, a zero entry -> 1)"""
    d = orc.get_diagonal(ai, aj, aa)
    return np.where(d == 0.0, 1.0, 1.0 / np.where(d == 0.0, 1.0, d))


class _Solve:
    """what the two drivers share: the operator, the preconditioner, the start residual and the convergence checkpoints"""

    def __init__(self, ai, aj, aa, b, pc, norm, x0, rtol, abstol, dtol, max_it):
        self.csr, self.b, self.pc, self.norm = (ai, aj, aa), np.ascontiguousarray(b, dtype=np.float64), pc, norm
        self.guess_zero = x0 is None
        self.x = np.zeros(b.size) if x0 is None else np.array(x0, dtype=np.float64)
        self.rtol, self.abstol, self.dtol, self.max_it = rtol, abstol, dtol, max_it
        self.hist, self.reason, self.applications, self.ttol, self.rn0 = [], 0, 0, None, None

    def mult(self, v):
        return orc.spmv(*self.csr, v)

    def apply(self, r):                                  # KSP_PCApply
        self.applications += 1
        if callable(self.pc):
            return np.ascontiguousarray(self.pc(r), dtype=np.float64)
        z = np.zeros(r.size)
        if self.pc is None:
            orc.vec_copy(r, z)
        else:
            orc.vec_pointwise_mult(z, r, self.pc)
        return z

    def residual_of(self, v):                            # KSP_MatMult(A, v, r); VecAYPX(r, -1, b)
        r = self.mult(v)
        orc.vec_aypx(r, -1.0, self.b)
        return r

    def start(self):
        if self.guess_zero:
            r = np.zeros(self.b.size)
            orc.vec_copy(self.b, r)
            return r
        return self.residual_of(self.x)

    def converged(self, it, rn):                         # KSPSkipConverged / KSPDefaultConverged (iterativ.c:536, 702-783)
        if self.norm == NONE:
            return CONVERGED_ITS if it >= self.max_it else 0
        if it == 0:
            if self.guess_zero:
                self.rn0 = rn
            else:                                        # the norm of the (preconditioned) right-hand side
                saved = self.applications
                s = float(orc.vec_norm(self.b if self.norm == UNPRECONDITIONED else self.apply(self.b), 1))
                self.applications = saved
                self.rn0 = s if s else rn
            self.ttol = max(self.rtol * self.rn0, self.abstol)
        if np.isnan(rn) or np.isinf(rn):
            return DIVERGED_NAN
        if rn <= self.ttol:
            return CONVERGED_ATOL if rn < self.abstol else CONVERGED_RTOL
        if rn >= self.dtol * self.rn0:
            return DIVERGED_DTOL
        return 0

    def checkpoint(self, it, rn):
        self.hist.append(rn)
        self.reason = self.converged(it, rn)
        return self.reason

    def out_of_iterations(self, its, rn):
        if its < self.max_it:
            return
        if self.norm == NONE:
            self.reason = CONVERGED_ITS
        else:
            self.reason = self.converged(its, rn) or DIVERGED_ITS


def chebychev(ai, aj, aa, b, emin, emax, pc=None, norm=NONE, x0=None, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4):
    """KSPSolve_Chebychev: p[km1] = x, p[k], p[kp1] rotated after every update; emin, emax: bounds of the spectrum of B A"""
    S = _Solve(ai, aj, aa, b, pc, norm, x0, rtol, abstol, dtol, max_it)
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    Gamma, mu, omegaprod = 1.0, 1.0 / alpha, 2.0 / alpha
    p = [S.x, None, None]
    c = [1.0, mu, 0.0]
    km1, k, kp1 = 0, 1, 2
    its, rn = 0, 0.0
    p[k] = S.apply(S.start())
    orc.vec_aypx(p[k], scale, S.x)                       # p[k] = x + scale B r
    for i in range(max_it):
        its += 1
        c[kp1] = 2.0 * mu * c[k] - c[km1]
        omega = omegaprod * c[k] / c[kp1]
        r = S.residual_of(p[k])
        p[kp1] = S.apply(r)
        if norm != NONE:
            rn = float(orc.vec_norm(r if norm == UNPRECONDITIONED else p[kp1], 1))
            if S.checkpoint(i, rn):
                break
        orc.vec_scale(p[kp1], omega * Gamma * scale)
        orc.vec_axpy(p[kp1], 1.0 - omega, p[km1])
        orc.vec_axpy(p[kp1], omega, p[k])
        km1, k, kp1 = k, kp1, km1
    if not S.reason:
        if norm != NONE:
            r = S.residual_of(p[k])
            rn = float(orc.vec_norm(r if norm == UNPRECONDITIONED else S.apply(r), 1))
            S.hist.append(rn)
        S.out_of_iterations(its, rn)
    return p[k].copy(), np.array(S.hist), its, S.reason, S.applications


def richardson(ai, aj, aa, b, scale=1.0, pc=None, norm=NONE, x0=None, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4):
    """KSPSolve_Richardson without PCApplyRichardson: x += scale B (b - A x)"""
    S = _Solve(ai, aj, aa, b, pc, norm, x0, rtol, abstol, dtol, max_it)
    x = S.x
    r = S.start()
    z = None
    its, rn = 0, 0.0
    for i in range(max_it):
        if norm == UNPRECONDITIONED:
            rn = float(orc.vec_norm(r, 1))
            if S.checkpoint(i, rn):
                break
        z = S.apply(r)
        if norm == PRECONDITIONED:
            rn = float(orc.vec_norm(z, 1))
            if S.checkpoint(i, rn):
                break
        orc.vec_axpy(x, scale, z)
        its += 1
        if i + 1 < max_it or norm != NONE:
            r = S.residual_of(x)
    if not S.reason:
        if norm != NONE:
            rn = float(orc.vec_norm(r if norm == UNPRECONDITIONED else S.apply(r), 1))
            S.hist.append(rn)
        S.out_of_iterations(its, rn)
    return x.copy(), np.array(S.hist), its, S.reason, S.applications


def step_ref(s, a, c, w, b, d, pm, pk):
    """mi355x_vec_cheby_step op by op through the oracle: (r, z, pn) -- VecAYPX(r, -1, b), PCApply_Jacobi / PCNONE, VecScale, VecAXPY x2"""
    r = np.array(w, dtype=np.float64)
    orc.vec_aypx(r, -1.0, np.ascontiguousarray(b))
    z = np.zeros(r.size)
    if d is None:
        orc.vec_copy(r, z)
    else:
        orc.vec_pointwise_mult(z, r, np.ascontiguousarray(d))
    pn = z.copy()
    orc.vec_scale(pn, s)
    orc.vec_axpy(pn, a, np.ascontiguousarray(pm))
    orc.vec_axpy(pn, c, np.ascontiguousarray(pk))
    return r, z, pn


def rich_step_ref(scale, w, b, d, x):
    """mi355x_vec_rich_step op by op through the oracle: (r, z, x)"""
    r = np.array(w, dtype=np.float64)
    orc.vec_aypx(r, -1.0, np.ascontiguousarray(b))
    z = np.zeros(r.size)
    if d is None:
        orc.vec_copy(r, z)
    else:
        orc.vec_pointwise_mult(z, r, np.ascontiguousarray(d))
    xn = np.array(x, dtype=np.float64)
    orc.vec_axpy(xn, scale, z)
    return r, z, xn
