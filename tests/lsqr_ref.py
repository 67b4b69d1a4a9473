"""Host model of the two fused LSQR sweeps (mi355x_vec_lsqr_bidiag / mi355x_vec_lsqr_update, include/mi355x_kernels.h) and of the solvers
built on them (KSPSolve_LSQR, petsc-dev_amd/harness/krylov.c; KSPSolve_LsqrHIP, petsc-dev_amd/host/kspfused.c) for tests/test_lsqr_*: every Vec
call through the oracle (tests/orc.py: vec_copy, vec_axpy, vec_aypx, vec_scale, vec_pointwise_mult, vec_dot, vec_norm), the two products
through orc.spmv and orc.spmv_t, the preconditioner of the normal equations an inverted diagonal (PCJACOBI on A^T A), None (PCNONE) or any
callable v -> z on vectors of the column space.  device_order=True runs the whole solve under orc.device_reduction_order(), so the sums
carry the device's bits.  The sequence is the one DESIGN.md states for KSPLSQR: Paige and Saunders' bidiagonalisation started from the
residual of the guess, one Givens rotation per step, the checkpoints with the estimate phibar of ||b - A x||."""
import contextlib
import math

import numpy as np

import orc

CONVERGED_RTOL_NORMAL, CONVERGED_RTOL, CONVERGED_ATOL, CONVERGED_HAPPY_BREAKDOWN, CONVERGED_ATOL_NORMAL = 1, 2, 3, 8, 9
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_NAN = -3, -4, -9


def _c(a):
    return np.array(a, dtype=np.float64)


def _r(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def bidiag_ref(coef, x, y):
    """the bidiagonalisation sweep op by op: VecAXPY(y, -coef, x), then VecNorm(y, NORM_2), the root of the sweep's sum.
    Returns (new y, norm); the arguments are left alone."""
    y = _c(y)
    orc.vec_axpy(y, -coef, _r(x))
    return y, float(orc.vec_norm(y, 1))


def update_ref(ialpha, step, cf, irho2, skip_w, v1, x, w, se):
    """the update sweep op by op: VecScale(v1), VecAXPY(x, step, w), the four calls of the standard-error sum, VecAYPX(w, cf, v1).
    Returns the new (v1, x, w, se); an argument that is None stays None.  The arguments are left alone."""
    v1n = _c(v1) if v1 is not None else None
    xn = _c(x) if x is not None else None
    wn = _c(w) if w is not None else None
    sen = _c(se) if se is not None else None
    if v1n is not None:
        orc.vec_scale(v1n, ialpha)
    if xn is not None and step != 0.0:
        orc.vec_axpy(xn, step, wn)
    if sen is not None:
        w2 = np.zeros(wn.size)
        orc.vec_copy(wn, w2)
        orc.vec_pointwise_mult(w2, w2.copy(), w2.copy())
        orc.vec_scale(w2, irho2)
        orc.vec_axpy(sen, 1.0, w2)
    if not skip_w:
        orc.vec_aypx(wn, cf, v1n)
    return v1n, xn, wn, sen


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __iter__(self):                                  # (x, history, its, reason): what tests compare first
        return iter((self.x, self.hist, self.its, self.reason))


def lsqr(ai, aj, aa, n, b, pc=None, x0=None, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4, normal_tests=False, se=False, device_order=False, skip_test=False):
    """A: m x n in CSR; b of length m.  normal_tests: KSPLSQRDefaultConverged instead of KSPDefaultConverged.  se: keep the running sum
    of (w .* w) / rho^2.  skip_test: KSPSkipConverged (what KSP_NORM_NONE installs): the reason stays unset until max_it.  Returns a Result: x, hist, its, reason, arnorm, rhs_norm, anorm, se (None unless asked for)."""
    with (orc.device_reduction_order() if device_order else contextlib.nullcontext()):
        return _lsqr(ai, aj, aa, n, _r(b), pc, x0, max_it, rtol, abstol, dtol, normal_tests, se, skip_test)


def _lsqr(ai, aj, aa, n, b, pc, x0, max_it, rtol, abstol, dtol, normal_tests, want_se, skip_test):
    m = ai.size - 1
    assert b.size == m
    x = np.zeros(n) if x0 is None else _c(x0)
    hist = []
    state = {"rn0": None, "ttol": None}
    out = Result(x=x, hist=None, its=0, reason=0, arnorm=0.0, rhs_norm=0.0, anorm=0.0, se=None)

    def apply(v):
        if callable(pc):
            return _c(pc(v))
        z = np.zeros(v.size)
        orc.vec_pointwise_mult(z, v, _r(pc))
        return z

    def converged(it, rn):                               # KSPDefaultConverged with the unpreconditioned norm, then the two normal tests
        if skip_test:
            return 4 if it >= max_it else 0              # KSP_CONVERGED_ITS
        if it == 0:
            if x0 is None:
                state["rn0"] = rn
            else:
                s = float(orc.vec_norm(b, 1))
                state["rn0"] = s if s else rn
            state["ttol"] = max(rtol * state["rn0"], abstol)
        if math.isnan(rn) or math.isinf(rn):
            return DIVERGED_NAN
        if rn <= state["ttol"]:
            return CONVERGED_ATOL if rn < abstol else CONVERGED_RTOL
        if rn >= dtol * state["rn0"]:
            return DIVERGED_DTOL
        if normal_tests and it:
            if out.arnorm <= abstol:
                return CONVERGED_ATOL_NORMAL
            if out.arnorm <= rtol * out.anorm * rn:
                return CONVERGED_RTOL_NORMAL
        return 0

    def checkpoint(it, rn):
        hist.append(rn)
        out.reason = converged(it, rn)
        return out.reason

    def done():
        out.hist = np.array(hist)
        out.x = x.copy()
        return out

    if x0 is None:
        u = np.zeros(m)
        orc.vec_copy(b, u)
    else:
        u = orc.spmv(ai, aj, aa, x)
        orc.vec_aypx(u, -1.0, b)
    beta = float(orc.vec_norm(u, 1))
    out.rhs_norm = beta
    if checkpoint(0, beta):
        return done()
    if beta != 0.0:
        orc.vec_scale(u, 1.0 / beta)
    v = orc.spmv_t(ai, aj, aa, u, n)
    z = None
    if pc is None:
        alpha = float(orc.vec_norm(v, 1))
    else:
        z = apply(v)
        alpha = math.sqrt(float(orc.vec_dot(v, z)))
        if alpha != 0.0:
            orc.vec_scale(z, 1.0 / alpha)
    if alpha == 0.0:
        out.reason = CONVERGED_ATOL_NORMAL
        return done()
    orc.vec_scale(v, 1.0 / alpha)
    w = np.zeros(n)
    orc.vec_copy(v if pc is None else z, w)
    se = np.zeros(n) if want_se else None
    phibar, rhobar, anorm2 = beta, alpha, alpha * alpha
    out.arnorm, out.anorm = alpha * beta, math.sqrt(anorm2)
    i = 0
    while i < max_it:
        u1 = orc.spmv(ai, aj, aa, v if pc is None else z)
        u1, beta = bidiag_ref(alpha, u, u1)
        if beta != 0.0:
            orc.vec_scale(u1, 1.0 / beta)
        v1 = orc.spmv_t(ai, aj, aa, u1, n)
        z1 = None
        if pc is None:
            v1, alpha = bidiag_ref(beta, v, v1)
        else:
            orc.vec_axpy(v1, -beta, v)
            z1 = apply(v1)
            alpha = math.sqrt(float(orc.vec_dot(v1, z1)))
            if alpha != 0.0:
                orc.vec_scale(z1, 1.0 / alpha)
        ialpha = 1.0 / alpha if alpha != 0.0 else 1.0
        broke = beta == 0.0 or alpha == 0.0
        rho = math.sqrt(rhobar * rhobar + beta * beta)
        c, s = rhobar / rho, beta / rho
        theta, rhobar = s * alpha, -c * alpha
        phi, phibar = c * phibar, s * phibar
        if pc is None:
            v1, x, w, se = update_ref(ialpha, phi / rho, -theta / rho, 1.0 / (rho * rho), broke, v1, x, w, se)
        else:
            orc.vec_scale(v1, ialpha)
            z1, x, w, se = update_ref(1.0, phi / rho, -theta / rho, 1.0 / (rho * rho), broke, z1, x, w, se)
        out.arnorm = alpha * abs(s * phi)
        anorm2 += alpha * alpha + beta * beta
        out.anorm = math.sqrt(anorm2)
        out.its = i + 1
        out.se = se
        if checkpoint(i + 1, phibar):
            break
        if broke:
            out.reason = CONVERGED_HAPPY_BREAKDOWN
            break
        u, v, z = u1, v1, z1
        i += 1
    if i >= max_it and not out.reason:
        out.reason = DIVERGED_ITS
    out.se = se
    return done()
