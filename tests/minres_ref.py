"""Host model of the two fused MINRES sweeps (mi355x_vec_minres_lanczos / mi355x_vec_minres_update, include/mi355x_kernels.h) and of
the driver built on them (KSPSolve_MinresHIP, petsc-dev_amd/host/kspfused.c) for tests/test_minres_*: every Vec call through the
oracle (tests/orc.py: vec_copy, vec_axpy, vec_scale, vec_pointwise_mult, vec_dot, vec_norm -- under orc.device_reduction_order() the
sums carry the device's bits), the product through orc.spmv, the preconditioner an inverted diagonal (PCJACOBI), None (PCNONE) or any
callable r -> z; the checkpoints are those of tests/cheby_ref.py (KSPDefaultConverged, preconditioned norm).  The sequence is
KSPSolve_MINRES of PETSc 3.3 (src/ksp/ksp/impls/minres/minres.c)."""
import math

import numpy as np

import cheby_ref as cr
import orc

HAPTOL = 1.0e-18
DIVERGED_ITS, DIVERGED_INDEFINITE_PC, DIVERGED_INDEFINITE_MAT = -3, -8, -10


def _c(a):
    return np.array(a, dtype=np.float64)


def _r(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def lanczos_ref(alpha, beta, d, r, z, v, u, vold, uold):
    """the Lanczos sweep op by op: PCApply_Jacobi (d is not None; z is not read), then VecAXPY x4 in the reference's order.
    Returns the new (r, z); the arguments are left alone.  r'z over the result is VecDot(r, z)."""
    r = _c(r)
    if d is None:
        z = _c(z)
    else:
        z = np.zeros(r.size)
        orc.vec_pointwise_mult(z, r, _r(d))
    orc.vec_axpy(r, -alpha, _r(v))
    orc.vec_axpy(z, -alpha, _r(u))
    orc.vec_axpy(r, -beta, _r(vold))
    orc.vec_axpy(z, -beta, _r(uold))
    return r, z


def update_ref(first, rho2, rho3, irho1, ceta, ibeta, u, w, wold, x, r, z):
    """the update sweep op by op: VecCopy, VecAXPY x2, VecScale (the new W), VecAXPY on x, VecCopy + VecScale x2 (the next V, U).
    Returns (wn, x, vnew, unew); first: (None, None, vnew, unew).  The arguments are left alone."""
    wn = xn = None
    if not first:
        wn = np.zeros(np.size(u))
        orc.vec_copy(_r(u), wn)
        orc.vec_axpy(wn, -rho2, _r(w))
        orc.vec_axpy(wn, -rho3, _r(wold))
        orc.vec_scale(wn, irho1)
        xn = _c(x)
        orc.vec_axpy(xn, ceta, wn)
    vnew, unew = np.zeros(np.size(r)), np.zeros(np.size(z))
    orc.vec_copy(_r(r), vnew)
    orc.vec_copy(_r(z), unew)
    orc.vec_scale(vnew, ibeta)
    orc.vec_scale(unew, ibeta)
    return wn, xn, vnew, unew


def givens(alpha, beta, betaold, c, cold, s, sold):
    """one step of the QR factorisation of the tridiagonal matrix: -> (rho1, rho2, rho3, c, cold, s, sold)"""
    coold, cold, soold, sold = cold, c, sold, s
    rho0 = cold * alpha - coold * sold * betaold
    rho1 = math.sqrt(rho0 * rho0 + beta * beta)
    rho2 = sold * alpha + coold * cold * betaold
    rho3 = soold * betaold
    return rho1, rho2, rho3, rho0 / rho1, cold, beta / rho1, sold


def minres(ai, aj, aa, b, pc=None, x0=None, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4):
    """the fused driver: the solve start through the separate calls, then lanczos_ref and update_ref per iteration with a host
    product; Jacobi rides in the Lanczos sweep, any other preconditioner forms z first.  Returns (x, history, its, reason)."""
    S = cr._Solve(ai, aj, aa, b, pc, cr.PRECONDITIONED, x0, rtol, abstol, dtol, max_it)
    n = S.b.size
    x = S.x
    d = None if (pc is None or callable(pc)) else pc
    vold, uold, w, wold = (np.zeros(n) for _ in range(4))
    r = S.start()
    z = S.apply(r)
    nrm = float(orc.vec_norm(z, 1))
    dp = float(orc.vec_dot(r, z))
    if dp < HAPTOL:
        return x.copy(), np.array(S.hist), 0, DIVERGED_INDEFINITE_MAT
    beta = math.sqrt(abs(dp))
    eta = beta
    _, _, v, u = update_ref(True, 0.0, 0.0, 0.0, 0.0, 1.0 / beta, None, None, None, None, r, z)
    c = cold = 1.0
    s = sold = 0.0
    rnorm = nrm
    if S.checkpoint(0, nrm):
        return x.copy(), np.array(S.hist), 0, S.reason
    its = 0
    for i in range(max_it):
        its = i + 1
        r = S.mult(u)
        alpha = float(orc.vec_dot(u, r))
        zin = None if d is not None else S.apply(r)
        r, z = lanczos_ref(alpha, beta, d, r, zin, v, u, vold, uold)
        betaold = beta
        dp = float(orc.vec_dot(r, z))
        if dp < HAPTOL:
            S.reason = DIVERGED_INDEFINITE_PC
            break
        beta = math.sqrt(abs(dp))
        rho1, rho2, rho3, c, cold, s, sold = givens(alpha, beta, betaold, c, cold, s, sold)
        wn, x, vnew, unew = update_ref(False, rho2, rho3, 1.0 / rho1, c * eta, 1.0 / beta, u, w, wold, x, r, z)
        w, wold = wn, w
        v, vold, u, uold = vnew, v, unew, u
        eta = -s * eta
        rnorm = rnorm * abs(s)
        if S.checkpoint(i + 1, rnorm):
            break
    else:
        S.reason = DIVERGED_ITS
    return x.copy(), np.array(S.hist), its, S.reason
