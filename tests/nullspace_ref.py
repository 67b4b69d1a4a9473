"""Pure-Python restatement of MatNullSpaceRemove (src/mat/interface/matnull.c) and of KSPSolve_CG (cg.c) with the removal after
every preconditioner application (kspimpl.h KSP_PCApply / KSP_RemoveNullSpace), for tests/test_nullspace_*.py.  Products, updates
and reductions are the oracle's (tests/orc.py): inside orc.device_reduction_order() the sums take the device's order, and the sum of
a vector is orc.vec_dot(x, ones) in that order (x * 1.0 is x).  Nothing here calls the code under test."""
import numpy as np

import orc


def neumann7(nx, ny, nz):
    """the 3-D 7-point Laplacian with pure Neumann boundaries as CSR (ascending columns): diagonal = number of neighbours,
    off-diagonals -1; singular, its null space is the constant vector"""
    ai, aj, aa = [0], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                row = (k * ny + j) * nx + i
                nb = []
                if k > 0: nb.append(row - nx * ny)
                if j > 0: nb.append(row - nx)
                if i > 0: nb.append(row - 1)
                if i < nx - 1: nb.append(row + 1)
                if j < ny - 1: nb.append(row + nx)
                if k < nz - 1: nb.append(row + nx * ny)
                for c in sorted(nb + [row]):
                    aj.append(c)
                    aa.append(float(len(nb)) if c == row else -1.0)
                ai.append(len(aj))
    return np.array(ai, dtype=np.int32), np.array(aj, dtype=np.int32), np.array(aa, dtype=np.float64)


def vec_sum(x):
    return float(orc.vec_dot(x, np.ones(x.size)))


def remove(v, has_cnst=True, vecs=()):
    """MatNullSpaceRemove on a copy of v: the constant (VecSum; sum / (-1.0 * N); VecShift), then the vectors (VecMDot, negate,
    VecMAXPY)"""
    v = np.array(v, dtype=np.float64)
    n = v.size
    if has_cnst and n > 0:
        s = vec_sum(v)
        s = s / (-1.0 * n)
        v = v + s
    if len(vecs):
        alpha = orc.vec_mdot(v, list(vecs))
        alpha = -alpha
        orc.vec_maxpy(v, alpha, list(vecs))
    return v


def orthonormal_pair(n):
    """two orthonormal vectors, both orthogonal to the constant as well (to rounding), so that constant + pair is an orthogonal basis
    and the removal a projection (for the removal tests: they need not be in any operator's null space)"""
    t = np.arange(n, dtype=np.float64)
    a = np.cos(0.11 * t) + 0.3
    b = np.sin(0.07 * t) - 0.2
    a = a - np.mean(a)
    b = b - np.mean(b)
    a = a / np.sqrt(a @ a)
    b = b - (a @ b) * a
    b = b / np.sqrt(b @ b)
    return a, b


def jacobi(ai, aj, aa):
    """PCSetUp_Jacobi's inverted diagonal (jacobi.c: 1/d, a zero entry -> 1)"""
    d = orc.get_diagonal(ai, aj, aa)
    return np.where(d == 0.0, 1.0, 1.0 / np.where(d == 0.0, 1.0, d))


def gmres(ai, aj, aa, b, rtol, dinv=None, nullsp=None, restart=30, abstol=1e-50, dtol=1e4, max_it=10000):
    """KSPSolve_GMRES (gmres.c:118-409; left preconditioning, zero guess, classical Gram-Schmidt without refinement, borthog2.c:35-119,
    KSPDefaultConverged) with the removal after every preconditioner application: KSPInitialResidual's KSP_PCApply and the
    KSP_PCApplyBAorAB of every step (MatMult, PCApply, remove).  Returns x, the residual history, its, reason."""
    n = b.size

    def apply(r):
        z = np.zeros(n)
        if dinv is None:
            z[:] = r
        else:
            orc.vec_pointwise_mult(z, r, dinv)
        return remove(z, *nullsp) if nullsp is not None else z

    def normalize(v):                                   # VecNormalize (rvector.c:299)
        nrm = float(orc.vec_norm(v, 1))
        if nrm != 0.0 and nrm != 1.0:
            orc.vec_scale(v, 1.0 / nrm)
        return nrm

    state = dict(rn0=None, ttol=None)

    def converged(it, rn):                              # KSPDefaultConverged (iterativ.c:702-783), zero guess
        if it == 0:
            state["rn0"] = rn
            state["ttol"] = max(rtol * rn, abstol)
        if np.isnan(rn) or np.isinf(rn):
            return -9
        if rn <= state["ttol"]:
            return 3 if rn < abstol else 2
        return -4 if rn >= dtol * state["rn0"] else 0

    x, hist, its, total, reason, guess_zero = np.zeros(n), [], 0, 0, 0, True
    while not reason:
        if guess_zero:                                  # KSPInitialResidual (itres.c:39-73)
            v0 = apply(b.copy())
        else:
            t1 = orc.matmult(ai, aj, aa, x)[0]
            t2 = b.copy()
            orc.vec_axpy(t2, -1.0, t1)
            v0 = apply(t2)
        V = [v0]
        H = np.zeros((restart + 2, restart + 1))        # H[i, k]: row i of column k
        c, s, rhs = np.zeros(restart + 2), np.zeros(restart + 2), np.zeros(restart + 2)
        beta = normalize(V[0])
        rhs[0] = beta
        rn = beta
        hist.append(rn)
        k, happy = 0, False
        if not rn:
            reason = 3
            break
        reason = converged(its, rn)
        while not reason and k < restart and its < max_it:
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
            for j in range(k):                          # KSPGMRESUpdateHessenberg (gmres.c:360-409)
                upper = H[j, k]
                H[j, k] = c[j] * upper + s[j] * H[j + 1, k]
                H[j + 1, k] = c[j] * H[j + 1, k] - (s[j] * upper)
            if happy:
                rn = 0.0
            else:
                ln = float(np.sqrt(H[k, k] * H[k, k] + H[k + 1, k] * H[k + 1, k]))
                if ln == 0.0:
                    reason = -2
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
        last = k - 1                                    # KSPGMRESBuildSoln (gmres.c:309-354)
        if last >= 0:
            y = np.zeros(last + 1)
            broke = False
            for r in range(last, -1, -1):
                acc = rhs[r]
                for j in range(r + 1, last + 1):
                    acc = acc - H[r, j] * y[j]
                if H[r, r] == 0.0:
                    reason, broke = -5, True
                    break
                y[r] = acc / H[r, r]
            if not broke:
                upd = np.zeros(n)
                orc.vec_maxpy(upd, y, V[:last + 1])
                orc.vec_axpy(x, 1.0, upd)
        total += k
        if total >= max_it:
            if not reason:
                reason = -3
            break
        guess_zero = False
    return x, np.array(hist), its, reason


def pcg(ai, aj, aa, b, rtol, dinv=None, nullsp=None, abstol=1e-50, dtol=1e4, max_it=10000):
    """KSPSolve_CG (cg.c; preconditioned norm, zero guess, KSPDefaultConverged) with z = remove(B r): B the Jacobi scaling (dinv) or the
    identity (None: PCApply_None's copy); nullsp = (has_cnst, vecs) or None.  Returns x, the residual history, its, reason."""
    n = b.size

    def apply(r):
        z = np.zeros(n)
        if dinv is None:
            z[:] = r
        else:
            orc.vec_pointwise_mult(z, r, dinv)
        return remove(z, *nullsp) if nullsp is not None else z

    x, res = np.zeros(n), b.copy()
    z = apply(res)
    rn = float(orc.vec_norm(z, 1))
    rn0 = rn
    hist, ttol = [rn], max(rtol * rn, abstol)

    def reason_of(rn):
        if np.isnan(rn) or np.isinf(rn):
            return -9
        if rn <= ttol:
            return 3 if rn < abstol else 2
        return -4 if rn >= dtol * rn0 else 0

    reason, k, its = reason_of(rn), 0, 0
    if reason:
        return x, np.array(hist), 0, reason
    rz, rz_last, pap_last, d = float(orc.vec_dot(z, res)), 1.0, 0.0, None
    while True:
        its = k + 1
        if rz == 0.0:
            reason = 3
            break
        if k > 0 and rz * rz_last < 0.0:
            reason = -8
            break
        if k == 0:
            d = z.copy()
        else:
            orc.vec_aypx(d, rz / rz_last, z)
        ad = orc.matmult(ai, aj, aa, d)[0]
        pap = float(orc.vec_dot(d, ad))
        rz_last = rz
        if pap == 0.0 or (k > 0 and pap * pap_last <= 0.0):
            reason = -10
            break
        pap_last = pap
        step = rz / pap
        orc.vec_axpy(x, step, d)
        orc.vec_axpy(res, -step, ad)
        z = apply(res)
        rn = float(orc.vec_norm(z, 1))
        hist.append(rn)
        reason = reason_of(rn)
        if reason:
            break
        rz = float(orc.vec_dot(z, res))
        k += 1
        if k >= max_it:
            reason = -3
            break
    return x, np.array(hist), its, reason
