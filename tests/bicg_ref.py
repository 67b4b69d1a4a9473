"""Host model for tests/test_bicg_* and tests/test_ilut_*: MatSolveTranspose_SeqAIJ (src/mat/impls/aij/seq/aijfact.c, natural ordering) on
the factor layout orc.ilu0_factor / iluk_ref.symbolic produce (bi / bj / bdiag / ba, the inverted diagonal at bdiag[i]) -- the
reference's scatter loop and the gather form the device runs (csrc/trisolve_transpose.hip) -- a numpy restatement of
mi355x_ilut_build_host, and KSPSolve_BiCG (src/ksp/ksp/impls/bicg/bicg.c) as the harness restates it (petsc-dev_amd/harness/krylov.c):
every Vec call through the oracle (under orc.device_reduction_order() the sums carry the device's bits), the products through orc.spmv /
orc.spmv_t, the preconditioner and its transpose an inverted diagonal, None or two callables."""
import numpy as np

import cheby_ref as cr
import iluk_ref
import orc
from tfqmr_ref import convdiff, dense  # noqa: F401 (the operators of the BiCG tests)

DIVERGED_ITS, DIVERGED_BREAKDOWN = -3, -5
PRECONDITIONED, UNPRECONDITIONED = cr.PRECONDITIONED, cr.UNPRECONDITIONED
mul, sub = np.multiply, np.subtract


# ------------------------------------------------------------------------------------------------ the transposed solves
def ilu_solve_transpose(f, b):
    """the scatter loop: forward with U^T (scaled by the inverted diagonal), backward with L^T; every product rounded before its
    subtraction"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    t = np.array(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = mul(t[i], ba[bd[i]])
            for k in range(int(bd[i + 1]) + 1, int(bd[i])):
                t[bj[k]] = sub(t[bj[k]], mul(s, ba[k]))
            t[i] = s
        for i in range(n - 1, -1, -1):
            s = t[i]
            for k in range(int(bi[i]), int(bi[i + 1])):
                t[bj[k]] = sub(t[bj[k]], mul(s, ba[k]))
    return t


def build_transposed(bi, bj, bd):
    """mi355x_ilut_build_host restated: dict with ti, tj, tperm (U^T, every row's columns ascending), si, sj, sperm (L^T, descending),
    lev1 / nlev1 and lev2 / nlev2 (0 for a row without entries, else one more than the deepest row it reads)"""
    n = bi.size - 1
    ut = [[] for _ in range(n)]
    lt = [[] for _ in range(n)]
    for i in range(n):
        for k in range(int(bd[i + 1]) + 1, int(bd[i])):
            ut[bj[k]].append((i, k))
    for i in range(n - 1, -1, -1):
        for k in range(int(bi[i]), int(bi[i + 1])):
            lt[bj[k]].append((i, k))

    def csr(rows):
        p = np.zeros(n + 1, np.int32)
        p[1:] = np.cumsum([len(r) for r in rows])
        flat = [e for r in rows for e in r]
        return p, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.int32)
    ti, tj, tperm = csr(ut)
    si, sj, sperm = csr(lt)
    lev1, lev2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for c in range(n):
        lev1[c] = max([lev1[i] + 1 for i, _ in ut[c]], default=0)
    for c in range(n - 1, -1, -1):
        lev2[c] = max([lev2[i] + 1 for i, _ in lt[c]], default=0)
    return dict(ti=ti, tj=tj, tperm=tperm, si=si, sj=sj, sperm=sperm, lev1=lev1, nlev1=int(lev1.max()) + 1 if n else 0,
                lev2=lev2, nlev2=int(lev2.max()) + 1 if n else 0)


def ilu_solve_transpose_gather(f, b):
    """the gather form over the transposed triangles, rows in any order that respects the levels (here: ascending, then descending)"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    T = build_transposed(bi, bj, bd)
    x = np.zeros(n)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(n):
            s = b[c]
            for q in range(int(T["ti"][c]), int(T["ti"][c + 1])):
                s = sub(s, mul(ba[T["tperm"][q]], x[T["tj"][q]]))
            x[c] = mul(s, ba[bd[c]])
        for c in range(n - 1, -1, -1):
            s = x[c]
            for q in range(int(T["si"][c]), int(T["si"][c + 1])):
                s = sub(s, mul(ba[T["sperm"][q]], x[T["sj"][q]]))
            x[c] = s
    return x


def dependents(f, c):
    """the entries of x = (LU)^-T b that b[c] reaches in the model: c, whatever the forward solve with U^T carries it to, and from all
    of those whatever the backward solve with L^T does"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    hit = np.zeros(n, bool)
    hit[c] = True
    for i in range(n):
        if hit[i]:
            hit[bj[int(bd[i + 1]) + 1:int(bd[i])]] = True
    for i in range(n - 1, -1, -1):
        if hit[i]:
            hit[bj[int(bi[i]):int(bi[i + 1])]] = True
    return hit


def iluk_factor(ai, aj, aa, levels):
    """the ILU(levels) factor in the same layout, through tests/iluk_ref.py (no shift; the pivots of the test operators pass)"""
    layout = iluk_ref.symbolic(ai, aj, levels)
    ba, frow, _, _ = iluk_ref.reference_pass(ai, aj, aa, None, [0.0], 100.0 * 2.220446049250313e-16, [1], layout=layout)
    assert frow[0] < 0
    return layout[0], layout[1], layout[2], ba


def dense_factors(f):
    """(L with its unit diagonal, U with the diagonal un-inverted), dense"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    L, U = np.eye(n), np.zeros((n, n))
    for i in range(n):
        L[i, bj[bi[i]:bi[i + 1]]] = ba[bi[i]:bi[i + 1]]
        U[i, bj[bd[i + 1] + 1:bd[i]]] = ba[bd[i + 1] + 1:bd[i]]
        U[i, i] = 1.0 / ba[bd[i]]
    return L, U


def bidiagonal(n):
    """a lower + upper bidiagonal matrix: the factor's two triangles are chains of n levels"""
    ai, aj, aa = [0], [], []
    for i in range(n):
        if i:
            aj.append(i - 1); aa.append(-1.0 - 0.01 * (i % 7))
        aj.append(i); aa.append(4.0 + 0.1 * (i % 5))
        if i < n - 1:
            aj.append(i + 1); aa.append(-1.5 + 0.02 * (i % 3))
        ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa)


def diagonal(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), 2.0 + 0.25 * np.arange(n)


# ------------------------------------------------------------------------------------------------ KSPSolve_BiCG
def bicg(ai, aj, aa, b, x0=None, pc=None, pct=None, norm=PRECONDITIONED, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4,
         dot=None, vnorm=None):
    """pc: None (PCNONE), an inverted diagonal (PCJACOBI) or a callable r -> B r, then pct is the callable r -> B^T r.  dot / vnorm:
    the reductions (default: the oracle's, i.e. the device's order under orc.device_reduction_order()).  Returns (x, history, its,
    reason)."""
    dot = dot or (lambda x, y: float(orc.vec_dot(x, y)))
    vnorm = vnorm or (lambda x: float(orc.vec_norm(x, 1)))
    S = cr._Solve(ai, aj, aa, b, pc, norm, x0, rtol, abstol, dtol, max_it)
    n = S.b.size
    pnorm = norm == PRECONDITIONED

    def applyT(r):
        if callable(pc):
            return np.ascontiguousarray(pct(r), dtype=np.float64)
        return S.apply(r)

    def multT(v):
        return orc.spmv_t(ai, aj, aa, np.ascontiguousarray(v), n)
    x = S.x
    rr = S.start()
    rl = np.zeros(n)
    orc.vec_copy(rr, rl)
    zr, zl = S.apply(rr), applyT(rl)
    its = 0
    if S.checkpoint(0, vnorm(zr if pnorm else rr)):
        return x.copy(), np.array(S.hist), 0, S.reason
    pr, pl = np.zeros(n), np.zeros(n)
    betaold = 1.0
    for i in range(max_it):
        beta = dot(zr, rl)
        if i == 0:
            if beta == 0.0:
                return x.copy(), np.array(S.hist), 0, DIVERGED_BREAKDOWN
            orc.vec_copy(zr, pr)
            orc.vec_copy(zl, pl)
        else:
            bb = beta / betaold
            orc.vec_aypx(pr, bb, zr)
            orc.vec_aypx(pl, bb, zl)
        betaold = beta
        zr, zl = S.mult(pr), multT(pl)
        dpi = dot(zr, pl)
        if dpi == 0.0:
            S.reason = DIVERGED_BREAKDOWN
            break
        a = beta / dpi
        orc.vec_axpy(x, a, pr)
        orc.vec_axpy(rr, -a, zr)
        orc.vec_axpy(rl, -a, zl)
        if pnorm:
            zr, zl = S.apply(rr), applyT(rl)
        its = i + 1
        if S.checkpoint(i + 1, vnorm(zr if pnorm else rr)):
            break
        if not pnorm:
            zr, zl = S.apply(rr), applyT(rl)
    else:
        S.reason = DIVERGED_ITS
    return x.copy(), np.array(S.hist), its, S.reason
