"""NumPy restatement of -pc_factor_hipmi355x_trisolve sweeps:<k> on an oracle factor (host/ilu.c, ilu0_sweeps_apply): the negated strict
triangles as CSR, one sweep step, and k steps per triangle.  test_ilu_sweeps_gpu.py and pcprog.py share it; nothing here touches the GPU."""
import numpy as np


def ref_add_scaled(ai, aj, aa, x, y, d=None):
    """numpy, one row after the other: s = y_r; s = s + a_j x_j in column order (product rounded, then the sum); d_r * s"""
    out = np.empty(ai.size - 1)
    for r in range(ai.size - 1):
        s = y[r]
        for q in range(ai[r], ai[r + 1]):
            s = s + aa[q] * x[aj[q]]
        out[r] = s if d is None else d[r] * s
    return out


def strict_triangles(f):
    """the negated strict triangles of an oracle factor as CSR, and the inverted pivots"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    iL, jL, aL = bi.copy(), bj[:bi[n]].copy(), -ba[:bi[n]]
    lenU = (bd[:-1] - bd[1:] - 1).astype(np.int32)
    iU = np.zeros(n + 1, np.int32); iU[1:] = np.cumsum(lenU)
    src = np.concatenate([np.arange(bd[i + 1] + 1, bd[i]) for i in range(n)]).astype(np.int64) if iU[n] else np.zeros(0, np.int64)
    return (iL, jL, aL), (iU, bj[src].astype(np.int32), -ba[src]), ba[bd[:-1]].copy()


def jacobi_sweeps(f, b, k):
    """k Jacobi sweeps per triangle: y^0 = b, y^j = b - Ls y^(j-1); x^0 = dinv .* y^k, x^j = dinv .* (y^k - Us x^(j-1))"""
    (iL, jL, aL), (iU, jU, aU), dinv = strict_triangles(f)
    y = np.array(b, dtype=np.float64)
    for _ in range(k):
        y = ref_add_scaled(iL, jL, aL, y, b)
    x = dinv * y
    for _ in range(k):
        x = ref_add_scaled(iU, jU, aU, x, y, dinv)
    return x
