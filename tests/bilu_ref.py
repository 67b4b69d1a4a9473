"""Host-side reference of block ILU(k) for BAIJ matrices (test_bilu_cpu.py checks it on its own and pins the host routine
mi355x_bilu_numeric_host with it, test_bilu_gpu.py compares the device solves and the plug-in with it).  Nothing here touches the GPU.

Every floating-point operation is one IEEE binary64 operation on Python floats (one rounding each, never fused), in exactly the order
include/mi355x_kernels.h ("Block ILU") states:

  numeric   block row i: the work blocks of the factor row start at +0.0 with A's blocks copied in; for every L block (i,k) in ascending
            k, fill included, that is not entirely == 0.0: M = W_k D_k^-1, then W_j = W_j - M U_kj for the strict-upper blocks (k,j) of
            row k whose column row i holds; every entry of a block product a left-to-right sum of bs products, then one subtraction;
            D_i^-1 by dgefa + dgedi (block_inverse);
  lower     s_r = b[bs i + r]; per stored L block in storage order s_r = s_r - (v[r] x_k[0] + v[r + bs] x_k[1] + ...); x[bs i + r] = s_r;
  upper     the same over the strict-upper blocks from x[bs i + r], then x[bs i + r] = d[r] s_0 + d[r + bs] s_1 + ...

The layout is the point ILU's (iluk_ref.symbolic on the BLOCK pattern): (bi, bj, bdiag), one column-major bs x bs block per entry."""
import numpy as np

import iluk_ref as ik


def symbolic(ai, aj, levels):
    """(bi, bj, bdiag) of the level-of-fill factor of a block pattern"""
    return ik.symbolic(np.asarray(ai, np.int32), np.asarray(aj, np.int32), levels)[:3]


def block_inverse(n, a):
    """in-place inverse of a column-major n x n block held in the list a (LINPACK dgefa + dgedi); the 1-based zero-pivot row or 0"""
    ipvt = [0] * n
    work = [0.0] * n
    for k in range(n - 1):
        l, big = k, abs(a[k + k * n])
        for i in range(k + 1, n):
            if abs(a[i + k * n]) > big:
                big, l = abs(a[i + k * n]), i
        ipvt[k] = l
        if a[l + k * n] == 0.0:
            return k + 1
        if l != k:
            a[l + k * n], a[k + k * n] = a[k + k * n], a[l + k * n]
        m = -1.0 / a[k + k * n]
        for i in range(k + 1, n):
            a[i + k * n] = a[i + k * n] * m
        for j in range(k + 1, n):
            t = a[l + j * n]
            if l != k:
                a[l + j * n] = a[k + j * n]
                a[k + j * n] = t
            for i in range(k + 1, n):
                a[i + j * n] = a[i + j * n] + t * a[i + k * n]
    ipvt[n - 1] = n - 1
    if a[(n - 1) + (n - 1) * n] == 0.0:
        return n
    for k in range(n):
        a[k + k * n] = 1.0 / a[k + k * n]
        t0 = -a[k + k * n]
        for i in range(k):
            a[i + k * n] = a[i + k * n] * t0
        for j in range(k + 1, n):
            t = a[k + j * n]
            a[k + j * n] = 0.0
            for i in range(k + 1):
                a[i + j * n] = a[i + j * n] + t * a[i + k * n]
    for k in range(n - 2, -1, -1):
        for i in range(k + 1, n):
            work[i] = a[i + k * n]
            a[i + k * n] = 0.0
        for j in range(k + 1, n):
            t = work[j]
            for i in range(n):
                a[i + k * n] = a[i + k * n] + t * a[i + j * n]
        l = ipvt[k]
        if l != k:
            for i in range(n):
                a[i + k * n], a[i + l * n] = a[i + l * n], a[i + k * n]
    return 0


def _product(bs, a, b):
    """c = a b, column-major lists; every entry a left-to-right sum of bs products"""
    c = [0.0] * (bs * bs)
    for col in range(bs):
        for r in range(bs):
            t = a[r] * b[col * bs]
            for k in range(1, bs):
                t = t + a[r + k * bs] * b[k + col * bs]
            c[r + col * bs] = t
    return c


def numeric(bs, ai, aj, aa, layout):
    """the factor's values on `layout` from A's block CSR: (ba with (nzb + 1) bs^2 doubles, the last block 0.0; the scalar row of a
    zero pivot or -1).  After a zero pivot the block rows before it are as computed."""
    bi, bj, bd = layout[:3]
    mbs = len(ai) - 1
    bs2 = bs * bs
    nzb = int(bd[0]) + 1 if mbs else 0
    ba = [0.0] * ((nzb + 1) * bs2)
    aa = np.asarray(aa, dtype=np.float64).tolist()
    for i in range(mbs):
        lcols = [int(c) for c in bj[bi[i]:bi[i + 1]]]
        ucols = [int(c) for c in bj[bd[i + 1] + 1:bd[i]]]
        work = {c: [0.0] * bs2 for c in lcols + [i] + ucols}
        for q in range(int(ai[i]), int(ai[i + 1])):
            work[int(aj[q])] = aa[q * bs2:(q + 1) * bs2]
        for k in lcols:
            wk = work[k]
            if all(v == 0.0 for v in wk):
                continue
            dk = int(bd[k])
            m = _product(bs, wk, ba[dk * bs2:(dk + 1) * bs2])
            work[k] = m
            for p in range(int(bd[k + 1]) + 1, dk):
                j = int(bj[p])
                if j in work:
                    mu = _product(bs, m, ba[p * bs2:(p + 1) * bs2])
                    wj = work[j]
                    work[j] = [wj[e] - mu[e] for e in range(bs2)]
        for q, c in zip(range(int(bi[i]), int(bi[i + 1])), lcols):
            ba[q * bs2:(q + 1) * bs2] = work[c]
        for q, c in zip(range(int(bd[i + 1]) + 1, int(bd[i])), ucols):
            ba[q * bs2:(q + 1) * bs2] = work[c]
        d = list(work[i])
        z = block_inverse(bs, d)
        ba[int(bd[i]) * bs2:(int(bd[i]) + 1) * bs2] = d
        if z:
            return np.array(ba), i * bs + z - 1
    return np.array(ba), -1


def level_rows(layout):
    """(rows of every dependency level of L in ascending order, the same for U): lists of int32 arrays, rows ascending inside a level"""
    bi, bj, bd = layout[:3]
    n = len(bi) - 1
    levL, levU = [0] * n, [0] * n
    for i in range(n):
        levL[i] = max([levL[int(c)] + 1 for c in bj[bi[i]:bi[i + 1]]], default=0)
    for i in range(n - 1, -1, -1):
        levU[i] = max([levU[int(c)] + 1 for c in bj[bd[i + 1] + 1:bd[i]]], default=0)

    def group(lev):
        return [np.array([i for i in range(n) if lev[i] == l], np.int32) for l in range(max(lev) + 1)] if n else []
    return group(levL), group(levU)


def _minus(bs, s, v, r, xk):
    t = v[r] * xk[0]
    for c in range(1, bs):
        t = t + v[r + c * bs] * xk[c]
    return s - t


def lower_rows(bs, layout, ba, b, x, rows):
    """the lower solve of the block rows `rows` (one dependency level): reads b and x, writes x (lists of floats)"""
    bi, bj = layout[0], layout[1]
    bs2 = bs * bs
    for i in (int(r) for r in rows):
        for r in range(bs):
            s = b[bs * i + r]
            for q in range(int(bi[i]), int(bi[i + 1])):
                k = int(bj[q])
                s = _minus(bs, s, ba[q * bs2:(q + 1) * bs2], r, x[bs * k:bs * k + bs])
            x[bs * i + r] = s


def upper_rows(bs, layout, ba, x, rows):
    bj, bd = layout[1], layout[2]
    bs2 = bs * bs
    for i in (int(r) for r in rows):
        s = []
        for r in range(bs):
            sr = x[bs * i + r]
            for q in range(int(bd[i + 1]) + 1, int(bd[i])):
                k = int(bj[q])
                sr = _minus(bs, sr, ba[q * bs2:(q + 1) * bs2], r, x[bs * k:bs * k + bs])
            s.append(sr)
        d = ba[int(bd[i]) * bs2:(int(bd[i]) + 1) * bs2]
        for r in range(bs):
            acc = d[r] * s[0]
            for c in range(1, bs):
                acc = acc + d[r + c * bs] * s[c]
            x[bs * i + r] = acc


def apply(bs, layout, ba, b):
    """x = U^-1 L^-1 b, level by level (the order inside a level does not matter: its rows do not read each other)"""
    ba = np.asarray(ba, dtype=np.float64).tolist()
    b = np.asarray(b, dtype=np.float64).tolist()
    x = [0.0] * len(b)
    L, U = level_rows(layout)
    for rows in L:
        lower_rows(bs, layout, ba, b, x, rows)
    for rows in U:
        upper_rows(bs, layout, ba, x, rows)
    return np.array(x)


# ------------------------------------------------------------------------------------------------ shapes
def block_tridiag(nb, bs, seed=11):
    """block-tridiagonal block CSR of nb block rows with dominant diagonal blocks (ILU(0) is its complete block LU): (bi, bj, ba)"""
    rng = np.random.default_rng(seed)
    bi, bj, blocks = [0], [], []
    for i in range(nb):
        for j in (i - 1, i, i + 1):
            if 0 <= j < nb:
                B = rng.standard_normal((bs, bs))
                if j == i:
                    B = B + 4.0 * bs * np.eye(bs)
                bj.append(j); blocks.append(B)
        bi.append(len(bj))
    ba = np.ascontiguousarray(np.array(blocks).transpose(0, 2, 1)).ravel()
    return np.array(bi, np.int32), np.array(bj, np.int32), ba


def independent_blocks(nb, bs, seed=12):
    """nb block rows, each coupled to no other (one dependency level of nb rows): (bi, bj, ba)"""
    rng = np.random.default_rng(seed)
    blocks = rng.standard_normal((nb, bs, bs)) + 3.0 * bs * np.eye(bs)
    return np.arange(nb + 1, dtype=np.int32), np.arange(nb, dtype=np.int32), np.ascontiguousarray(blocks.transpose(0, 2, 1)).ravel()


def dense_of(bs, bi, bj, ba):
    """the expanded dense matrix of a block CSR matrix with column-major blocks"""
    mbs = len(bi) - 1
    A = np.zeros((mbs * bs, mbs * bs))
    for i in range(mbs):
        for q in range(int(bi[i]), int(bi[i + 1])):
            j = int(bj[q])
            A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs] = np.asarray(ba[q * bs * bs:(q + 1) * bs * bs]).reshape(bs, bs).T
    return A
