"""The model of the matrix reductions (MatNorm, MatGetRowMaxAbs / Max / Min, MatGetRowSum, MatGetColumnNorms): plain Python loops
over a CSR matrix that state the contracts of DESIGN.md literally, one scalar at a time, no vectorised sums.  A BAIJ matrix is
modelled through its expanded point CSR (specials.bsr_to_csr: block after block, a block's columns left to right)."""
import math

import numpy as np

SUM, ABSSUM, SQSUM, MAXABS, MAX, MIN = range(6)      # MI355X_ROW_* of include/mi355x_kernels.h


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _term(op, v):
    if op in (ABSSUM, MAXABS):
        return abs(v)
    if op == SQSUM:
        return np.float64(v) * np.float64(v)
    return v


def row_sums(op, ai, aa, acc=None):
    """s_i = acc_i (or 0.0); s_i = s_i + term(a_ik), left to right in storage order"""
    m = len(ai) - 1
    out = np.zeros(m)
    with np.errstate(all="ignore"):
        for i in range(m):
            s = np.float64(0.0 if acc is None else acc[i])
            for k in range(ai[i], ai[i + 1]):
                s = s + _term(op, np.float64(aa[k]))
            out[i] = s
    return out


def row_extrema(op, ai, aj, aa, ncols):
    """(values, columns).  A strict comparison in storage order: the first of equals stays, a NaN never replaces anything and nothing
    replaces a NaN.  Max-abs starts at (0.0, 0).  Max / min: a row with fewer entries than columns starts at the implicit (0.0, its
    smallest missing column), a full row at its first entry, a row without entries gives (0.0, 0)."""
    m = len(ai) - 1
    val = np.zeros(m); idx = np.zeros(m, dtype=np.int32)
    for i in range(m):
        k0, k1 = int(ai[i]), int(ai[i + 1])
        n = k1 - k0
        cur, col = np.float64(0.0), 0
        if op != MAXABS and 0 < n < ncols:
            while col < n and aj[k0 + col] == col:
                col += 1
        for k in range(k0, k1):
            v = _term(op, np.float64(aa[k]))
            first = op != MAXABS and k == k0 and n == ncols
            if first or (v < cur if op == MIN else cur < v):
                cur, col = v, int(aj[k])
        val[i], idx[i] = cur, col
    return val, idx


def col_reduce(op, ai, aj, aa, ncols):
    """per column, its entries taken in ascending row order: sums of |a| (ABSSUM), of a * a (SQSUM), or max-abs (MAXABS)"""
    out = np.zeros(ncols)
    with np.errstate(all="ignore"):
        for i in range(len(ai) - 1):
            for k in range(ai[i], ai[i + 1]):
                v, c = _term(op, np.float64(aa[k])), aj[k]
                if op == MAXABS:
                    if out[c] < v:
                        out[c] = v
                else:
                    out[c] = out[c] + v
    return out


def vec_max(x):
    """VecMax's loop: starts from x[0], replaced on a strict >; 0.0 for no elements (the norm of a matrix without rows)"""
    if len(x) == 0:
        return 0.0
    m = x[0]
    for v in x[1:]:
        if v > m:
            m = v
    return float(m)


def norm_inf(ai, aa):
    return vec_max(row_sums(ABSSUM, ai, aa))


def norm_1(ai, aj, aa, ncols):
    return vec_max(col_reduce(ABSSUM, ai, aj, aa, ncols))


def sum_squares(aa):
    """the sequential sum of a * a over the stored values"""
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in aa:
            s = s + np.float64(v) * np.float64(v)
    return float(s)


def norm_frobenius(aa):
    return math.sqrt(sum_squares(aa))


def sum_bound(nterms, total):
    """the standard bound on a sum of nterms non-negative terms, whatever its order: (n - 1) 2^-53 times the sum"""
    return np.maximum(np.asarray(nterms) - 1, 0) * 2.0 ** -53 * total


def column_norms(kind, ai, aj, aa, ncols):
    """kind: 0 NORM_1, 1 NORM_2, 3 NORM_INFINITY"""
    if kind == 1:
        return np.sqrt(col_reduce(SQSUM, ai, aj, aa, ncols))
    return col_reduce(ABSSUM if kind == 0 else MAXABS, ai, aj, aa, ncols)


def transpose(ai, aj, aa, ncols):
    """CSR of the transpose, a row's entries in ascending original row"""
    m = len(ai) - 1
    rows = np.repeat(np.arange(m), np.diff(ai))
    o = np.argsort(aj, kind="stable")
    ti = np.concatenate(([0], np.cumsum(np.bincount(aj, minlength=ncols)))).astype(np.int32)
    return ti, rows[o].astype(np.int32), np.asarray(aa)[o]


def competing_slab_matrix(nx, ny, nz, ranges):
    """P7(nx, ny, nz) with non-constant values, rows split at `ranges`; the rows that store entries of both blocks of an MPIAIJ matrix
    are made to compete: by turns the row's maximum lies in the off-diagonal block, equal maxima lie in both blocks, nothing is
    positive (the implicit zero of the whole row), equal minima lie in both blocks"""
    import orc
    ai, aj, aa = orc.gen_p7(nx, ny, nz)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    owner = np.searchsorted(np.asarray(ranges), np.arange(n), side="right") - 1
    cross = np.flatnonzero(owner[rows] != owner[aj])
    for q, k in enumerate(cross):
        r = rows[k]
        own = np.flatnonzero((rows == r) & (owner[aj] == owner[r]))
        row = slice(int(ai[r]), int(ai[r + 1]))
        if q % 4 == 0:
            aa[k] = 9.0 + 0.01 * q
        elif q % 4 == 1:
            aa[row] = np.clip(aa[row], -7.0, 7.0); aa[k] = 7.5; aa[own[0]] = 7.5; aa[own[-1]] = -7.5
        elif q % 4 == 2:
            aa[row] = -np.abs(aa[row])
        else:
            aa[row] = np.abs(aa[row]); aa[k] = -7.5; aa[own[0]] = -7.5
    return ai, aj, aa, cross.size
