"""Host-side reference of ILU(k) (test_iluk_cpu.py checks it on its own, test_iluk_gpu.py compares the device with it); pure numpy,
nothing here touches the GPU.

  symbolic         the level-of-fill rule of MatILUFactorSymbolic_SeqAIJ with natural ordering, restated: (bi, bj, bdiag, bjlev) in the
                   layout of MatILUFactorSymbolic_SeqAIJ_ilu0 (ilufactor.layout is its levels == 0 case);
  reference_pass   ilufactor.reference_pass on a factor pattern that contains A's: the work row runs over the FACTOR's row, fill starts
                   at +0.0, one numpy operation per rounding;
  shapes           the named patterns of the tests, each with the feature it is there for."""
import functools

import numpy as np

import ilufactor as ilf
from ilufactor import MARK, _values, bits, differing  # noqa: F401 (re-exported to the two test modules)

WAVE = ilf.WAVE


# ------------------------------------------------------------------------------------------------ symbolic
def symbolic(ai, aj, levels):
    """A stored a_ij has level 0.  Row i is built in ascending row order from the sorted list of its columns: for every list column
    k < i in ascending order -- fill that entered earlier included -- incr = lev(i,k) + 1, and every strict-upper entry (k,j) of row
    k with lev(k,j) + incr <= levels enters the list with that level; an entry already there keeps the smaller level.
    Returns (bi, bj, bdiag, bjlev); bj and bjlev hold bdiag[0] + 2 ints, the last one 0."""
    n = ai.size - 1
    assert levels >= 0
    upper = []                                        # per row: [(column, level)] of the strict upper part, ascending
    lower = []
    for i in range(n):
        row = {int(c): 0 for c in aj[ai[i]:ai[i + 1]]}
        assert i in row, "row %d without its diagonal entry" % i
        done = -1
        while True:
            todo = [k for k in row if done < k < i]
            if not todo:
                break
            k = min(todo)
            done = k
            incr = row[k] + 1
            for j, lv in upper[k]:
                if lv + incr <= levels:
                    row[j] = min(row.get(j, lv + incr), lv + incr)
        lower.append(sorted((c, lv) for c, lv in row.items() if c < i))
        upper.append(sorted((c, lv) for c, lv in row.items() if c > i))
    bi = np.zeros(n + 1, np.int32); bd = np.zeros(n + 1, np.int32)
    for i in range(n):
        bi[i + 1] = bi[i] + len(lower[i])
    bd[n] = bi[n] - 1
    for i in range(n - 1, -1, -1):
        bd[i] = bd[i + 1] + len(upper[i]) + 1
    nz = int(bd[0]) + 1 if n else 0
    bj = np.zeros(nz + 1, np.int32); bl = np.zeros(nz + 1, np.int32)
    for i in range(n):
        for q, (c, lv) in enumerate(lower[i]):
            bj[bi[i] + q], bl[bi[i] + q] = c, lv
        for q, (c, lv) in enumerate(upper[i]):
            bj[bd[i + 1] + 1 + q], bl[bd[i + 1] + 1 + q] = c, lv
        bj[bd[i]] = i
    return bi, bj, bd, bl


def factor_rows(layout):
    """per row: (columns ascending, the slot of ba of each, number of L columns)"""
    bi, bj, bd = layout[:3]
    out = []
    for i in range(bi.size - 1):
        ls = np.arange(bi[i], bi[i + 1], dtype=np.int64)
        us = np.arange(bd[i + 1] + 1, bd[i], dtype=np.int64)
        slot = np.concatenate((ls, [int(bd[i])], us)).astype(np.int64)
        out.append((bj[slot].astype(np.int64), slot, ls.size))
    return out


def widest(layout):
    bi, _, bd = layout[:3]
    n = bi.size - 1
    return int((np.diff(bi) + (bd[:n] - bd[1:])).max()) if n else 1


def lanes_of(layout):
    """the smallest power of two that is at least the widest FACTOR row, capped at 64"""
    return min(WAVE, 1 << (widest(layout) - 1).bit_length())


def levels_L(layout):
    """dependency level of L of every row of the factor, and the rows sorted by it (levptr, rows)"""
    bi, bj = layout[0], layout[1]
    n = bi.size - 1
    lev = np.zeros(n, np.int64)
    for i in range(n):
        cols = bj[bi[i]:bi[i + 1]]
        lev[i] = lev[cols].max() + 1 if cols.size else 0
    nlev = int(lev.max()) + 1 if n else 0
    levptr = np.zeros(nlev + 1, np.int32)
    if n:
        levptr[1:] = np.cumsum(np.bincount(lev, minlength=nlev))
    return lev, nlev, levptr, np.argsort(lev, kind="stable").astype(np.int32)


# ------------------------------------------------------------------------------------------------ the reference of one pass
def reference_pass(ai, aj, aa, blk, shifts, zeropivot, pending, ba=None, layout=None):
    """ilufactor.reference_pass on a factor pattern that contains A's (layout = (bi, bj, bdiag[, bjlev]); None: A's own pattern).
    One call of mi355x_ilu0_factor_run on a context made by mi355x_ilu0_factor_create_fill: every pending block is factored row by
    row as the sequential loop does -- the work row is the factor's row, A's entries scattered into it and +0.0 where A stores none,
    the block's shift added to the diagonal (also a shift of 0.0), the L columns of the FACTOR in order with `work value != 0.0` (a
    fill entry nothing has touched is skipped), m = w * inverted pivot, w_j = w_j - m * u_kj with two roundings for the strict-upper
    entries of row k whose column is in row i's factor pattern, rs over L then U in storage order, |w_i| <= zeropivot * rs -- and
    stops at its first failing row, whose L and U values are stored and whose pivot slot holds |w_i|.  A block that is not pending
    is not touched.  Returns (ba, failing row per block or -1, |w_i| of that row or 0.0, the new pending state)."""
    n = ai.size - 1
    layout = ilf.layout(ai, aj) if layout is None else layout
    bi, bj, bd = layout[:3]
    nz = int(bd[0]) + 1 if n else 0
    rows = factor_rows(layout)
    ba = np.zeros(nz + 1) if ba is None else np.array(ba, dtype=np.float64)
    blk = [0, n] if blk is None else [int(b) for b in blk]
    nblk = len(blk) - 1
    frow, fabs_, pend = np.full(nblk, -1, np.int32), np.zeros(nblk), np.array(pending, dtype=np.int32).copy()
    mul, sub, add, div, absf = np.multiply, np.subtract, np.add, np.divide, np.abs
    zp = np.float64(zeropivot)
    with np.errstate(all="ignore"):
        for b in range(nblk):
            if not pend[b]:
                continue
            sh = np.float64(shifts[b])
            failed = False
            for i in range(blk[b], blk[b + 1]):
                cols, slot, nl = rows[i]
                pos = {int(c): p for p, c in enumerate(cols)}
                w = np.zeros(cols.size)
                for q in range(int(ai[i]), int(ai[i + 1])):
                    w[pos[int(aj[q])]] = aa[q]
                w[nl] = add(w[nl], sh)
                for kk in range(nl):
                    k = int(cols[kk])
                    if w[kk] != 0.0:
                        m = mul(w[kk], ba[bd[k]])
                        w[kk] = m
                        for q in range(int(bd[k + 1]) + 1, int(bd[k])):
                            p = pos.get(int(bj[q]))
                            if p is not None:
                                w[p] = sub(w[p], mul(m, ba[q]))
                rs = np.float64(0.0)
                for p in range(cols.size):
                    if p != nl:
                        rs = add(rs, absf(w[p]))
                ba[slot] = w
                if absf(w[nl]) <= mul(zp, rs):
                    frow[b], fabs_[b], failed = i, absf(w[nl]), True
                    ba[bd[i]] = absf(w[nl])
                    break
                ba[bd[i]] = div(np.float64(1.0), w[nl])
            if not failed:
                pend[b] = 0
    return ba, frow, fabs_, pend


def row_slots(layout, mask):
    """bool over ba: the slots of the factor rows in `mask`"""
    nz = int(layout[2][0]) + 1
    out = np.zeros(nz + 1, dtype=bool)
    for i, (_, slot, _) in enumerate(factor_rows(layout)):
        if mask[i]:
            out[slot] = True
    return out


def compared_slots(layout, blk, frow):
    """ilufactor.compared_slots on the factor's pattern: a block that passed: all of its rows; a block that failed: the earlier rows
    of the levels before the failing row's level and that row itself.  Slot nz is nobody's."""
    n = layout[0].size - 1
    blk = [0, n] if blk is None else blk
    lev = levels_L(layout)[0]
    keep = np.zeros(n, dtype=bool)
    for b in range(len(blk) - 1):
        r = np.arange(blk[b], blk[b + 1])
        keep[r] = True if frow[b] < 0 else (((r < frow[b]) & (lev[r] < lev[frow[b]])) | (r == frow[b]))
    return row_slots(layout, keep)


# ------------------------------------------------------------------------------------------------ shapes
def pattern_of(ai, aj):
    return [[int(c) for c in aj[ai[i]:ai[i + 1]]] for i in range(ai.size - 1)]


def p7_pattern(nx, ny, nz):
    """the 7-point operator on an nx x ny x nz grid, x fastest"""
    pat = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                i = x + nx * (y + ny * z)
                p = [i]
                p += [i - 1] if x else []
                p += [i + 1] if x + 1 < nx else []
                p += [i - nx] if y else []
                p += [i + nx] if y + 1 < ny else []
                p += [i - nx * ny] if z else []
                p += [i + nx * ny] if z + 1 < nz else []
                pat.append(sorted(p))
    return pat


def random_pattern(n, seed, per_row=4):
    """non-symmetric: every row its diagonal and up to per_row columns drawn anywhere; every 37th row the diagonal alone"""
    rng = np.random.default_rng(seed)
    pat = []
    for i in range(n):
        extra = set() if i % 37 == 0 else {int(c) for c in rng.integers(0, n, size=int(rng.integers(1, per_row + 1)))}
        pat.append(sorted(extra | {i}))
    return pat


def _fill_wide_pattern():
    """A's rows have at most 41 entries; rows 0, 1, 2 hold 40 strict-upper columns each (three disjoint sets), and the rows that
    name two or three of them gain those columns as fill of level 1 -- rows 10 and 12 in their U part, rows 150, 151, 200 and 259
    in their L part, where every fill entry is then a multiplier: factor rows of 80 .. 125 entries, wider than a wavefront, next
    to register rows.  260 rows."""
    n = 260
    rng = np.random.default_rng(31)
    pat = [[i] for i in range(n)]
    for h in range(3):
        pat[h] = [h] + [int(c) for c in range(20 + h, 140, 3)]
    hubs = {10: (0, 1, 2), 12: (0, 1), 150: (0, 1), 151: (0, 1), 200: (0, 1, 2), 259: (0, 1)}
    for i in range(3, n):
        if i in hubs:
            pat[i] = sorted(set(hubs[i]) | {i} | {c for c in (i + 2, i + 5, i + 9) if c < n})
        elif i % 5:
            pat[i] = sorted({int(rng.integers(3, i + 1)), i, min(n - 1, i + 1 + int(rng.integers(0, 7)))})
    return pat


UCHUNK_FILL = {3: (0, 10 + 2 * np.arange(40), 11 + 2 * np.arange(24)),       # row k: (the row its L entry names, that row's U, k's own U)
               4: (1, 10 + 2 * np.arange(40), 11 + 2 * np.arange(25)),
               5: (2, 150 + np.arange(100), 250 + np.arange(28))}
UCHUNK_SIZES = {3: 64, 4: 65, 5: 128}


def _uchunk_fill_pattern():
    """rows 3, 4, 5 whose strict-upper parts reach exactly 64, 65 and 128 entries only AFTER fill of level 1 (stored and fill
    columns interleaved); later rows whose L entry names one of them and that hold columns at the chunk edges of U(k) -- its first,
    64th, 65th and last -- and columns U(k) lacks; row 290 names all three"""
    n = 300
    pat = [[i] for i in range(n)]
    for k, (src, donor, own) in UCHUNK_FILL.items():
        pat[src] = [src] + [int(c) for c in donor]
        pat[k] = sorted({src, k} | {int(c) for c in own})
    def uk(k):
        return np.sort(np.concatenate((UCHUNK_FILL[k][1], UCHUNK_FILL[k][2])))
    for k, t, i, extra in [(3, 0, 9, (13,)), (3, 63, 136, (141,)), (4, 0, 12, (14, 16)), (4, 63, 135, (140,)), (4, 64, 139, (142, 144)),
                           (5, 0, 149, (279,)), (5, 63, 213, (280, 281)), (5, 64, 215, (282,)), (5, 127, 276, (283,)), (5, 64, 214, (284,))]:
        pat[i] = sorted(set(pat[i]) | {k, i, int(uk(k)[t])} | set(extra))
    pat[290] = sorted({3, 4, 5, 290} | {int(c) for c in uk(5)[60:70]} | {136, 139, 291, 292, 295})
    return pat


def _csr_of(pattern_or_rows):
    return ilf._csr(pattern_or_rows)


def skipped_fill_case():
    """levels = 1.  Fill entries (2,1) and (3,1) are fed by the stored u_01 = 0.0 alone: 0 - m * 0.0 = +0.0, so the multiplier
    through row 1 must be skipped (row 1's pivot is NEGATIVE: a multiplier formed all the same would be stored as -0.0).  Next to
    it the fill entry (3,2) becomes -0.5 and IS a multiplier, against row 2 whose U part holds the fill entry (2,5)."""
    return ilf._csr([[(0, 2.0), (1, 0.0), (2, 1.0), (5, 1.0)],
                     [(1, -4.0), (3, 1.0)],
                     [(0, 1.0), (2, 3.0), (4, 1.0)],
                     [(0, 1.0), (3, 5.0), (4, 0.5)],
                     [(4, 2.0)],
                     [(5, 2.0)]])


@functools.lru_cache(maxsize=None)
def shape(name):
    """(ai, aj, aa) with a strictly row-dominant diagonal (ilufactor._values)"""
    import problems as pb
    if name == "lap2d":
        return _values(pattern_of(*pb.lap2d(9, 7)[:2]), 41)
    if name == "p7":
        return _values(p7_pattern(7, 6, 5), 42)
    if name == "ex10":
        return _values(pattern_of(*pb.ex10_elasticity()[0][:2]), 43)
    if name == "random":
        return _values(random_pattern(300, 44), 44)
    if name == "fill_wide":
        return _values(_fill_wide_pattern(), 45)
    if name == "a_wide":
        return ilf.shape("mini_wide")
    if name == "uchunk_fill":
        return _values(_uchunk_fill_pattern(), 46)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def layout_of(name, levels):
    ai, aj, _ = shape(name)
    return symbolic(ai, aj, levels)


@functools.lru_cache(maxsize=None)
def clean_factor(name, levels):
    """reference_pass of the shape with zero shift and the default zeropivot: (ba, failing rows)"""
    ai, aj, aa = shape(name)
    ba, frow, _, _ = reference_pass(ai, aj, aa, None, [0.0], ilf.ZP, [1], layout=layout_of(name, levels))
    return ba, frow


# ------------------------------------------------------------------------------------------------ blocks over three passes
NBLOCKS = 40
BLOCK_ROWS = 7


@functools.lru_cache(maxsize=None)
def blocks_case():
    """ilufactor.blocks_case on a fill pattern, levels = 1.  40 blocks, kind b % 5.  Kinds 0 and 3: 7 rows, row r holds columns 0,
    r - 1, r, r + 1 and row 0 holds them all -- fill of level 1 makes every row of the block full, and every row's L part names the
    row before it, so the rows of a block are a chain of levels and the first failing row is the one any schedule reports.  Kind 0:
    diagonal 8 + b / 4, off-diagonals -1 (passes at once); kind 3: all values 1 (a zero pivot in its second row; fails again with
    the tiny shift; passes with the large one).  Kind 1: an empty range; kind 2: one row of value 0.0; kind 4: one row of value 3.
    Three passes as the plug-in drives them: shift 0; a failed block gets 100 eps (1 + b % 3) / 64; a block that failed again gets
    0.05 (b + 1).  After pass 1 the slots of the finished blocks are overwritten with the marker.
    Returns dict(ai, aj, aa, blk, layout, passes: [(shifts, ba after the pass, failing rows, failed_abs, pending after it)],
    finished1: slots of the blocks finished in pass 1)."""
    rows, blk = [], [0]
    m = BLOCK_ROWS
    for b in range(NBLOCKS):
        o, kind = len(rows), b % 5
        if kind in (0, 3):
            di, off = (8.0 + 0.25 * b, -1.0) if kind == 0 else (1.0, 1.0)
            for r in range(m):
                cols = range(m) if r == 0 else sorted({0, r - 1, r, min(r + 1, m - 1)})
                rows.append([(o + c, di if c == r else off) for c in cols])
        elif kind in (2, 4):
            rows.append([(o, 0.0 if kind == 2 else 3.0)])
        blk.append(len(rows))
    ai, aj, aa = ilf._csr(rows)
    blk = np.array(blk, np.int32)
    lay = symbolic(ai, aj, 1)
    inblock = np.repeat(np.arange(NBLOCKS), np.diff(blk))
    nz = int(lay[2][0]) + 1
    shifts, pend, ba = np.zeros(NBLOCKS), np.ones(NBLOCKS, np.int32), np.zeros(nz + 1)
    passes, finished1 = [], None
    for ps in range(3):
        ba, frow, fabs_, pend = reference_pass(ai, aj, aa, blk, shifts, ilf.ZP, pend, ba, layout=lay)
        if ps == 0:
            finished1 = row_slots(lay, (pend == 0)[inblock])
            ba[finished1] = MARK
        passes.append((shifts.copy(), ba.copy(), frow, fabs_, pend.copy()))
        for b in np.flatnonzero(frow >= 0):
            shifts[b] = ilf.ZP * (1 + b % 3) / 64.0 if ps == 0 else 0.05 * (b + 1)
    return dict(ai=ai, aj=aj, aa=aa, blk=blk, layout=lay, passes=passes, finished1=finished1)


# ------------------------------------------------------------------------------------------------ complete LU, independently
def full_lu_pattern(ai, aj):
    """the pattern of complete LU by boolean elimination of the dense pattern: bool (n, n)"""
    n = ai.size - 1
    S = np.zeros((n, n), dtype=bool)
    S[np.repeat(np.arange(n), np.diff(ai)), aj] = True
    for k in range(n):
        below = np.flatnonzero(S[k + 1:, k]) + k + 1
        S[np.ix_(below, np.arange(k + 1, n))] |= S[k, k + 1:]
    return S


def dense_pattern(layout):
    n = layout[0].size - 1
    S = np.zeros((n, n), dtype=bool)
    for i, (cols, _, _) in enumerate(factor_rows(layout)):
        S[i, cols] = True
    return S


def dense_factors(layout, ba):
    """(L with its unit diagonal, U) as dense matrices from the factor's arrays (pivots stored inverted)"""
    n = layout[0].size - 1
    L, U = np.eye(n), np.zeros((n, n))
    for i, (cols, slot, nl) in enumerate(factor_rows(layout)):
        L[i, cols[:nl]] = ba[slot[:nl]]
        U[i, cols[nl + 1:]] = ba[slot[nl + 1:]]
        U[i, i] = 1.0 / ba[slot[nl]]
    return L, U
