"""Host-side machinery of the device ILU(0) factorisation's lane-width / IEEE-special / containment tests
(test_ilu_factor_specials_gpu.py), checked on its own by test_ilu_factor_specials_cpu.py (which holds the comparisons with the oracle); pure
numpy, nothing here touches the GPU.

csrc/ilu_factor.hip factors a row of <= W entries in registers (W = 1 .. 64 lanes per row, from the widest row) and a wider row in
place in ba, matches U(k) to the row's columns by a shuffle binary search over chunks of W entries, skips a multiplier whose work
value is 0.0, tests |w_i| <= zeropivot * rs and reports a failing row per block.  What is here:
  reference_pass   one call of mi355x_ilu0_factor_run restated with numpy float64 scalars, one explicit operation per rounding;
  SHAPES           named, deterministic patterns, one per lane width and per path, each with the features it is there for;
  special_cases    hand-built matrices of IEEE special cases with the class of every factor entry stated, in three row forms;
  containment      four independent sub-blocks factored as one block, a special in one row, the rows it can reach from the graph;
  failure cases    one failing row per block, about 40 blocks over three passes, several failing rows in one block."""
import functools

import numpy as np

from vecspecials import bits, differing  # noqa: F401 (re-exported to the two test modules)

EPS = 2.220446049250313e-16
ZP = 100.0 * EPS                        # PCILU's default zeropivot
WAVE, BLOCK = 64, 256                   # MI355X_WAVE, MI355X_BLOCK
MARK = -7.25e300                        # the marker of guard bands, of slot nz and of a finished block's overwritten values
BAND = 64                               # doubles of marker on either side of a guarded array
NAN, INF = np.nan, np.inf


# ------------------------------------------------------------------------------------------------ layout and graph
def layout(ai, aj):
    """(bi, bj, bdiag) of MatILUFactorSymbolic_SeqAIJ_ilu0 from A's sorted CSR pattern with a full diagonal"""
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    nzl = np.bincount(rows[aj < rows], minlength=n).astype(np.int64)
    assert np.array_equal(aj[ai[:-1] + nzl], np.arange(n)), "a row without its diagonal entry"
    nzu = np.diff(ai) - nzl - 1
    bi = np.zeros(n + 1, np.int32); bi[1:] = np.cumsum(nzl)
    bd = np.zeros(n + 1, np.int32); bd[n] = bi[n] - 1
    bd[:n] = bd[n] + np.cumsum((nzu + 1)[::-1])[::-1]
    bj = np.zeros(int(ai[-1]) + 1, np.int32)
    bj[slots(ai, aj)] = aj
    return bi, bj, bd


def slots(ai, aj):
    """the slot of ba that every entry of A's CSR goes to"""
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    nzl = np.bincount(rows[aj < rows], minlength=n).astype(np.int64)
    nzu = np.diff(ai) - nzl - 1
    bil = np.concatenate(([0], np.cumsum(nzl)))
    bd = np.zeros(n + 1, np.int64); bd[n] = bil[n] - 1
    bd[:n] = bd[n] + np.cumsum((nzu + 1)[::-1])[::-1]
    p = np.arange(aj.size) - np.repeat(ai[:-1], np.diff(ai))
    nl = nzl[rows]
    return np.where(p < nl, bil[rows] + p, np.where(p == nl, bd[rows], bd[rows + 1] + p - nl)).astype(np.int64)


def nzl_of(ai, aj):
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    return np.bincount(rows[aj < rows], minlength=ai.size - 1).astype(np.int64)


def levels(ai, aj):
    """dependency level of L of every row"""
    n = ai.size - 1
    nzl = nzl_of(ai, aj)
    lev = np.zeros(n, np.int64)
    for i in range(n):
        if nzl[i]:
            lev[i] = lev[aj[ai[i]:ai[i] + nzl[i]]].max() + 1
    return lev


def tame(ai, aj):
    """diagonally dominant values on the pattern: what the layout is taken from when A's values are not finite"""
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    return np.where(aj == rows, np.repeat(np.diff(ai), np.diff(ai)) + 1.0, 1.0)


def lanes_of(ai):
    return min(WAVE, 1 << (int(np.diff(ai).max()) - 1).bit_length())


# ------------------------------------------------------------------------------------------------ the reference of one pass
def reference_pass(ai, aj, aa, blk, shifts, zeropivot, pending, ba=None):
    """One call of mi355x_ilu0_factor_run: every pending block is factored row by row as the sequential loop does
    (oracle/ksp_oracle.c, orc_ilu0_factor_shift: scatter, the block's shift added to the diagonal -- also a shift of 0.0 --, the L
    columns in order with `work value != 0.0`, m = w * inverted pivot, w_j = w_j - m * u_kj with two roundings, rs over L then U in
    storage order, |w_i| <= zeropivot * rs) and stops at its first failing row, whose L and U values are stored and whose pivot slot
    holds |w_i|.  A block that is not pending is not touched.  Returns (ba, failing row per block or -1, |w_i| of that row or 0.0,
    the new pending state); `ba` continues from the array handed in (zeros without one)."""
    n, nz = ai.size - 1, int(ai[-1])
    bi, bj, bd = layout(ai, aj)
    slot = slots(ai, aj)
    nzl = nzl_of(ai, aj)
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
                a0, a1, nl = int(ai[i]), int(ai[i + 1]), int(nzl[i])
                cols = aj[a0:a1]
                w = np.array(aa[a0:a1], dtype=np.float64)
                pos = {int(c): p for p, c in enumerate(cols)}
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
                for p in range(a1 - a0):
                    if p != nl:
                        rs = add(rs, absf(w[p]))
                ba[slot[a0:a1]] = w
                if absf(w[nl]) <= mul(zp, rs):
                    frow[b], fabs_[b], failed = i, absf(w[nl]), True
                    ba[bd[i]] = absf(w[nl])
                    break
                ba[bd[i]] = div(np.float64(1.0), w[nl])
            if not failed:
                pend[b] = 0
    return ba, frow, fabs_, pend


def compared_slots(ai, aj, blk, frow):
    """bool over ba[0 .. nz]: the slots one pass defines.  A block that passed: all of its rows; a block that failed with ONE
    failing row: the earlier rows of the levels before that row's level (they all ran, on the device too) and the row itself; later
    rows are not the reference's, earlier rows of the same or a later level may have been skipped on the device.  Slot nz is nobody's."""
    n = ai.size - 1
    blk = [0, n] if blk is None else blk
    lev, slot = levels(ai, aj), slots(ai, aj)
    rows = np.repeat(np.arange(n), np.diff(ai))
    keep = np.zeros(n, dtype=bool)
    for b in range(len(blk) - 1):
        r = np.arange(blk[b], blk[b + 1])
        keep[r] = True if frow[b] < 0 else (((r < frow[b]) & (lev[r] < lev[frow[b]])) | (r == frow[b]))
    out = np.zeros(int(ai[-1]) + 1, dtype=bool)
    out[slot[keep[rows]]] = True
    return out


def rule_violations(got, ref):
    """the comparison rule: the same bits where the reference is finite (+-0.0 and subnormals included) or +-Inf, a NaN where it is NaN"""
    return differing(got, ref)


# ------------------------------------------------------------------------------------------------ shapes
def _values(pattern, seed, negative=()):
    """CSR of the pattern (sorted column lists holding the diagonal): off-diagonal values of magnitude 0.25 .. 1 and either sign,
    a dominant diagonal (negative in the rows `negative`)"""
    rng = np.random.default_rng(seed)
    n = len(pattern)
    ai = np.zeros(n + 1, np.int32); ai[1:] = np.cumsum([len(p) for p in pattern])
    aj = np.concatenate([np.asarray(p, dtype=np.int32) for p in pattern]).astype(np.int32)
    aa = rng.uniform(0.25, 1.0, aj.size) * rng.choice([-1.0, 1.0], aj.size)
    rows = np.repeat(np.arange(n), np.diff(ai))
    d = np.flatnonzero(aj == rows)
    assert d.size == n and all(np.all(np.diff(p) > 0) for p in pattern if len(p) > 1)
    off = np.abs(aa); off[d] = 0.0
    aa[d] = np.add.reduceat(off, ai[:-1]) + 1.0 + rng.uniform(0.0, 1.0, n)
    aa[d[np.asarray(negative, dtype=np.int64)]] *= -1.0
    return ai, aj, aa


def _pick(rng, cand, k, forced=()):
    cand = [c for c in cand if c not in forced]
    k -= len(forced)
    assert 0 <= k <= len(cand), (k, len(cand))
    return sorted(list(forced) + [int(c) for c in rng.choice(cand, size=k, replace=False)]) if k else sorted(forced)


def _rows_from_spec(n, spec, hubs, seed):
    """spec[i] = (row length, nzl, L columns it must hold, U columns it must hold); the other L columns are drawn from `hubs`
    of row i (so that the levels stay few), the other U columns from all later rows"""
    rng = np.random.default_rng(seed)
    pattern = []
    for i in range(n):
        ln, nl, fl, fu = spec[i]
        L = _pick(rng, [h for h in hubs(i) if h < i], nl, tuple(fl))
        U = _pick(rng, range(i + 1, n), ln - 1 - nl, tuple(fu))
        pattern.append(L + [i] + U)
    return pattern


def _chains(n, k, lower, upper):
    """chains of k rows (the last one 2 k rows): lower and / or upper neighbour inside a chain"""
    last = n - 2 * k
    start = lambda i: i >= last and i == last or i < last and i % k == 0       # noqa: E731
    pattern = []
    for i in range(n):
        p = [i]
        if lower and not start(i):
            p.insert(0, i - 1)
        if upper and i + 1 < n and not start(i + 1):
            p.append(i + 1)
        pattern.append(p)
    return pattern


def _lane_shape(W, seed):
    """rows of exactly W and of W / 2 + 1 entries among shorter ones; m0 rows of level 0, m1 rows of level 1 that name them, a
    chain of four single-row levels at the end"""
    m0 = max(BLOCK // W + 12, W + 6)
    n = 2 * m0 + 4
    lens = [W, W // 2 + 1, 1, max(2, W // 4), W - 1, 63 if W == 64 else 2]
    spec = []
    for i in range(n):
        ln = lens[i % len(lens)]
        right = n - 1 - i
        if i < m0:
            spec.append((min(ln, right + 1), 0, (), ()))
        elif i < 2 * m0:
            nl = 0 if ln == 1 else (1, ln - 1, ln // 2)[i % 3]
            nl = max(nl, ln - 1 - right)
            spec.append((ln, nl, (), ()))
        else:
            ln = W if i in (2 * m0, n - 1) else W // 2 + 1
            nl = max(1, ln - 1 - right)
            spec.append((ln, nl, (i - 1,), ()))
    return _values(_rows_from_spec(n, spec, lambda i: range(m0), seed), seed)


# (row, row length, nzl, wide rows its L columns must name)
WIDE_ROWS = [(5, 65, 0, ()), (70, 128, 63, (5,)), (100, 129, 64, (70,)), (120, 150, 65, (70, 100)), (200, 65, 64, (100, 120)),
             (250, 129, 128, (120, 200)), (329, 150, 149, (5, 70, 100, 120, 200, 250))]
MINI_WIDE_ROWS = [(3, 65, 0, ()), (70, 100, 64, (3,)), (139, 80, 79, (3, 70))]


def _wide_shape(n, wides, seed):
    """rows wider than a wavefront among rows of 1 .. 9 entries; the narrow rows' L columns name rows 0 .. 59 (level 0) and the wide
    rows, the wide rows' L columns those and each other"""
    wide = {r: (ln, nl, fl) for r, ln, nl, fl in wides}
    lens = [1, 2, 3, 5, 9]
    spec = []
    for i in range(n):
        right = n - 1 - i
        if i in wide:
            ln, nl, fl = wide[i]
            spec.append((ln, nl, fl, ()))
            continue
        ln = min(lens[i % 5], 1 + right + (0 if i < 60 else 2))
        before = [w for w in wide if w < i]
        if i < 60 or ln == 1:
            spec.append((min(ln, right + 1), 0, (), ()))
        else:
            nl = max(min(ln - 1, 1 + i % 2), ln - 1 - right)
            spec.append((ln, nl, (before[i % len(before)],) if before else (), ()))
    # narrow rows name only the rows before 60 and the wide rows, wide rows any earlier row: the levels stay few
    few = sorted(set(range(60)) | set(wide))
    return _values(_rows_from_spec(n, spec, lambda i: range(n) if i in wide else few, seed), seed)


UCHUNK_K = {0: 10 + 2 * np.arange(64), 1: 11 + 2 * np.arange(65), 2: 150 + np.arange(128)}     # row k -> its strict-upper columns
# (row k, position t in U(k) of the shared column, the register row i, i's further columns)
UCHUNK_ROWS = [(0, 0, 9, (13,)), (0, 63, 136, (141,)), (1, 0, 12, (14, 16)), (1, 63, 135, (140,)), (1, 64, 139, (142, 144)),
               (2, 0, 149, (279,)), (2, 63, 213, (280, 281)), (2, 64, 215, (282,)), (2, 127, 276, (283,)), (2, 64, 214, (284,))]


def _uchunk_shape(seed):
    """rows 0, 1, 2 with exactly 64, 65 and 128 strict-upper entries; register rows whose L column names one of them and that share
    the column at position 0 / 63 / 64 / last of U(k) -- as a U column, as the diagonal or as an L column -- and hold columns U(k)
    lacks; row 290 names all three"""
    n = 300
    pattern = [[i] for i in range(n)]
    for k, cols in UCHUNK_K.items():
        pattern[k] = [k] + [int(c) for c in cols]
    for k, t, i, extra in UCHUNK_ROWS:
        pattern[i] = sorted({k, i, int(UCHUNK_K[k][t])} | set(extra))
    pattern[290] = sorted({0, 1, 2, 290} | {int(c) for c in UCHUNK_K[2][60:70]} | {136, 139, 291, 292, 295})
    return _values(pattern, seed)


def _csr(rows):
    ai = np.zeros(len(rows) + 1, np.int32); ai[1:] = np.cumsum([len(r) for r in rows])
    aj = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    aa = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return ai, aj, aa


def _zeros_narrow():
    """stored +0.0 and -0.0 in L positions whose row k has a NEGATIVE pivot (a multiplier formed all the same is a zero of the other
    sign), a work value that cancels to +0.0 before its turn (row 5, column 4: 2 - 2 * 1), a zero in U(3)"""
    return _csr([[(0, -2.0), (1, 1.0), (2, 0.5)],
                 [(0, 0.0), (1, 4.0), (2, 1.0)],
                 [(0, -0.0), (1, 1.0), (2, 5.0), (3, 1.0)],
                 [(3, 2.0), (4, 1.0), (5, 0.0)],
                 [(4, -3.0), (5, 1.0)],
                 [(3, 4.0), (4, 2.0), (5, 3.0), (6, 1.0)],
                 [(6, 1.0)]])


def _zeros_wide():
    """the same in a row wider than a wavefront (row 100: 80 L columns, 31 U columns): stored zeros at positions 0, 3, 64 and 70,
    the cancellation at position 65 (row 10 holds column 65: 8 * -0.25 = -2, -2 - (-2 * 1) = +0.0), a zero in U(20)"""
    n = 200
    rows = [[(i, -4.0), (150, 1.0)] if i < 80 else [(i, 3.0)] for i in range(n)]
    rows[10] = [(10, -4.0), (65, 1.0), (150, 1.0)]
    rows[20] = [(20, -4.0), (150, 0.0)]
    rng = np.random.default_rng(5)
    lv = rng.uniform(0.25, 1.0, 80) * rng.choice([-1.0, 1.0], 80)
    lv[0], lv[3], lv[64], lv[70], lv[10], lv[65] = 0.0, -0.0, 0.0, -0.0, 8.0, -2.0
    rows[100] = [(k, float(lv[k])) for k in range(80)] + [(100, 90.0)] + [(c, 0.5) for c in range(120, 151)]
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "diagonal":
        return _values([[i] for i in range(300)], 1)
    if name == "lower_bidiagonal":
        return _values(_chains(568, 4, True, False), 2)
    if name == "upper_bidiagonal":
        return _values(_chains(300, 4, False, True), 3)
    if name == "tridiagonal":
        return _values(_chains(288, 4, True, True), 4)
    if name.startswith("rows"):
        return _lane_shape(int(name[4:]), 10 + int(name[4:]))
    if name == "wide":
        return _wide_shape(330, WIDE_ROWS, 21)
    if name == "mini_wide":
        return _wide_shape(140, MINI_WIDE_ROWS, 22)
    if name == "uchunk":
        return _uchunk_shape(23)
    if name == "zeros_narrow":
        return _zeros_narrow()
    if name == "zeros_wide":
        return _zeros_wide()
    raise KeyError(name)


# name -> (lanes, does a row wider than a wavefront exist)
SHAPES = {"diagonal": (1, False), "lower_bidiagonal": (2, False), "upper_bidiagonal": (2, False), "tridiagonal": (4, False),
          "rows4": (4, False), "rows8": (8, False), "rows16": (16, False), "rows32": (32, False), "rows64": (64, False),
          "wide": (64, True), "uchunk": (64, True), "zeros_narrow": (4, False), "zeros_wide": (64, True)}
LANE_SHAPES = ["diagonal", "lower_bidiagonal", "upper_bidiagonal", "tridiagonal", "rows4", "rows8", "rows16", "rows32", "rows64"]
ONE_LEVEL = ("diagonal", "upper_bidiagonal")       # no L entry at all: one level, which is the level of many rows
SWEEP_SHAPES = ["diagonal", "upper_bidiagonal", "tridiagonal", "rows8", "rows16", "rows32", "rows64", "wide"]


@functools.lru_cache(maxsize=None)
def clean_factor(name):
    """reference_pass of the shape with zero shift and the default zeropivot: (ba, failing rows)"""
    ai, aj, aa = shape(name)
    ba, frow, _, _ = reference_pass(ai, aj, aa, None, [0.0], ZP, [1])
    return ba, frow


ZP_LARGE = 0.75
LARGE_ZP_SHAPES = ["rows4", "rows64", "wide"]


@functools.lru_cache(maxsize=None)
def large_zeropivot_case(name):
    """zeropivot is the caller's: with 0.75 a dominant pivot (|w_i| > rs) still passes, and |w_i| <= 0.75 (rs + |w_i|) -- the test
    with the pivot inside rs -- holds for every row with |w_i| <= 3 rs.  Returns (ba, failing rows, number of such rows)."""
    ai, aj, aa = shape(name)
    ba, frow, _, _ = reference_pass(ai, aj, aa, None, [0.0], ZP_LARGE, [1])
    bd, slot = layout(ai, aj)[2], slots(ai, aj)
    n = ai.size - 1
    w = np.abs(1.0 / ba[bd[:n]])
    rs = np.add.reduceat(np.abs(ba[slot]), ai[:-1]) - np.abs(ba[bd[:n]])
    return ba, frow, int((w <= 3.0 * rs).sum())


# ------------------------------------------------------------------------------------------------ IEEE specials, hand-built
T_SUB = 2.0 ** -1030            # a subnormal pivot: 1 / T_SUB overflows
FORMS = ["narrow", "reg64", "wide"]
PAD = 64                        # U columns a core row gains in the wide form


def classify(v):
    v = float(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0.0:
        return "-0" if np.signbit(v) else "+0"
    return "sub" if abs(v) < 2.2250738585072014e-308 else "fin"


def _case(name, rows, shift, default, zero):
    """default / zero: (failing row or -1, class of |w_i| or None, the class of every factor entry row by row in A's column order --
    the pivot's slot holds the inverted pivot, or |w_i| in the failing row; None for a row after the failing row) with the default
    zeropivot and with zeropivot = 0"""
    return dict(name=name, rows=rows, shift=shift, expect={"default": default, "zero": zero})


def special_cases():
    F3 = ["fin", "fin", "fin"]
    r0 = [(0, 2.0), (1, 1.0), (2, 1.0)]
    out = []
    # --- NaN / +-Inf in an L position of A (row 1, column 0).  m = x * 0.5; w_1 = 4 - m, w_2 = 1 - m.
    out.append(_case("nan_in_L", [r0, [(0, NAN), (1, 4.0), (2, 1.0)], [(1, 1.0), (2, 3.0)]], 0.0,
                     *[(-1, None, [F3, ["nan"] * 3, ["nan", "nan"]])] * 2))            # the NaN pivot passes and is stored as 1 / NaN
    # +Inf: w_1 = w_2 = -Inf, rs = Inf: |w_1| <= 100 eps * Inf fails; with zeropivot 0 the bound is NaN, the pivot passes and is stored as
    # 1 / -Inf = -0.0; row 2's multiplier through it is 1 * -0.0, and -0.0 * u_12 = -0.0 * -Inf is NaN
    out.append(_case("pinf_in_L", [r0, [(0, INF), (1, 4.0), (2, 1.0)], [(1, 1.0), (2, 3.0)]], 0.0,
                     (1, "+inf", [F3, ["+inf", "+inf", "-inf"], None]), (-1, None, [F3, ["+inf", "-0", "-inf"], ["-0", "nan"]])))
    out.append(_case("ninf_in_L", [r0, [(0, -INF), (1, 4.0), (2, 1.0)], [(1, 1.0), (2, 3.0)]], 0.0,
                     (1, "+inf", [F3, ["-inf", "+inf", "+inf"], None]), (-1, None, [F3, ["-inf", "+0", "+inf"], ["+0", "nan"]])))
    # --- NaN / +-Inf in a U position of A (row 0, column 1).  Row 2 names row 0 and lacks column 1: the fill is discarded.
    lower = [[(0, 1.0), (1, 4.0), (2, 1.0)], [(0, 1.0), (2, 3.0)], [(1, 5.0), (3, 7.0)]]
    out.append(_case("nan_in_U", [[(0, 2.0), (1, NAN), (2, 1.0)]] + lower, 0.0,
                     *[(-1, None, [["fin", "nan", "fin"], ["fin", "nan", "fin"], ["fin", "fin"], ["nan", "fin"]])] * 2))
    # an Inf in rs: the finite pivot 2 fails with the default zeropivot and passes with 0 (0 * Inf is NaN); row 1's pivot is then
    # 4 - 0.5 * +-Inf, stored as -+0.0, and row 3's multiplier through it is 5 * -+0.0
    out.append(_case("pinf_in_U", [[(0, 2.0), (1, INF), (2, 1.0)]] + lower, 0.0,
                     (0, "fin", [["fin", "+inf", "fin"], None, None, None]),
                     (-1, None, [["fin", "+inf", "fin"], ["fin", "-0", "fin"], ["fin", "fin"], ["-0", "fin"]])))
    out.append(_case("ninf_in_U", [[(0, 2.0), (1, -INF), (2, 1.0)]] + lower, 0.0,
                     (0, "fin", [["fin", "-inf", "fin"], None, None, None]),
                     (-1, None, [["fin", "-inf", "fin"], ["fin", "+0", "fin"], ["fin", "fin"], ["+0", "fin"]])))
    # --- the skip next to a special: row 0's pivot is subnormal with rs = 0 (its U entry is a stored 0.0): it passes and inverts to
    # +Inf.  Rows 1 and 2 hold a stored zero in the L position that names row 0: skipped, they stay finite (0 * Inf would be NaN).
    # Row 3's L entry 1.0 is not skipped: m = +Inf, w_2 = 1 - Inf * 0.0 = NaN, and the NaN is the next multiplier
    out.append(_case("skip_next_to_inf", [[(0, T_SUB), (2, 0.0)], [(0, 0.0), (1, 4.0), (2, 1.0)], [(0, -0.0), (2, 3.0)], [(0, 1.0), (2, 1.0), (3, 5.0)]], 0.0,
                     *[(-1, None, [["+inf", "+0"], ["+0", "fin", "fin"], ["-0", "fin"], ["+inf", "nan", "fin"]])] * 2))
    out.append(_case("skip_next_to_nan", [[(0, NAN)], [(0, 0.0), (1, 4.0)], [(0, -0.0), (1, 1.0), (2, 3.0)]], 0.0,
                     *[(-1, None, [["nan"], ["+0", "fin"], ["-0", "fin", "fin"]])] * 2))
    # --- signed zeros.  The shift is added even when it is 0.0: -0.0 + 0.0 = +0.0.  With a NaN in rs the zero pivot passes and its
    # inverse shows its sign: +Inf after a shift of +0.0, -Inf after a shift of -0.0
    out.append(_case("zero_pivot_plus_shift", [[(0, -0.0), (1, NAN)], [(1, 1.0)]], 0.0, *[(-1, None, [["+inf", "nan"], ["fin"]])] * 2))
    out.append(_case("zero_pivot_minus_shift", [[(0, -0.0), (1, NAN)], [(1, 1.0)]], -0.0, *[(-1, None, [["-inf", "nan"], ["fin"]])] * 2))
    # diagonal-only rows of value 0: 0 <= zeropivot * 0 fails, also with zeropivot = 0; |w_i| is +0.0 whatever the pivot's sign
    out.append(_case("minus_zero_row", [[(0, -0.0)]], 0.0, *[(0, "+0", [["+0"]])] * 2))
    out.append(_case("zero_row", [[(0, 0.0)]], 0.0, *[(0, "+0", [["+0"]])] * 2))
    out.append(_case("minus_zero_pivot", [[(0, -0.0)]], -0.0, *[(0, "+0", [["+0"]])] * 2))
    # --- the pivot is no part of rs: an Inf pivot next to a finite rs passes (Inf <= zeropivot * 1 is false; with |w_i| inside rs the bound
    # would be Inf) and is stored as +0.0
    out.append(_case("inf_pivot", [[(0, INF), (1, 1.0)], [(1, 1.0)]], 0.0, *[(-1, None, [["+0", "fin"], ["fin"]])] * 2))
    # --- subnormals and overflow.  m * u_01 = 2^-540 * 2^-532 is subnormal; the pivot 2^-1070 - 2^-1072 is subnormal: it fails with
    # the default zeropivot, passes with 0 and inverts to +Inf
    out.append(_case("product_underflows", [[(0, 1.0), (1, 2.0 ** -532), (2, 1.0)], [(0, 2.0 ** -540), (1, 2.0 ** -1070), (2, 1.0)], [(2, 1.0)]], 0.0,
                     (1, "sub", [F3, ["fin", "sub", "fin"], None]), (-1, None, [F3, ["fin", "+inf", "fin"], ["fin"]])))
    # m * u_02 = 2^1023 * 2 overflows: w_2 = 1 - Inf; the pivot 2^1023 + 2^1013 is finite, rs = Inf; its inverse is subnormal
    out.append(_case("product_overflows", [[(0, 1.0), (1, -2.0 ** -10), (2, 2.0)], [(0, 2.0 ** 1023), (1, 2.0 ** 1023), (2, 1.0)], [(2, 1.0)]], 0.0,
                     (1, "fin", [F3, ["fin", "fin", "-inf"], None]), (-1, None, [F3, ["fin", "sub", "-inf"], ["fin"]])))
    return out


@functools.lru_cache(maxsize=None)
def specials_matrix(form):
    """every case a diagonal block of one matrix and a block of the factorisation (nblk = number of cases + 1).  `narrow`: as
    written (4 lanes).  `reg64`: a last block with a row of 40 entries makes it 64 lanes, the cases stay in registers.  `wide`:
    core row r of a case gains the 64 U columns of pad set r, stored +0.0 -- no row it names has them, so they match nothing, add
    0.0 to rs and stay +0.0 -- which makes every core row wider than a wavefront.  The last block: the pad rows.
    Returns dict(ai, aj, aa, blk, shifts, first: the first row of every case)."""
    cases = special_cases()
    first = np.concatenate(([0], np.cumsum([len(c["rows"]) for c in cases]))).astype(int)
    ncore = int(first[-1])
    rows = []
    for c, o in zip(cases, first):
        for r, ent in enumerate(c["rows"]):
            row = [(o + col, v) for col, v in ent]
            if form == "wide":
                row += [(ncore + PAD * r + q, 0.0) for q in range(PAD)]
            rows.append(row)
    if form == "narrow":
        rows.append([(ncore, 1.0)])
    elif form == "reg64":
        rows.append([(ncore, 50.0)] + [(ncore + q, 1.0) for q in range(1, 40)])
        rows += [[(ncore + q, 1.0)] for q in range(1, 40)]
    else:
        rows += [[(ncore + q, 1.0)] for q in range(PAD * 5)]
    ai, aj, aa = _csr(rows)
    blk = np.concatenate((first, [len(rows)])).astype(np.int32)
    return dict(ai=ai, aj=aj, aa=aa, blk=blk, shifts=np.array([c["shift"] for c in cases] + [0.0]), first=first)


def stated_classes(form, which):
    """(failing row per block or -1, class of |w_i| per block, {slot of ba: stated class}) of specials_matrix(form)"""
    cases, m = special_cases(), specials_matrix(form)
    ai = m["ai"]
    slot = slots(ai, m["aj"])
    frow, fcls, cls = [], [], {}
    for c, o in zip(cases, m["first"]):
        fr, fc, per_row = c["expect"][which]
        frow.append(-1 if fr < 0 else int(o + fr)); fcls.append(fc)
        for r, names in enumerate(per_row):
            if names is None:
                continue
            a0 = int(ai[o + r])
            for p, nm in enumerate(names):
                cls[int(slot[a0 + p])] = nm
            for p in range(len(names), int(ai[o + r + 1]) - a0):     # the pad columns of the wide form
                cls[int(slot[a0 + p])] = "+0"
    return np.array(frow + [-1], np.int32), fcls + [None], cls


# ------------------------------------------------------------------------------------------------ containment
CONTAIN = {"narrow": "rows8", "reg64": "rows64", "wide": "mini_wide"}
SPECIALS3 = [NAN, INF, -INF]


@functools.lru_cache(maxsize=None)
def containment_case(form):
    """four copies of a shape on the diagonal, factored as ONE block with zeropivot = 0 (no pivot fails: a finite one is nonzero, a
    non-finite one makes the comparison false).  Three rounds: an off-diagonal entry of one row of copy `round` becomes NaN, +Inf,
    -Inf.  reach: the row itself and, transitively, every row with an L entry of nonzero clean value naming a reached row.
    Returns dict(ai, aj, aa, clean, rounds: [(row, entry of A, poisoned values, reference, reach)])."""
    bi_, bj_, ba_ = shape(CONTAIN[form])
    nb, nzb = bi_.size - 1, int(bi_[-1])
    ai = np.concatenate([[0]] + [bi_[1:] + s * nzb for s in range(4)]).astype(np.int32)
    aj = np.concatenate([bj_ + s * nb for s in range(4)]).astype(np.int32)
    aa = np.concatenate([ba_ * (1.0 + 0.125 * s) for s in range(4)])
    n = 4 * nb
    nzl, slot = nzl_of(ai, aj), slots(ai, aj)
    clean = reference_pass(ai, aj, aa, None, [0.0], 0.0, [1])[0]
    named = np.zeros(n, dtype=bool)
    for i in range(n):
        named[aj[ai[i]:ai[i] + nzl[i]]] = True
    rounds = []
    for rd in range(3):
        cand = [i for i in range(rd * nb, (rd + 1) * nb) if named[i] and ai[i + 1] - ai[i] > 1]
        want_l = rd == 1                                        # round 1 poisons an L position, the others a U position
        cand = [i for i in cand if (nzl[i] > 0 if want_l else ai[i + 1] - ai[i] - nzl[i] > 1)] or cand
        r = cand[(len(cand) * (rd + 1)) // 4]
        q = int(ai[r]) if (want_l and nzl[r]) else int(ai[r + 1]) - 1
        if aj[q] == r:
            q = int(ai[r])
        aap = aa.copy(); aap[q] = SPECIALS3[rd]
        reach = np.zeros(n, dtype=bool); reach[r] = True
        for i in range(r + 1, n):
            a0 = int(ai[i])
            for p in range(int(nzl[i])):
                if reach[aj[a0 + p]] and clean[slot[a0 + p]] != 0.0:
                    reach[i] = True
        ref, frow, _, _ = reference_pass(ai, aj, aap, None, [0.0], 0.0, [1])
        assert frow[0] == -1
        rounds.append((r, q, aap, ref, reach))
    return dict(ai=ai, aj=aj, aa=aa, clean=clean, rounds=rounds)


def row_slots(ai, aj, mask):
    """bool over ba: the slots of the rows in `mask`"""
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    out = np.zeros(int(ai[-1]) + 1, dtype=bool)
    out[slots(ai, aj)[mask[rows]]] = True
    return out


# ------------------------------------------------------------------------------------------------ failure report
FAIL_SHAPES = LANE_SHAPES + ["wide"]


def failing_rows(name):
    """the rows that are made to fail, one per run: a row of level 0 and the row of the deepest level; `wide` also a register row of
    level 0, a register row of a later level and the wide row of level 0"""
    ai, aj, _ = shape(name)
    lev, ln = levels(ai, aj), np.diff(ai)
    lvl0 = np.flatnonzero((lev == 0) & (ln > 1))
    lvl0 = lvl0 if lvl0.size else np.flatnonzero(lev == 0)
    out = [int(lvl0[lvl0.size // 2]), int(np.flatnonzero(lev == lev.max())[-1])]
    if name == "wide":
        out += [5, int(np.flatnonzero((lev > 0) & (ln <= 9))[7])]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def failing_case(name, r):
    """A's values with row r's diagonal changed so that row r is the one failing row: a row without L entries gets the pivot
    -2^-70 (0.0 where it has no U entry either: rs = 0); any other row's diagonal loses (1 - 2^-50) of its clean pivot, which leaves
    a pivot of about 2^-50 of it, nonzero.  Returns (aa, reference ba, failed_abs)."""
    ai, aj, aa = shape(name)
    nzl = nzl_of(ai, aj)
    bd = layout(ai, aj)[2]
    d = int(ai[r] + nzl[r])
    aa = aa.copy()
    if nzl[r] == 0:
        aa[d] = -2.0 ** -70 if ai[r + 1] - ai[r] > 1 else 0.0
    else:
        aa[d] = aa[d] - (1.0 / clean_factor(name)[0][bd[r]]) * (1.0 - 2.0 ** -50)
    ba, frow, fabs_, pend = reference_pass(ai, aj, aa, None, [0.0], ZP, [1])
    assert frow[0] == r and pend[0] == 1, (name, r, frow)
    return aa, ba, float(fabs_[0])


NBLOCKS = 40


@functools.lru_cache(maxsize=None)
def blocks_case():
    """40 blocks, kind b % 5: tridiag(-1, 4, -1) of 5 rows; an empty range; one row of value 0.0 (fails until it is shifted); tridiag(1, 1,
    1) of 9 rows (a zero pivot in its second row); one row of value 3.  Three passes as the plug-in drives them: shift 0; a failed
    block gets 100 eps * (1 + b % 3) / 64; a block that failed again gets 0.05 * (b + 1).  After pass 1 the slots of the finished blocks
    are overwritten with the marker.  Returns dict(ai, aj, aa, blk, passes: [(shifts, ba after the pass -- with the marker from pass
    1 on --, failing rows, failed_abs, pending after it)], finished1: slots of the blocks finished in pass 1)."""
    rows, blk = [], [0]
    for b in range(NBLOCKS):
        o, kind = len(rows), b % 5
        if kind in (0, 3):
            m = 5 if kind == 0 else 9
            lo, di, up = (-1.0, 4.0 + 0.25 * b, -1.0) if kind == 0 else (1.0, 1.0, 1.0)
            for i in range(m):
                rows.append(([(o + i - 1, lo)] if i else []) + [(o + i, di)] + ([(o + i + 1, up)] if i + 1 < m else []))
        elif kind in (2, 4):
            rows.append([(o, 0.0 if kind == 2 else 3.0)])
        blk.append(len(rows))
    ai, aj, aa = _csr(rows)
    blk = np.array(blk, np.int32)
    inblock = np.repeat(np.arange(NBLOCKS), np.diff(blk))
    shifts, pend, ba = np.zeros(NBLOCKS), np.ones(NBLOCKS, np.int32), np.zeros(int(ai[-1]) + 1)
    passes, finished1 = [], None
    for ps in range(3):
        ba, frow, fabs_, pend = reference_pass(ai, aj, aa, blk, shifts, ZP, pend, ba)
        if ps == 0:
            finished1 = row_slots(ai, aj, (pend == 0)[inblock])
            ba[finished1] = MARK
        passes.append((shifts.copy(), ba.copy(), frow, fabs_, pend.copy()))
        for b in np.flatnonzero(frow >= 0):
            shifts[b] = ZP * (1 + b % 3) / 64.0 if ps == 0 else 0.05 * (b + 1)
    return dict(ai=ai, aj=aj, aa=aa, blk=blk, passes=passes, finished1=finished1)


MULTI_FAIL = {6: -2.0 ** -80, 129: 2.0 ** -81, 299: 0.0}      # two rows with a U entry, the last row (rs = 0) with value 0


@functools.lru_cache(maxsize=None)
def multi_fail_case():
    """the upper bidiagonal shape (every row of level 0: mutually independent) with three failing rows in its one block; each row's
    |w_i| is its own.  Returns (ai, aj, aa, {row: |w_i|}, the shift that lets every row pass, the reference with that shift)."""
    ai, aj, aa = shape("upper_bidiagonal")
    aa = aa.copy()
    nzl = nzl_of(ai, aj)
    for r, v in MULTI_FAIL.items():
        aa[ai[r] + nzl[r]] = v
    ref = reference_pass(ai, aj, aa, None, [0.5], ZP, [1])
    assert ref[1][0] == -1
    return ai, aj, aa, {r: abs(v) for r, v in MULTI_FAIL.items()}, 0.5, ref[0]


# ------------------------------------------------------------------------------------------------ the sweep form
def sweep_factor(name):
    """the clean factor of the shape with +0.0, -0.0, +Inf, -Inf and NaN written into L, U and pivot slots"""
    ai, aj, _ = shape(name)
    ba = clean_factor(name)[0].copy()
    nz = ba.size - 1
    kinds = [0.0, -0.0, INF, -INF, NAN]
    for j, s in enumerate(np.linspace(0, nz - 1, 25).astype(int)):
        ba[s] = kinds[j % 5]
    return ba
