"""Host side of the column-tiled SpMV's IEEE-special / containment / layout-edge tests (test_tiled_specials_gpu.py), checked on its
own by test_tiled_specials_cpu.py: numpy, the oracle and the library's host-only layout builder; nothing here touches the GPU.

What is here: `Layout` (a built plan with the walk of tests/tiled.py done ONCE, so that `replay` -- tiled.apply's sums on that walk --
costs one pass per vector), `padding` (where the padding entries of a layout gather and how many blocks and which windows every
wavefront's remainder has), the comparison with the oracle, and the builders of the cases:
  A  containment()    a matrix with a staged part and a remainder in two windows and a set P of unreferenced columns to poison
  B  specials()       hand-built rows with IEEE specials, the expected value of each stated beside it
  C  boundary()       m around the panel size, NaN at every column a padding entry gathers
  D  tail()           n = k * tile + r: the short last tile as a panel's first, second and third staged tile; unstaged_panel()
  E  window_skip(), window_blocks()   the remainder's windows: a skipped window, 1 .. 9 blocks per wavefront
  F  changed_values()  a value array with specials at known positions
The geometry (panel rows, tile width, wavefronts, block entries) always comes from mi355x_spmv_tiled_geometry."""
import numpy as np

import orc
import tiled
from test_tiled_cpu import random_csr
from vecspecials import DBL_MAX, DBL_MIN, INF, MID_SUB, MIN_SUB, NAN, same

WIN = tiled.FW_SHIFT


def csr_of(m, r, c, v):
    """CSR arrays of the entries (r, c, v), columns ascending inside a row; no entry twice"""
    r, c, v = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64)
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    assert not np.any((r[1:] == r[:-1]) & (c[1:] == c[:-1])), "an entry twice"
    ai = np.concatenate(([0], np.cumsum(np.bincount(r, minlength=m)))).astype(np.int32)
    return ai, c.astype(np.int32), v


def coo_of(ai, aj, aa):
    return np.repeat(np.arange(ai.size - 1), np.diff(ai)), aj.astype(np.int64), aa


def klass(v):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 3, np.where(v == INF, 1, np.where(v == -INF, 2, 0)))


class Layout:
    """one matrix cut with one stage_min: the plan (alive until destroy()), what tiled.walk reads from it, the panels' first rows"""

    def __init__(self, k, name, ai, aj, aa, n, stage_min):
        self.k, self.name, self.n, self.stage_min = k, name, int(n), stage_min
        self.ai, self.aj, self.aa = np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(aa, np.float64)
        self.m = self.ai.size - 1
        self.g = tiled.geometry(k)
        self.plan = tiled.build(k, self.ai, self.aj, self.n, stage_min)
        self.info = tiled.info(k, self.plan)
        self.near, self.far = tiled.walk(k, self.plan, self.m)
        tiled.remainder(self.far, self.m)
        self.prow = tiled.get(k, self.plan, 11, np.int32)
        self.rowof = np.repeat(np.arange(self.m), np.diff(self.ai))
        assert self.near[0].size == self.info["staged"] and self.far[0].size == self.info["remainder"]

    def destroy(self):
        if self.plan is not None:
            self.k.mi355x_spmv_tiled_destroy(self.plan)
            self.plan = None

    def replay(self, x, yin=None, which=0, aa=None):
        """tiled.apply on the stored walk: (yin or 0) + the staged products in stream order (which 0 or 1), then the remainder's (0 or 2),
        every product rounded and added to the row's sum one after the other (Python floats: IEEE doubles, no exception on overflow)"""
        aa = self.aa if aa is None else aa
        y = [0.0] * self.m if yin is None else np.asarray(yin, dtype=np.float64).tolist()
        with np.errstate(all="ignore"):
            for part, (r, c, q) in ((1, self.near), (2, self.far)):
                if which in (0, part):
                    for i, p in zip(r.tolist(), (aa[q] * x[c]).tolist()):
                        y[i] = y[i] + p
        return np.array(y, dtype=np.float64)

    def scale(self, x, yin=None, aa=None):
        """sum_j |a_ij x_j| (+ |yin_i|): what BASELINE.md's 1e-12 bound is relative to"""
        aa = self.aa if aa is None else aa
        s = np.zeros(self.m) if yin is None else np.abs(yin)
        with np.errstate(all="ignore"):
            np.add.at(s, self.rowof, np.abs(aa * x[self.aj]))
        return s

    def oracle(self, x, yin=None, aa=None):
        aa = self.aa if aa is None else np.ascontiguousarray(aa, np.float64)
        x = np.ascontiguousarray(x, np.float64)
        if self.m == 0:
            return np.zeros(0)
        return orc.spmv(self.ai, self.aj, aa, x) if yin is None else orc.spmv_add(self.ai, self.aj, aa, x, np.ascontiguousarray(yin, np.float64))

    def against_oracle(self, y, x, yin=None, aa=None, what=""):
        """the class of every row is the oracle's; finite rows within 1e-12 * sum |a_ij x_j|; the oracle's bits when one stream in
        column order made the sums (nothing staged, or nothing left to the remainder)"""
        ref = self.oracle(x, yin, aa)
        ky, kr = klass(y), klass(ref)
        bad = np.flatnonzero(ky != kr)
        assert bad.size == 0, "%s %s: row %d is %r, the oracle has %r" % (self.name, what, bad[0], y[bad[0]], ref[bad[0]])
        fin = ky == 0
        with np.errstate(all="ignore"):
            tol = 1e-12 * self.scale(x, yin, aa) + 1e-300
            err = np.abs(y - ref)
        bad = np.flatnonzero(fin & ~(err <= tol))
        assert bad.size == 0, "%s %s: row %d: %r against the oracle's %r, allowed %g" % (self.name, what, bad[0], y[bad[0]], ref[bad[0]], tol[bad[0]])
        if self.info["staged"] == 0 or self.info["remainder"] == 0:
            same(y, ref, "%s %s against the oracle (one stream in column order)" % (self.name, what))
        return ref

    def panel_edges(self):
        """[(last row of a panel, first row of the next)]"""
        return [(int(r) - 1, int(r)) for r in self.prow[1:-1]]


def padding(k, plan):
    """Where the padding entries of a layout gather x: {column: padding entries} of the staged runs (a tile's first column) and of the
    remainder's runs (a window's first column); per wavefront the number of remainder blocks and its windows; per panel its staged
    tiles."""
    g = tiled.geometry(k)
    W, B = g["waves"], g["block"]
    pt_ptr, pt_tile, pw_e0 = tiled.get(k, plan, 0, np.int32), tiled.get(k, plan, 1, np.int32), tiled.get(k, plan, 2, np.int32)
    word, perm = tiled.get(k, plan, 3, np.uint32), tiled.get(k, plan, 4, np.int32)
    pw_f0, fw_ptr, fw_win = tiled.get(k, plan, 7, np.int32), tiled.get(k, plan, 8, np.int32), tiled.get(k, plan, 9, np.int32)
    staged, rem, blocks, wins = {}, {}, [], []
    for ipw in range(pw_f0.size):
        p, it, iw = ipw // W, -1, -1
        for b0 in range(int(pw_e0[ipw]), int(pw_f0[ipw]), B):
            it += bool(word[b0] & tiled.NEWTILE)
            npad = int((perm[b0:b0 + B] < 0).sum())
            if npad:
                assert np.all((word[b0:b0 + B][perm[b0:b0 + B] < 0] & ~np.uint32(tiled.NEWTILE)) == g["panel"] << 16)
                col = int(pt_tile[pt_ptr[p] + it]) * g["tw"]
                staged[col] = staged.get(col, 0) + npad
        for b0 in range(int(pw_f0[ipw]), int(pw_e0[ipw + 1]), B):
            iw += bool(word[b0] & tiled.NEWWIN)
            npad = int((perm[b0:b0 + B] < 0).sum())
            if npad:
                col = int(fw_win[fw_ptr[ipw] + iw]) << WIN
                rem[col] = rem.get(col, 0) + npad
        blocks.append(int(pw_e0[ipw + 1] - pw_f0[ipw]) // B)
        wins.append([int(v) for v in fw_win[fw_ptr[ipw]:fw_ptr[ipw + 1]]])
    tiles = [[int(t) for t in pt_tile[pt_ptr[p]:pt_ptr[p + 1]]] for p in range(pt_ptr.size - 1)]
    return {"staged": staged, "remainder": rem, "blocks": blocks, "windows": wins, "tiles": tiles}


def plain_x(n):
    return np.cos(0.11 * np.arange(n)) + 2.0


# ------------------------------------------------------------------------------------------------------------- A: containment
def containment(k):
    """A matrix of two panels whose banded part is staged and whose scattered quarter is the remainder, in windows 0 and 1 (n a little
    over 2^18), about 10^5 nonzeros.  No row references: the first column of any tile (staged padding gathers there; a window's first
    column is one of them: remainder padding), the first pair of the short last tile, n - 1, n - 2, both neighbours of three referenced
    columns.  P is the part of those the layout really reads or that lies beside real data.  Row `big` has hundreds of entries in one
    staged tile (all 64 lanes of a ds_add_f64 on one accumulator).
    The second matrix MOVES columns of P into the pattern: `big` takes the first column of its heavy tile (x there: +Inf), the rows
    on both sides of the panel boundary the first column of window 1 (NaN), row `mid` column n - 1 (-Inf)."""
    g = tiled.geometry(k)
    tw, panel = g["tw"], g["panel"]
    rng = np.random.default_rng(41)
    m, n = panel + 301, (1 << WIN) + 5000
    lens = rng.integers(11, 21, m)
    ai, aj, aa = random_csr(rng, m, n, lens, band=3000, far_frac=0.25)
    r, c, _ = coo_of(ai, aj, aa)
    big, mid = m // 3, m // 2 + 7
    heavy = (big * n // m) // tw                                   # the tile around the centre of big's band
    last0 = (n - 1) // tw * tw
    assert n - last0 < tw and n - last0 > 8
    extra_r = [np.full(600, big), np.repeat(np.arange(m - 200, m), 3)]
    extra_c = [heavy * tw + 1 + rng.choice(tw - 1, 600, replace=False), rng.integers(last0 + 2, n - 2, 600)]
    r, c = np.concatenate([r] + extra_r), np.concatenate([c] + extra_c)
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    free = set(range(0, n, tw)) | {last0, last0 + 1, n - 1, n - 2}
    kept = c[~np.isin(c, list(free))]
    refs = []
    for cand in kept[[kept.size // 7, kept.size // 2, kept.size - kept.size // 9]]:
        cand = int(cand)
        if all(abs(cand - q) > 2 for q in refs) and not ({cand - 1, cand, cand + 1} & free) and 0 < cand < n - 1:
            refs.append(cand)
    neighbours = sorted({q - 1 for q in refs} | {q + 1 for q in refs})
    free |= set(neighbours)
    keep = ~np.isin(c, list(free))
    r, c = r[keep], c[keep]
    v = rng.standard_normal(r.size) * 10.0 ** rng.integers(-3, 4, r.size)
    A = csr_of(m, r, c, v)
    stage_min = 300
    # the columns moved into the pattern (the rows around the boundary: two on each side, so that the boundary of the second matrix,
    # cut by nonzeros, still lies between poisoned rows)
    pre = Layout(k, "containment", *A, n, stage_min)
    edge = int(pre.prow[1])
    pad = padding(k, pre.plan)
    pre.destroy()
    P = sorted(set(pad["staged"]) | set(pad["remainder"]) | {last0, last0 + 1, n - 1, n - 2} | set(neighbours))
    moved = [(big, heavy * tw, 1.5)] + [(row, 1 << WIN, -2.0) for row in range(edge - 2, edge + 2)] + [(mid, n - 1, 0.75)]
    r2 = np.concatenate((r, [t[0] for t in moved])); c2 = np.concatenate((c, [t[1] for t in moved])); v2 = np.concatenate((v, [t[2] for t in moved]))
    A2 = csr_of(m, r2, c2, v2)
    x = plain_x(n)
    xin = x.copy()
    xin[P] = NAN
    xin[heavy * tw], xin[1 << WIN], xin[n - 1] = INF, NAN, -INF
    return {"m": m, "n": n, "A": A, "A2": A2, "stage_min": stage_min, "P": np.array(P), "listed": sorted({last0, last0 + 1, n - 1, n - 2} | set(neighbours)),
            "refs": refs, "neighbours": neighbours, "big": big, "mid": mid, "heavy": heavy, "moved": moved, "x": x, "x_moved": xin,
            "expect_class": {big: 1, mid: 2, **{row: 3 for row in range(edge - 2, edge + 2)}}}


# ------------------------------------------------------------------------------------------------- B: specials inside the pattern
# One hand-built row: (name, entries (value, x) in tile 0, entries in tile 2, yin, expected without yin, expected with yin,
# (what a plausible wrong kernel gives without yin, with yin)).  A row's entries of tile 0 come first in column order, so the expected
# value is the same whether the row is all staged, all remainder or split (tile 0 staged, tile 2 remainder: staged first).
_H = DBL_MAX / 2
SPECIAL_ROWS = [
    # a stored 0.0 times an x of Inf: NaN, as in the reference (a kernel that skips stored zeros: 3.0)
    ("zero_times_inf", [(1.5, 2.0)], [(0.0, INF)], 0.25, NAN, NAN, (3.0, 3.25)),
    # Inf times a stored -0.0: NaN
    ("inf_times_negzero", [(-0.0, INF)], [(1.0, 1.0)], 0.0, NAN, NAN, (1.0, 1.0)),
    ("nan_value", [(NAN, 1.0)], [(2.0, 3.0)], 0.0, NAN, NAN, (6.0, 6.0)),
    ("nan_x", [(1.0, 2.0)], [(2.0, NAN)], 0.0, NAN, NAN, (2.0, 2.0)),
    # +Inf and -Inf products in one row: NaN -- both in the first part, both in the second, one in each
    ("inf_pair_first_part", [(1.0, INF), (1.0, -INF)], [(1.0, 1.0)], 0.0, NAN, NAN, (-INF, -INF)),
    ("inf_pair_second_part", [(1.0, 1.0)], [(1.0, INF), (2.0, -INF)], 0.0, NAN, NAN, (-INF, -INF)),
    ("inf_one_per_part", [(1.0, INF)], [(1.0, -INF)], 0.0, NAN, NAN, (INF, INF)),
    # DBL_MAX + DBL_MAX: +Inf and not NaN (a saturating sum: DBL_MAX)
    ("overflow", [(_H, 2.0)], [(_H, 2.0)], 0.0, INF, INF, (DBL_MAX, DBL_MAX)),
    # DBL_MAX - DBL_MAX + DBL_MAX - DBL_MAX + 3 in column order: 3.0 (pairs summed first: Inf - Inf = NaN)
    ("dmax_cancel", [(_H, 2.0), (-_H, 2.0)], [(_H, 2.0), (-_H, 2.0), (3.0, 1.0)], 0.0, 3.0, 3.0, (NAN, NAN)),
    # subnormal values times normal x: 3 * 2^-1050 + 7 * 2^-1074, exact (subnormal inputs flushed: 0.0)
    ("subnormal_values", [(MID_SUB, 3.0)], [(MIN_SUB, 7.0)], 0.0, 3 * MID_SUB + 7 * MIN_SUB, 3 * MID_SUB + 7 * MIN_SUB, (0.0, 0.0)),
    # normal values whose products are subnormal: rounded 1e-320, then + 2^-1070 (exact)
    ("subnormal_products", [(1e-160, 1e-160)], [(2.0 ** -600, 2.0 ** -470)], 0.0, 1e-160 * 1e-160 + 2.0 ** -1070, 1e-160 * 1e-160 + 2.0 ** -1070, (0.0, 0.0)),
    # normal products, subnormal sum: 1.5 DBL_MIN - DBL_MIN = DBL_MIN / 2 (a flushed result: 0.0)
    ("subnormal_sum", [(1.5 * DBL_MIN, 1.0)], [(-DBL_MIN, 1.0)], 0.0, 0.5 * DBL_MIN, 0.5 * DBL_MIN, (0.0, 0.0)),
    # DBL_MIN and 200 products of 2^-1074 (100 stored subnormal, 100 from normal operands): DBL_MIN + 200 * 2^-1074, exact (subnormal addends flushed: DBL_MIN)
    ("unflushed", [(DBL_MIN, 1.0)] + [(MIN_SUB, 1.0)] * 100, [(2.0 ** -600, 2.0 ** -474)] * 100, 0.0, DBL_MIN + 200 * MIN_SUB, DBL_MIN + 200 * MIN_SUB, (DBL_MIN, DBL_MIN)),
    # all products -0.0: +0.0 + -0.0 = +0.0 without yin; -0.0 + -0.0 = -0.0 with yin = -0.0; +0.0 with yin = +0.0
    ("negzero_products_yin_negzero", [(-0.0, 1.0), (1.0, -0.0)], [(0.0, -2.0)], -0.0, 0.0, -0.0, (-0.0, 0.0)),
    ("negzero_products_yin_zero", [(-0.0, 1.0), (1.0, -0.0)], [(0.0, -2.0)], 0.0, 0.0, 0.0, (-0.0, -0.0)),
    # yin = +Inf meets a -Inf product: NaN with yin, -Inf without (sums started from yin when there is none to add: NaN; from 0.0 whatever yin: -Inf)
    ("yin_inf_meets_minus_inf", [(2.0, 1.0)], [(1.0, -INF)], INF, -INF, NAN, (NAN, -INF)),
    # empty rows: yin passes through bit for bit, +0.0 without yin
    ("empty_yin_negzero", [], [], -0.0, 0.0, -0.0, (-0.0, 0.0)),
    ("empty_yin_nan", [], [], NAN, 0.0, NAN, (NAN, 0.0)),
    ("empty_yin_inf", [], [], INF, 0.0, INF, (INF, 0.0)),
    ("empty_yin_subnormal", [], [], MID_SUB, 0.0, MID_SUB, (MID_SUB, 0.0)),
]


def specials(k):
    """SPECIAL_ROWS among 150 ordinary rows, n = 3 tiles.  Special row i has columns of its own in tile 0 and tile 2 (x is set per
    column); ordinary rows have 12 entries in tile 0, 6 in tile 1, every third one in tile 2.  stage_min 1: all staged; 10^9: all
    remainder; entries of tile 2 + 1: tiles 0 and 1 staged, tile 2 left to the remainder -- every special row is split."""
    g = tiled.geometry(k)
    tw = g["tw"]
    assert tw >= 1024
    rng = np.random.default_rng(43)
    nord, ns = 150, len(SPECIAL_ROWS)
    m, n = nord + ns, 3 * tw
    srow = [3 + 6 * i for i in range(ns)]
    assert srow[-1] < m
    ordinary = [i for i in range(m) if i not in set(srow)]
    x = np.sin(0.37 * np.arange(n)) + 1.5
    yin = rng.standard_normal(m)
    r, c, v = [], [], []
    big0 = 300                                                     # the long row's columns: 300 .. 300 + 101 of tiles 0 and 2; the others: 8 i + 8 ..
    for i, (name, t0, t2, yv, _, _, _) in enumerate(SPECIAL_ROWS):
        yin[srow[i]] = yv
        for base, ent in ((0, t0), (2 * tw, t2)):
            first = base + (big0 if len(ent) > 8 else 8 + 8 * i)
            assert len(ent) <= 8 or name == "unflushed"
            for j, (a, xv) in enumerate(ent):
                r.append(srow[i]); c.append(first + j); v.append(a)
                x[first + j] = xv
    assert 8 + 8 * ns < big0 and big0 + 101 < 512
    for row in ordinary:
        cols = np.concatenate((rng.choice(np.arange(512, tw), 12, replace=False), tw + rng.choice(np.arange(1, tw), 6, replace=False),
                               2 * tw + rng.choice(np.arange(512, tw), 1 if row % 3 == 0 else 0, replace=False)))
        r += [row] * cols.size; c += cols.tolist(); v += rng.standard_normal(cols.size).tolist()
    A = csr_of(m, r, c, v)
    in2 = int((A[1] >= 2 * tw).sum())
    assert in2 + 1 <= int(((A[1] >= tw) & (A[1] < 2 * tw)).sum())
    return {"m": m, "n": n, "A": A, "x": x, "yin": yin, "srow": srow, "ordinary": ordinary,
            "stage_min": {"staged": 1, "remainder": 10 ** 9, "split": in2 + 1}}


def special_expectation(case, with_yin):
    """(rows, expected values, wrong values) of the special rows"""
    j = 5 if with_yin else 4
    return (np.array(case["srow"]), np.array([s[j] for s in SPECIAL_ROWS], dtype=np.float64),
            np.array([s[6][1 if with_yin else 0] for s in SPECIAL_ROWS], dtype=np.float64))


# ---------------------------------------------------------------------------------------- C: the spare accumulator, the panel boundary
def boundary_sizes(k):
    p = tiled.geometry(k)["panel"]
    return [p - 1, p, p + 1, 2 * p + 1]


BOUNDARY_STAGE_MIN = (1, 200)        # everything staged; the thin pairs of tiles 2 and 3 left to the remainder


def boundary(k, m):
    """m rows of 5 entries in a band over tiles 0 and 1, every 97th row one more in tile 2 or 3 (thin pairs: the remainder of the
    second stage_min); n = 3 tiles + 100.  x holds NaN at the first column of every tile (column 0 is window 0's first as well), and no
    row references those: every padding product is NaN and belongs to the spare accumulator alone."""
    g = tiled.geometry(k)
    tw = g["tw"]
    n = 3 * tw + 100
    rng = np.random.default_rng(1000 + m % 97)
    r = np.repeat(np.arange(m), 5)
    c = np.clip(r * (2 * tw) // m + rng.integers(-300, 301, r.size), 1, 2 * tw - 2)
    thin = np.arange(0, m, 97)
    r = np.concatenate((r, thin)); c = np.concatenate((c, rng.integers(2 * tw + 1, n - 1, thin.size)))
    c = c + (c % tw == 0)
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    A = csr_of(m, r, c, rng.standard_normal(r.size))
    x = plain_x(n)
    x[::tw] = NAN
    return {"m": m, "n": n, "A": A, "x": x, "yin": rng.standard_normal(m)}


# ------------------------------------------------------------------------------------------- D: the short last tile and the loader
def tail_remainders(k):
    tw = tiled.geometry(k)["tw"]
    return [1, 2, 3, 127, 128, 129, 130, tw - 1, 0]


def tail(k, r, depth):
    """n = 2 tiles + r (r = 0: three full tiles); 24 rows with entries in the last `depth` tiles only, stage_min 1: the last tile is the
    panel's only staged tile (everybody loads it), its second (the loader wavefront, into the other buffer) or its third (the loader,
    into the buffer that held tile 0).  Rows reference n - 1, n - 2 and the last tile's first column; x differs in every column."""
    g = tiled.geometry(k)
    tw = g["tw"]
    n = 2 * tw + r if r else 3 * tw
    lo = (3 - depth) * tw
    last0 = 2 * tw
    rng = np.random.default_rng(7000 + 10 * r + depth)
    m = 24
    rr, cc = [], []
    for row in range(m):
        cols = set(int(q) for q in ([n - 1, last0] if row % 2 == 0 else [n - 2]) if q >= lo)
        for t in range(3 - depth, 3):
            width = min(tw, n - t * tw)
            cols |= set((t * tw + rng.choice(width, min(3, width), replace=False)).tolist())
        rr += [row] * len(cols); cc += sorted(cols)
    A = csr_of(m, rr, cc, rng.standard_normal(len(rr)))
    x = 1.0 + np.arange(n) / 4096.0
    return {"m": m, "n": n, "A": A, "x": x, "yin": rng.standard_normal(m), "depth": depth, "stage_min": 1, "last_tile": 2}


def unstaged_panel(k):
    """two panels: the first has one entry per row anywhere in four tiles (no pair reaches stage_min), the second three per row in tile
    1 (staged): a workgroup without any staged tile beside one with some"""
    g = tiled.geometry(k)
    tw, panel = g["tw"], g["panel"]
    rng = np.random.default_rng(77)
    m, n = panel + 1, 3 * tw + 129
    nthin = (m * 3) // 4
    r = np.concatenate((np.arange(nthin), np.repeat(np.arange(nthin, m), 3)))
    c = np.concatenate((rng.integers(0, n, nthin), tw + np.concatenate([rng.choice(tw, 3, replace=False) for _ in range(nthin, m)])))
    A = csr_of(m, r, c, rng.standard_normal(r.size))
    return {"m": m, "n": n, "A": A, "x": 1.0 + np.arange(n) / 4096.0, "yin": rng.standard_normal(m), "stage_min": 2000}


# ----------------------------------------------------------------------------------------------------- E: the remainder's windows
WINDOW_N = (1 << 19) + 17
BLOCK_COUNTS = list(range(1, 10))    # remainder blocks of one wavefront: 2 TL_FG and 2 TL_FG + 1 are among them for any TL_FG <= 4 (the source: 2)


def window_x():
    return np.sin(0.013 * np.arange(WINDOW_N)) + 1.25


def window_skip(k):
    """8 rows of 40 entries, everything remainder (stage_min 10^9).  Row 0 holds columns 2^18 - 1, 2^18, 2^18 + 1; rows 2 .. 7 have
    entries in windows 0 and 2 only: the wavefronts that own them skip window 1."""
    rng = np.random.default_rng(91)
    n, w = WINDOW_N, 1 << WIN
    rr, cc = [], []
    for row in range(8):
        if row < 2:
            cols = set([w - 1, w, w + 1]) if row == 0 else set()
            cols |= set(rng.integers(0, n, 40 - len(cols)).tolist())
        else:
            cols = set(rng.integers(0, w, 20).tolist()) | set(rng.integers(2 * w, n, 20).tolist())
        rr += [row] * len(cols); cc += sorted(cols)
    A = csr_of(8, rr, cc, rng.standard_normal(len(rr)))
    return {"m": 8, "n": n, "A": A, "x": window_x(), "yin": rng.standard_normal(8), "stage_min": 10 ** 9}


def window_blocks(k, count):
    """one row (its wavefront: the first) with `count` remainder blocks: count - 1 blocks of window 0 ending in column 2^18 - 1, then
    one block of window 1 with columns 2^18 and 2^18 + 1; count = 1: the block of window 1 alone"""
    g = tiled.geometry(k)
    B, w = g["block"], 1 << WIN
    rng = np.random.default_rng(300 + count)
    cols = {w, w + 1}
    if count > 1:
        n0 = B * (count - 2) + 1 + (B // 3 if count > 2 else 0)
        cols |= {w - 1} | set(rng.choice(w - 1, n0 - 1, replace=False).tolist())
    cols = sorted(cols)
    A = csr_of(1, [0] * len(cols), cols, rng.standard_normal(len(cols)) * 10.0 ** rng.integers(-4, 5, len(cols)))
    return {"m": 1, "n": WINDOW_N, "A": A, "x": window_x(), "yin": np.array([0.625]), "stage_min": 10 ** 9, "count": count}


# ---------------------------------------------------------------------------------------------------------- F: values that change
def changed_values(aa, seed):
    """a value array of the same pattern with NaN, +Inf, -Inf and subnormals at known positions"""
    rng = np.random.default_rng(seed)
    out = aa * 1.7 - 0.3
    pos = rng.choice(aa.size, 8, replace=False)
    out[pos] = [NAN, INF, -INF, MIN_SUB, -MID_SUB, DBL_MIN / 4, -0.0, 0.0]
    return out, pos
