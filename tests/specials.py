"""Host-side machinery of the SpMV containment / IEEE-special tests (test_spmv_specials_gpu.py, test_spmv_cprow_gpu.py); pure
numpy + the oracle, checked on its own by test_spmv_specials_cpu.py.

The row-block kernels of csrc/spmv_csr.hip load and gather unconditionally: a lane without work, or the half of a 16-byte pair
outside the block, reads something real, multiplies it and the result is discarded by a select or parked in an LDS slot no row
reads.  With finite data a leak from such a lane is a small perturbation; with NaN / +-Inf in the columns those lanes read it
changes the class of a row.  What is here: the plan's row blocks recovered on the host, the columns idle lanes read (targets),
which rows a set P of poisoned columns may touch (hit), the class of a result, and the hand-built matrices of special values."""
import ctypes as C
import functools

import numpy as np

import orc

CAP = 2046            # SPMV_BLOCK_CAP: nonzeros of a row block
BLOCK_ROWS = 256      # SPMV_BLOCK_ROWS
SEQ_AVG = 16          # SPMV_SEQ_AVG: a block with <= this many nonzeros per row on average sums each row on one lane
ROUNDS = 3            # rounds of poisoned columns per shape at least; more where the budget of hit rows keeps block targets out (MAX_ROUNDS)
MAX_ROUNDS = 16
SPECIALS = np.array([np.nan, np.inf, -np.inf])
FIN, NAN, PINF, NINF = 0, 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def row_blocks(ai):
    """spmv_plan_create's greedy rule: at most 256 rows and at most 2046 nonzeros per block, a longer row alone.
    Returns (first row of every block + the row count at the end, number of long rows)."""
    m = ai.size - 1
    rb, r, nlong = [0], 0, 0
    while r < m:
        start, nnz = r, 0
        while r < m and r - start < BLOCK_ROWS:
            ln = int(ai[r + 1] - ai[r])
            if nnz + ln > CAP:
                break
            nnz += ln
            r += 1
        if r == start:
            r += 1
            nlong += 1
        rb.append(r)
    return np.array(rb, dtype=np.int64), nlong


def one_lane_rows(ai, rb):
    """rows whose block sums every row on one lane in the reference's order (lanes_per_row: nnz <= 16 * nrows), so that the
    result carries the oracle's bits; rows of the other blocks and long rows are summed by a tree"""
    out = np.zeros(ai.size - 1, dtype=bool)
    for b in range(rb.size - 1):
        nnz = int(ai[rb[b + 1]] - ai[rb[b]])
        out[rb[b]:rb[b + 1]] = nnz <= CAP and nnz <= SEQ_AVG * (rb[b + 1] - rb[b])
    return out


def classify(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), NAN, np.where(v == np.inf, PINF, np.where(v == -np.inf, NINF, FIN))).astype(np.int8)


def hit_rows(ai, aj, P, n):
    """rows whose column list intersects P"""
    mask = np.zeros(n, dtype=bool)
    mask[np.asarray(P, dtype=np.int64)] = True
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    hit = np.zeros(ai.size - 1, dtype=bool)
    hit[rows[mask[aj]]] = True
    return hit


def poison(x, P, shift=0, stride=1, kinds=SPECIALS):
    """x with entry stride * c (+ a position inside the block for stride > 1) of every column c of P overwritten, cycling NaN, +Inf, -Inf"""
    xp = x.copy()
    P = np.asarray(P, dtype=np.int64)
    i = np.arange(P.size)
    xp[P * stride + (i % stride)] = np.asarray(kinds)[(i + shift) % len(kinds)]
    return xp


def block_targets(ai, aj, rb):
    """per row block, the columns its idle lanes and cut pairs read: of the block's first and last nonzero, and of the stream
    elements next to them, aj[k0 - 1] and aj[k1], where they exist"""
    groups = []
    for b in range(rb.size - 1):
        k0, k1 = int(ai[rb[b]]), int(ai[rb[b + 1]])
        if k1 == k0:
            continue
        g = [int(aj[k0]), int(aj[k1 - 1])]
        if k0 > 0:
            g.append(int(aj[k0 - 1]))
        if k1 < aj.size:
            g.append(int(aj[k1]))
        groups.append(g)
    return groups


def choose_P(ai, aj, n, rb, c_slack, rnd, seed, extras=(), budget=None, own_rows=0, first=(), ends=True):
    """The poisoned columns of round `rnd`: c_slack always, columns 0 and n - 1 with it unless `ends` is off; then `first` (block targets no earlier round took), `extras`, the block targets (the list of blocks
    rotated by a third per round, so that every round starts with other blocks) and 1 % random columns, each taken unless it
    would push the number of hit rows over `budget` (half the rows: the other half must stay to show containment); last,
    `own_rows` columns r of rows r that are clean so far (the x_r of the x'y by-product)."""
    m = ai.size - 1
    budget = m // 2 if budget is None else budget
    rows = np.repeat(np.arange(m), np.diff(ai))
    o = np.argsort(aj, kind="stable")
    ptr = np.searchsorted(aj[o], np.arange(n + 1))
    crow = rows[o]
    groups = block_targets(ai, aj, rb)
    s = (rnd * len(groups)) // ROUNDS
    groups = groups[s:] + groups[:s]
    rng = np.random.default_rng(seed + 1000 * rnd)
    must = [c_slack, 0, n - 1] if ends else [c_slack]
    order = must + [int(c) for c in first] + [int(c) for c in extras] + [c for g in groups for c in g] + \
        [int(c) for c in rng.choice(n, size=max(1, n // 100), replace=False)]
    hit = np.zeros(m, dtype=bool)
    P = []

    def take(c, must=False):
        if c in P:
            return
        new = hit.copy()
        new[crow[ptr[c]:ptr[c + 1]]] = True
        if new.sum() > budget:
            assert not must, "column %d alone exceeds the budget of %d rows" % (c, budget)
            return
        hit[:] = new
        P.append(c)
    for i, c in enumerate(order):
        take(c, must=i < len(must))
    for r in rng.permutation(np.flatnonzero(~hit)) if own_rows else ():
        if own_rows > 0 and int(r) < n and int(r) not in P:
            before = len(P)
            take(int(r))
            own_rows -= len(P) - before
    return np.array(sorted(P), dtype=np.int64)


def row_class_two_orders(ai, prod, start=None):
    """class of every row's sum, the products added in np.longdouble front to back and back to front: (forward, backward)"""
    m = ai.size - 1
    rows = np.repeat(np.arange(m), np.diff(ai))
    out = []
    with np.errstate(all="ignore"):
        for sl in (slice(None), slice(None, None, -1)):
            s = np.zeros(m, dtype=np.longdouble) if start is None else start.astype(np.longdouble)
            np.add.at(s, rows[sl], prod.astype(np.longdouble)[sl])
            out.append(classify(s.astype(np.float64)))     # (|a|, |x| <= 1e3: a finite long-double sum is a finite double)
    return out


def finite_scale(ai, aj, aa, x):
    """sum |a_ij x_j| over the finite products of every row: the scale of BASELINE.md's 1e-12 bound"""
    with np.errstate(all="ignore"):
        p = np.abs(aa * x[aj])
    p = np.where(np.isfinite(p), p, 0.0)
    s = np.zeros(ai.size - 1)
    with np.errstate(over="ignore"):                              # (the hand-built rows whose sum overflows: the bound is then +Inf, and not used)
        np.add.at(s, np.repeat(np.arange(ai.size - 1), np.diff(ai)), p)
    return s


def spmv_inode_add(ai, aj, aa, x, y):
    """MatMultAdd_SeqAIJ_Inode's order (two products at a time, starting from y)"""
    z = np.zeros(ai.size - 1)
    orc.lib().orc_spmv_csr_inode_add(C.c_int(ai.size - 1), orc.I(ai), orc.I(aj), orc.D(aa), orc.D(x), orc.D(y), orc.D(z))
    return z


def oracle(mode, pairsum, ai, aj, aa, x, y0, d):
    """what each entry point computes, from the oracle's loops: mult / dot: A x; add, add_alias: y0 + A x; scaled: MatMult then
    VecPointwiseMult, d .* (A x); add_scaled: d .* (y0 + A x)"""
    mult = orc.spmv_inode if pairsum else orc.spmv
    add = spmv_inode_add if pairsum else orc.spmv_add
    with np.errstate(all="ignore"):
        if mode in ("mult", "dot"):
            return mult(ai, aj, aa, x)
        if mode in ("add", "add_alias"):
            return add(ai, aj, aa, x, y0)
        if mode == "scaled":
            return mult(ai, aj, aa, x) * d
        assert mode == "add_scaled"
        return d * add(ai, aj, aa, x, y0)


def mode_bound(mode, scale, y0, d):
    if mode in ("mult", "dot"):
        return scale
    if mode in ("add", "add_alias"):
        return scale + np.abs(y0)
    if mode == "scaled":
        return np.abs(d) * scale
    return np.abs(d) * (scale + np.abs(y0))


def check_against_reference(got, ref, exact, bound, what, rows=None):
    """class by class: NaN where the reference is NaN, +-Inf where it is; everything else bit for bit on `exact` rows and
    within 1e-12 * bound on the others"""
    rows = np.ones(got.size, dtype=bool) if rows is None else rows
    cg, cr = classify(got), classify(ref)
    bad = rows & (cg != cr)
    assert not bad.any(), "%s: class differs in rows %s: got %s, reference %s" % (what, np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])
    ex = rows & exact & (cr != NAN)
    badx = ex & (bits(got) != bits(ref))
    assert not badx.any(), "%s: bits differ in rows %s: got %r, reference %r" % (what, np.flatnonzero(badx)[:8], got[badx][:8], ref[badx][:8])
    fin = rows & ~exact & (cr == FIN)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        badf = fin & ~(err <= 1e-12 * bound)
    assert not badf.any(), "%s: rows %s off by %s, bound %s" % (what, np.flatnonzero(badf)[:8], err[badf][:8], 1e-12 * bound[badf][:8])


def check_containment(clean, pois, ref, hit, exact, bound, what):
    """rows not in hit: the poisoned run equals the clean one bit for bit; rows in hit: check_against_reference"""
    leak = ~hit & (bits(pois) != bits(clean))
    assert not leak.any(), "%s: rows %s have no poisoned column and changed: %r -> %r" % (what, np.flatnonzero(leak)[:8], clean[leak][:8], pois[leak][:8])
    check_against_reference(pois, ref, exact, bound, what, rows=hit)


def expand_rows(cai, rows, m):
    """row pointer of the m-row matrix whose row rows[i] is row i of the compressed matrix, every other row empty"""
    ai = np.zeros(m + 1, dtype=np.int64)
    ai[np.asarray(rows, dtype=np.int64) + 1] = np.diff(cai)
    return np.cumsum(ai).astype(np.int32)


# ------------------------------------------------------------------------------------------------ shapes of the containment rounds
def band(nb, half=40):
    cols = [np.arange(max(0, r - half), min(nb, r + half + 1)) for r in range(nb)]
    return np.concatenate(([0], np.cumsum([c.size for c in cols]))).astype(np.int32), np.concatenate(cols).astype(np.int32)


def csr_shape(name):
    """(ai, aj, aa, n, extras): the smallest shape at which each path of the CSR kernels exists; |a| <= 1e3.  extras: columns
    poisoned on top of the block targets (stencils: r +- (largest offset + 1) of a few rows r; stored zeros: their columns)"""
    from test_kernels_gpu import grouped_csr, random_csr, rnd
    import problems as pb
    extras = []
    if name.startswith("p7"):
        ai, aj, aa = orc.gen_p7(13, 11, 9)
        n = ai.size - 1
        if name == "p7":
            aa = aa * (1.0 + 0.01 * np.cos(np.arange(aa.size)))
        far = 13 * 11 + 1
        extras = [c for r in (200, 640, 1100) for c in (r - far, r + far) if 0 <= c < n]
        if name == "p7const_zeros":
            aa = aa.copy()
            k0, k1 = int(ai[300]) + 2, int(ai[777]) + 4
            aa[k0], aa[k1] = 0.0, -0.0
            extras += [int(aj[k0]), int(aj[k1])]
    elif name == "rand16":
        ai, aj, aa = random_csr(600, 500, lambda rng, m: rng.integers(0, 17, m), 66)
        n = 500
    elif name == "band81":
        ai, aj = band(300)
        aa = rnd(aj.size, 68)
        n = 300
    elif name == "longrow":
        def lens(rng, m):
            ln = rng.integers(0, 9, m)
            ln[7] = 2500
            return ln
        ai, aj, aa = random_csr(40, 3000, lens, 67)
        n = 3000
    elif name == "groups16":
        ai, aj, aa = grouped_csr(600, 3000, 71, maxlen=16)
        n = 3000
    else:
        assert name == "fem3"
        ai, aj, aa = pb.gen_fem3(5, 5, 4)
        n = ai.size - 1
    assert np.max(np.abs(aa)) <= 1e3
    return ai, aj, np.ascontiguousarray(aa), n, extras


def clean_x(n, seed):
    return np.clip(np.random.default_rng(seed).standard_normal(n), -1e3, 1e3)


# ------------------------------------------------------------------------------------------------ specials inside the pattern
def special_matrix():
    """The 64 x 64 matrix of IEEE special cases, every row on one lane (<= 16 nonzeros per row on average, one row block).
    Returns dict(ai, aj, aa, x, y0, d, c_slack, expect); expect[row] = (A x, y0 + A x, d .* (A x)) stated by hand for the rows
    described below (None: NaN), the two-at-a-time order of pairsum 1 in expect_pair where it differs."""
    inf, nan = np.inf, np.nan
    n = 64
    x = np.sin(np.arange(n)) + 1.5
    x[:16] = [1.0, -1.0, 2.0, inf, -inf, nan, 0.0, -0.0, 1e-160, 1e300, 3.0, 0.5, 1e300, 1e300, 1e300, nan]
    x[60:] = [inf, -inf, nan, 0.25]
    y0 = np.cos(np.arange(n)) + 2.0
    d = -(np.cos(np.arange(n)) + 1.25)
    rows = [[] for _ in range(n)]
    expect, expect_pair = {}, {}
    # row 0: one entry, product -0.0 * 1.0 = -0.0.  A x = 0.0 + -0.0 = +0.0; y0 = -0.0: -0.0 + -0.0 = -0.0; d = -2 < 0: -2 * +0.0 = -0.0
    rows[0] = [(0, -0.0)]; y0[0] = -0.0; d[0] = -2.0; expect[0] = (0.0, -0.0, -0.0)
    # row 1: the same product from -1.0 * 0.0; d = -0.0: -0.0 * +0.0 = -0.0
    rows[1] = [(6, -1.0)]; y0[1] = -0.0; d[1] = -0.0; expect[1] = (0.0, -0.0, -0.0)
    # row 2: four products, all -0.0: the sum started from +0.0 stays +0.0, started from y0 = -0.0 stays -0.0
    rows[2] = [(0, -0.0), (2, -0.0), (6, -1.0), (7, 1.0)]; y0[2] = -0.0; d[2] = -3.0; expect[2] = (0.0, -0.0, -0.0)
    # rows 3..7: no entries; y0 = d = -0.0, Inf, NaN, -2.5, -Inf.  A x = +0.0; y0 + A x = y0 itself; d .* (A x) = d * 0.0
    for r, v, dz in zip(range(3, 8), (-0.0, inf, nan, -2.5, -inf), (-0.0, None, None, -0.0, None)):
        y0[r] = v; d[r] = v
        expect[r] = (0.0, None if np.isnan(v) else v, dz)
    # rows 8..10: a stored 0.0 / -0.0 times +-Inf: the reference multiplies, NaN
    rows[8] = [(3, 0.0)]
    rows[9] = [(0, 1.0), (3, -0.0)]
    rows[10] = [(4, 0.0)]
    # row 11: +Inf and -Inf products in one row: NaN
    rows[11] = [(3, 1.0), (4, 1.0)]
    for r in (8, 9, 10, 11):
        expect[r] = (None, None, None)
    # row 12: +Inf with finite products: +Inf, y0 + Inf = +Inf, d = -2: -Inf.  Row 13: -Inf likewise
    rows[12] = [(0, 1.0), (2, 5.0), (3, 2.0)]; d[12] = -2.0; expect[12] = (inf, inf, -inf)
    rows[13] = [(0, 1.0), (4, 2.0)]; d[13] = -2.0; expect[13] = (-inf, -inf, inf)
    # row 14: a denormal product (1e-160 * 1e-160); y0 = 0, d = 1: the product itself in every mode
    rows[14] = [(8, 1e-160)]; y0[14] = 0.0; d[14] = 1.0
    p = 1e-160 * 1e-160
    assert 0.0 < p < np.finfo(np.float64).tiny
    expect[14] = (p, p, p)
    # row 15: normal products whose sum ends denormal: 2.5e-308 * 1 + 2.4e-308 * -1
    rows[15] = [(0, 2.5e-308), (1, 2.4e-308)]; y0[15] = 0.0; d[15] = 1.0
    s = 2.5e-308 + (2.4e-308 * -1.0)
    assert 0.0 < s < np.finfo(np.float64).tiny
    expect[15] = (s, s, s)
    # row 16: finite products (1e308 each) that overflow only in the sum: +Inf
    rows[16] = [(9, 1e8), (12, 1e8)]; y0[16] = 1.0; d[16] = 1.0; expect[16] = (inf, inf, inf)
    # row 17: products -1.5e308, 1e308, 1e308, 1e308.  One at a time: -1.5e308 -> -0.5e308 -> 0.5e308 -> 1.5e308, finite.
    # Two at a time (pairsum 1): (-1.5e308 + 1e308) + (1e308 + 1e308 = +Inf) = +Inf
    rows[17] = [(9, -1.5e8), (12, 1e8), (13, 1e8), (14, 1e8)]; y0[17] = 0.0; d[17] = 1.0
    q = [-1.5e8 * 1e300, 1e8 * 1e300]
    s = ((0.0 + q[0]) + q[1]) + q[1] + q[1]
    assert np.isfinite(s) and np.isinf(q[1] + q[1])
    expect[17] = (s, s, s); expect_pair[17] = (inf, inf, inf)
    # rows 18..21: rows across the 8-wide steps of the sum: 9 entries ending in +Inf, 17 ending in -Inf, 8 ending in NaN, 7 finite
    base = [0, 1, 2, 10, 11, 16, 17]
    rows[18] = [(c, 1.0 + 0.25 * i) for i, c in enumerate(base + [18])] + [(60, 1.0)]; d[18] = 2.0; expect[18] = (inf, inf, inf)
    rows[19] = [(c, 1.0 - 0.125 * i) for i, c in enumerate(base + [18, 19, 20, 21, 22, 24, 25, 26, 27])] + [(61, 1.0)]; d[19] = 2.0
    expect[19] = (-inf, -inf, -inf)
    rows[20] = [(c, 2.0) for c in base] + [(62, 1.0)]; expect[20] = (None, None, None)
    rows[21] = [(c, 0.5 + i) for i, c in enumerate(base)]
    # rows 22, 23: -0.0 products from x = -0.0 and from -0.0 * 0.0
    rows[22] = [(7, 5.0)]; y0[22] = 2.5; d[22] = -1.0; expect[22] = (0.0, 2.5, -0.0)
    rows[23] = [(6, -0.0)]; y0[23] = -0.0; d[23] = 4.0; expect[23] = (0.0, -0.0, 0.0)
    # rows 24..59: nine groups of four rows sharing the columns 24 + 4 g .. + 3 (what Mat_CheckInode finds); finite
    for g in range(9):
        for i in range(4):
            rows[24 + 4 * g + i] = [(24 + 4 * g + c, (1.0 + i) * (c - 1.5)) for c in range(4)]
    # rows 60..63: +Inf on the diagonal, 0.0 * -Inf, no entries, the last row finite
    rows[60] = [(60, 1.0)]; d[60] = -1.0; expect[60] = (inf, inf, -inf)
    rows[61] = [(61, 0.0)]; expect[61] = (None, None, None)
    y0[62] = -0.0; d[62] = -7.0; expect[62] = (0.0, -0.0, -0.0)
    rows[63] = [(63, 2.0)]
    ai = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    aj = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    aa = np.array([v for r in rows for _, v in r], dtype=np.float64)
    assert ai[-1] <= SEQ_AVG * n and all(list(c for c, _ in r) == sorted(c for c, _ in r) for r in rows)
    assert not np.any(aj == 5) and not np.any(aj == 15)      # NaN columns no row uses: c_slack, what idle lanes gather
    return dict(ai=ai, aj=aj, aa=aa, x=x, y0=y0, d=d, c_slack=5, expect=expect, expect_pair=expect_pair)


def special_matrix_multilane():
    """17 rows, 12 of them with 81 entries: one row block of more than 16 nonzeros per row, so 8 lanes serve a row and the order
    of the sum is the kernel's tree.  expect[row] = (A x, y0 + A x, d .* (A x)) where IEEE arithmetic fixes the value whatever
    the tree (a float, None for NaN), "any" where it does not:
      * a row without entries: there is nothing to add, so A x = +0.0, y0 + A x = y0 itself (bits, -0.0 included), d .* (A x) = d * 0.0;
      * products that are all -0.0: every partial sum is a sum of +-0.0, and the reference's start +0.0 is one of the terms of
        A x, so A x = +0.0 (x + -0.0 = x, +0.0 + -0.0 = +0.0) and d .* (A x) = d * +0.0; y0 + A x with a non-zero y0 is y0.  With
        y0 = -0.0 every term is -0.0 and the result is -0.0 unless a lane's empty partial sum brings in a +0.0: that depends on
        the tree and is not asserted;
      * a stored 0.0 or -0.0 times +-Inf is NaN and NaN survives every addition."""
    inf, nan = np.inf, np.nan
    n = 200
    x = np.cos(0.3 * np.arange(n)) + 1.5
    x[190:194] = [inf, -inf, nan, nan]
    m = 17
    y0 = np.sin(np.arange(m)) + 2.0
    d = -(np.sin(np.arange(m)) + 1.5)
    rows = [[] for _ in range(m)]
    expect = {}
    for r in (0, 2, 5, 6, 9, 12, 15):                           # finite rows: the 1e-12 bound against the oracle
        rows[r] = [(r + c, 0.5 + 0.01 * ((r * 7 + c * 3) % 11)) for c in range(81)]
    for r, v in zip((1, 3, 7, 10, 13), (-0.0, inf, nan, -2.5, 3.0)):          # no entries
        y0[r] = v; d[r] = v
        with np.errstate(all="ignore"):
            dz = v * 0.0
        expect[r] = (0.0, None if np.isnan(v) else v, None if np.isnan(dz) else dz)
    rows[4] = [(c, -0.0) for c in range(81)]; y0[4] = 2.5; d[4] = -2.0; expect[4] = (0.0, 2.5, -0.0)
    rows[8] = [(c, -0.0) for c in range(81)]; y0[8] = -0.0; d[8] = 3.0; expect[8] = (0.0, "any", 0.0)
    rows[11] = [(20 + c, 1.0) for c in range(80)] + [(190, 0.0)]; expect[11] = (None, None, None)
    rows[14] = [(30 + c, 1.0) for c in range(80)] + [(191, -0.0)]; expect[14] = (None, None, None)
    rows[16] = [(40 + c, 1.0) for c in range(80)] + [(190, 2.0)]; d[16] = -1.0; expect[16] = (inf, inf, -inf)
    ai = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    aj = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    aa = np.array([v for r in rows for _, v in r], dtype=np.float64)
    assert SEQ_AVG * m < ai[-1] <= CAP
    return dict(ai=ai, aj=aj, aa=aa, x=x, y0=y0, d=d, c_slack=192, expect=expect)


def assert_expected(got, expect, col, what):
    """got[row] against the hand-stated value: NaN where None, else the same bits; "any": not asserted"""
    for r, e in expect.items():
        v = e[col]
        if isinstance(v, str):
            continue
        if v is None:
            assert np.isnan(got[r]), "%s row %d: %r, expected NaN" % (what, r, got[r])
        else:
            assert bits(np.array([got[r]]))[0] == bits(np.array([v]))[0], "%s row %d: %r, expected %r" % (what, r, got[r], v)


# ------------------------------------------------------------------------------------------------ the cases both test files walk
C_SLACK = 1           # the valid column the two slack entries behind aj hold (next to column 0, so that the budget of hit rows is not spent twice)
CPROW_M = 5000        # output rows of the compressed-row plans

# form -> shapes (test_spmv_specials_gpu.py: section 1)
CSR_FORMS = [("plain", "p7"), ("plain", "rand16"), ("plain", "band81"), ("plain", "longrow"), ("scalar", "p7"), ("scalar", "longrow"),
             ("idx8", "p7"), ("idx8", "band81"), ("rowpat", "p7"), ("valpat", "p7const"), ("valpat", "p7const_zeros"),
             ("grouped", "groups16"), ("grouped", "fem3")]


def rounds_of(ai, aj, n, rb, extras=(), budget=None, own_rows=0, seed=5):
    """The rounds of a shape: ROUNDS at least, each with c_slack, column 0 and column n - 1.  A block target that the budget of hit
    rows kept out of every round so far comes first in the next one, and rounds are added (up to MAX_ROUNDS) as long as one of
    them takes such a target; the added rounds leave columns 0 and n - 1 out, whose rows would use up the budget (on the
    81-entry band one column hits 81 of 300 rows: columns 0, 1 and 299 leave room for no target in the middle).  The union of
    the rounds then holds every target that fits the budget next to c_slack."""
    targets = list(dict.fromkeys(c for g in block_targets(ai, aj, rb) for c in g))
    Ps, covered = [], set()
    while len(Ps) < MAX_ROUNDS:
        open_ = [c for c in targets if c not in covered]
        P = choose_P(ai, aj, n, rb, C_SLACK, len(Ps), seed, extras, budget, own_rows, first=open_, ends=len(Ps) < ROUNDS)
        if len(Ps) >= ROUNDS and not set(P.tolist()) & set(open_):
            break
        Ps.append(P)
        covered |= set(P.tolist())
    return Ps


def target_coverage(ai, aj, n, rb, Ps, budget=None):
    """(block targets in the union of the rounds, targets that fit the budget next to c_slack, all targets)"""
    budget = (ai.size - 1) // 2 if budget is None else budget
    targets = {c for g in block_targets(ai, aj, rb) for c in g}
    fits = {c for c in targets if hit_rows(ai, aj, [C_SLACK, c], n).sum() <= budget}
    return targets & {int(c) for P in Ps for c in P}, fits, targets


@functools.lru_cache(maxsize=None)
def csr_case(name):
    ai, aj, aa, n, extras = csr_shape(name)
    m = ai.size - 1
    rb, nlong = row_blocks(ai)
    rng = np.random.default_rng(11)
    return dict(ai=ai, aj=aj, aa=aa, n=n, m=m, rb=rb, nlong=nlong, x=clean_x(n, 12), y0=rng.standard_normal(m), d=rng.standard_normal(m),
                Ps=rounds_of(ai, aj, n, rb, extras, own_rows=3 if n == m else 0), one_lane=one_lane_rows(ai, rb))


@functools.lru_cache(maxsize=None)
def cprow_case(k):
    """the compressed-row shapes: (1) 700 listed rows of 0..16 entries, the first 300 of them and every ninth after empty;
    (2) 300 listed rows of 81 entries; (3) 40 listed rows of 0..8 entries, row 7 and the last one of 2500; (4) is (1), uploaded
    off the pair alignment by the test; (5) one listed row; (6) none.  Full-size ai for the oracle next to the compressed one."""
    from test_kernels_gpu import random_csr, rnd
    rng = np.random.default_rng(900 + k)
    if k in (1, 4):
        nl, n = 700, 700
        lens = rng.integers(0, 17, nl); lens[:300] = 0; lens[300::9] = 0
    elif k == 2:
        nl, n = 300, 300
    elif k == 3:
        nl, n = 40, 3000
        lens = rng.integers(0, 9, nl); lens[7] = 2500; lens[-1] = 2500
    else:
        nl, n = (1, 50) if k == 5 else (0, 50)
        lens = np.full(nl, 5)
    if k == 2:
        cai, aj = band(300)
        aa = rnd(aj.size, 901)
    else:
        cai, aj, aa = random_csr(nl, n, lambda r, mm: lens, 902 + (1 if k == 4 else k))
    rows = np.sort(np.random.default_rng(903 + (1 if k == 4 else k)).choice(CPROW_M, size=nl, replace=False)).astype(np.int32)
    rb, nlong = row_blocks(cai)
    ai = expand_rows(cai, rows, CPROW_M)
    listed = np.zeros(CPROW_M, dtype=bool); listed[rows] = True
    one_lane = np.zeros(CPROW_M, dtype=bool); one_lane[rows] = one_lane_rows(cai, rb)
    y0 = -(1e200 + np.arange(CPROW_M, dtype=np.float64) * 1e186)       # a marker that differs per row (step >> ulp(1e200) = 2e184); listed rows: data
    y0[rows] = rng.standard_normal(nl)
    Ps = rounds_of(cai, aj, n, rb, budget=nl // 2) if k in (1, 3) else []
    return dict(cai=cai, ai=ai, aj=aj, aa=np.ascontiguousarray(aa), rows=rows, n=n, m=CPROW_M, rb=rb, nlong=nlong, listed=listed, one_lane=one_lane,
                x=clean_x(n, 13), y0=y0, d=rng.standard_normal(CPROW_M), Ps=Ps)


def bsr_to_csr(bs, ai, aj, aa):
    """point CSR of a BSR matrix (blocks column-major), the entries of a point row in the order blocks, then columns"""
    A = aa.reshape(aj.size, bs, bs)                                    # [blk][col][row]
    cnt = np.diff(ai)
    pai = np.concatenate(([0], np.cumsum(np.repeat(cnt * bs, bs)))).astype(np.int32)
    paj = np.empty(aj.size * bs * bs, dtype=np.int32); paa = np.empty(aj.size * bs * bs)
    for i in range(ai.size - 1):
        blk = slice(int(ai[i]), int(ai[i + 1]))
        cols = (aj[blk, None] * bs + np.arange(bs)[None, :]).ravel()
        for r in range(bs):
            k = pai[i * bs + r]
            paj[k:k + cols.size] = cols
            paa[k:k + cols.size] = A[blk, :, r].ravel()
    return pai, paj, paa


@functools.lru_cache(maxsize=None)
def bsr_case(bs):
    """the `ragged` block structure (block rows of 0..30 blocks, 400 x 500): P in block columns, hit in block rows"""
    from test_abi_kernels_gpu import bsr_shape
    from test_kernels_gpu import rnd
    mbs, nbs, ai, aj = bsr_shape("ragged", bs, 1000 + 10 * bs)
    rb, nlong = row_blocks((ai.astype(np.int64) * bs * bs).astype(np.int32))
    aa = rnd(aj.size * bs * bs, 21)
    pai, paj, paa = bsr_to_csr(bs, ai, aj, aa)
    y0 = rnd(mbs * bs, 23)
    empty = np.flatnonzero(np.repeat(np.diff(ai) == 0, bs))          # point rows of block rows without blocks: z = y0 itself, bit for bit;
    y0[empty[::2]] = -0.0                                            # -0.0 on every other one (y0 + 0.0 would give +0.0)
    return dict(bs=bs, mbs=mbs, nbs=nbs, ai=ai, aj=aj, aa=aa, rb=rb, nlong=nlong, x=clean_x(nbs * bs, 22), y0=y0, empty=empty,
                Ps=rounds_of(ai, aj, nbs, rb), pai=pai, paj=paj, paa=paa)
