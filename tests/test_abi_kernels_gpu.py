"""Parity tests, through the C ABI, for the exported entry points test_kernels_gpu.py does not call (the ledger in
test_host_cpu.py keeps the two modules honest about what include/mi355x_kernels.h exports).

Two kinds of comparison only:
  * bit for bit, where the header names the reference's expression order: the reference is a plain float64 loop written here in
    that order, or the oracle's C loop where one exists;
  * rounding-bounded, for the BSR products (they sum in another order than baij2.c): the same sum in np.longdouble and the
    worst-case bound of test_kernels_gpu.bsr_reference -- derived from the number formats, no chosen constant, no margin."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
from test_kernels_gpu import (SIZES, assert_bitexact, assert_bsr_within_rounding, bits, dev, make_plan, random_csr, rnd,  # noqa: F401 (dev: fixture)
                              upload_csr)
from tri import tri_factor, tri_reference_apply

pytestmark = pytest.mark.gpu

MARK = -7.25e300            # pre-fill of output vectors: a value no product of the test data comes near
CAP = 2046                  # SPMV_BLOCK_CAP (csrc/spmv_csr.hip): values one workgroup of the row-block kernel stages
LANES = 256                 # SPMV_THREADS = SPMV_BLOCK_ROWS


def put_values(dev, aa):
    """the value array with the 16 bytes of slack the header asks for (the kernels read aligned pairs); NaN there: never used"""
    return dev.put(np.concatenate((aa, [np.nan, np.nan])))


def upload_bsr(dev, ai, aj, aa):
    return dev.put(ai), dev.put(aj if aj.size else np.zeros(1, np.int32)), put_values(dev, aa)


def value_plan(dev, ai, bs):
    return make_plan(dev, (ai.astype(np.int64) * bs * bs).astype(np.int32))


def csr_from_counts(cnt, nbs, rng):
    ai = np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)
    aj = np.concatenate([np.sort(rng.choice(nbs, int(c), replace=False)) for c in cnt] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ai, aj


BSR_SHAPES = ["ragged", "few", "wide", "empty_runs", "one_block_row", "few_point_rows"]


def bsr_shape(name, bs, seed):
    """block structures, one per branch of bsr_rowblock_kernel (csrc/spmv_csr.hip): returns (mbs, nbs, ai, aj)"""
    rng = np.random.default_rng(seed)
    if name == "ragged":                 # (a) block rows of 0..30 blocks, rectangular: the staged path, several block rows per row block
        mbs, nbs = 400, 500
        cnt = rng.integers(0, 31, mbs)
    elif name == "few":                  # (b) 0, 1 or 2 blocks: a row block of 256 block rows holds 256 bs point rows > 256 lanes (v2 loop)
        mbs, nbs = 1500, 1500
        cnt = rng.integers(0, 3, mbs); cnt[::5] = 1
    elif name == "wide":                 # (c) block rows of more than SPMV_BLOCK_CAP values among short ones: whole-workgroup path
        wide = CAP // (bs * bs) + 3
        assert wide * bs * bs > CAP
        mbs, nbs = 40, wide + 50
        cnt = np.where(np.arange(mbs) % 7 == 3, wide, rng.integers(0, min(20, CAP // (bs * bs)), mbs))
    elif name == "empty_runs":           # (d) 300 empty block rows in a row (a whole row block with k1 == k0), empty ones between
        mbs, nbs = 1000, 300             # non-empty ones inside a row block, a trailing run of empty ones, a last non-empty one
        cnt = np.zeros(mbs, dtype=np.int64)
        cnt[300:700] = np.tile([2, 0, 0, 1, 0, 3, 0, 0], 50)
        cnt[-1] = 1
        assert LANES < 300
    elif name == "one_block_row":        # (e) mbs = 1
        mbs, nbs = 1, 7
        cnt = np.array([3])
    else:                                # (f) so few point rows per row block that several lanes share a point row (tpr > 1)
        mbs, nbs = 6, 40
        cnt = np.full(mbs, min(20, CAP // (bs * bs)))
        assert 2 * mbs * bs <= LANES
    ai, aj = csr_from_counts(cnt, nbs, rng)
    return mbs, nbs, ai, aj


# ------------------------------------------------------------------------------------------------ 1. BSR products
@pytest.mark.parametrize("shape", BSR_SHAPES)
@pytest.mark.parametrize("bs", [2, 3, 4, 5, 6, 7, 8])
def test_spmv_bsr_rowblock_every_instantiation_and_path(dev, bs, shape):
    """bsr_rowblock_kernel<bs, XLDS> for bs 2..8, both forms (mi355x_spmv_bsr_planned_form), the default entry and the add
    entry: every point row within the worst-case rounding bound of the long-double sum and overwritten; the two forms and two
    runs bit-identical (the "same bits" claim next to MI355X_BSR_XLDS_DEFAULT); z = y + A x with z aliasing y and with a
    separate z (y then untouched)."""
    k = dev.k
    mbs, nbs, ai, aj = bsr_shape(shape, bs, 1000 + 10 * bs + BSR_SHAPES.index(shape))
    m = mbs * bs
    aa = rnd(aj.size * bs * bs, 11); x = rnd(nbs * bs, 12); y0 = rnd(m, 13)
    dai, daj, daa = upload_bsr(dev, ai, aj, aa)
    dx = dev.put(x)
    plan = value_plan(dev, ai, bs)
    nblk, nlong, ws = C.c_int(), C.c_int(), C.c_size_t()
    dev.chk(k.mi355x_spmv_plan_info(plan, C.byref(nblk), C.byref(nlong), C.byref(ws)))
    assert nlong.value == int(np.sum(np.diff(ai) * bs * bs > CAP)) and nlong.value == (6 if shape == "wide" else 0)     # the shape does hit its branch
    assert nblk.value >= max(1, -(-mbs // LANES)) and (shape != "empty_runs" or nblk.value >= 4)
    outs = {}
    for tag in ("form1", "form0", "default", "form1_again"):
        dy = dev.put(np.full(m, MARK))
        if tag == "default":
            dev.chk(k.mi355x_spmv_bsr_planned(dev.h, plan, bs, dai, daj, daa, dx, dy))
        else:
            dev.chk(k.mi355x_spmv_bsr_planned_form(dev.h, plan, bs, 0 if tag == "form0" else 1, dai, daj, daa, dx, dy))
        outs[tag] = dev.get(dy, m)
        dev.free(dy)
        assert not np.any(outs[tag] == MARK), "%s %s: point rows not written: %s" % (shape, tag, np.flatnonzero(outs[tag] == MARK)[:8])
    for tag in ("form1", "form0"):
        assert_bsr_within_rounding(outs[tag], bs, ai, aj, aa, x, what="bsr_rowblock %s %s" % (shape, tag))
    for tag in ("form0", "default", "form1_again"):
        assert np.array_equal(bits(outs[tag]), bits(outs["form1"])), "%s: %s differs from form 1 in %d rows" % (shape, tag, np.sum(bits(outs[tag]) != bits(outs["form1"])))
    # z = y + A x: z aliasing y, then a separate z
    dy = dev.put(y0)
    dev.chk(k.mi355x_spmv_bsr_planned_add(dev.h, plan, bs, dai, daj, daa, dx, dy, dy))
    alias = dev.get(dy, m)
    assert_bsr_within_rounding(alias, bs, ai, aj, aa, x, y0=y0, what="bsr_rowblock %s add" % shape)
    dev.chk(k.mi355x_memcpy_h2d(dev.h, dy, y0.ctypes.data, y0.nbytes))
    dz = dev.put(np.full(m, MARK))
    dev.chk(k.mi355x_spmv_bsr_planned_add(dev.h, plan, bs, dai, daj, daa, dx, dy, dz))
    assert_bitexact(dev.get(dz, m), alias)
    assert_bitexact(dev.get(dy, m), y0)
    dev.chk(k.mi355x_spmv_plan_destroy(plan))
    for q in (dai, daj, daa, dx, dy, dz):
        dev.free(q)


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_spmv_bsr_kernels_exact_on_small_integers(dev, bs):
    """small-integer values and x: every product and partial sum is an exact integer whatever the order, so any swapped row,
    column or block is an integer difference (np.array_equal against MatMult_SeqBAIJ's loop in the oracle).  The wavefront
    kernel for bs 1..8, the row-block kernel's two forms and its add entry for bs 2..8, on every shape."""
    k = dev.k
    for shape in BSR_SHAPES:
        mbs, nbs, ai, aj = bsr_shape(shape, max(bs, 2), 2000 + bs)
        rng = np.random.default_rng(2100 + bs)
        aa = rng.integers(-4, 5, aj.size * bs * bs).astype(np.float64)
        x = rng.integers(-3, 4, nbs * bs).astype(np.float64)
        y0 = rng.integers(-9, 10, mbs * bs).astype(np.float64)
        ref = orc.spmv_bsr(bs, ai, aj, aa, x)
        dai, daj, daa = upload_bsr(dev, ai, aj, aa)
        dx = dev.put(x); dy = dev.put(np.full(mbs * bs, MARK))
        dev.chk(k.mi355x_spmv_bsr(dev.h, mbs, bs, dai, daj, daa, dx, dy))
        assert np.array_equal(dev.get(dy, mbs * bs), ref), (shape, "wavefront kernel")
        if bs > 1:
            plan = value_plan(dev, ai, bs)
            for form in (1, 0):
                dev.chk(k.mi355x_vec_set(dev.h, mbs * bs, MARK, dy))
                dev.chk(k.mi355x_spmv_bsr_planned_form(dev.h, plan, bs, form, dai, daj, daa, dx, dy))
                assert np.array_equal(dev.get(dy, mbs * bs), ref), (shape, "row-block kernel, form %d" % form)
            dev.chk(k.mi355x_memcpy_h2d(dev.h, dy, y0.ctypes.data, y0.nbytes))
            dev.chk(k.mi355x_spmv_bsr_planned_add(dev.h, plan, bs, dai, daj, daa, dx, dy, dy))
            assert np.array_equal(dev.get(dy, mbs * bs), y0 + ref), (shape, "row-block kernel, add")
            dev.chk(k.mi355x_spmv_plan_destroy(plan))
        for q in (dai, daj, daa, dx, dy):
            dev.free(q)


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_spmv_bsr_wavefront_kernel(dev, bs):
    """mi355x_spmv_bsr (one wavefront per block row) for bs 1..8: ragged block rows, and block rows of more than 256 / bs^2
    blocks (beyond the four elements per lane requested up front); rounding bound, empty rows exactly +0.0, reproducible"""
    k = dev.k
    rng = np.random.default_rng(3000 + bs)
    cases = [bsr_shape("ragged", bs, 3100 + bs)]
    long_ = 256 // (bs * bs) + 45
    cnt = np.where(np.arange(20) % 6 == 5, long_, rng.integers(0, 6, 20))
    cases.append((20, long_ + 30) + csr_from_counts(cnt, long_ + 30, rng))
    for mbs, nbs, ai, aj in cases:
        aa = rnd(aj.size * bs * bs, 31); x = rnd(nbs * bs, 32)
        dai, daj, daa = upload_bsr(dev, ai, aj, aa)
        dx = dev.put(x)
        got = []
        for _ in range(2):
            dy = dev.put(np.full(mbs * bs, MARK))
            dev.chk(k.mi355x_spmv_bsr(dev.h, mbs, bs, dai, daj, daa, dx, dy))
            got.append(dev.get(dy, mbs * bs)); dev.free(dy)
        assert not np.any(got[0] == MARK)
        assert_bsr_within_rounding(got[0], bs, ai, aj, aa, x, what="bsr_wave mbs=%d" % mbs)
        assert_bitexact(got[1], got[0])
        for q in (dai, daj, daa, dx):
            dev.free(q)


def test_spmv_bsr_rejects_block_sizes_without_a_kernel(dev):
    """bs = 0 and bs = 9: an error code from each BSR entry, y left alone"""
    k = dev.k
    mbs, nbs, ai, aj = bsr_shape("one_block_row", 2, 1)
    aa = rnd(aj.size * 81, 1); x = rnd(nbs * 9, 2)
    dai, daj, daa = upload_bsr(dev, ai, aj, aa)
    dx = dev.put(x)
    y = np.full(mbs * 9, MARK)
    dy = dev.put(y); dz = dev.put(y)
    plan = value_plan(dev, ai, 2)
    for bs in (0, 9):
        assert k.mi355x_spmv_bsr(dev.h, mbs, bs, dai, daj, daa, dx, dy) != 0
        assert k.mi355x_spmv_bsr_planned(dev.h, plan, bs, dai, daj, daa, dx, dy) != 0
        assert k.mi355x_spmv_bsr_planned_form(dev.h, plan, bs, 0, dai, daj, daa, dx, dy) != 0
        assert k.mi355x_spmv_bsr_planned_add(dev.h, plan, bs, dai, daj, daa, dx, dy, dz) != 0
        assert k.mi355x_pbjacobi_apply(dev.h, mbs, 0, daa, dx, dy) != 0
    assert_bitexact(dev.get(dy, y.size), y); assert_bitexact(dev.get(dz, y.size), y)
    dev.chk(k.mi355x_spmv_plan_destroy(plan))
    for q in (dai, daj, daa, dx, dy, dz):
        dev.free(q)


# ------------------------------------------------------------------------------------------------ 2. the small kernels
@pytest.mark.parametrize("mbs", [1, 63, 64, 65, 100003])
@pytest.mark.parametrize("bs", [1, 2, 3, 5, 7, 8, 11])
def test_pbjacobi_apply_bitexact(dev, bs, mbs):
    """y_i = D_i^-1 x_i, the row's products added left to right (pbjacobi.c:20-200; d[r] x0 + d[r + bs] x1 + ...): the oracle's
    C loop, bit for bit, for any bs >= 1 and random (not SPD-derived) blocks"""
    idiag = rnd(mbs * bs * bs, 40 + bs); x = rnd(mbs * bs, 41)
    did, dx, dy = dev.put(idiag), dev.put(x), dev.put(np.full(mbs * bs, MARK))
    dev.chk(dev.k.mi355x_pbjacobi_apply(dev.h, mbs, bs, did, dx, dy))
    got = dev.get(dy, mbs * bs)
    assert_bitexact(got, orc.pbjacobi_apply(bs, idiag, x))
    if mbs <= 65:                        # the left-to-right loop itself, so that the comparison does not rest on the oracle alone
        ref = np.empty(mbs * bs)
        for row in range(mbs * bs):
            b, r = divmod(row, bs)
            s = idiag[b * bs * bs + r] * x[b * bs]
            for c in range(1, bs):
                s = s + idiag[b * bs * bs + c * bs + r] * x[b * bs + c]
            ref[row] = s
        assert_bitexact(got, ref)
    for q in (did, dx, dy):
        dev.free(q)


@pytest.mark.parametrize("n", SIZES)
def test_jacobi_invert_bitexact_and_refuses_a_count(dev, n):
    """PCSetUp_Jacobi's host loop, jacobi.c:182-190: `if (*x == 0.0) { *x = 1.0; ... } else *x = 1.0 / *x` -- so -0.0 becomes
    1.0 (it compares equal to zero), a denormal is divided (inf or a huge value), 1/inf is 0.0 with inf's sign.  The zero
    entries are not counted: the header says nzero_dev must be NULL; a pointer is refused (hipErrorInvalidValue) and d is
    left alone, instead of the count silently not being written."""
    k = dev.k
    d = rnd(n, 50)
    special = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, np.inf, -np.inf, 1.0, -1.0]
    for j, v in enumerate(special):
        if n:
            d[(j * 37) % n] = v          # n = 1: the last one wins; larger n: all of them somewhere
    if n > 100:
        d[-1] = 0.0; d[n // 2] = -0.0
    with np.errstate(divide="ignore", over="ignore"):
        ref = np.array([1.0 if v == 0.0 else 1.0 / v for v in d.tolist()], dtype=np.float64).reshape(n) if n <= 70000 else np.where(d == 0.0, 1.0, 1.0 / np.where(d == 0.0, 1.0, d))
    dd = dev.put(d)
    cnt = dev.put(np.full(4, -77, dtype=np.int32))
    assert k.mi355x_vec_jacobi_invert(dev.h, n, dd, cnt) == 1          # hipErrorInvalidValue
    assert_bitexact(dev.get(dd, n), d)
    assert np.array_equal(dev.get(cnt, 4, np.int32), np.full(4, -77, dtype=np.int32))
    dev.chk(k.mi355x_vec_jacobi_invert(dev.h, n, dd, None))
    assert_bitexact(dev.get(dd, n), ref)
    dev.free(dd); dev.free(cnt)


def test_csr_diagonal_scale_every_argument_form(dev):
    """a[k] = (a[k] * l[row]) * r[col] (aij.c:2055-2092) with both vectors, either one, neither (values untouched, bit for bit);
    rectangular, rows without entries, m = 0"""
    k = dev.k
    m, n = 1500, 700
    ai, aj, aa = random_csr(m, n, lambda rng, mm: np.where(rng.random(mm) < 0.3, 0, rng.integers(1, 12, mm)), 60)
    l, r = rnd(m, 61), rnd(n, 62)
    dai, daj, _ = upload_csr(dev, ai, aj, aa)
    dl, dr = dev.put(l), dev.put(r)
    for lv, rv in ((l, r), (l, None), (None, r), (None, None)):
        daa = dev.put(aa)
        dev.chk(k.mi355x_csr_diagonal_scale(dev.h, m, dai, daj, daa, dl if lv is not None else None, dr if rv is not None else None))
        got = dev.get(daa, aa.size)
        ref = aa.copy()                                   # the stated order, one entry after the other
        if lv is not None or rv is not None:
            for row in range(m):
                for q in range(ai[row], ai[row + 1]):
                    v = ref[q]
                    if lv is not None:
                        v = v * lv[row]
                    if rv is not None:
                        v = v * rv[aj[q]]
                    ref[q] = v
        assert_bitexact(got, ref)
        assert_bitexact(got, orc.diagonal_scale(ai, aj, aa, lv, rv))
        dev.chk(k.mi355x_csr_diagonal_scale(dev.h, 0, dai, daj, daa, dl, dr))          # m = 0: nothing happens
        assert_bitexact(dev.get(daa, aa.size), got)
        dev.free(daa)
    for q in (dai, daj, dl, dr):
        dev.free(q)


def test_csr_assemble_adds_in_the_reference_order(dev):
    """aa[segslot[s]] += v[order[k]], k = segptr[s] .. segptr[s+1] - 1 in that order, starting from the slot's current value
    (MatSetValues(ADD_VALUES) one after the other, matrix.c:1715-1718).  Contributions spread over 24 orders of magnitude, so
    another order of additions changes bits; segments of 0, 1 and many contributions; `order` a shuffled permutation; slots no
    segment names are untouched; nseg = 0 does nothing."""
    k = dev.k
    rng = np.random.default_rng(70)
    nslots, nseg = 4000, 2500
    aa = rng.standard_normal(nslots)
    segslot = rng.choice(nslots, nseg, replace=False).astype(np.int32)
    cnt = rng.choice([0, 1, 2, 7, 40, 300], nseg, p=[0.1, 0.2, 0.2, 0.3, 0.15, 0.05])
    segptr = np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)
    K = int(segptr[-1])
    order = rng.permutation(K).astype(np.int32)
    assert not np.array_equal(order, np.arange(K))
    v = rng.standard_normal(K) * 10.0 ** rng.uniform(-12, 12, K)
    ref = aa.copy()
    for s in range(nseg):
        acc = ref[segslot[s]]
        for q in range(segptr[s], segptr[s + 1]):
            acc = acc + v[order[q]]
        ref[segslot[s]] = acc
    resorted = aa.copy()                                  # the test's own teeth: the same sums in sorted order differ in bits
    for s in range(nseg):
        resorted[segslot[s]] += np.sum(np.sort(v[order[segptr[s]:segptr[s + 1]]]))
    assert np.sum(bits(resorted) != bits(ref)) > nseg // 10
    daa, dptr, dslot, dord, dv = dev.put(aa), dev.put(segptr), dev.put(segslot), dev.put(order), dev.put(v)
    dev.chk(k.mi355x_csr_assemble(dev.h, 0, dptr, dslot, dord, dv, daa))
    assert_bitexact(dev.get(daa, nslots), aa)
    dev.chk(k.mi355x_csr_assemble(dev.h, nseg, dptr, dslot, dord, dv, daa))
    got = dev.get(daa, nslots)
    assert_bitexact(got, ref)
    untouched = np.setdiff1d(np.arange(nslots), segslot)
    assert untouched.size and np.array_equal(bits(got[untouched]), bits(aa[untouched]))
    for q in (daa, dptr, dslot, dord, dv):
        dev.free(q)


def test_unpack_max_is_petscmax_element_by_element(dev):
    """UnPack_1 with MAX_VALUES (vpscat.c:503-534): y[idx[k]] = PetscMax(y[idx[k]], buf[k]) with petscmath.h's
    `#define PetscMax(a,b) (((a)<(b)) ? (b) : (a))`.  Evaluated as written: equal values keep y; +0.0 against -0.0 keeps y
    either way round (0.0 < -0.0 and -0.0 < 0.0 are both false); NaN in buf is dropped (y < NaN is false: y stays); NaN in y
    STAYS (NaN < v is false as well) -- an fmax would return the other operand in both NaN cases and +0.0 for (-0.0, +0.0).
    The expected bits are written out below; np.maximum / fmax are not consulted."""
    k = dev.k
    nan = np.nan
    #            y      buf    expected
    table = [(1.0, 2.0, 2.0), (2.0, 1.0, 2.0), (3.0, 3.0, 3.0), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (1.0, nan, 1.0), (nan, 1.0, nan),
             (-np.inf, -1e308, -1e308), (np.inf, 1.0, np.inf), (-5e-324, 0.0, 0.0), (nan, nan, nan), (-2.0, -3.0, -2.0)]
    reps = 1201
    yv = np.tile([t[0] for t in table], reps); bv = np.tile([t[1] for t in table], reps); ev = np.tile([t[2] for t in table], reps)
    n = yv.size
    ref = np.array([(v if a < v else a) for a, v in zip(yv.tolist(), bv.tolist())])      # (y < v) ? v : y
    assert np.array_equal(np.isnan(ref), np.isnan(ev)) and np.array_equal(bits(ref[~np.isnan(ev)]), bits(ev[~np.isnan(ev)]))

    def check(got, exp):
        assert np.array_equal(np.isnan(got), np.isnan(exp))
        ok = ~np.isnan(exp)
        assert np.array_equal(bits(got[ok]), bits(exp[ok])), np.flatnonzero(bits(got[ok]) != bits(exp[ok]))[:8]
    # contiguous (idx == NULL)
    dy, db = dev.put(yv), dev.put(bv)
    dev.chk(k.mi355x_unpack_max(dev.h, n, None, db, dy))
    check(dev.get(dy, n), ev)
    # distinct indices into a longer vector: the entries not named keep their bits
    big = 3 * n + 5
    idx = np.random.default_rng(80).permutation(big)[:n].astype(np.int32)
    ybig = rnd(big, 81); ybig[idx] = yv
    exp = ybig.copy(); exp[idx] = ev
    dyb, didx = dev.put(ybig), dev.put(idx)
    dev.chk(k.mi355x_unpack_max(dev.h, n, didx, db, dyb))
    check(dev.get(dyb, big), exp)
    # n = 0 for pack and the three unpacks: nothing is read or written
    before = dev.get(dyb, big)
    dev.chk(k.mi355x_pack(dev.h, 0, didx, dyb, db))
    for fn in (k.mi355x_unpack_insert, k.mi355x_unpack_add, k.mi355x_unpack_max):
        dev.chk(fn(dev.h, 0, didx, db, dyb)); dev.chk(fn(dev.h, 0, None, db, dyb))
    after = dev.get(dyb, big)
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    check(dev.get(db, n), bv)
    for q in (dy, db, dyb, didx):
        dev.free(q)


def test_stream_triad_memset_memcpy_d2d(dev):
    """a = b + alpha c (a rounded product, then a rounded sum), mi355x_memset and mi355x_memcpy_d2d: sizes 0, 1, 4097, on
    16-byte aligned vectors and on views that start 8 bytes off; what lies around the range keeps its bits"""
    k = dev.k
    for n in (0, 1, 4097):
        for off in (0, 1):
            tot = n + off + 3
            a0, b, c = rnd(tot, 90), rnd(tot, 91), rnd(tot, 92)
            da, db, dc = dev.put(a0), dev.put(b), dev.put(c)

            def view(p):
                return C.c_void_p(p.value + 8 * off)
            dev.chk(k.mi355x_stream_triad(dev.h, n, 0.37, view(db), view(dc), view(da)))
            exp = a0.copy(); t = 0.37 * c[off:off + n]; exp[off:off + n] = b[off:off + n] + t
            assert_bitexact(dev.get(da, tot), exp)
            dev.chk(k.mi355x_memcpy_d2d(dev.h, view(dc), view(da), 8 * n))
            expc = c.copy(); expc[off:off + n] = exp[off:off + n]
            assert_bitexact(dev.get(dc, tot), expc)
            dev.chk(k.mi355x_memset(dev.h, view(db), 0xA5, 8 * n))
            expb = b.copy(); expb[off:off + n] = np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.float64)
            assert_bitexact(dev.get(db, tot), expb)
            for q in (da, db, dc):
                dev.free(q)


def test_graph_capture_replays_with_the_buffers_current_contents(dev):
    """mi355x_graph_capture_begin / _end / _launch / _destroy on one stream, a linear chain (as ilu.c captures its level
    launches): y += a x; s = x'y into a device scalar; p = x + (s / den) p reading it.  Replayed three times with the CONTENTS of
    the buffers changed between replays (scalars passed by value are frozen at capture): each replay leaves the bits of the same
    three calls issued directly."""
    k = dev.k
    n, a, den = 4097, 0.37, 1.9
    dx, dy, dp, ds = dev.alloc(8 * n), dev.alloc(8 * n), dev.alloc(8 * n), dev.alloc(16)
    ex, ey, ep, es = dev.alloc(8 * n), dev.alloc(8 * n), dev.alloc(8 * n), dev.alloc(16)

    def chain(x, y, p, s):
        rc = k.mi355x_vec_axpy(dev.h, n, a, x, y)
        rc = rc or k.mi355x_vec_dot(dev.h, n, x, y, s)
        return rc or k.mi355x_vec_aypx_dev(dev.h, n, s, den, x, p)

    def load(bufs, seed):
        for j, q in enumerate(bufs):
            v = rnd(n, seed + j)
            dev.chk(k.mi355x_memcpy_h2d(dev.h, q, v.ctypes.data, v.nbytes)); dev.sync()
    load((dx, dy, dp), 100)
    dev.sync()
    dev.chk(k.mi355x_graph_capture_begin(dev.h))
    rc = chain(dx, dy, dp, ds)
    g = C.c_void_p()
    rc_end = k.mi355x_graph_capture_end(dev.h, C.byref(g))
    assert rc == 0 and rc_end == 0 and g.value
    for rep in range(3):
        load((dx, dy, dp), 200 + 10 * rep); load((ex, ey, ep), 200 + 10 * rep)
        dev.chk(k.mi355x_graph_launch(dev.h, g))
        dev.chk(chain(ex, ey, ep, es))
        dev.sync()
        for u, v, cnt in ((dy, ey, n), (dp, ep, n), (ds, es, 1), (dx, ex, n)):
            assert_bitexact(dev.get(u, cnt), dev.get(v, cnt))
        xh, yh = rnd(n, 200 + 10 * rep), rnd(n, 201 + 10 * rep)
        orc.vec_axpy(yh, a, xh)
        assert_bitexact(dev.get(dy, n), yh)               # and the replay did run on the new contents
    dev.chk(k.mi355x_graph_destroy(g))
    for q in (dx, dy, dp, ds, ex, ey, ep, es):
        dev.free(q)


# ------------------------------------------------------------------------------------------------ 3. triangular solves
TRI_APPLY_SHAPES = ["wide", "ragged", "chain", "tiny", "empty_rows", "n1", "n64", "n65", "longrow"]    # not deepchain: 47 000 sequential hand-offs


@functools.lru_cache(maxsize=None)
def _tri_case(shape, scaled):
    f = tri_factor(shape, 4000 + TRI_APPLY_SHAPES.index(shape), scaled)
    rhs = [rnd(f["n"], 4100 + j) for j in range(3)]
    return f, rhs, [tri_reference_apply(f, b) for b in rhs]


# (route, family): `onewave` switches the split-role kernels off; `default` leaves MI355X_TRISOLVE_SPLIT unset, which sends these
# narrow shapes (n >= 64) through "every row a node of its own" -- that route ignores the build route, so it runs once, under host
@pytest.mark.parametrize("route,family", [pytest.param("host", "onewave", id="host"), pytest.param("device", "onewave", id="device"),
                                          pytest.param("host", "default", id="host-default")])
@pytest.mark.parametrize("kind", ["upper", "upper_scaled"])
@pytest.mark.parametrize("shape", TRI_APPLY_SHAPES)
def test_trisolve_apply_on_synthetic_shapes_bitexact(dev, shape, kind, route, family, monkeypatch):
    """mi355x_trisolve_plan_create_pair (both build routes) + mi355x_trisolve_apply / _apply_levels on the shapes the plan-build
    test generates: long rows of thousands of entries, n = 1 / 64 / 65, rows without entries, a dense 5 x 5.  Lower plan from the
    structure, upper plan from its mirror image with an inverted diagonal, `upper_scaled` with ICC(0)'s right-hand-side scale.
    Three applications in a row with different right-hand sides each equal their own reference bit for bit (a hand-off buffer not
    returned to the sentinel shows up only then); the level-by-level application leaves the same bits; no application reports an
    abort.  family `default`: the kernel family the library chooses by itself -- for n >= 64 single-row node plans (NB = 1) on the
    split-role kernels with their end-aligned lists and right-hand-side scale (n64 / n65: slice boundaries; longrow: more batches than
    the LDS ring holds; chain: sub-steps inside a slice, solved by the solver wavefront with the one-wavefront routine); one product
    after the other, so the same reference.  Reference: tri.tri_reference_apply, validated on the CPU against scipy (test_host_cpu.py).  ilu.c never applies with
    b aliasing y, so that is not exercised."""
    k = dev.k
    monkeypatch.setenv("MI355X_TRISOLVE_BUILD", route)
    if family == "onewave":
        monkeypatch.setenv("MI355X_TRISOLVE_SPLIT", "0")
    else:
        monkeypatch.delenv("MI355X_TRISOLVE_SPLIT", raising=False)
    f, rhs, refs = _tri_case(shape, kind == "upper_scaled")
    n = f["n"]
    where = "shape %s, %s, build route %s, family %s" % (shape, kind, route, family)
    lo, up = C.c_void_p(), C.c_void_p()
    p = lambda a: a.ctypes.data if a is not None else None      # noqa: E731
    rc = k.mi355x_trisolve_plan_create_pair(dev.h, n, 0, f["nlev"], p(f["lev"]), p(f["rp"]), p(f["rl"]), p(f["cj"]), p(f["cv"]),
                                            f["nlev"], p(f["levu"]), p(f["rpu"]), p(f["rlu"]), p(f["cju"]), p(f["cvu"]), p(f["dinv"]), p(f["rscale"]),
                                            C.byref(lo), C.byref(up))
    assert rc == 0 and lo.value and up.value, "plan_create_pair rc = %d (%s)" % (rc, where)
    db, dy = dev.alloc(8 * n), dev.alloc(8 * n)
    flag = C.c_int(-1)
    try:
        for levels in (False, True):
            for j, (b, ref) in enumerate(zip(rhs, refs)):
                dev.chk(k.mi355x_memcpy_h2d(dev.h, db, b.ctypes.data, b.nbytes))
                dev.chk(k.mi355x_vec_set(dev.h, n, MARK, dy))
                rc = (k.mi355x_trisolve_apply_levels if levels else k.mi355x_trisolve_apply)(dev.h, lo, up, db, dy)
                assert rc == 0, "application %d returned %d (%s, levels = %s)" % (j, rc, where, levels)
                got = dev.get(dy, n)
                for pl in (lo, up):
                    dev.chk(k.mi355x_trisolve_aborted(pl, C.byref(flag)))
                    assert flag.value == 0, "application %d reported an abort (%s, levels = %s)" % (j, where, levels)
                assert np.array_equal(bits(got), bits(ref)), "application %d (%s, levels = %s): %d of %d entries differ, max |diff| %g" % (
                    j, where, levels, int(np.sum(bits(got) != bits(ref))), n, float(np.max(np.abs(got - ref))))
                assert_bitexact(dev.get(db, n), b)                # the right-hand side is read only
    finally:
        k.mi355x_trisolve_plan_destroy(lo); k.mi355x_trisolve_plan_destroy(up)
        dev.free(db); dev.free(dy)


def _ilu0_levels(f):
    bi, bj, bd, _ = f
    n = bi.size - 1
    levL = np.zeros(n, dtype=np.int64); levU = np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = bj[bi[i]:bi[i + 1]]
        levL[i] = levL[c].max() + 1 if c.size else 0
    for i in range(n - 1, -1, -1):
        c = bj[bd[i + 1] + 1:bd[i]]
        levU[i] = levU[c].max() + 1 if c.size else 0
    return levL, levU


@pytest.mark.parametrize("problem", ["p7", "random"])
def test_ilu0_level_kernels_bitexact(dev, problem):
    """mi355x_ilu0_lower_level / _upper_level on the reference's own factor layout (aijfact.c:1628-1700), one launch per
    dependency level with the level lists computed here: all levels in order == MatSolve_SeqAIJ_NaturalOrdering (the oracle's
    loop), bit for bit; the lower sweep with b aliasing x, as the captured form in ilu.c runs it, and with a separate b."""
    k = dev.k
    if problem == "p7":
        ai, aj, aa = orc.gen_p7(9, 7, 5)
        aa = aa * (1.0 + 0.05 * np.cos(np.arange(aa.size)))
    else:
        import scipy.sparse as sp
        n = 900
        rng = np.random.default_rng(5000)
        A = sp.random(n, n, density=0.01, random_state=rng, data_rvs=rng.standard_normal).tocsr()
        A = (A + sp.diags(np.abs(A).sum(axis=1).A1 + 1.0)).tocsr(); A.sort_indices()
        ai, aj, aa = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()
    n = ai.size - 1
    f = orc.ilu0_factor(ai, aj, aa)
    bi, bj, bd, ba = f
    levL, levU = _ilu0_levels(f)
    assert levL.max() >= 3 and levU.max() >= 3
    b = rnd(n, 5001)
    ref = orc.ilu0_solve(f, b)
    dbi, dbj, dbd, dba = dev.put(bi), dev.put(bj), dev.put(bd), dev.put(ba)
    rowsL = [np.flatnonzero(levL == l).astype(np.int32) for l in range(int(levL.max()) + 1)]
    rowsU = [np.flatnonzero(levU == l).astype(np.int32) for l in range(int(levU.max()) + 1)]
    dL = [dev.put(r) for r in rowsL]; dU = [dev.put(r) for r in rowsU]
    for alias in (True, False):
        db = dev.put(b)
        dx = db if alias else dev.put(np.full(n, MARK))
        for r, dr in zip(rowsL, dL):
            dev.chk(k.mi355x_ilu0_lower_level(dev.h, r.size, dr, dbi, dbj, dba, db, dx))
        for r, dr in zip(rowsU, dU):
            dev.chk(k.mi355x_ilu0_upper_level(dev.h, r.size, dr, dbj, dba, dbd, dx))
        assert_bitexact(dev.get(dx, n), ref)
        if not alias:
            assert_bitexact(dev.get(db, n), b)
            dev.free(dx)
        dev.free(db)
    dev.chk(k.mi355x_ilu0_lower_level(dev.h, 0, dL[0], dbi, dbj, dba, None, None))       # an empty level launches nothing
    dev.chk(k.mi355x_ilu0_upper_level(dev.h, 0, dU[0], dbj, dba, dbd, None))
    for q in [dbi, dbj, dbd, dba] + dL + dU:
        dev.free(q)


def _ilu0_row_arrays(f):
    """the arguments ilu.c derives from the reference's factor layout (ilu0_row_arrays): L rows at bi, U row i at bdiag[i+1]+1 with
    bdiag[i] - bdiag[i+1] - 1 entries, the inverted diagonal at bdiag[i]"""
    bi, bj, bd, ba = f
    n = bi.size - 1
    rlL = np.diff(bi).astype(np.int32)
    rpU = (bd[1:] + 1).astype(np.int32); rlU = (bd[:-1] - bd[1:] - 1).astype(np.int32)
    dinv = ba[bd[:n]].copy()
    return np.ascontiguousarray(bi[:n]), rlL, rpU, rlU, dinv


def _apply_and_compare(dev, lo, up, rhs, refs, where, levels=(False, True)):
    k = dev.k
    n = rhs[0].size
    db, dy = dev.alloc(8 * n), dev.alloc(8 * n)
    flag = C.c_int(-1)
    for lv in levels:
        for j, (b, ref) in enumerate(zip(rhs, refs)):
            dev.chk(k.mi355x_memcpy_h2d(dev.h, db, b.ctypes.data, b.nbytes))
            dev.chk(k.mi355x_vec_set(dev.h, n, MARK, dy))
            rc = (k.mi355x_trisolve_apply_levels if lv else k.mi355x_trisolve_apply)(dev.h, lo, up, db, dy)
            assert rc == 0, "application %d returned %d (%s, levels = %s)" % (j, rc, where, lv)
            got = dev.get(dy, n)
            for pl in (lo, up):
                dev.chk(k.mi355x_trisolve_aborted(pl, C.byref(flag)))
                assert flag.value == 0, "application %d reported an abort (%s, levels = %s)" % (j, where, lv)
            assert np.array_equal(bits(got), bits(ref)), "application %d (%s, levels = %s): %d of %d entries differ" % (
                j, where, lv, int(np.sum(bits(got) != bits(ref))), n)
    dev.free(db); dev.free(dy)


def test_trisolve_plans_built_one_by_one_on_a_real_factor_and_the_abort_flag(dev, monkeypatch):
    """mi355x_trisolve_plan_create_ordered (column order) for the lower and the upper factor of an ILU(0) factorisation, with the
    arguments of ilu.c: MatSolve_SeqAIJ_NaturalOrdering's bits.  mi355x_trisolve_debug_set_aborted raises the flag a wait that
    gave up would raise: the sync-free application then refuses (hipErrorLaunchFailure, y untouched), the level-by-level one does
    not consult it and leaves the same bits, and with the flag lowered again the sync-free application runs as before."""
    k = dev.k
    monkeypatch.setenv("MI355X_TRISOLVE_SPLIT", "0")
    ai, aj, aa = orc.gen_p7(12, 9, 7)
    aa = aa * (1.0 + 0.05 * np.cos(np.arange(aa.size)))
    f = orc.ilu0_factor(ai, aj, aa)
    bi, bj, bd, ba = f
    n = ai.size - 1
    rpL, rlL, rpU, rlU, dinv = _ilu0_row_arrays(f)
    levL, levU = [a.astype(np.int32) for a in _ilu0_levels(f)]
    rhs = [rnd(n, 6000 + j) for j in range(3)]
    refs = [orc.ilu0_solve(f, b) for b in rhs]
    lo, up = C.c_void_p(), C.c_void_p()
    dev.chk(k.mi355x_trisolve_plan_create_ordered(dev.h, n, int(levL.max()) + 1, levL.ctypes.data, rpL.ctypes.data, rlL.ctypes.data, bj.ctypes.data,
                                                  ba.ctypes.data, None, 0, C.byref(lo)))
    dev.chk(k.mi355x_trisolve_plan_create_ordered(dev.h, n, int(levU.max()) + 1, levU.ctypes.data, rpU.ctypes.data, rlU.ctypes.data, bj.ctypes.data,
                                                  ba.ctypes.data, dinv.ctypes.data, 0, C.byref(up)))
    try:
        _apply_and_compare(dev, lo, up, rhs, refs, "create_ordered on ILU(0) of P7")
        flag = C.c_int(-1)
        db, dy = dev.put(rhs[0]), dev.put(np.full(n, MARK))
        for pl in (lo, up):
            dev.chk(k.mi355x_trisolve_debug_set_aborted(pl, 1))
            dev.chk(k.mi355x_trisolve_aborted(pl, C.byref(flag))); assert flag.value == 1
            assert k.mi355x_trisolve_apply(dev.h, lo, up, db, dy) == 719          # hipErrorLaunchFailure, nothing launched
            assert_bitexact(dev.get(dy, n), np.full(n, MARK))
            dev.chk(k.mi355x_trisolve_apply_levels(dev.h, lo, up, db, dy))
            assert_bitexact(dev.get(dy, n), refs[0])
            dev.chk(k.mi355x_trisolve_aborted(pl, C.byref(flag))); assert flag.value == 1      # ... and does not change it
            dev.chk(k.mi355x_trisolve_debug_set_aborted(pl, 0))
            dev.chk(k.mi355x_vec_set(dev.h, n, MARK, dy))
        dev.free(db); dev.free(dy)
        _apply_and_compare(dev, lo, up, rhs[:1], refs[:1], "after the flag was lowered", levels=(False,))
    finally:
        k.mi355x_trisolve_plan_destroy(lo); k.mi355x_trisolve_plan_destroy(up)


@pytest.mark.parametrize("how", ["pair", "single"])
def test_trisolve_node_plans_built_directly_bitexact(dev, how):
    """mi355x_trisolve_plan_create_nodes_pair / _create_nodes on the ILU(0) factor of a matrix with inodes (3 dof per node), with
    the arguments ilu.c hands over: node levels from a node's first row (lower) / last row (upper), column order.  Bit for bit
    MatSolve_SeqAIJ_Inode (the oracle's restatement), sync-free and level by level, three right-hand sides in a row."""
    import problems as pb
    k = dev.k
    ai, aj, aa = pb.gen_fem3(7, 6, 5)
    n = ai.size - 1
    nodes, ns = orc.check_inode(ai, aj)
    assert nodes > 0 and int(np.sum(ns)) == n
    f = orc.ilu0_factor(ai, aj, aa)
    bi, bj, bd, ba = f
    rpL, rlL, rpU, rlU, dinv = _ilu0_row_arrays(f)
    nstart = np.concatenate(([0], np.cumsum(ns))).astype(np.int32)
    nodeof = np.repeat(np.arange(nodes), ns)
    nlevL = np.zeros(nodes, dtype=np.int32); nlevU = np.zeros(nodes, dtype=np.int32)
    for u in range(nodes):
        r0 = nstart[u]
        c = nodeof[bj[bi[r0]:bi[r0 + 1]]]
        nlevL[u] = nlevL[c].max() + 1 if c.size else 0
    for u in range(nodes - 1, -1, -1):
        rl_ = nstart[u + 1] - 1
        c = nodeof[bj[rpU[rl_]:rpU[rl_] + rlU[rl_]]]
        nlevU[u] = nlevU[c].max() + 1 if c.size else 0
    nlL, nlU = int(nlevL.max()) + 1, int(nlevU.max()) + 1
    rhs = [rnd(n, 6100 + j) for j in range(3)]
    refs = [orc.ilu0_solve_inode(f, ns, b) for b in rhs]
    lo, up = C.c_void_p(), C.c_void_p()
    p = lambda a: a.ctypes.data      # noqa: E731
    if how == "pair":
        dev.chk(k.mi355x_trisolve_plan_create_nodes_pair(dev.h, n, nodes, p(nstart), 0, 0, nlL, p(nlevL), p(rpL), p(rlL), nlU, p(nlevU), p(rpU), p(rlU),
                                                         p(bj), p(ba), p(dinv), C.byref(lo), C.byref(up)))
    else:
        dev.chk(k.mi355x_trisolve_plan_create_nodes(dev.h, n, nodes, p(nstart), nlL, p(nlevL), p(rpL), p(rlL), p(bj), p(ba), None, 0, 0, C.byref(lo)))
        dev.chk(k.mi355x_trisolve_plan_create_nodes(dev.h, n, nodes, p(nstart), nlU, p(nlevU), p(rpU), p(rlU), p(bj), p(ba), p(dinv), 0, 0, C.byref(up)))
    try:
        _apply_and_compare(dev, lo, up, rhs, refs, "node plans (%s) on ILU(0) of fem3" % how)
    finally:
        k.mi355x_trisolve_plan_destroy(lo); k.mi355x_trisolve_plan_destroy(up)


def test_spmv_tiled_drop_host_keeps_the_device_product(dev):
    """mi355x_spmv_tiled_drop_host releases the host copy of the layout only: the layout can no longer be read back
    (hipErrorInvalidValue), the product on the device carries the same bits as before, new values still reach it"""
    import tiled
    k = dev.k
    m = n = 5000
    ai, aj, aa = random_csr(m, n, lambda rng, mm: rng.integers(0, 30, mm), 7000)
    x = rnd(n, 7001)
    plan = tiled.build(k, ai, aj, n, 64)
    try:
        daa = put_values(dev, aa); dx = dev.put(x); dy = dev.put(np.full(m, MARK))
        dev.chk(k.mi355x_spmv_tiled_upload(dev.h, plan, daa))
        ref = tiled.apply(k, plan, m, aa, x)                      # the layout's own order, from the host copy
        dev.chk(k.mi355x_spmv_tiled(dev.h, plan, dx, None, dy))
        assert_bitexact(dev.get(dy, m), ref)
        dev.chk(k.mi355x_spmv_tiled_drop_host(plan))
        nb = C.c_size_t()
        assert k.mi355x_spmv_tiled_debug_get(plan, 0, None, 0, C.byref(nb)) == 1
        dev.chk(k.mi355x_vec_set(dev.h, m, MARK, dy))
        dev.chk(k.mi355x_spmv_tiled(dev.h, plan, dx, None, dy))
        assert_bitexact(dev.get(dy, m), ref)
        aa2 = aa * 1.7 - 0.3
        dev.chk(k.mi355x_memcpy_h2d(dev.h, daa, aa2.ctypes.data, aa2.nbytes)); dev.sync()
        dev.chk(k.mi355x_spmv_tiled_refresh_values(dev.h, plan, daa))
        dev.chk(k.mi355x_spmv_tiled(dev.h, plan, dx, None, dy))
        scale = np.zeros(m); np.add.at(scale, np.repeat(np.arange(m), np.diff(ai)), np.abs(aa2 * x[aj]))
        assert np.all(np.abs(dev.get(dy, m) - orc.spmv(ai, aj, aa2, x)) <= 1e-12 * scale + 1e-300)      # the header's stated tolerance
        for q in (daa, dx, dy):
            dev.free(q)
    finally:
        k.mi355x_spmv_tiled_destroy(plan)
