"""mi355x_spmv_csr_residual (r = b - A x in the product's own launch) against the two calls it replaces -- mi355x_spmv_csr into a work
vector, then mi355x_vec_aypx(w, -1, b) -- bit for bit, through the C ABI.

Every form launch_spmv dispatches (plain with pair loads, plain with the scalar stream, 8-bit offsets, row patterns, value patterns,
grouped rows), forced the way test_spmv_specials_gpu.py forces them, both summation orders (pairsum), m in {1, 63, 64, 65, 257, 1000},
row lengths from 0 up to 257 in runs of equal length, so that blocks of empty rows, one-lane rows and the lane tree (few long rows per
block) all occur; the dictionary forms stop at the row length their analysis accepts (256 distinct offsets, 512 table slots).  r sits
between 64 poisoned doubles on either side.  Where a NaN is produced its position is compared, everything else by bits.  The matrices
of the dictionary forms and of the grouped form are rectangular by construction (n = m + the widest row's reach); test_rectangular adds
wide, tall and one-column shapes for the two plain forms.  The row-pattern form runs with run-coded blocks switched on and off."""
import ctypes as C

import numpy as np
import pytest

from test_kernels_gpu import assert_bitexact, dev  # noqa: F401 (dev: fixture)
import pattern_runs as pr
from test_spmv_specials_gpu import Csr

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = np.uint64(0xFFF8DEADBEEF0BAD)                      # a NaN payload no kernel produces
SIZES = (1, 63, 64, 65, 257, 1000)
FORMS = ("plain", "scalar", "idx8", "rowpat", "valpat", "grouped")
LENS = {"plain": (3, 0, 1, 2, 8, 17, 40, 100, 257, 16, 130), "scalar": (3, 0, 1, 2, 8, 17, 40, 100, 257, 16, 130),
        "grouped": (3, 0, 1, 2, 8, 17, 40, 100, 257, 16, 130),
        "idx8": (3, 0, 1, 2, 8, 17, 40, 100, 256), "rowpat": (3, 0, 1, 2, 8, 17, 40, 100, 200), "valpat": (3, 0, 1, 2, 7, 9, 17, 40, 100)}
RUN = 4                                                     # consecutive rows of one length (<= the inode limit of 5: grouped rows)
STRIDE = 3


class Banded:
    """row r has LENS[(r // RUN) % ..] entries at columns base + STRIDE q: base = r (the dictionary forms: a fixed offset list per
    length) or the first row of r's run (grouped: the rows of a run share one column list); n = m + the widest row, so no row is cut.
    The plain forms get random columns of a square matrix instead.  pattern_values: a row's values depend on its length only."""
    def __init__(self, form, m, seed=0, n=None, special_values=False):
        rng = np.random.default_rng(1000 * m + seed)
        cyc = LENS[form]
        lens = np.array([cyc[(r // RUN) % len(cyc)] for r in range(m)], dtype=np.int64)
        self.m = m
        if form in ("plain", "scalar"):
            self.n = m if n is None else n
            lens = np.minimum(lens, self.n)
            cols = [np.sort(rng.choice(self.n, int(L), replace=False)) for L in lens]
        else:
            self.n = m + STRIDE * max(cyc) + 1
            base = (np.arange(m) // RUN) * RUN if form == "grouped" else np.arange(m)
            cols = [base[r] + STRIDE * np.arange(int(lens[r])) for r in range(m)]
        self.ai = np.zeros(m + 1, dtype=np.int32)
        self.ai[1:] = np.cumsum(lens)
        self.aj = (np.concatenate(cols) if m else np.zeros(0)).astype(np.int32)
        if form == "valpat":
            table = {L: np.random.default_rng(L).standard_normal(L) for L in cyc}
            if special_values:
                table[7][[1, 4]] = [np.inf, -0.0]; table[17][3] = np.nan; table[40][[0, 39]] = [-np.inf, -0.0]
            self.aa = np.concatenate([table[int(L)] for L in lens]) if m else np.zeros(0)
        else:
            self.aa = rng.standard_normal(self.aj.size)
            if special_values and self.aa.size:
                at = rng.choice(self.aa.size, min(self.aa.size, 12), replace=False)
                self.aa[at] = np.resize([np.nan, np.inf, -np.inf, -0.0], at.size)
        self.lens = lens

    def csr(self, dev, form, rows=None):
        return Csr(dev, self.ai, self.aj, self.aa, 0, self.n, form=form, rows=rows, nan_values=form == "valpat")


class Guarded:
    def __init__(self, dev, a):
        self.dev, self.m = dev, a.size
        h = np.empty(a.size + 2 * GUARD)
        h.view(np.uint64)[:] = POISON
        h[GUARD:GUARD + a.size] = a
        self.base = dev.put(h)
        self.p = C.c_void_p(self.base.value + 8 * GUARD)

    def get(self):
        h = self.dev.get(self.base, self.m + 2 * GUARD)
        g = np.concatenate((h.view(np.uint64)[:GUARD], h.view(np.uint64)[GUARD + self.m:]))
        assert np.all(g == POISON), "poisoned doubles around r were overwritten: %s" % np.flatnonzero(g != POISON)
        return h[GUARD:GUARD + self.m].copy()


def two_calls(dev, csr, dx, b):
    """the sequence the kernel replaces: w = A x, then w = b - w (mi355x_vec_aypx with alpha = -1)"""
    k = dev.k
    w = Guarded(dev, np.full(b.size, 7.0))
    db = dev.put(b)
    dev.chk(k.mi355x_spmv_csr(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, w.p))
    dev.chk(k.mi355x_vec_aypx(dev.h, b.size, -1.0, db, w.p))
    out = w.get()
    dev.free(db); dev.free(w.base)
    return out


def fused(dev, csr, dx, b, alias=False):
    k = dev.k
    if alias:
        r = Guarded(dev, b)
        dev.chk(k.mi355x_spmv_csr_residual(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, r.p, r.p))
    else:
        r = Guarded(dev, np.full(b.size, -3.0))
        db = dev.put(b)
        dev.chk(k.mi355x_spmv_csr_residual(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, db, r.p))
        assert_bitexact(dev.get(db, b.size), b)
        dev.free(db)
    out = r.get()
    dev.free(r.base)
    return out


def assert_same(got, ref, what):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at rows %s, the two calls give them at %s" % (what, np.flatnonzero(np.isnan(got)), np.flatnonzero(nan))
    bad = np.flatnonzero((got.view(np.uint64) != ref.view(np.uint64)) & ~nan)
    assert bad.size == 0, "%s: %d rows differ from the two calls, first %d: %r against %r" % (what, bad.size, bad[0], got[bad[0]], ref[bad[0]])


# (a matrix of one row has no grouped form: a group is two or more rows that share a column list, and the analysis declines)
@pytest.mark.parametrize("form,m", [(f, m) for f in FORMS for m in SIZES if not (f == "grouped" and m == 1)])
def test_residual_carries_the_bits_of_product_and_aypx(dev, form, m):
    A = Banded(form, m)
    rng = np.random.default_rng(m)
    x, b = rng.standard_normal(A.n), rng.standard_normal(m)
    csr = A.csr(dev, form)
    dx = dev.put(x)
    for pairsum in (0, 1):
        csr.pairsum(pairsum)
        ref = two_calls(dev, csr, dx, b)
        assert_same(fused(dev, csr, dx, b), ref, "%s m=%d pairsum %d" % (form, m, pairsum))
        assert_same(fused(dev, csr, dx, b, alias=True), ref, "%s m=%d pairsum %d, r aliasing b" % (form, m, pairsum))
    empty = np.flatnonzero(A.lens == 0)
    if empty.size:
        assert_bitexact(ref[empty], b[empty])                  # a row without entries: b - 0.0
    dev.free(dx); csr.free()


@pytest.mark.parametrize("shape", [(65, 300), (257, 40), (64, 1)])
@pytest.mark.parametrize("form", ("plain", "scalar"))
def test_rectangular(dev, form, shape):
    m, n = shape
    A = Banded(form, m, n=n)
    rng = np.random.default_rng(n)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    csr = A.csr(dev, form)
    dx = dev.put(x)
    assert_same(fused(dev, csr, dx, b), two_calls(dev, csr, dx, b), "%s %dx%d" % (form, m, n))
    dev.free(dx); csr.free()


@pytest.mark.parametrize("name", ["stack_empty", "lap257", "p7_8_8_8"])     # run-coded and per-row-word blocks in one launch; two blocks; no run-coded block
def test_row_patterns_with_pattern_runs_on_and_off(dev, name):
    ai, aj, aa, n = pr.matrix(name)
    m = ai.size - 1
    csr = Csr(dev, ai, aj, aa, int(aj[0]), n, form="rowpat")
    x, b = pr.mixed(n, 1), pr.mixed(m, 2)
    dx = dev.put(x)
    coded = {}
    for on in (1, 0):
        nb = C.c_int(-1)
        dev.chk(dev.k.mi355x_spmv_plan_use_pattern_runs(csr.plan, on, C.byref(nb)))
        coded[on] = nb.value
        ref = two_calls(dev, csr, dx, b)
        assert_same(fused(dev, csr, dx, b), ref, "%s runs %d" % (name, on))
        assert_same(fused(dev, csr, dx, b, alias=True), ref, "%s runs %d, r aliasing b" % (name, on))
    assert (coded[1] > 0) == (name != "p7_8_8_8"), coded       # with runs on, the first two matrices have run-coded blocks
    dev.free(dx); csr.free()


@pytest.mark.parametrize("form", FORMS)
def test_specials_in_values_x_and_b(dev, form):
    m = 257
    A = Banded(form, m, seed=5, special_values=True)
    rng = np.random.default_rng(77)
    x, b = rng.standard_normal(A.n), rng.standard_normal(m)
    x[rng.choice(A.n, 10, replace=False)] = np.resize([np.nan, np.inf, -np.inf, -0.0, 0.0], 10)
    b[rng.choice(m, 40, replace=False)] = np.resize([np.nan, np.inf, -np.inf, -0.0, 0.0], 40)
    b[np.flatnonzero(A.lens == 0)[:6]] = [-0.0, 0.0, np.inf, -np.inf, np.nan, -0.0]     # empty rows: b - 0.0 keeps the sign of a zero
    csr = A.csr(dev, form)
    dx = dev.put(x)
    for pairsum in (0, 1):
        csr.pairsum(pairsum)
        ref = two_calls(dev, csr, dx, b)
        got = fused(dev, csr, dx, b)
        assert_same(got, ref, "%s specials pairsum %d" % (form, pairsum))
        assert np.isnan(ref).any() and np.isinf(ref).any() and (np.signbit(ref) & (ref == 0)).any()   # the inputs produce every class
        assert_same(fused(dev, csr, dx, b, alias=True), ref, "%s specials pairsum %d, r aliasing b" % (form, pairsum))
    dev.free(dx); csr.free()


def test_compressed_row_plan_is_refused_and_bad_arguments(dev):
    k = dev.k
    m = 65
    A = Banded("plain", m)
    x, b = np.ones(A.n), np.ones(m)
    rows = np.flatnonzero(A.lens > 0).astype(np.int32)
    cai = np.concatenate(([0], A.ai[1:][rows])).astype(np.int32)
    cp = Csr(dev, cai, A.aj, A.aa, 0, A.n, form="plain", rows=rows, m_out=m)
    full = A.csr(dev, "plain")
    dx, db = dev.put(x), dev.put(b)
    r = Guarded(dev, np.full(m, -3.0))
    assert k.mi355x_spmv_csr_residual(dev.h, cp.plan, cp.dai, cp.daj, cp.daa, dx, db, r.p) == 801
    a = (full.dai, full.daj, full.daa)
    assert k.mi355x_spmv_csr_residual(dev.h, None, *a, dx, db, r.p) == 1
    assert k.mi355x_spmv_csr_residual(dev.h, full.plan, *a, None, db, r.p) == 1
    assert k.mi355x_spmv_csr_residual(dev.h, full.plan, *a, dx, None, r.p) == 1
    assert k.mi355x_spmv_csr_residual(dev.h, full.plan, *a, dx, db, None) == 1
    assert k.mi355x_spmv_csr_residual(dev.h, full.plan, full.dai, full.daj, None, dx, db, r.p) == 1
    assert k.mi355x_spmv_csr_residual(dev.h, full.plan, *a, r.p, db, r.p) == 1          # x must not alias r
    dev.sync()
    assert_bitexact(r.get(), np.full(m, -3.0))                                           # nothing was written
    dev.free(dx); dev.free(db); dev.free(r.base); cp.free(); full.free()
