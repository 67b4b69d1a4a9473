"""The column-tiled SpMV (csrc/spmv_tiled.hip) on the inputs where kernels go wrong: non-finite x where padding, idle lanes and the
loader read (A, C), IEEE specials inside the pattern through the LDS adder (B), the panel boundary and the spare accumulator (C), the
short last tile in either LDS buffer (D), the remainder's window switches and its clamped look-ahead (E), refreshed values (F), and
MatMult's way out for an x the kernel cannot take (G).

Every product is launched with yin == NULL, with a separate yin and in place, where a layout has both parts also through
mi355x_spmv_tiled_parts; the value array is followed by two NaN (padding's value is the kernel's own 0.0), yout and yin lie between
guard words, yout starts as a per-row marker, x is 16-byte aligned.  A device vector must carry the bits of tests/tiled.py's order
on the same data (tiledspecials.Layout.replay; any NaN equals any NaN), have the oracle's class in every row, and where finite lie
within 1e-12 * sum |a_ij x_j| of the oracle -- bit for bit when one stream in column order made the sums.  The inputs and the
reference are checked on their own in test_tiled_specials_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import orc
import tiledspecials as ts
from test_tiled_cpu import random_csr
from tiledspecials import Layout, klass
from vecspecials import NAN, Guarded, bits, guards_intact, same

pytestmark = pytest.mark.gpu

MODES = ("none", "separate", "inplace")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def marker(m):
    """what yout holds before a launch: one value per row, far from any result"""
    return -(3.0e77 + 1.0e63 * np.arange(m))


class Session:
    """one layout on the device: the values (followed by two NaN), x, and yout / yin between guard words"""

    def __init__(self, dev, L, aa=None):
        self.dev, self.L, k = dev, L, dev.k
        aa = L.aa if aa is None else aa
        self.daa = dev.alloc(8 * (aa.size + 2))
        self.values(aa)
        dev.chk(k.mi355x_spmv_tiled_upload(dev.h, L.plan, self.daa))
        self.dx = dev.alloc(8 * max(L.n, 2))
        assert self.dx.value % 16 == 0
        self.gy, self.gyin = Guarded(dev, L.m, 1, tag=1), Guarded(dev, L.m, 0, tag=2)

    def values(self, aa):
        buf = np.concatenate((aa, [NAN, NAN]))
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, self.daa, buf.ctypes.data, buf.nbytes))
        self.dev.sync()

    def refresh(self, aa):
        self.values(aa)
        self.dev.chk(self.dev.k.mi355x_spmv_tiled_refresh_values(self.dev.h, self.L.plan, self.daa))

    def x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.L.n
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, self.dx, x.ctypes.data, x.nbytes))
        self.dev.sync()

    def run(self, mode, yin, which=None):
        """one launch (which None: mi355x_spmv_tiled, else _parts); the guards of yout and yin survive, a separate yin comes back unchanged"""
        dev, k, L = self.dev, self.dev.k, self.L
        if mode == "inplace":
            self.gy.load(yin)
            src = self.gy.ptr
        else:
            self.gy.load(marker(L.m))
            src = self.gyin.load(yin).ptr if mode == "separate" else None
        if which is None:
            dev.chk(k.mi355x_spmv_tiled(dev.h, L.plan, self.dx, src, self.gy.ptr))
        else:
            dev.chk(k.mi355x_spmv_tiled_parts(dev.h, L.plan, self.dx, src, self.gy.ptr, which))
        y = self.gy.get()
        guards_intact(self.gy, names=["yout (%s, %s, which %s)" % (L.name, mode, which)])
        if mode == "separate":
            guards_intact(self.gyin, names=["yin (%s)" % L.name])
            assert np.array_equal(bits(self.gyin.get()), bits(yin)), "%s: a separate yin changed" % L.name
        return y

    def free(self):
        for p in (self.daa, self.dx, self.gy.base, self.gyin.base):
            self.dev.free(p)


def launches(S, yin, parts):
    """{(mode, which): y} of every way to call the product"""
    out = {}
    for which in (None, 1, 2) if parts else (None,):
        for mode in MODES:
            out[mode, which] = S.run(mode, yin, which)
    return out


def verify(L, out, x, yin, aa=None, what=""):
    """the bits of the layout's order, the oracle's classes and bound"""
    ref = {}
    for (mode, which), y in out.items():
        add = None if mode == "none" else yin
        key = (mode == "none", which)
        if key not in ref:
            ref[key] = L.replay(x, add, which or 0, aa)
        label = "%s %s (%s, which %s)" % (L.name, what, mode, which)
        same(y, ref[key], label + " against the layout's order")
        if which is None:
            L.against_oracle(y, x, add, aa, label)


def whole_case(dev, L, x, yin, parts=None, what=""):
    S = Session(dev, L)
    try:
        S.x(x)
        out = launches(S, yin, (L.info["staged"] > 0 and L.info["remainder"] > 0) if parts is None else parts)
        verify(L, out, x, yin, what=what)
        return out
    finally:
        S.free()


# ------------------------------------------------------------------------------------------------------------- A: containment
@pytest.fixture(scope="module")
def cont(dev):
    c = ts.containment(dev.k)
    c["L"] = Layout(dev.k, "containment", *c["A"], c["n"], c["stage_min"])
    c["L2"] = Layout(dev.k, "containment/moved", *c["A2"], c["n"], c["stage_min"])
    c["yin"] = np.sin(np.arange(c["m"]) * 0.7)
    c["clean"] = None
    yield c
    c["L"].destroy(); c["L2"].destroy()


def clean_products(dev, c):
    if c["clean"] is None:
        c["clean"] = whole_case(dev, c["L"], c["x"], c["yin"], what="clean x")
    return c["clean"]


def test_tiled_specials_non_finite_x_at_unreferenced_columns_changes_no_bit(dev, cont):
    """x holds NaN, +Inf, -Inf in turn at every column padding gathers (a staged tile's first column, a used window's first column), at
    the short last tile's first pair (re-read by the loader's lanes past its end), at n - 1, n - 2 and beside referenced columns: y
    keeps the bits of the clean run in every mode and part"""
    L = cont["L"]
    assert L.info["staged"] > 0 and L.info["remainder"] > 0
    clean = clean_products(dev, cont)
    S = Session(dev, L)
    try:
        for v in (NAN, np.inf, -np.inf):
            x = cont["x"].copy()
            x[cont["P"]] = v
            S.x(x)
            for key, y in launches(S, cont["yin"], True).items():
                same(y, clean[key], "containment, x = %r at the unreferenced columns, %s" % (v, key))
    finally:
        S.free()


def test_tiled_specials_poisoned_columns_moved_into_the_pattern_reach_their_rows_only(dev, cont):
    """three poisoned columns now referenced: by the row with hundreds of entries in one staged tile (+Inf), by the rows on both sides of
    the panel boundary (NaN: the last row of a panel, the first of the next), by a short row (-Inf, column n - 1); the other poisoned
    columns stay unreferenced.  Those rows have the oracle's class and the layout's bits, every other row the clean run's bits."""
    L2 = cont["L2"]
    clean = clean_products(dev, cont)
    out = whole_case(dev, L2, cont["x_moved"], cont["yin"], what="moved columns")
    rows = np.array(sorted(cont["expect_class"]))
    (last, first), = L2.panel_edges()
    assert last in cont["expect_class"] and first in cont["expect_class"]
    other = np.setdiff1d(np.arange(L2.m), rows)
    for key, y in out.items():
        if key[1] is None:
            got = klass(y[rows])
            assert np.array_equal(got, [cont["expect_class"][int(r)] for r in rows]), "rows %s (panel edge: %d | %d): classes %s, %s" % (rows, last, first, got, key)
        same(y[other], clean[key][other], "rows that reference no poisoned column, %s" % (key,))


# ------------------------------------------------------------------------------------------------- B: specials inside the pattern
@pytest.mark.parametrize("placement", ["staged", "remainder", "split"])
def test_tiled_specials_rows_through_the_lds_adder(dev, placement):
    """tiledspecials.SPECIAL_ROWS: 0 * Inf, Inf * -0.0, NaN, opposite infinities, overflow, DBL_MAX cancelling in column order,
    subnormal values / products / sums, -0.0 sums, empty rows with special yin -- all staged, all remainder, split between the two"""
    case = ts.specials(dev.k)
    L = Layout(dev.k, "specials/" + placement, *case["A"], case["n"], case["stage_min"][placement])
    try:
        out = whole_case(dev, L, case["x"], case["yin"])
        assert (("none", 1) in out) == (placement == "split"), "the split placement runs the parts as well"
        for (mode, which), y in out.items():
            if which is None:
                rows, want, _ = ts.special_expectation(case, mode != "none")
                for row, spec, got, exp in zip(rows, ts.SPECIAL_ROWS, y[rows], want):
                    same([got], [exp], "special row %s (row %d, %s, %s)" % (spec[0], row, placement, mode))
    finally:
        L.destroy()


# ---------------------------------------------------------------------------------------- C: the spare accumulator, the panel boundary
@pytest.mark.parametrize("size", [0, 1, 2, 3], ids=["panel-1", "panel", "panel+1", "2panel+1"])
def test_tiled_specials_nan_padding_products_stay_in_the_spare_accumulator(dev, size):
    """NaN at every tile's and window's first column, unreferenced: every padding product is NaN; all of y is finite.  stage_min 1 (all
    staged) and 200 (the thin pairs are a remainder, so that a remainder run is padded too)."""
    m = ts.boundary_sizes(dev.k)[size]
    case = ts.boundary(dev.k, m)
    for stage_min in ts.BOUNDARY_STAGE_MIN:
        L = Layout(dev.k, "boundary m=%d stage_min=%d" % (m, stage_min), *case["A"], case["n"], stage_min)
        S = Session(dev, L)
        try:
            S.x(case["x"])
            out = launches(S, case["yin"], stage_min > 1)
            for (mode, which), y in out.items():
                want = L.replay(case["x"], None if mode == "none" else case["yin"], which or 0)
                for last, first in L.panel_edges() + [(L.m - 1, 0)]:
                    for row, name in ((last, "the last row of its panel"), (first, "the first row of its panel")):
                        assert np.isfinite(y[row]) and bits(y[row:row + 1])[0] == bits(want[row:row + 1])[0], \
                            "%s (%s, which %s): row %d, %s: %r, expected %r" % (L.name, mode, which, row, name, y[row], want[row])
                assert np.all(np.isfinite(y)), "%s (%s, which %s): rows %s are not finite" % (L.name, mode, which, np.flatnonzero(~np.isfinite(y))[:8])
            verify(L, out, case["x"], case["yin"])
        finally:
            S.free()
            L.destroy()


# ------------------------------------------------------------------------------------------- D: the short last tile and the loader
@pytest.mark.parametrize("ir", range(9), ids=["r=1", "r=2", "r=3", "r=127", "r=128", "r=129", "r=130", "r=tile-1", "r=0"])
def test_tiled_specials_short_last_tile_as_first_second_and_third_staged_tile(dev, ir):
    """n = 2 tiles + r: the last tile loaded by everybody, by the loader into the other buffer, by the loader into the buffer that held
    tile 0; rows reference n - 1, n - 2 and the tile's first column, x differs in every column.  All staged: the oracle's bits."""
    r = ts.tail_remainders(dev.k)[ir]
    for depth in (1, 2, 3):
        case = ts.tail(dev.k, r, depth)
        L = Layout(dev.k, "tail r=%d depth=%d" % (r, depth), *case["A"], case["n"], 1)
        try:
            whole_case(dev, L, case["x"], case["yin"])
        finally:
            L.destroy()


def test_tiled_specials_panel_without_a_staged_tile_beside_one_with_some(dev):
    case = ts.unstaged_panel(dev.k)
    L = Layout(dev.k, "unstaged panel", *case["A"], case["n"], case["stage_min"])
    try:
        whole_case(dev, L, case["x"], case["yin"])
    finally:
        L.destroy()


# ----------------------------------------------------------------------------------------------------- E: the remainder's windows
def test_tiled_specials_remainder_skips_a_window(dev):
    """columns 2^18 - 1, 2^18, 2^18 + 1 in one row of the remainder; wavefronts with entries in windows 0 and 2 only"""
    case = ts.window_skip(dev.k)
    L = Layout(dev.k, "window skip", *case["A"], case["n"], case["stage_min"])
    try:
        whole_case(dev, L, case["x"], case["yin"], parts=True)
    finally:
        L.destroy()


def test_tiled_specials_remainder_block_counts_around_the_look_ahead(dev):
    """a wavefront with 1 .. 9 remainder blocks (one, 2 TL_FG, 2 TL_FG + 1 among them): the stream loads and gathers issued for blocks
    past the end are clamped and never added"""
    for count in ts.BLOCK_COUNTS:
        case = ts.window_blocks(dev.k, count)
        L = Layout(dev.k, "window blocks %d" % count, *case["A"], case["n"], case["stage_min"])
        try:
            whole_case(dev, L, case["x"], case["yin"], parts=False)
        finally:
            L.destroy()


# ---------------------------------------------------------------------------------------------------------- F: values that change
def test_tiled_specials_refreshed_values_with_specials_before_and_after_drop_host(dev):
    case = ts.specials(dev.k)
    L = Layout(dev.k, "specials/split refreshed", *case["A"], case["n"], case["stage_min"]["split"])
    S = Session(dev, L)
    try:
        S.x(case["x"])
        for step, seed in (("refresh_values", 5), ("drop_host, refresh_values", 6)):
            aa2, pos = ts.changed_values(L.aa, seed)
            if step.startswith("drop"):
                dev.chk(dev.k.mi355x_spmv_tiled_drop_host(L.plan))
            S.refresh(aa2)
            out = launches(S, case["yin"], True)
            verify(L, out, case["x"], case["yin"], aa2, what="after " + step)
            rows = L.rowof[pos[:3]]
            assert np.all(klass(out["none", None][rows]) != 0), "the rows of the new NaN / Inf values"
    finally:
        S.free()
        L.destroy()


# ------------------------------------------------------------------------------------ G: through MatMult, the x the kernel cannot take
def test_matmult_takes_the_row_block_kernel_for_an_x_borrowed_at_an_odd_entry(built):
    """-mat_hipmi355x_tiled 1 -mat_hipmi355x_tiled_stage_min 1: the product with an ordinary x is the tiled one (all staged, column
    order: the oracle's bits); an x that borrows another vector's storage from entry 1 on is 8 bytes off a 16-byte boundary, the tiled
    kernel answers 801 and the row-block kernel serves (the oracle's bits in rows of at most 13 entries, 1e-12 beyond); then the
    ordinary x again.  MatMult, MatMultAdd, MatMultTranspose (the cached transpose takes the tiled form as well)."""
    from petsc_dev_amd import petsc as P
    import vecprog
    L = P.lib()
    rng = np.random.default_rng(23)
    m = n = 3000
    lens = rng.integers(1, 14, m)
    lens[::50] = 40
    ai, aj, aa = random_csr(rng, m, n, lens, band=400, far_frac=0.3)
    rowof = np.repeat(np.arange(m), np.diff(ai))
    xh, zh = np.cos(0.3 * np.arange(n)) + 0.5, np.sin(0.01 * np.arange(m))

    def bound(a, rows, size):
        s = np.zeros(size)
        np.add.at(s, rows, np.abs(a))
        return 1e-12 * s + 1e-300

    L.PetscOptionsClear()
    L.PetscOptionsInsertString(b"-mat_hipmi355x_tiled 1 -mat_hipmi355x_tiled_stage_min 1")
    try:
        A = P.Mat.from_csr(ai, aj, aa)
        x = P.Vec.from_array(xh, comm=L.COMM_SELF)
        parent = P.Vec.from_array(np.concatenate(([7.5], xh, [-3.25, 9.0])), comm=L.COMM_SELF)
        xs = P.Vec.from_array(np.full(n, 123.0), comm=L.COMM_SELF)
        z = P.Vec.from_array(zh, comm=L.COMM_SELF)
        y = z.duplicate()
        begin, end = vecprog.share_functions(P, xs)

        def three(product):
            """the product with the ordinary x, with the borrower, with the ordinary x again"""
            out = [product(x)]
            L.chk(begin(xs.h, parent.h, 1, 0))
            try:
                out.append(product(xs))
            finally:
                L.chk(end(xs.h, parent.h, 1, 0))
            out.append(product(x))
            return out

        def mult(v):
            A.mult(v, y)
            return y.array().copy()

        def multadd(v):
            L.MatMultAdd(A.h, v.h, z.h, y.h)
            return y.array().copy()

        def multt(v):
            L.MatMultTranspose(A.h, v.h, y.h)
            return y.array().copy()

        short = np.diff(ai) <= 13
        assert short.sum() > m // 2 and (~short).sum() >= m // 50
        ref = orc.spmv(ai, aj, aa, xh)
        tol = bound(aa * xh[aj], rowof, m)
        ys = three(mult)
        st, rm = C.c_int(), C.c_int()
        L.MatHIPMI355XGetTiledInfo(A.h, C.byref(st), C.byref(rm))
        assert st.value == aj.size and rm.value == 0
        for j, got in enumerate(ys):
            assert np.array_equal(bits(got[short]), bits(ref[short])), "MatMult %d: short rows" % j
            assert np.all(np.abs(got - ref) <= tol), "MatMult %d" % j
        assert np.array_equal(bits(ys[0]), bits(ref)) and np.array_equal(bits(ys[2]), bits(ref)), "the tiled product, all staged: the oracle's bits"
        refadd = orc.spmv_add(ai, aj, aa, xh, zh)
        ys = three(multadd)
        for j, got in enumerate(ys):
            assert np.array_equal(bits(got[short]), bits(refadd[short])), "MatMultAdd %d: short rows" % j
            assert np.all(np.abs(got - refadd) <= tol + 1e-12 * np.abs(zh)), "MatMultAdd %d" % j
        assert np.array_equal(bits(ys[0]), bits(refadd)) and np.array_equal(bits(ys[2]), bits(refadd))
        assert np.array_equal(bits(z.array()), bits(zh))
        # the transpose: x has m entries (the matrix is square: the same vectors serve)
        reft = orc.spmv_t(ai, aj, aa, xh, n)
        shortt = np.bincount(aj, minlength=n) <= 13
        tolt = bound(aa * xh[rowof], aj, n)
        assert shortt.sum() > n // 2
        for j, got in enumerate(three(multt)):
            assert np.array_equal(bits(got[shortt]), bits(reft[shortt])), "MatMultTranspose %d: short rows" % j
            assert np.all(np.abs(got - reft) <= tolt), "MatMultTranspose %d" % j
        assert np.array_equal(bits(parent.array()), bits(np.concatenate(([7.5], xh, [-3.25, 9.0])))), "the lender's storage is read only"
    finally:
        L.PetscOptionsClear()
