"""MatZeroRows (MAT_KEEP_NONZERO_PATTERN) and MatZeroRowsColumns on the device copy of AIJ matrices: host and device copies updated side by
side, the right-hand side corrected on the device, no re-upload, the derived forms following by a gather; MatZeroRows in its default mode
through the pattern-change route.  Expected values come from the numpy loops of tests/test_mat_zero_rows_cpu.py (one multiply, one subtract,
stored column order); comparisons are bit for bit unless said otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
import problems as pb
import vecspecials as vs
from gpu import Dev, ksp_type_for
from test_mat_value_ops_cpu import host_pattern, host_values
from test_mat_value_ops_gpu import V, bits, tcounts, uploads, vpatterns
from test_mat_zero_rows_cpu import (ARG_SIZ, ARG_WRONGSTATE, ERR_SUP, LISTS, arrow, perturbed, raises, ref_zero_rows, ref_zero_rows_columns,
                                    ref_zero_rows_new_pattern)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEEP = 9          # MAT_KEEP_NONZERO_PATTERN
OPS = ("rows", "columns")
DIAGS = (0.0, 1.0, 2.5)


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.free_all()


def zcounts(P, A):
    a, b = C.c_int(-1), C.c_int(-1)
    P.lib().MatHIPMI355XGetZeroRowsCounts(A.h, C.byref(a), C.byref(b))
    return a.value, b.value


def boundary(ai):
    """the rows a grid's stencil cuts short"""
    return [int(r) for r in np.flatnonzero(np.diff(ai) < np.diff(ai).max())]


class Mat0:
    """a matrix, the vectors of its tests and the numpy side of every (operation, list, diag), computed once"""

    def __init__(self, ai, aj, aa):
        self.ai, self.aj, self.aa = ai, aj, aa
        self.n = ai.size - 1
        self.x = np.cos(0.3 * np.arange(self.n))            # what the products multiply
        self.xb = 1.0 + np.sin(0.7 * np.arange(self.n))     # the x and b of the update
        self.b0 = np.cos(1.1 * np.arange(self.n)) - 0.2
        self.lists = {k: mk(self.n) for k, mk in LISTS.items()}
        self.lists["boundary"] = boundary(ai)
        self._ref = {}

    def ref(self, op, lname, diag):
        key = (op, lname, diag)
        if key not in self._ref:
            f = ref_zero_rows if op == "rows" else ref_zero_rows_columns
            self._ref[key] = f(self.ai, self.aj, self.aa, self.lists[lname], diag, self.xb, self.b0)
        return self._ref[key]

    def mat(self, P, aa=None):
        A = P.Mat.from_csr(self.ai, self.aj, self.aa if aa is None else aa)
        A.set_option(KEEP, True)
        return A


def apply(A, op, rows, diag, x=None, b=None):
    (A.zero_rows if op == "rows" else A.zero_rows_columns)(rows, diag, x=x, b=b)


def check(P, m, A, vals, vx, vy, what, exact=True):
    L = P.lib()
    A.mult(vx, vy)
    if exact:
        assert np.array_equal(bits(vy.array()), bits(orc.matmult(m.ai, m.aj, vals, m.x)[0])), what + ": MatMult"
    else:
        # a form whose row sums take another order than the reference's: the bits of a matrix assembled from the same values, and the
        # reference to the bound of a sum of `width` terms in any order (tests/test_mat_value_ops_gpu.py, Case.check)
        got = vy.array().copy()
        F = P.Mat.from_csr(m.ai, m.aj, vals)
        F.mult(vx, vy)
        assert np.array_equal(bits(got), bits(vy.array())), what
        F.destroy()
        width = int(np.diff(m.ai).max())
        bound = width * 2.220446049250313e-16 * orc.matmult(m.ai, m.aj, np.abs(vals), np.abs(m.x))[0]
        assert np.all(np.abs(got - orc.matmult(m.ai, m.aj, vals, m.x)[0]) <= bound), what
    L.MatGetDiagonal(A.h, vy.h)
    assert np.array_equal(bits(vy.array()), bits(orc.get_diagonal(m.ai, m.aj, vals))), what + ": MatGetDiagonal"
    L.MatMultTranspose(A.h, vx.h, vy.h)
    assert np.allclose(vy.array(), orc.spmv_t(m.ai, m.aj, vals, m.x, m.n), rtol=0, atol=1e-12), what + ": MatMultTranspose"
    assert np.array_equal(bits(host_values(P, A, vals.size)), bits(vals)), what + ": host copy"


@pytest.fixture(scope="module")
def mats():
    return {"lap2d": Mat0(*perturbed(pb.lap2d(23, 19))), "p7": Mat0(*perturbed(orc.gen_p7(11, 9, 7))), "arrow": Mat0(*arrow())}


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["lap2d", "p7", "arrow"])
def test_each_update_used_first_and_not(P, mats, name, op):
    """1. every list, diag in {0, 1, 2.5}, with and without (x, b), after the matrix has been used on the device (device-side update: no
    upload, the list sent once) and before (host update, one upload at the first use)"""
    m = mats[name]
    L = P.lib()
    assert m.n == {"lap2d": 437, "p7": 693, "arrow": 300}[name]
    if name == "arrow":
        assert m.ai[1] - m.ai[0] == 300 and m.ai[8] - m.ai[7] == 1
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))
    for lname, rows in m.lists.items():
        for diag in DIAGS:
            ref_a, ref_b = m.ref(op, lname, diag)
            for with_vecs in (True, False):
                for used_first in (True, False):
                    what = "%s %s %s diag=%g vecs=%s used_first=%s" % (name, op, lname, diag, with_vecs, used_first)
                    A = m.mat(P)
                    xv, bv = (V(P, m.xb), V(P, m.b0)) if with_vecs else (None, None)
                    if used_first:
                        A.mult(vx, vy); L.MatMultTranspose(A.h, vx.h, vy.h)
                    apply(A, op, rows, diag, xv, bv)
                    apply(A, op, rows, diag, xv, bv)        # the same list again: idempotent on the values and on b, and not sent again
                    check(P, m, A, ref_a, vx, vy, what)
                    if with_vecs:
                        assert np.array_equal(bits(bv.array()), bits(ref_b)), what + ": b"
                        assert np.array_equal(bits(xv.array()), bits(m.xb)), what + ": x"
                    assert uploads(P, A) == 1, "%s: the values crossed %d times" % (what, uploads(P, A))
                    if used_first:
                        assert tcounts(P, A) == (1, 1 if rows else 0), what
                        assert zcounts(P, A) == ((1, 2) if rows else (0, 0)), what
                    else:
                        assert zcounts(P, A) == (0, 0), what
                    A.destroy()


def test_second_pass_is_idempotent_only_because_of_the_contract(mats):
    """(the numpy side of the line above: a second MatZeroRowsColumns with the same list finds every listed column already +0.0, so it
    subtracts +-0.0 products from b -- which can only turn a -0.0 of b into +0.0 -- and b of this file has no zero)"""
    m = mats["lap2d"]
    a1, b1 = m.ref("columns", "boundary", 2.5)
    a2, b2 = ref_zero_rows_columns(m.ai, m.aj, a1, m.lists["boundary"], 2.5, m.xb, b1)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(b1), bits(b2))


def test_a_changed_list_is_sent_again(P, mats):
    m = mats["p7"]
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))
    A = m.mat(P)
    A.mult(vx, vy)
    cur = m.aa
    for k, (lname, want) in enumerate((("boundary", 1), ("boundary", 1), ("dups", 2), ("dups", 2), ("boundary", 3), ("first", 4), ("last", 5))):
        A.zero_rows_columns(m.lists[lname], 1.0)
        cur, _ = ref_zero_rows_columns(m.ai, m.aj, cur, m.lists[lname], 1.0)
        assert zcounts(P, A) == (want, k + 1), lname
    check(P, m, A, cur, vx, vy, "a sequence of lists")
    assert uploads(P, A) == 1


def run_sequence(P, m, opts, vx, vy, before=None, between=None, exact=True):
    """both operations, three lists, on one matrix after a first use; the products' bits after every update"""
    L = P.lib()
    L.PetscOptionsClear()
    if opts:
        L.PetscOptionsInsertString(opts.encode())
    try:
        A = m.mat(P)
        A.mult(vx, vy); L.MatMultTranspose(A.h, vx.h, vy.h)
        if before:
            before(A)
        cur, b, out = m.aa, m.b0, []
        xv = V(P, m.xb)
        steps = (("rows", "first", 2.5), ("columns", "straddle", 0.0), ("columns", "boundary", 1.0), ("rows", "dups", 1.0))
        for op, lname, diag in steps:
            bv = V(P, b)
            apply(A, op, m.lists[lname], diag, xv, bv)
            cur, b = (ref_zero_rows if op == "rows" else ref_zero_rows_columns)(m.ai, m.aj, cur, m.lists[lname], diag, m.xb, b)
            if between:
                between(A, op)
            check(P, m, A, cur, vx, vy, "%s after %s %s" % (opts, op, lname), exact)
            assert np.array_equal(bits(bv.array()), bits(b)), (opts, op, lname)
            A.mult(vx, vy)
            out.append(vy.array().copy())
        return A, out, len(steps)
    finally:
        L.PetscOptionsClear()


def test_update_on_device_0_is_the_route_through_an_upload(P, mats):
    """2. -mat_hipmi355x_update_on_device 0: the same product bits, one upload per update"""
    m = mats["p7"]
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))
    A1, on, n = run_sequence(P, m, "", vx, vy)
    A0, off, _ = run_sequence(P, m, "-mat_hipmi355x_update_on_device 0", vx, vy)
    for a, b in zip(on, off):
        assert np.array_equal(bits(a), bits(b))
    assert uploads(P, A1) == 1 and tcounts(P, A1) == (1, n) and zcounts(P, A1)[1] == n
    assert uploads(P, A0) == 1 + n and zcounts(P, A0) == (0, 0)


def test_derived_forms_follow(P, mats):
    """3. the column-tiled layout, the blocked companion and the value-pattern dictionary after device-side updates"""
    L = P.lib()
    m = mats["p7"]
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))

    def tiled(A):
        s, r = C.c_int(), C.c_int()
        L.MatHIPMI355XGetTiledInfo(A.h, C.byref(s), C.byref(r))
        assert s.value + r.value == m.aj.size, "the column-tiled layout was not taken"
    A, _, n = run_sequence(P, m, "-mat_hipmi355x_tiled 1 -mat_hipmi355x_index_compression 0", vx, vy, before=tiled)
    assert uploads(P, A) == 1 and tcounts(P, A) == (1, n)
    # a 3-dof matrix through its blocked companion
    (ai, aj, aa), _ = pb.elasticity_like(6, 5, 4)
    mb = Mat0(ai.astype(np.int32), aj.astype(np.int32), aa)
    assert mb.n == 360
    bx, by = V(P, mb.x), V(P, np.zeros(mb.n))

    def blocked(A):
        bs, nb = C.c_int(), C.c_int()
        L.MatHIPMI355XGetBlockedInfo(A.h, C.byref(bs), C.byref(nb))
        assert bs.value == 3 and nb.value * 9 == mb.aj.size
    A, _, n = run_sequence(P, mb, "-mat_hipmi355x_blocked 1", bx, by, before=blocked, exact=False)
    assert uploads(P, A) == 1 and tcounts(P, A) == (0, 0)
    # constant coefficients: the dictionary describes the old values and is dropped by the update
    mc = Mat0(*[np.ascontiguousarray(a) for a in orc.gen_p7(11, 9, 7)])

    def has_dictionary(A):
        assert vpatterns(P, A) == 27

    def dropped(A, op):
        assert vpatterns(P, A) == 0, op
    A, _, n = run_sequence(P, mc, "", vx, vy, before=has_dictionary, between=dropped)
    assert uploads(P, A) == 1 and tcounts(P, A) == (1, n)


def test_default_mode_goes_through_an_upload(P, mats):
    """4. MatZeroRows without MAT_KEEP_NONZERO_PATTERN: the shrunken pattern, the product numpy's, one more upload, MatShift still works"""
    for name in ("lap2d", "arrow"):
        m = mats[name]
        vx, vy = V(P, m.x), V(P, np.zeros(m.n))
        for used_first in (True, False):
            for diag in (0.0, 2.5):
                A = P.Mat.from_csr(m.ai, m.aj, m.aa)
                if used_first:
                    A.mult(vx, vy)
                xv, bv = V(P, m.xb), V(P, m.b0)
                rows = m.lists["boundary"]
                A.zero_rows(rows, diag, x=xv, b=bv)
                ni, nj, na = ref_zero_rows_new_pattern(m.ai, m.aj, m.aa, rows, diag)
                assert ni[-1] < m.ai[-1]
                gi, gj = host_pattern(P, A)
                assert np.array_equal(gi, ni) and np.array_equal(gj, nj)
                A.mult(vx, vy)
                assert np.array_equal(bits(vy.array()), bits(orc.matmult(ni, nj, na, m.x)[0])), (name, used_first, diag)
                bref = m.b0.copy(); bref[rows] = diag * m.xb[rows]
                assert np.array_equal(bits(bv.array()), bits(bref))
                assert uploads(P, A) == (2 if used_first else 1)
                assert zcounts(P, A) == (0, 0)
                if diag != 0.0:                             # every row kept its diagonal entry: the device route of MatShift
                    A.shift(0.37)
                    A.mult(vx, vy)
                    sh = na.copy(); sh[np.repeat(np.arange(m.n), np.diff(ni)) == nj] += 0.37
                    assert np.array_equal(bits(vy.array()), bits(orc.matmult(ni, nj, sh, m.x)[0]))
                    assert uploads(P, A) == (2 if used_first else 1)
                A.destroy()


SPECIAL_DIAGS = [-0.0, np.inf, np.nan, 4.9406564584124654e-324, 1.0]


def test_ieee_specials(P, mats):
    """5. values holding +-Inf, NaN and -0.0 in listed rows and in eliminated columns, x the same, diag in {-0.0, Inf, NaN, a denormal}:
    zeroed entries are +0.0 whatever was there, b carries the NaN / Inf the subtraction gives, -0.0 does not set the diagonal"""
    m = mats["lap2d"]
    nz = m.aj.size
    vy = V(P, np.zeros(m.n))
    rows = m.lists["boundary"]
    listed = np.zeros(m.n, bool); listed[rows] = True
    rowof = np.repeat(np.arange(m.n), np.diff(m.ai))
    with np.errstate(all="ignore"):
        for rot, diag in enumerate(SPECIAL_DIAGS):
            aa = vs.special_vector(nz, 11, vs.SHARE, rot)
            xs = vs.special_vector(m.n, 12, vs.SHARE, rot)
            bs = vs.special_vector(m.n, 13, vs.SHARE, rot)
            assert np.isnan(aa[listed[rowof]]).any() and np.isinf(aa[listed[m.aj] & ~listed[rowof]]).any()
            for op in OPS:
                for used_first in (True, False):
                    what = "%s diag=%r used_first=%s" % (op, diag, used_first)
                    A = m.mat(P, aa)
                    if used_first:
                        A.mult(V(P, m.x), vy)
                    xv, bv = V(P, xs), V(P, bs)
                    apply(A, op, rows, diag, xv, bv)
                    ra, rb = (ref_zero_rows if op == "rows" else ref_zero_rows_columns)(m.ai, m.aj, aa, rows, diag, xs, bs)
                    vs.same(host_values(P, A, nz), ra, what + ": host copy")
                    vs.same(bv.array(), rb, what + ": b")
                    P.lib().MatGetDiagonal(A.h, vy.h)
                    vs.same(vy.array(), ra[rowof == m.aj], what + ": device diagonal")
                    gone = listed[rowof] | (listed[m.aj] if op == "columns" else False)
                    gone &= ~((rowof == m.aj) & listed[rowof] & (diag != 0))
                    assert np.all(bits(host_values(P, A, nz))[gone] == 0), what + ": +0.0 bits"
                    if op == "columns":
                        assert np.isnan(rb[~listed]).any()
                    if diag == 0.0:
                        assert np.all(bits(ra[(rowof == m.aj) & listed[rowof]]) == 0)
                    assert uploads(P, A) == 1
                    A.destroy()


def test_kernels_on_guarded_arrays(P, dev, mats):
    """6. the two kernels through the C ABI on guarded value and b arrays, both alignments: nothing outside aa[0, nz) and b[0, m) is
    written; nrows == 0 and a mask without a bit leave every bit alone"""
    k = dev.k
    for name in ("lap2d", "arrow"):
        m = mats[name]
        nz = m.aj.size
        dai = dev.put(m.ai)
        daj = dev.put(np.concatenate([m.aj, np.zeros(4, np.int32)]))      # (the pair loads may read one index past the last)
        plan = C.c_void_p()
        dev.chk(k.mi355x_spmv_plan_create(dev.h, m.n, m.ai.ctypes.data_as(C.c_void_p), None, C.byref(plan)))
        dx = dev.put(m.xb)
        for lname in ("boundary", "dups", "first", "last", "all", "empty"):
            rows = np.array(m.lists[lname], np.int32)
            mask = np.zeros((m.n + 31) // 32, np.uint32)
            for r in rows.tolist():
                mask[r >> 5] |= np.uint32(1 << (r & 31))
            drows, dmask = dev.put(rows), dev.put(mask)
            for off in (0, 1):
                for diag, vecs in ((2.5, True), (0.0, False)):
                    ga = vs.guarded(dev, m.aa, off, tag=1)
                    gb = vs.guarded(dev, m.b0, 1 - off, tag=2)
                    xb = (dx, gb.ptr) if vecs else (None, None)
                    dev.chk(k.mi355x_csr_zero_columns(dev.h, plan, dai, daj, ga.ptr, dmask, *xb))
                    dev.chk(k.mi355x_csr_zero_rows(dev.h, rows.size, drows, dai, daj, ga.ptr, diag, *xb))
                    ra, rb = ref_zero_rows_columns(m.ai, m.aj, m.aa, rows, diag, m.xb if vecs else None, m.b0 if vecs else None)
                    what = "%s %s off=%d diag=%g" % (name, lname, off, diag)
                    vs.same(ga.get(), ra, what)
                    vs.same(gb.get(), rb if vecs else m.b0, what + ": b")
                    if lname == "empty":
                        assert np.array_equal(bits(ga.get()), bits(m.aa))
                    vs.guards_intact(ga, gb, names=["aa", "b"])
                    ga.free(); gb.free()
            dev.free(drows); dev.free(dmask)
        # x without b is refused, nothing launched
        assert k.mi355x_csr_zero_rows(dev.h, 1, dai, dai, daj, dx, 1.0, dx, None) != 0
        assert k.mi355x_csr_zero_columns(dev.h, plan, dai, daj, dx, dai, None, dx) != 0
        k.mi355x_spmv_plan_destroy(plan)


def test_a_row_longer_than_the_stage(P, dev):
    """a row of more than 2046 entries is a row block of its own and is swept a stage at a time: its correction in stored order, whether
    the row is listed or crossed by listed columns"""
    k = dev.k
    n = 5000
    cols = [[0], [1], [2], list(range(3, n))] + [[3, r] for r in range(4, n)]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    aj = np.concatenate(cols).astype(np.int32)
    aa = 1.0 + np.cos(0.37 * np.arange(aj.size))
    assert ai[4] - ai[3] > 2 * 2046
    x = 1.0 + np.sin(0.7 * np.arange(n)); b0 = np.cos(1.1 * np.arange(n))
    dai, daj, dx = dev.put(ai), dev.put(np.concatenate([aj, np.zeros(4, np.int32)])), dev.put(x)
    plan = C.c_void_p()
    dev.chk(k.mi355x_spmv_plan_create(dev.h, n, ai.ctypes.data_as(C.c_void_p), None, C.byref(plan)))
    for rows in ([3], [7, 2050, 2051, 4095, 4096, 4999], list(range(4, n, 3))):
        rows = np.array(rows, np.int32)
        mask = np.zeros((n + 31) // 32, np.uint32)
        for r in rows.tolist():
            mask[r >> 5] |= np.uint32(1 << (r & 31))
        drows, dmask = dev.put(rows), dev.put(mask)
        ga, gb = vs.guarded(dev, aa, 1, tag=3), vs.guarded(dev, b0, 0, tag=4)
        dev.chk(k.mi355x_csr_zero_columns(dev.h, plan, dai, daj, ga.ptr, dmask, dx, gb.ptr))
        dev.chk(k.mi355x_csr_zero_rows(dev.h, rows.size, drows, dai, daj, ga.ptr, 2.5, dx, gb.ptr))
        ra, rb = ref_zero_rows_columns(ai, aj, aa, rows, 2.5, x, b0)
        vs.same(ga.get(), ra, "long row, %d listed" % rows.size)
        vs.same(gb.get(), rb, "long row, %d listed: b" % rows.size)
        vs.guards_intact(ga, gb, names=["aa", "b"])
        ga.free(); gb.free(); dev.free(drows); dev.free(dmask)
    k.mi355x_spmv_plan_destroy(plan)


def test_errors_leave_both_copies_alone(P, mats):
    """7. diag != 0 on a matrix with a missing diagonal entry: values and b untouched, on the host and on the device; a matrix that is
    not square"""
    m = mats["lap2d"]
    rowof = np.repeat(np.arange(m.n), np.diff(m.ai))
    keep = ~((rowof == m.aj) & (rowof == 300))
    xi = np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=m.n))]).astype(np.int32)
    xj, xa = m.aj[keep], m.aa[keep]
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))
    A = P.Mat.from_csr(xi, xj, xa)
    A.set_option(KEEP, True)
    A.mult(vx, vy)
    y0 = vy.array().copy()
    xv, bv = V(P, m.xb), V(P, m.b0)
    for f in (A.zero_rows, A.zero_rows_columns):
        assert "row 300" in raises(P, ARG_WRONGSTATE, lambda: f([1, 2], 1.0, x=xv, b=bv))
    assert np.array_equal(bits(host_values(P, A, xa.size)), bits(xa)) and np.array_equal(bits(bv.array()), bits(m.b0))
    A.mult(vx, vy)
    assert np.array_equal(bits(vy.array()), bits(y0)) and uploads(P, A) == 1 and zcounts(P, A) == (0, 0)
    A.zero_rows_columns([1, 2], 0.0, x=xv, b=bv)            # diag == 0 does not ask for the diagonal
    ra, rb = ref_zero_rows_columns(xi, xj, xa, [1, 2], 0.0, m.xb, m.b0)
    A.mult(vx, vy)
    assert np.array_equal(bits(vy.array()), bits(orc.matmult(xi, xj, ra, m.x)[0])) and np.array_equal(bits(bv.array()), bits(rb))
    assert uploads(P, A) == 1 and zcounts(P, A) == (1, 1)
    ri = np.array([0, 2, 3, 5], np.int32); rj = np.array([0, 3, 1, 2, 4], np.int32); ra_ = np.arange(1.0, 6.0)
    R = P.Mat.from_csr(ri, rj, ra_, ncols=5)
    R.set_option(KEEP, True)
    x5, y3 = V(P, np.ones(5)), V(P, np.zeros(3))
    R.mult(x5, y3)
    raises(P, ARG_SIZ, lambda: R.zero_rows_columns([0], 0.0))
    raises(P, ERR_SUP, lambda: R.zero_rows([0], 1.0))
    R.zero_rows([2, 0], 0.0)
    R.mult(x5, y3)
    assert list(y3.array()) == [0.0, 3.0, 0.0] and uploads(P, R) == 1


def test_mpiaij_on_one_rank(P, mats):
    """MPIAIJ on one rank: MatZeroRows goes through the blocks in both modes; MatZeroRowsColumns is not supported"""
    m = mats["p7"]
    L = P.lib()
    vx, vy = V(P, m.x), V(P, np.zeros(m.n))
    rows = m.lists["boundary"]
    for keep in (True, False):
        A = P.Mat.from_csr_mpi(m.ai, m.aj, m.aa, m.n, m.n, m.n, comm=L.COMM_SELF)
        A.set_option(KEEP, keep)
        A.mult(vx, vy)
        xv, bv = V(P, m.xb), V(P, m.b0)
        A.zero_rows(rows, 2.5, x=xv, b=bv)
        ra, rb = ref_zero_rows(m.ai, m.aj, m.aa, rows, 2.5, m.xb, m.b0)
        A.mult(vx, vy)
        assert np.array_equal(bits(vy.array()), bits(orc.matmult(m.ai, m.aj, ra, m.x)[0])), keep
        assert np.array_equal(bits(bv.array()), bits(rb)), keep
        Ad = C.c_void_p()
        L.MatMPIAIJGetSeqAIJ(A.h, C.byref(Ad), None, None)
        assert uploads(P, P.Mat(Ad, own=False)) == (1 if keep else 2)
        raises(P, ERR_SUP, lambda: A.zero_rows_columns(rows, 1.0))


def test_ksp_tests_ex4_boundary_rows_through_matzerorows(P):
    """8. src/ksp/ksp/examples/tests/ex4.c -m 5 -pc_type jacobi refine_always vs output/ex4_1.out, with the boundary rows applied by
    MatZeroRows(C, 4m, rows, 1.0, NULL, NULL) in its default mode instead of numpy (tests/problems.py: ex3_fem): the iteration count
    and the printed digits test_ksp_tests_ex4_golden requires of the oracle"""
    L = P.lib()
    m = 5
    N = (m + 1) * (m + 1)
    h = 1.0 / m
    H = h * h
    Ke = np.array([H / 6.0, -.125 * H, H / 12.0, -.125 * H, -.125 * H, H / 6.0, -.125 * H, H / 12.0,
                   H / 12.0, -.125 * H, H / 6.0, -.125 * H, -.125 * H, H / 12.0, -.125 * H, H / 6.0]).reshape(4, 4)
    K = np.zeros((N, N))
    for e in range(m * m):
        i0 = (m + 1) * (e // m) + (e % m)
        idx = [i0, i0 + 1, i0 + 1 + m + 1, i0 + 1 + m]
        for a in range(4):
            for b_ in range(4):
                K[idx[a], idx[b_]] += Ke[a, b_]
    import scipy.sparse as sp
    ai, aj, aa = pb.csr(sp.csr_matrix(K))
    rows = list(range(m + 1)) + list(range(m + 1, m * (m + 1), m + 1)) + list(range(2 * m + 1, m * (m + 1), m + 1)) + [m * (m + 1) + i for i in range(m + 1)]
    assert len(rows) == 4 * m
    u0 = np.zeros(N); b = np.zeros(N)
    for r in rows:
        u0[r] = b[r] = h * (r // (m + 1))
    ustar = np.array([h * (i // (m + 1)) for i in range(N)])
    A = P.Mat.from_csr(ai, aj, aa)
    A.zero_rows(rows, 1.0)
    (ri, rj, ra), _, _, _ = pb.ex3_fem(m)
    gi, gj = host_pattern(P, A)
    assert np.array_equal(gi, ri) and np.array_equal(gj, rj)
    assert np.array_equal(bits(host_values(P, A, ra.size)), bits(ra))
    gold = pb.parse_monitor(os.path.join(G, "ksp_tests", "ex4_1.out"))[0]
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type %s -pc_type jacobi -ksp_gmres_cgs_refinement_type refine_always" % ksp_type_for("gmres")).encode())
    try:
        k.set_from_options()
        L.KSPSetInitialGuessNonzero(k.h, 1)
        k.record_history()
        vb, vx = V(P, b), V(P, u0)
        k.solve(vb, vx)
    finally:
        L.PetscOptionsClear()
    pb.check_monitor(k.history(), gold)
    assert k.its == len(gold) - 1
    assert np.linalg.norm(vx.array() - ustar) * 0.2 <= 1e-14
