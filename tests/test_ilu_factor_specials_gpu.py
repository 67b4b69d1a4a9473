"""The numeric ILU(0) on the device (csrc/ilu_factor.hip, mi355x_ilu0_factor_*) against the restatement of one pass
(ilufactor.reference_pass) on data that is not tame: every lane width 1 .. 64 and both row forms asserted to have run, the
row-length and chunk edges, stored zeros, IEEE specials inside the arithmetic, containment of a special along L's dependency
graph, the failure report in every lane width, 40 blocks over three passes, the sweep form and the layout checks of _create.

Every comparison is on bit patterns; where the reference is NaN a NaN is asked for.  ba lives between guard bands of 64 doubles of
a marker, is pre-filled with the marker (slot nz included, which the layout does not name) and A's arrays are read back: the
kernel writes the slots of the rows it factors and nothing else.  The machinery (ilufactor.py) is checked on its own, without a
GPU, by test_ilu_factor_specials_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import ilufactor as ilf
from ilufactor import BAND, MARK, ZP, bits
from test_ilu_device_factor_gpu import symbolic
from test_ilu_sweeps_gpu import strict_triangles
from test_kernels_gpu import dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
INVALID = 1                                     # hipErrorInvalidValue


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _create(dev, n, bi, bj, bd, nlev, levptr, rows, nblk, blk):
    ctx = C.c_void_p()
    keep = [_i32(a) for a in (bi, bj, bd, levptr, rows)] + [None if blk is None else _i32(blk)]
    rc = dev.k.mi355x_ilu0_factor_create(dev.h, n, *[a.ctypes.data for a in keep[:3]], nlev, keep[3].ctypes.data, keep[4].ctypes.data,
                                         nblk, None if blk is None else keep[5].ctypes.data, C.byref(ctx))
    return rc, ctx


class Guarded:
    """`count` doubles on the device between two bands of the marker; the caller owns them"""

    def __init__(self, dev, count, fill=MARK):
        self.dev, self.count = dev, count
        host = np.full(count + 2 * BAND, MARK)
        host[BAND:BAND + count] = fill
        self.base = dev.put(host)
        self.ptr = C.c_void_p(self.base.value + 8 * BAND)

    def put(self, values):
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.size == self.count
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, self.ptr, values.ctypes.data, values.nbytes))
        self.dev.sync()

    def get(self, what):
        """the values; the bands are as they were"""
        full = self.dev.get(self.base, self.count + 2 * BAND)
        mark = bits(np.array([MARK]))[0]
        assert (bits(full[:BAND]) == mark).all() and (bits(full[BAND + self.count:]) == mark).all(), "%s: a guard band was written" % what
        return full[BAND:BAND + self.count]

    def free(self):
        self.dev.free(self.base)


class Factor:
    """the context of A's pattern (layout and levels from test_ilu_device_factor_gpu.symbolic on tame values), A on the device, ba
    between guard bands and pre-filled with the marker"""

    def __init__(self, dev, ai, aj, aa, blk=None):
        self.dev, self.ai, self.aj, self.aa = dev, _i32(ai), _i32(aj), np.ascontiguousarray(aa, dtype=np.float64)
        self.n, self.nz = self.ai.size - 1, int(self.ai[-1])
        self.nblk = 1 if blk is None else len(blk) - 1
        bi, bj, bd, nlev, levptr, rows = symbolic(self.ai, self.aj, ilf.tame(self.ai, self.aj))
        lay = ilf.layout(self.ai, self.aj)
        assert np.array_equal(bi, lay[0]) and np.array_equal(bj[:-1], lay[1][:-1]) and np.array_equal(bd, lay[2])
        self.layout, self.nlev = (bi, bj, bd), nlev
        rc, self.ctx = _create(dev, self.n, bi, bj, bd, nlev, levptr, rows, self.nblk, blk)
        dev.chk(rc)
        self.dai, self.daj, self.daa = dev.put(self.ai), dev.put(self.aj), dev.put(self.aa)
        self.ba = Guarded(dev, self.nz + 1)
        dev.chk(dev.k.mi355x_ilu0_factor_reset(self.ctx))
        lanes, nl = C.c_int(), C.c_int()
        dev.chk(dev.k.mi355x_ilu0_factor_info(self.ctx, C.byref(lanes), C.byref(nl)))
        assert nl.value == nlev
        self.lanes = lanes.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.k.mi355x_ilu0_factor_destroy(self.ctx)
        for p in (self.dai, self.daj, self.daa):
            self.dev.free(p)
        self.ba.free()

    def run(self, shifts=None, zeropivot=ZP):
        sh = np.zeros(self.nblk) if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64)
        frow, fabs_ = np.full(self.nblk, -7, np.int32), np.full(self.nblk, -7.0)
        self.dev.chk(self.dev.k.mi355x_ilu0_factor_run(self.dev.h, self.ctx, self.dai, self.daj, self.daa, zeropivot, sh.ctypes.data, self.ba.ptr,
                                                       frow.ctypes.data, fabs_.ctypes.data))
        return frow, fabs_

    def values(self, what):
        """ba read back; the bands, slot nz and A's arrays on the device are as they were"""
        ba = self.ba.get(what)
        assert bits(ba[-1:])[0] == bits(np.array([MARK]))[0], "%s: slot nz was written" % what
        assert np.array_equal(self.dev.get(self.dai, self.n + 1, np.int32), self.ai) and np.array_equal(self.dev.get(self.daj, self.nz, np.int32), self.aj), what
        assert np.array_equal(bits(self.dev.get(self.daa, self.nz)), bits(self.aa)), "%s: A's values were modified" % what
        return ba


def _same_bits(got, ref, mask, what):
    bad = mask & (bits(got) != bits(ref))
    assert not bad.any(), "%s: %d slots differ from the reference, first %s: got %r, reference %r" % (
        what, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])


def _by_rule(got, ref, mask, what):
    bad = mask & ilf.rule_violations(got, ref)
    assert not bad.any(), "%s: %d slots break the comparison rule, first %s: got %r, reference %r" % (
        what, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])


def _untouched(got, mask, what):
    bad = mask & (bits(got) != bits(np.array([MARK]))[0])
    assert not bad.any(), "%s: slots %s hold %r instead of the marker" % (what, np.flatnonzero(bad)[:8], got[bad][:8])


# ---------------------------------------------------------------- 3. every path, finite data
@pytest.mark.parametrize("name", list(ilf.SHAPES))
def test_every_path_on_finite_data_carries_the_reference_bits(dev, name):
    ai, aj, aa = ilf.shape(name)
    ref, _ = ilf.clean_factor(name)
    lanes, wide = ilf.SHAPES[name]
    with Factor(dev, ai, aj, aa) as F:
        assert F.lanes == lanes and (np.diff(ai).max() > ilf.WAVE) == wide, "%s: %d lanes" % (name, F.lanes)
        frow, fabs_ = F.run()
        assert frow[0] == -1 and fabs_[0] == 0.0, name
        ba = F.values(name)
        every = np.ones(ba.size, dtype=bool); every[-1] = False
        _same_bits(ba, ref, every, name)
        # nothing pending: a second pass reports success and touches nothing
        F.ba.put(np.full(ba.size, MARK))
        frow, _ = F.run()
        assert frow[0] == -1
        _untouched(F.values(name + ", second pass"), np.ones(ba.size, dtype=bool), name + ", second pass")


@pytest.mark.parametrize("name", ilf.LARGE_ZP_SHAPES)
def test_a_large_zeropivot_passes_every_dominant_pivot(dev, name):
    """zeropivot = 0.75: |w_i| > rs in every row, nothing fails -- a test that counted |w_i| into rs would fail the rows with
    |w_i| <= 3 rs"""
    ai, aj, aa = ilf.shape(name)
    ref, rfrow, _ = ilf.large_zeropivot_case(name)
    with Factor(dev, ai, aj, aa) as F:
        frow, fabs_ = F.run(zeropivot=ilf.ZP_LARGE)
        assert frow[0] == rfrow[0] == -1 and fabs_[0] == 0.0, "%s: row %d reported" % (name, frow[0])
        every = np.ones(ref.size, dtype=bool); every[-1] = False
        _same_bits(F.values(name), ref, every, name)


def test_every_lane_width_and_both_row_forms_have_run(dev):
    """what the other tests of this module rely on, from mi355x_ilu0_factor_info alone"""
    seen = set()
    for name, (lanes, wide) in ilf.SHAPES.items():
        ai, aj, aa = ilf.shape(name)
        with Factor(dev, ai, aj, aa) as F:
            assert F.lanes == lanes
            seen.add((F.lanes, bool(np.diff(ai).max() > ilf.WAVE)))
    assert seen == {(1, False), (2, False), (4, False), (8, False), (16, False), (32, False), (64, False), (64, True)}


# ---------------------------------------------------------------- 4. IEEE specials inside the arithmetic
@pytest.mark.parametrize("which", ["default", "zero"])
@pytest.mark.parametrize("form", ilf.FORMS)
def test_specials_inside_the_arithmetic(dev, form, which):
    """ilufactor.special_cases: NaN / +-Inf in an L and in a U position of A, the skip of a stored zero next to an inverted pivot of
    Inf / NaN, signed zeros with shifts of +0.0 and -0.0, products that underflow and overflow, a subnormal pivot that inverts to
    Inf; every case a block of its own, in registers at 4 and at 64 lanes and in rows wider than a wavefront; with the default
    zeropivot and with zeropivot = 0"""
    m = ilf.specials_matrix(form)
    zp = ZP if which == "default" else 0.0
    nblk = m["blk"].size - 1
    ref, rfrow, rfabs, _ = ilf.reference_pass(m["ai"], m["aj"], m["aa"], m["blk"], m["shifts"], zp, np.ones(nblk, np.int32))
    with Factor(dev, m["ai"], m["aj"], m["aa"], blk=m["blk"]) as F:
        assert F.lanes == (4 if form == "narrow" else 64)
        frow, fabs_ = F.run(m["shifts"], zp)
        what = "specials, %s, zeropivot %s" % (form, which)
        assert np.array_equal(frow, rfrow), what
        assert np.array_equal(bits(fabs_), bits(rfabs)), what
        ba = F.values(what)
        _by_rule(ba, ref, ilf.compared_slots(m["ai"], m["aj"], m["blk"], rfrow), what)
        assert np.array_equal(bits(ba[F.layout[2][frow[frow >= 0]]]), bits(fabs_[frow >= 0])), what


@pytest.mark.parametrize("form", ilf.FORMS)
def test_a_special_stays_inside_the_rows_it_can_reach(dev, form):
    """four independent sub-blocks factored as one block; NaN, +Inf, -Inf in one off-diagonal entry, three rounds: the rows out of
    reach carry the clean factor's bits, the rows in reach follow the reference by the comparison rule"""
    c = ilf.containment_case(form)
    ai, aj = c["ai"], c["aj"]
    n = ai.size - 1
    for rd, (r, q, aap, ref, reach) in enumerate(c["rounds"]):
        what = "containment, %s, round %d (row %d)" % (form, rd, r)
        with Factor(dev, ai, aj, aap) as F:
            frow, _ = F.run(zeropivot=0.0)
            assert frow[0] == -1, what
            ba = F.values(what)
            _same_bits(ba, c["clean"], ilf.row_slots(ai, aj, ~reach), what + ", out of reach")
            _by_rule(ba, ref, ilf.row_slots(ai, aj, np.ones(n, dtype=bool)), what)


# ---------------------------------------------------------------- 5. failure report, blocks, passes
@pytest.mark.parametrize("name", ilf.FAIL_SHAPES)
def test_one_failing_row_is_reported_with_its_pivot(dev, name):
    """a row of level 0 and the row of the deepest level (wide: register and wide rows of both), one per run: failed_row is that row,
    failed_abs the bits of the reference's |w_i| -- zero, nonzero, of a negative pivot --, the pivot's slot holds the same value, the
    rows that ran before it carry the reference's bits"""
    ai, aj, _ = ilf.shape(name)
    for r in ilf.failing_rows(name):
        aa, ref, rabs = ilf.failing_case(name, r)
        what = "%s, failing row %d" % (name, r)
        with Factor(dev, ai, aj, aa) as F:
            frow, fabs_ = F.run()
            assert frow[0] == r, "%s: row %d reported" % (what, frow[0])
            assert bits(fabs_)[0] == bits(np.array([rabs]))[0], "%s: failed_abs %r, reference %r" % (what, fabs_[0], rabs)
            ba = F.values(what)
            assert bits(ba[F.layout[2][r]:F.layout[2][r] + 1])[0] == bits(fabs_)[0], what
            _same_bits(ba, ref, ilf.compared_slots(ai, aj, None, np.array([r])), what)


def test_forty_blocks_three_passes_each_block_its_own_shift(dev):
    """ilufactor.blocks_case: empty ranges, one-row blocks, blocks that pass at once, after one shift, after two.  After pass 1 the
    finished blocks' slots are overwritten with the marker on the device: later passes leave it there bit for bit (recomputing a
    finished block would give the same values and go unseen otherwise).  Every pass: failed_row, failed_abs and ba as the reference."""
    c = ilf.blocks_case()
    ai, aj, blk = c["ai"], c["aj"], c["blk"]
    with Factor(dev, ai, aj, c["aa"], blk=blk) as F:
        for ps, (shifts, ref, rfrow, rfabs, _) in enumerate(c["passes"]):
            what = "40 blocks, pass %d" % (ps + 1)
            frow, fabs_ = F.run(shifts)
            assert np.array_equal(frow, rfrow), what
            assert np.array_equal(bits(fabs_), bits(rfabs)), what
            ba = F.values(what)
            if ps == 0:
                ba[c["finished1"]] = MARK
                F.ba.put(ba)
            _untouched(ba, c["finished1"], what)
            _same_bits(ba, ref, ilf.compared_slots(ai, aj, blk, rfrow) & ~c["finished1"], what)
        assert (frow == -1).all()


def test_several_failing_rows_in_one_block_report_one_of_them(dev):
    """three mutually independent failing rows of level 0 in one block: the row reported is one of them, failed_abs and the pivot's
    slot are that row's, the block stays pending -- the next pass, with a shift, factors it"""
    ai, aj, aa, absof, shift, ref = ilf.multi_fail_case()
    with Factor(dev, ai, aj, aa) as F:
        frow, fabs_ = F.run()
        assert int(frow[0]) in absof, frow
        assert bits(fabs_)[0] == bits(np.array([absof[int(frow[0])]]))[0]
        ba = F.values("several failing rows")
        assert bits(ba[F.layout[2][frow[0]]:F.layout[2][frow[0]] + 1])[0] == bits(fabs_)[0]
        frow, _ = F.run([shift])
        assert frow[0] == -1
        every = np.ones(ba.size, dtype=bool); every[-1] = False
        _same_bits(F.values("several failing rows, shifted"), ref, every, "several failing rows, shifted")


# ---------------------------------------------------------------- 6. the sweep form and the layout checks
@pytest.mark.parametrize("name", ilf.SWEEP_SHAPES)
def test_sweep_form_of_a_factor_with_specials(dev, name):
    """aL = -ba over the L part, aU = -ba over the strict upper triangle as CSR, dinv the pivots' slots: negation flips the sign bit
    of +-0.0 and +-Inf, a NaN stays a NaN; guard bands around the three outputs, ba unchanged"""
    ai, aj, aa = ilf.shape(name)
    ba = ilf.sweep_factor(name)
    with Factor(dev, ai, aj, aa) as F:
        bi, bj, bd = F.layout
        n = F.n
        (iL, jL, aL), (iU, jU, aU), dinv = strict_triangles((bi, bj, bd, ba))
        F.ba.put(ba)
        diU = dev.put(_i32(iU))
        outs = [Guarded(dev, a.size) for a in (aL, aU, dinv)]
        dev.chk(dev.k.mi355x_ilu0_factor_to_sweeps(dev.h, F.ctx, diU, F.ba.ptr, *[g.ptr for g in outs]))
        dev.sync()
        for g, a, nm in zip(outs, (aL, aU, dinv), ("aL", "aU", "dinv")):
            what = "%s, %s" % (name, nm)
            _by_rule(g.get(what), a, np.ones(a.size, dtype=bool), what)
        assert np.array_equal(bits(F.ba.get(name)), bits(ba))
        assert (aL.size == 0) == (name in ilf.ONE_LEVEL) and dinv.size == n
        dev.free(diU)
        for g in outs:
            g.free()


def _corruptions(bi, bj, bd, nlev, levptr, rows, blk):
    """name -> the arguments of _create with one array corrupted in one place"""
    n = bi.size - 1
    good = dict(bi=bi, bj=bj, bd=bd, levptr=levptr, rows=rows, blk=blk)

    def changed(key, idx, value):
        a = good[key].copy(); a[idx] = value
        return dict(good, **{key: a})
    i = int(np.flatnonzero(np.diff(bi) >= 2)[0])                # a row with two L entries at least
    u = int(np.flatnonzero(bd[:-1] - bd[1:] - 1 >= 1)[0])       # a row with a U entry
    swapped = bj.copy(); swapped[bi[i]], swapped[bi[i] + 1] = bj[bi[i] + 1], bj[bi[i]]
    return {
        "bi[0]": changed("bi", 0, 1), "bdiag[n]": changed("bd", n, bd[n] + 1), "levptr[0]": changed("levptr", 0, 1),
        "levptr[nlev]": changed("levptr", nlev, n - 1), "decreasing levptr": changed("levptr", 1, levptr[2] + 1),
        "duplicated row": changed("rows", 1, rows[0]), "row out of range": changed("rows", 0, n), "negative row": changed("rows", 0, -1),
        "L column >= i": changed("bj", bi[i + 1] - 1, i), "unsorted L row": dict(good, bj=swapped),
        "U column <= i": changed("bj", bd[u + 1] + 1, u), "U column >= n": changed("bj", bd[u] - 1, n),
        "bj[bdiag[i]] != i": changed("bj", bd[u], u + 1), "blk[0]": changed("blk", 0, 1), "blk[nblk]": changed("blk", blk.size - 1, n - 1),
        "decreasing blk": changed("blk", 1, blk[2] + 1), "decreasing blk, past n": changed("blk", 1, n + 8),
    }


def test_create_refuses_every_layout_that_does_not_hold_together(dev):
    """one array corrupted in one place for every check in mi355x_ilu0_factor_create's list: hipErrorInvalidValue and a NULL context,
    decided on the host before anything is allocated or launched; the uncorrupted arguments are accepted"""
    ai, aj, _ = ilf.shape("rows8")
    bi, bj, bd, nlev, levptr, rows = symbolic(ai, aj, ilf.tame(ai, aj))
    blk = np.array([0, 10, 10, 50, ai.size - 1], np.int32)       # (the checks do not ask whether the blocks are independent)
    n, nblk = ai.size - 1, blk.size - 1
    assert nlev >= 3 and levptr[2] < n
    rc, ctx = _create(dev, n, bi, bj, bd, nlev, levptr, rows, nblk, blk)
    assert rc == 0 and ctx.value
    dev.chk(dev.k.mi355x_ilu0_factor_destroy(ctx))
    bad = _corruptions(bi, bj, bd, nlev, levptr, rows, blk)
    assert len(bad) == 17
    for name, a in bad.items():
        rc, ctx = _create(dev, n, a["bi"], a["bj"], a["bd"], nlev, a["levptr"], a["rows"], nblk, a["blk"])
        assert rc == INVALID and not ctx.value, "%s: returned %d" % (name, rc)
