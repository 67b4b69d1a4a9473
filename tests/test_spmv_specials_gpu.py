"""What the idle lanes of the SpMV kernels read must not reach y, and IEEE special values inside the pattern must come out as the
reference's loops give them (tests/specials.py holds the host side; test_spmv_specials_cpu.py checks it without a GPU).

1. Containment.  Every product runs twice on one plan, with a clean x and with a set P of columns of x overwritten by NaN, +Inf,
   -Inf (the columns idle lanes and cut pairs gather: the slack entries behind aj, the ends of every row block and their
   neighbours in the stream, columns 0 and n - 1, ...).  Rows without a column in P must not change by a bit; rows with one must
   have the class of the oracle's result and, where that is not NaN, its bits (one-lane rows) or 1e-12 * sum|a_ij x_j| over the
   finite products (lane trees, long rows, MFMA: BASELINE.md).
2. Special values inside the pattern: hand-built matrices (specials.special_matrix*), the expected value of each row stated there.

Every upload goes through `upload`: two NaN behind aa, two copies of a valid column behind aj; every output vector sits between
guard words that must survive the launch."""
import ctypes as C

import numpy as np
import pytest

import orc
import specials as sp
from test_abi_kernels_gpu import BSR_SHAPES
from test_kernels_gpu import assert_bitexact, dev, make_plan  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu

GUARD = 8                                                     # doubles on each side of an output vector
GUARD_BITS = np.uint64(0xC0DEC0DEFACEFEED)                    # (a finite negative double no test value equals)
assert "ragged" in BSR_SHAPES


def marker(m):
    """pre-fill of an output vector: differs per row, far from every result"""
    return -(1e250 + np.arange(m, dtype=np.float64) * 1e235)


class Guarded:
    """a device vector of m doubles with GUARD marker words before and after it; .p is the 16-byte aligned interior"""
    def __init__(self, dev, a):
        self.dev, self.m = dev, a.size
        h = np.empty(a.size + 2 * GUARD)
        h.view(np.uint64)[:GUARD] = GUARD_BITS
        h.view(np.uint64)[GUARD + a.size:] = GUARD_BITS
        h[GUARD:GUARD + a.size] = a
        self.base = dev.put(h)
        self.p = C.c_void_p(self.base.value + 8 * GUARD)
        assert self.p.value % 16 == 0

    def get(self):
        h = self.dev.get(self.base, self.m + 2 * GUARD)
        g = np.concatenate((h.view(np.uint64)[:GUARD], h.view(np.uint64)[GUARD + self.m:]))
        assert np.all(g == GUARD_BITS), "guard words around an output vector were overwritten: %s" % np.flatnonzero(g != GUARD_BITS)
        return h[GUARD:GUARD + self.m].copy()

    def free(self):
        self.dev.free(self.base)


def upload(dev, ai, aj, aa, c_slack, nx, scalar=False):
    """(ai, aj, aa) on the device: aa followed by two NaN, aj by two copies of the valid column c_slack (what a pair load past the
    end reads).  scalar: aa 8 bytes off a 16-byte boundary and aj 4 bytes off an 8-byte one (the scalar stream)."""
    assert 0 <= c_slack < nx and (aj.size == 0 or 0 <= int(aj.min()) <= int(aj.max()) < nx)    # every index the kernels can gather with is a column of x (nx of them)
    pre_j, pre_a = ([c_slack], [np.nan]) if scalar else ([], [])
    bj = dev.put(np.concatenate((pre_j, aj, [c_slack, c_slack])).astype(np.int32))
    ba = dev.put(np.concatenate((pre_a, aa, [np.nan, np.nan])))
    daj = C.c_void_p(bj.value + 4) if scalar else bj
    daa = C.c_void_p(ba.value + 8) if scalar else ba
    assert (daa.value % 16 == 8 and daj.value % 8 == 4) if scalar else (daa.value % 16 == 0 and daj.value % 8 == 0)
    return dev.put(ai), daj, daa, [bj, ba]


class Csr:
    """one plan + its uploads; run(mode, dx) launches one product between guards and returns the whole output vector"""
    def __init__(self, dev, ai, aj, aa, c_slack, nx, form="plain", rows=None, m_out=None, nan_values=False):
        self.dev, self.k = dev, dev.k
        k = dev.k
        self.ai, self.aj, self.aa = ai, aj, np.ascontiguousarray(aa)
        self.m_out = ai.size - 1 if m_out is None else m_out
        up = np.full(aa.size, np.nan) if nan_values else self.aa          # value patterns: the device value array is not read
        self.dai, self.daj, self.daa, self.bufs = upload(dev, ai, aj, up, c_slack, nx, scalar=form == "scalar")
        self.plan = make_plan(dev, ai, rows)
        self.form = form
        if form in ("idx8", "rowpat"):
            dev.chk(k.mi355x_spmv_plan_compress_indices(dev.h, self.plan, ai.ctypes.data, aj.ctypes.data))
            nt, npat = C.c_int(), C.c_int()
            k.mi355x_spmv_plan_is_compressed(self.plan, C.byref(nt))
            dev.chk(k.mi355x_spmv_plan_use_patterns(self.plan, int(form == "rowpat"), C.byref(npat)))
            assert nt.value > 0 and (form == "idx8" or npat.value > 0), "the analysis declined: the %s kernel would not run" % form
        elif form == "valpat":
            nv = C.c_int()
            dev.chk(k.mi355x_spmv_plan_value_patterns(dev.h, self.plan, ai.ctypes.data, aj.ctypes.data, self.aa.ctypes.data, C.byref(nv)))
            assert nv.value > 0, "the value-pattern analysis declined"
        elif form == "grouped":
            nodes, ns = orc.check_inode(ai, aj)
            ns = np.ascontiguousarray(ns, dtype=np.int32)
            dev.chk(k.mi355x_spmv_plan_group_rows(dev.h, self.plan, ai.ctypes.data, aj.ctypes.data, nodes, ns.ctypes.data))
            ng = C.c_int()
            k.mi355x_spmv_plan_group_info(self.plan, C.byref(ng), None, None)
            assert ng.value > 0, "the grouping declined"
        yes = C.c_int()
        dev.chk(k.mi355x_spmv_plan_dot_available(self.plan, self.daa, C.byref(yes)))
        self.dot = yes.value == 1
        assert self.dot == (form in ("idx8", "rowpat", "valpat"))

    def info(self):
        nb, nl = C.c_int(), C.c_int()
        self.dev.chk(self.k.mi355x_spmv_plan_info(self.plan, C.byref(nb), C.byref(nl), None))
        return nb.value, nl.value

    def pairsum(self, on):
        self.dev.chk(self.k.mi355x_spmv_plan_set_pairsum(self.plan, int(on)))

    def modes(self):
        return ["mult", "add_alias", "add", "scaled"] + (["add_scaled"] if self.form in ("plain", "scalar") else []) + (["dot"] if self.dot else [])

    def run(self, mode, dx, y0=None, d=None, zfill=None):
        """-> (output vector, x'y or None).  mult / scaled / add / add_scaled / dot write a vector pre-filled with zfill (default: the
        per-row marker); add_alias writes into y0's own vector."""
        dev, k, a = self.dev, self.k, (self.dai, self.daj, self.daa)
        out = Guarded(dev, marker(self.m_out) if zfill is None else zfill)
        held = [out]
        dot = None
        if mode == "mult":
            dev.chk(k.mi355x_spmv_csr(dev.h, self.plan, *a, dx, out.p))
        elif mode == "dot":
            dout = Guarded(dev, marker(1)); held.append(dout)
            dev.chk(k.mi355x_spmv_csr_dot(dev.h, self.plan, *a, dx, out.p))
            dev.chk(k.mi355x_spmv_dot_finish(dev.h, self.plan, dout.p))
            dot = dout.get()[0]
        elif mode == "scaled":
            dd = Guarded(dev, d); held.append(dd)
            dev.chk(k.mi355x_spmv_csr_scaled(dev.h, self.plan, *a, dx, dd.p, out.p))
            assert_bitexact(dd.get(), d)
        else:
            yv = Guarded(dev, y0); held.append(yv)
            if mode == "add_alias":
                dev.chk(k.mi355x_spmv_csr_add(dev.h, self.plan, *a, dx, yv.p, yv.p))
                out, yv = yv, out
            elif mode == "add":
                dev.chk(k.mi355x_spmv_csr_add(dev.h, self.plan, *a, dx, yv.p, out.p))
                assert_bitexact(yv.get(), y0)                                 # y is an input
            else:
                assert mode == "add_scaled"
                dd = Guarded(dev, d); held.append(dd)
                dev.chk(k.mi355x_spmv_csr_add_scaled(dev.h, self.plan, *a, dx, yv.p, dd.p, out.p))
                assert_bitexact(yv.get(), y0)
        got = out.get()
        for h in held:
            h.get()                                                           # every vector's guards
            h.free()
        return got, dot

    def free(self):
        self.dev.chk(self.k.mi355x_spmv_plan_destroy(self.plan))
        for q in [self.dai] + self.bufs:
            self.dev.free(q)


def check_dot(got, x, y, what):
    """the x'y by-product: NaN / +-Inf exactly when the oracle's dot of the device y is (the class of a sum of x_r y_r does not
    depend on its order either), else within 1e-13 * sum|x_r y_r|"""
    x = np.ascontiguousarray(x[:y.size])                                      # (the by-product reads x_r of the rows only)
    with np.errstate(all="ignore"):
        ref = orc.vec_dot(x, y)
        assert sp.classify(got) == sp.classify(ref), "%s: x'y = %r, oracle %r" % (what, got, ref)
        if np.isfinite(ref):
            assert abs(got - ref) <= 1e-13 * np.sum(np.abs(x * y)), "%s: x'y = %r, oracle %r" % (what, got, ref)


def containment_rounds(dev, csr, A, x, y0, d, Ps, exact, pairsums, unlisted=None, what="", inf_dot=False):
    """section 1 for one plan: every mode (and summation order) with the clean x, then with every P of Ps.  A = (ai, aj, aa, n) is
    the matrix the oracle multiplies (the expanded one for a compressed-row plan: `unlisted` rows must keep their pre-fill)."""
    ai, aj, aa, n = A
    dxc = dev.put(x)
    for pairsum in pairsums:
        csr.pairsum(pairsum)
        for mode in csr.modes():
            tag = "%s %s pairsum %d" % (what, mode, pairsum)
            pre = y0 if mode == "add_alias" or unlisted is not None and mode == "add" else marker(csr.m_out)
            zfill = y0 if unlisted is not None and mode == "add" else None      # compressed rows: z pre-filled with y
            # the clean run, against the oracle
            clean, cdot = csr.run(mode, dxc, y0, d, zfill)
            ref = sp.oracle(mode, pairsum, ai, aj, aa, x, y0, d)
            if unlisted is not None:
                ref[unlisted] = pre[unlisted]
                assert_bitexact(clean[unlisted], pre[unlisted])
            sp.check_against_reference(clean, ref, exact, sp.mode_bound(mode, sp.finite_scale(ai, aj, aa, x), y0, d), tag + " clean")
            if mode == "dot":
                check_dot(cdot, x, clean, tag + " clean")
            for r, P in enumerate(Ps):
                xp = sp.poison(x, P, shift=r)
                hit = sp.hit_rows(ai, aj, P, n)
                listed = hit.size if unlisted is None else int((~unlisted).sum())
                assert 0 < hit.sum() <= listed // 2                                # the round is informative (a condition on the inputs)
                dxp = dev.put(xp)
                got, gdot = csr.run(mode, dxp, y0, d, zfill)
                dev.free(dxp)
                ref = sp.oracle(mode, pairsum, ai, aj, aa, xp, y0, d)
                if unlisted is not None:
                    ref[unlisted] = pre[unlisted]
                sp.check_containment(clean, got, ref, hit, exact, sp.mode_bound(mode, sp.finite_scale(ai, aj, aa, xp), y0, d), "%s round %d" % (tag, r))
                if mode == "dot":
                    check_dot(gdot, xp, got, "%s round %d" % (tag, r))
            if mode == "dot" and inf_dot:
                # The rounds above all hold a NaN, so their x'y is NaN.  An infinite one: x > 0 but for one -Inf, on an operator with
                # a positive diagonal and negative off-diagonals: every infinite x_r y_r is +Inf (a condition on the inputs, asserted)
                xi = np.abs(x) + 0.5
                xi[n // 2] = -np.inf
                ref = sp.oracle(mode, pairsum, ai, aj, aa, xi, y0, d)
                with np.errstate(all="ignore"):
                    assert np.isposinf(orc.vec_dot(xi, ref)) and np.isinf(ref).sum() >= 2 and not np.isnan(ref).any()
                dxi = dev.put(xi)
                got, gdot = csr.run(mode, dxi, y0, d, zfill)
                dev.free(dxi)
                sp.check_against_reference(got, ref, exact, sp.mode_bound(mode, sp.finite_scale(ai, aj, aa, xi), y0, d), tag + " one -Inf")
                check_dot(gdot, xi, got, tag + " one -Inf")
    dev.free(dxc)


# ------------------------------------------------------------------------------------------------ 1. containment
@pytest.mark.parametrize("form,shape", sp.CSR_FORMS)
def test_csr_idle_lanes_are_contained(dev, form, shape):
    """the CSR row-block family: plain (pair stream and scalar stream), 8-bit offsets, row patterns, value patterns, grouped rows;
    mi355x_spmv_csr, _add (aliased and not), _scaled, _add_scaled (plain), _csr_dot where the plan offers it; both summation
    orders where every row is a one-lane row"""
    c = sp.csr_case(shape)
    csr = Csr(dev, c["ai"], c["aj"], c["aa"], sp.C_SLACK, c["n"], form=form, nan_values=form == "valpat")
    if form != "grouped":                                                     # (grouping rebuilds the blocks from whole groups)
        assert csr.info() == (c["rb"].size - 1, c["nlong"])                   # the host recovery of the row blocks is the plan's
    if form in ("rowpat", "valpat"):
        exact = np.ones(c["m"], dtype=bool)                                   # one lane per row whatever its length
    elif form == "grouped":
        exact = np.full(c["m"], bool(np.max(np.diff(c["ai"])) <= sp.SEQ_AVG))  # whatever the groups' blocks are: no block above 16 per row, or no claim
    else:
        exact = c["one_lane"]
    pairsums = (0, 1) if exact.all() else (0,)
    containment_rounds(dev, csr, (c["ai"], c["aj"], c["aa"], c["n"]), c["x"], c["y0"], c["d"], c["Ps"], exact, pairsums, what="%s %s" % (form, shape),
                       inf_dot=shape.startswith("p7"))
    csr.free()


def bsr_rounds(dev, c, launch, what, add=None):
    """containment for one BSR kernel: launch(dx, out_ptr) is y = A x; add(dx, y_ptr, z_ptr) the MatMultAdd entry, if any.
    P is a set of block columns (one point entry of each poisoned), hit the block rows with one of them: all their point rows."""
    bs, m = c["bs"], c["mbs"] * c["bs"]
    never = np.zeros(m, dtype=bool)                                           # point rows are summed with stride bs by a tree: no bit claim,
    never[c["empty"]] = True                                                  # but for block rows without blocks: +0.0 / y0's own bits
    assert c["empty"].size >= 2 * bs and np.signbit(c["y0"][c["empty"][::2]]).all() and np.all(c["y0"][c["empty"][::2]] == 0.0)
    blk = np.searchsorted(c["rb"], c["empty"] // bs, side="right") - 1        # their row blocks hold values: not the only-empty-rows exit
    assert np.all(c["ai"][c["rb"][blk + 1]] > c["ai"][c["rb"][blk]])

    def run(dx, mode):
        out = Guarded(dev, marker(m))
        if mode == "mult":
            launch(dx, out.p); res = out
        else:
            yv = Guarded(dev, c["y0"])
            add(dx, yv.p, yv.p if mode == "add_alias" else out.p)
            res = yv if mode == "add_alias" else out
            if mode == "add":
                assert_bitexact(yv.get(), c["y0"])
            (out if mode == "add_alias" else yv).get()
            (out if mode == "add_alias" else yv).free()
        got = res.get(); res.free()
        return got

    def reference(x, mode):
        with np.errstate(all="ignore"):
            ref = orc.spmv_bsr(bs, c["ai"], c["aj"], c["aa"], x)
            scale = sp.finite_scale(c["pai"], c["paj"], c["paa"], x)
            if mode == "mult":
                return ref, scale
            radd = c["y0"] + ref
            radd[c["empty"]] = c["y0"][c["empty"]]                            # MatMultAdd on a block row without blocks: z = y0 itself, -0.0 included
            return radd, scale + np.abs(c["y0"])
    dxc = dev.put(c["x"])
    for mode in ["mult"] + (["add_alias", "add"] if add else []):
        clean = run(dxc, mode)
        ref, bound = reference(c["x"], mode)
        sp.check_against_reference(clean, ref, never, bound, "%s %s clean" % (what, mode))
        for r, P in enumerate(c["Ps"]):
            xp = sp.poison(c["x"], P, shift=r, stride=bs)
            hit = sp.hit_rows(c["ai"], c["aj"], P, c["nbs"])
            assert 0 < hit.sum() <= c["mbs"] // 2
            dxp = dev.put(xp)
            got = run(dxp, mode)
            dev.free(dxp)
            ref, bound = reference(xp, mode)
            sp.check_containment(clean, got, ref, np.repeat(hit, bs), never, bound, "%s %s round %d" % (what, mode, r))
    dev.free(dxc)


@pytest.mark.parametrize("bs", [3, 4, 5])
def test_bsr_idle_lanes_are_contained(dev, bs):
    """bsr_rowblock_kernel with x gathered and with x staged in LDS (+ the add entry, aliased and not), the wavefront kernel,
    and for bs = 4 the two v_mfma_f64_4x4x4 variants (lanes past the row contribute 0 * 0 whatever x holds), on the `ragged` shape"""
    k = dev.k
    c = sp.bsr_case(bs)
    dai, daj, daa, bufs = upload(dev, c["ai"], c["aj"], c["aa"], sp.C_SLACK, c["nbs"])
    plan = make_plan(dev, (c["ai"].astype(np.int64) * bs * bs).astype(np.int32))
    nb, nl = C.c_int(), C.c_int()
    dev.chk(k.mi355x_spmv_plan_info(plan, C.byref(nb), C.byref(nl), None))
    assert (nb.value, nl.value) == (c["rb"].size - 1, c["nlong"])
    for xlds in (0, 1):
        bsr_rounds(dev, c, lambda dx, y: dev.chk(k.mi355x_spmv_bsr_planned_form(dev.h, plan, bs, xlds, dai, daj, daa, dx, y)), "bsr planned bs %d x_in_lds %d" % (bs, xlds),
                   add=(lambda dx, y, z: dev.chk(k.mi355x_spmv_bsr_planned_add(dev.h, plan, bs, dai, daj, daa, dx, y, z))) if xlds else None)
    bsr_rounds(dev, c, lambda dx, y: dev.chk(k.mi355x_spmv_bsr(dev.h, c["mbs"], bs, dai, daj, daa, dx, y)), "bsr wavefront bs %d" % bs)
    if bs == 4:
        for variant in (0, 1):
            bsr_rounds(dev, c, lambda dx, y: dev.chk(k.mi355x_spmv_bsr4_mfma(dev.h, c["mbs"], variant, dai, daj, daa, dx, y)), "bsr4_mfma variant %d" % variant)
    dev.chk(k.mi355x_spmv_plan_destroy(plan))
    for q in [dai] + bufs:
        dev.free(q)


# ------------------------------------------------------------------------------------------------ 2. specials inside the pattern
def run_all_modes(dev, csr, s, pairsum, what, exact, expect):
    """every mode of the plan on a special-value matrix: NaN where the oracle has NaN, everything else its bits (`exact`) or within
    the bound, and the hand-stated values of specials.py"""
    ai, aj, aa, x, y0, d = (s[k] for k in ("ai", "aj", "aa", "x", "y0", "d"))
    ex = np.full(ai.size - 1, exact)
    csr.pairsum(pairsum)
    dx = dev.put(x)
    for mode in csr.modes():
        got, gdot = csr.run(mode, dx, y0, d)
        ref = sp.oracle(mode, pairsum, ai, aj, aa, x, y0, d)
        sp.check_against_reference(got, ref, ex, sp.mode_bound(mode, sp.finite_scale(ai, aj, aa, x), np.where(np.isfinite(y0), y0, 0.0), np.where(np.isfinite(d), d, 0.0)),
                                   "%s %s pairsum %d" % (what, mode, pairsum))
        col = {"mult": 0, "dot": 0, "add": 1, "add_alias": 1, "scaled": 2}.get(mode)
        if col is not None:
            sp.assert_expected(got, expect, col, "%s %s pairsum %d" % (what, mode, pairsum))
        if mode == "dot":
            check_dot(gdot, x, got, what)
    dev.free(dx)


@pytest.mark.parametrize("form", ["plain", "scalar", "idx8", "rowpat", "valpat", "grouped"])
def test_special_values_inside_the_pattern_one_lane_rows(dev, form):
    """specials.special_matrix (each row described there): signed zeros, rows without entries with y0 / d = -0.0, Inf, NaN, < 0,
    0.0 * Inf, Inf - Inf, Inf + finite, denormal products and sums, overflow in the sum only, and the row on which the
    two-at-a-time order overflows and the one-at-a-time order does not -- in every form, mode and both orders, bit for bit"""
    s = sp.special_matrix()
    csr = Csr(dev, s["ai"], s["aj"], s["aa"], s["c_slack"], s["x"].size, form=form, nan_values=form == "valpat")
    assert csr.info()[0] == 1 or form == "grouped"
    for pairsum in (0, 1):
        expect = dict(s["expect"])
        if pairsum:
            expect.update(s["expect_pair"])
        run_all_modes(dev, csr, s, pairsum, "specials %s" % form, True, expect)
    csr.free()


@pytest.mark.parametrize("form", ["plain", "scalar", "idx8"])
def test_special_values_inside_the_pattern_lane_trees(dev, form):
    """specials.special_matrix_multilane: 81-entry rows, 8 lanes per row.  The values asserted are the ones IEEE arithmetic fixes
    whatever the tree (argued there); finite rows within 1e-12 * sum|a_ij x_j| of the oracle"""
    t = sp.special_matrix_multilane()
    csr = Csr(dev, t["ai"], t["aj"], t["aa"], t["c_slack"], t["x"].size, form=form)
    assert csr.info() == (1, 0)
    run_all_modes(dev, csr, t, 0, "multilane specials %s" % form, False, t["expect"])
    csr.free()


@pytest.mark.parametrize("form", ["plain", "scalar", "idx8", "rowpat", "valpat"])
def test_blocks_of_only_empty_rows_in_every_output_mode(dev, form):
    """row blocks without a nonzero take the kernels' early exit (spmv_empty<ADD>): 600 rows, the first 300 without entries (one
    whole block), y0 / d cycling -0.0, Inf, NaN, -2.5, 3.0 there.  A x = +0.0; y0 + A x = y0; d .* (A x) = d * 0.0 (MatMult then
    VecPointwiseMult: -0.0 for d < 0, NaN for d = Inf); d .* (y0 + A x) = d * y0"""
    m = 600
    lens = np.where(np.arange(m) < 300, 0, 1 + np.arange(m) % 3)
    ai = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    aj = np.concatenate([np.sort((r + np.arange(ln) - 1) % m) for r, ln in enumerate(lens)]).astype(np.int32)
    aa = np.tile([2.0, -1.0, 0.5], aj.size)[:aj.size] if form == "valpat" else sp.clean_x(aj.size, 31)
    x = sp.clean_x(m, 32)
    vals = np.resize([-0.0, np.inf, np.nan, -2.5, 3.0], m)
    y0 = np.where(np.arange(m) < 300, vals, sp.clean_x(m, 33))
    d = np.where(np.arange(m) < 300, np.roll(vals, 1), sp.clean_x(m, 34))
    csr = Csr(dev, ai, aj, aa, 1, m, form=form, nan_values=form == "valpat")
    assert csr.info() == (3, 0)
    with np.errstate(all="ignore"):
        dz = d * 0.0
    run_all_modes(dev, csr, dict(ai=ai, aj=aj, aa=aa, x=x, y0=y0, d=d), 0, "empty blocks %s" % form, True,
                  {r: (0.0, None if np.isnan(y0[r]) else y0[r], None if np.isnan(dz[r]) else dz[r]) for r in range(300)})
    csr.free()
