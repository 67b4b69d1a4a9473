"""The fused-level block solves on the device: mi355x_bilu_lower_chain / _upper_chain (csrc/bilu.hip: a run of consecutive dependency
levels in ONE launch of one workgroup, a barrier between levels) through the C ABI, and the plug-in's -pc_factor_hipmi355x_trisolve fused
on a MATSEQBAIJHIPMI355X operator (host/bilu.c).

The chain runs the level kernel's arithmetic in the level kernel's order, so every comparison is on bit patterns and there is no
tolerance anywhere: against bilu_ref, and against the level kernels launched one by one as a second witness.  x and ba live between guard
bands of a marker."""
import ctypes as C

import numpy as np
import pytest

import bilu_ref as br
import problems as pb
from ilufactor import MARK, bits
from test_bilu_chain_cpu import plan_ref
from test_bilu_gpu import BlockFactor, bilu_info, bilu_pc, dominant, factor_of, gmres_right, ref_info
from test_ilu_device_factor_gpu import numeric_info, setup_again
from test_ilu_factor_specials_gpu import Guarded
from test_ilu_sweeps_gpu import V, apply
from test_kernels_gpu import dev, rnd  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu
INVALID, ERR_SUP = 1, 56
WAVE = 64


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def width(bs):
    """lanes of a block row's group"""
    return 2 if bs <= 2 else 4 if bs <= 4 else 8


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


# ---------------------------------------------------------------- shapes with prescribed levels
def coupled_blocks(nb, bs, pairs, seed=31):
    """block CSR of nb block rows: a dominant diagonal block in every row and the blocks (i, j) and (j, i) of every pair: (bi, bj, ba)"""
    rng = np.random.default_rng(seed)
    cols = [{i} for i in range(nb)]
    for i, j in pairs:
        cols[i].add(j); cols[j].add(i)
    bi, bj, blocks = [0], [], []
    for i in range(nb):
        for j in sorted(cols[i]):
            B = rng.standard_normal((bs, bs))
            if j == i:
                B = B + (4.0 * bs * len(cols[i])) * np.eye(bs)
            bj.append(j); blocks.append(B)
        bi.append(len(bj))
    return _i32(bi), _i32(bj), np.ascontiguousarray(np.array(blocks).transpose(0, 2, 1)).ravel()


def crossing(nlev, per, shift):
    """nlev levels of `per` block rows; row g of level l + 1 is coupled to row (g + shift) mod per of level l"""
    return nlev * per, [((l + 1) * per + g, l * per + (g + shift) % per) for l in range(nlev - 1) for g in range(per)]


def wide_between(before, wide, after):
    """a chain of `before` block rows, `wide` rows that all hang on its last one, and a chain of `after` rows whose first one hangs on
    all of them: levels of one row, one level of `wide` rows, levels of one row -- in L and, read backwards, in U"""
    pairs = [(i, i - 1) for i in range(1, before)] + [(before + g, before - 1) for g in range(wide)]
    pairs += [(before + wide, before + g) for g in range(wide)] + [(i, i - 1) for i in range(before + wide + 1, before + wide + after)]
    return before + wide + after, pairs


class ChainFactor(BlockFactor):
    """a BlockFactor with the rows of all levels in one device array per triangle and levptr next to it: what the chain kernels walk"""

    def __init__(self, dev, bs, layout, ba):
        super().__init__(dev, bs, layout, ba)
        self.set_levels(self.L, self.U)

    def set_levels(self, L, U):
        self.cL, self.cU = list(L), list(U)
        self.ptrL = _i32(np.concatenate(([0], np.cumsum([r.size for r in L])))); self.ptrU = _i32(np.concatenate(([0], np.cumsum([r.size for r in U]))))
        self.d_rowsL, self.d_rowsU = self.dev.put(_i32(np.concatenate(L))), self.dev.put(_i32(np.concatenate(U)))
        self.d_ptrL, self.d_ptrU = self.dev.put(self.ptrL), self.dev.put(self.ptrU)

    def lower_chain(self, l0, l1, db, dx, bs=None):
        return self.dev.k.mi355x_bilu_lower_chain(self.dev.h, l1 - l0, C.c_void_p(self.d_ptrL.value + 4 * l0), self.d_rowsL, bs or self.bs, self.d[0], self.d[1],
                                                  self.gba.ptr, db, dx)

    def upper_chain(self, l0, l1, dx, bs=None):
        return self.dev.k.mi355x_bilu_upper_chain(self.dev.h, l1 - l0, C.c_void_p(self.d_ptrU.value + 4 * l0), self.d_rowsU, bs or self.bs, self.d[1], self.gba.ptr,
                                                  self.d[2], dx)

    def run(self, b, planL=None, planU=None, alias=False, what=""):
        """lower then upper by a plan [(l0, l1, fused)] per triangle (default: one chain over all levels); x between guard bands,
        pre-filled with the marker (b itself when it aliases x).  A segment that is not fused is launched level by level."""
        planL = [(0, len(self.cL), 1)] if planL is None else planL
        planU = [(0, len(self.cU), 1)] if planU is None else planU
        gx = Guarded(self.dev, b.size)
        if alias:
            gx.put(b)
        db = gx.ptr if alias else self.dev.put(b)
        for l0, l1, fused in planL:
            if fused:
                self.dev.chk(self.lower_chain(l0, l1, db, gx.ptr))
            else:
                for l in range(l0, l1):
                    self.dev.chk(self.lower(l, db, gx.ptr))
        for l0, l1, fused in planU:
            if fused:
                self.dev.chk(self.upper_chain(l0, l1, gx.ptr))
            else:
                for l in range(l0, l1):
                    self.dev.chk(self.upper(l, gx.ptr))
        x = gx.get(what + ": x")
        self.unchanged(what)
        for p, a in ((self.d_rowsL, np.concatenate(self.cL)), (self.d_rowsU, np.concatenate(self.cU)), (self.d_ptrL, self.ptrL), (self.d_ptrU, self.ptrU)):
            assert np.array_equal(self.dev.get(p, a.size, np.int32), a), what + ": a level array was written"
        if not alias:
            assert np.array_equal(bits(self.dev.get(db, b.size)), bits(b)), what + ": b was written"
        gx.free()
        return x


def check_chain(dev, bs, bcsr, seed, sizes=None, what=""):
    """the chain over all levels == the reference == the level kernels one by one; returns the factor for more"""
    lay, f = factor_of(bs, bcsr)
    F = ChainFactor(dev, bs, lay, f)
    if sizes is not None:
        assert [r.size for r in F.L] == sizes and [r.size for r in F.U] == sizes
    b = rnd((bcsr[0].size - 1) * bs, seed)
    ref = br.apply(bs, lay, f, b)
    x = F.run(b, what=what)
    assert np.array_equal(bits(x), bits(ref)), what + ": chain against the reference"
    assert np.array_equal(bits(F.solve(b, what=what + ", level by level")), bits(x)), what + ": chain against the level kernels"
    return F, lay, f, b, ref


# ---------------------------------------------------------------- 1. the kernels through the C ABI
@pytest.mark.parametrize("bs", [2, 3, 4, 5, 6, 7])
def test_chain_over_all_levels_equals_the_reference_and_the_level_kernels(dev, bs):
    F = check_chain(dev, bs, pb.elasticity_like(3, 3, 2, dof=bs)[1], 40 + bs, what="bs %d" % bs)[0]
    assert len(F.L) > 1 and len(F.U) > 1


@pytest.mark.parametrize("bs", [3, 5])
def test_every_value_is_read_by_another_wave_than_the_one_that_wrote_it(dev, bs):
    """30 levels of 40 block rows; row g of level l + 1 reads row (g + 17) mod 40 of level l, in L, and the other way round in U.  A wave
    holds 64 / W = 16 (bs = 3) or 8 (bs = 5) block rows, fewer than the shift either way round, so no wave reads what it wrote itself:
    every dependency goes through the barrier and memory."""
    per, shift, nlev = 40, 17, 30
    groups = WAVE // width(bs)
    assert all(g // groups != ((g + shift) % per) // groups for g in range(per))
    nb, pairs = crossing(nlev, per, shift)
    check_chain(dev, bs, coupled_blocks(nb, bs, pairs), 50 + bs, sizes=[per] * nlev, what="crossing, bs %d" % bs)


@pytest.mark.parametrize("bs", [3, 5])
def test_a_level_of_several_passes_inside_a_chain(dev, bs):
    """levels of one block row, one level of 300, levels of one block row: the 300 are 2 passes of 256 groups (bs = 3) or 3 passes of 128
    (bs = 5), the last pass partly idle, and the rows after it read what every pass wrote"""
    nb, pairs = wide_between(5, 300, 5)
    passes = -(-300 // (1024 // width(bs)))
    assert passes == (2 if bs == 3 else 3)
    check_chain(dev, bs, coupled_blocks(nb, bs, pairs), 60 + bs, sizes=[1] * 5 + [300] + [1] * 5, what="wide level, bs %d" % bs)


def test_edge_chains(dev):
    """70 levels of one block row; the same with an empty level in the middle; one level; no level; a sub-range of the levels between
    level launches (what a mixed plan does)"""
    bs, n = 3, 70
    F, lay, f, b, ref = check_chain(dev, bs, br.block_tridiag(n, bs), 70, sizes=[1] * n, what="70 levels of one row")
    # a chain that is a sub-range of the levels, level launches before and after it
    plan = [(0, 9, 0), (9, 41, 1), (41, n, 0)]
    assert np.array_equal(bits(F.run(b, plan, plan, what="sub-range")), bits(ref))
    plan = [(0, 1, 1), (1, 2, 1), (2, 30, 0), (30, 31, 1), (31, n, 1)]                       # nlev = 1 three times
    assert np.array_equal(bits(F.run(b, plan, plan, what="chains of one level")), bits(ref))
    # nlev = 0 (and less) launches nothing: x keeps the marker
    gx = Guarded(dev, b.size)
    dev.chk(F.lower_chain(5, 5, gx.ptr, gx.ptr)); dev.chk(F.upper_chain(5, 5, gx.ptr))
    dev.chk(dev.k.mi355x_bilu_lower_chain(dev.h, -2, None, None, bs, None, None, None, None, None))
    dev.chk(dev.k.mi355x_bilu_upper_chain(dev.h, 0, None, None, bs, None, None, None, None))
    dev.sync()
    assert (bits(gx.get("nlev = 0")) == bits(np.array([MARK]))[0]).all()
    gx.free()
    F.unchanged("nlev = 0")
    # an empty level in the middle (and one at either end): the same rows, one barrier more each
    empty = np.zeros(0, np.int32)
    F.set_levels([empty] + F.L[:35] + [empty] + F.L[35:] + [empty], F.U[:20] + [empty, empty] + F.U[20:])
    assert np.array_equal(bits(F.run(b, what="empty levels")), bits(ref))


def test_one_level_alone_in_a_chain(dev):
    """nlev = 1 over 300 uncoupled block rows: the chain is the level kernel's 300 rows in two passes"""
    bs = 4
    check_chain(dev, bs, br.independent_blocks(300, bs), 75, sizes=[300], what="one level")


def test_b_may_alias_x_in_the_lower_chain(dev):
    bs = 4
    lay, f = factor_of(bs, pb.elasticity_like(3, 3, 2, dof=bs)[1])
    F = ChainFactor(dev, bs, lay, f)
    b = rnd(18 * bs, 71)
    x = F.run(b, alias=True, what="aliased")
    assert np.array_equal(bits(x), bits(F.run(b, what="separate"))) and np.array_equal(bits(x), bits(br.apply(bs, lay, f, b)))
    nb, pairs = crossing(6, 40, 17)
    bcsr = coupled_blocks(nb, 3, pairs)
    lay, f = factor_of(3, bcsr)
    F = ChainFactor(dev, 3, lay, f)
    b = rnd(nb * 3, 72)
    assert np.array_equal(bits(F.run(b, alias=True, what="aliased, crossing")), bits(br.apply(3, lay, f, b)))


def lower_ref(bs, lay, f, b):
    """L^-1 b alone, level by level"""
    ba, bl, x = np.asarray(f, dtype=np.float64).tolist(), np.asarray(b, dtype=np.float64).tolist(), [0.0] * b.size
    for rows in br.level_rows(lay)[0]:
        br.lower_rows(bs, lay, ba, bl, x, rows)
    return np.array(x)


def two_chains(bs):
    """two uncoupled block-tridiagonal chains of four block rows each"""
    bi, bj, ba = br.block_tridiag(8, bs)
    keep = np.array([not ((i, int(j)) in ((3, 4), (4, 3))) for i in range(8) for j in bj[bi[i]:bi[i + 1]]])
    bi2 = _i32(np.concatenate(([0], np.cumsum([int(keep[bi[i]:bi[i + 1]].sum()) for i in range(8)]))))
    return bi2, bj[keep], ba.reshape(-1, bs * bs)[keep].ravel()


def test_nan_inf_and_minus_zero_stay_where_the_reference_puts_them(dev):
    """A NaN, an Inf or -0.0 in block row 1 of the right-hand side: where the reference has a NaN the device has one (payloads are not
    compared), every other value carries the reference's bits -- the sign of a zero included -- and the rows of the second, uncoupled
    chain carry the bits of the solve without specials."""
    bs = 3
    lay, f = factor_of(bs, two_chains(bs))
    F = ChainFactor(dev, bs, lay, f)
    assert [r.size for r in F.L] == [2] * 4
    b = rnd(8 * bs, 80)
    clean = F.run(b, what="clean")
    assert np.array_equal(bits(clean), bits(br.apply(bs, lay, f, b)))
    for name, special in (("nan", np.nan), ("inf", np.inf), ("-inf and nan", None), ("-0.0", -0.0)):
        bsp = b.copy()
        if special is None:
            bsp[bs * 1 + 0] = -np.inf; bsp[bs * 2 + 1] = np.nan
        elif name == "-0.0":
            bsp[:4 * bs] = -0.0                                     # the whole first chain: x = -0.0 or +0.0 as the reference's sums say
        else:
            bsp[bs * 1 + 1] = special
        ref = br.apply(bs, lay, f, bsp)
        x = F.run(bsp, what=name)
        if name == "-0.0":
            assert (ref[:4 * bs] == 0.0).all() and np.signbit(ref[:4 * bs]).any()
        else:
            assert not np.isfinite(ref[:4 * bs]).all()
        assert np.isfinite(ref[4 * bs:]).all()
        assert np.array_equal(np.isnan(x), np.isnan(ref)), name
        ok = ~np.isnan(ref)
        assert np.array_equal(bits(x[ok]), bits(ref[ok])), name
        assert np.array_equal(bits(x[4 * bs:]), bits(clean[4 * bs:])), name
        assert np.array_equal(np.isnan(F.solve(bsp, what=name + ", level by level")), np.isnan(x))
        # the lower chain alone, before the upper solve mixes an Inf into NaNs
        low, xl = lower_ref(bs, lay, f, bsp), F.run(bsp, planU=[], what=name + ", lower")
        assert np.array_equal(np.isnan(xl), np.isnan(low)), name
        assert np.array_equal(bits(xl[~np.isnan(low)]), bits(low[~np.isnan(low)])), name
        if name == "inf":
            assert np.isinf(low[:4 * bs]).any()


@pytest.mark.parametrize("bs", [1, 8])
def test_a_block_size_outside_2_to_7_is_refused_with_nothing_written(dev, bs):
    lay, f = factor_of(3, br.block_tridiag(4, 3))
    F = ChainFactor(dev, 3, lay, f)
    gx = Guarded(dev, 12 * 8)
    assert F.lower_chain(0, len(F.L), gx.ptr, gx.ptr, bs=bs) == INVALID
    assert F.upper_chain(0, len(F.U), gx.ptr, bs=bs) == INVALID
    dev.sync()
    assert (bits(gx.get("bad bs")) == bits(np.array([MARK]))[0]).all()
    gx.free()
    F.unchanged("bad bs")


# ---------------------------------------------------------------- 2. the plug-in
def solve_plan(P, pc):
    v = [C.c_int(-1) for _ in range(3)]
    assert P.lib().raw("PCBILUGetSolvePlan_HIPMI355X")(pc, *[C.byref(a) for a in v]) == 0
    return tuple(a.value for a in v)


def ref_plan(lay, max_rows):
    """(1, segments of L, segments of U) of the planner's rule on the factor's levels"""
    L, U = br.level_rows(lay)
    return 1, len(plan_ref([r.size for r in L], max_rows)), len(plan_ref([r.size for r in U], max_rows))


DEFAULT_ROWS = 128         # of -pc_factor_hipmi355x_bilu_chain_rows


@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("bs", [3, 4])
def test_trisolve_fused_gives_the_level_route_and_the_reference_bits(P, bs, levels):
    """the plug-in test that fails without the feature: -pc_factor_hipmi355x_trisolve fused was PETSC_ERR_SUP"""
    L = P.lib()
    bi, bj, ba = dominant(bs)
    A = P.Mat.from_bsr(bs, bi, bj, ba)
    lay, f = factor_of(bs, (bi, bj, ba), levels)
    nL, nU = ref_info(bs, lay)[1:3]
    b = rnd(18 * bs, 90 + bs)
    ref = br.apply(bs, lay, f, b)
    fill = "-pc_factor_levels %d" % levels
    # without the option: level by level, one launch per level
    ksp0, pc0, rc = bilu_pc(P, A, fill)
    assert rc == 0 and solve_plan(P, pc0) == (0, nL, nU)
    x_level = apply(P, pc0, b)
    assert np.array_equal(bits(x_level), bits(ref))
    ksp1, pc1, rc = bilu_pc(P, A, fill + " -pc_factor_hipmi355x_trisolve level")
    assert rc == 0 and solve_plan(P, pc1) == (0, nL, nU)
    # fused at the default bound: every level of this factor is narrow, 1 + 1 launches
    ksp, pc, rc = bilu_pc(P, A, fill + " -pc_factor_hipmi355x_trisolve fused")
    assert rc == 0
    assert solve_plan(P, pc) == ref_plan(lay, DEFAULT_ROWS) == (1, 1, 1)
    vb, vx = V(P, b), V(P, np.zeros(b.size))
    ksp.solve(vb, vx)
    assert ksp.reason > 0
    assert np.array_equal(bits(vx.array()), bits(ref)) and np.array_equal(bits(apply(P, pc, b)), bits(x_level))
    assert bilu_info(P, pc) == ref_info(bs, lay) and numeric_info(P, pc) == (0, 1, 1)
    # bounds small enough for a mixed plan, and a large one: the same bits, the planner's counts
    for rows in (1, 2, 1 << 30):
        opts = fill + " -pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows %d" % rows
        assert setup_again(P, ksp, pc, A, opts) == 0
        plan = solve_plan(P, pc)
        assert plan == ref_plan(lay, rows), rows
        if rows == 1 << 30:
            assert plan == (1, 1, 1)
        elif levels == 0:
            assert 1 < plan[1] < nL and 1 < plan[2] < nU                   # chained runs and levels of their own
        assert np.array_equal(bits(apply(P, pc, b)), bits(ref)), rows
    assert numeric_info(P, pc) == (0, 1, 1)                                # the same operator and values: nothing was factored again
    # chain_rows 0: fused, and no level narrow
    assert setup_again(P, ksp, pc, A, fill + " -pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows 0") == 0
    assert solve_plan(P, pc) == (1, nL, nU) and np.array_equal(bits(apply(P, pc, b)), bits(ref))
    # new values on the same pattern: the numeric pass and the upload only, the plan kept
    L.MatScale(A.h, 1.75)
    opts = fill + " -pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows 2"
    assert setup_again(P, ksp, pc, A, opts) == 0
    assert numeric_info(P, pc) == (0, 1, 2) and bilu_info(P, pc) == ref_info(bs, lay) and solve_plan(P, pc) == ref_plan(lay, 2)
    f2, z = br.numeric(bs, bi, bj, 1.75 * ba, lay)
    assert z == -1 and np.array_equal(bits(apply(P, pc, b)), bits(br.apply(bs, lay, f2, b)))
    # the option gone: level by level again, on the same factor
    assert setup_again(P, ksp, pc, A, fill) == 0
    assert solve_plan(P, pc) == (0, nL, nU) and numeric_info(P, pc) == (0, 1, 2)
    assert np.array_equal(bits(apply(P, pc, b)), bits(br.apply(bs, lay, f2, b)))


def test_unknown_routes_stay_err_sup_and_name_both_routes(P):
    bs = 3
    A = P.Mat.from_bsr(bs, *dominant(bs))
    for value in ("syncfree", "sweeps:2", "chain"):
        ksp, pc, rc = bilu_pc(P, A, "-pc_factor_hipmi355x_trisolve " + value)
        assert rc == ERR_SUP
        msg = P.lib()._h.PetscGetLastErrorMessage().decode(errors="replace")
        assert "level" in msg and "fused" in msg
    ksp, pc, rc = bilu_pc(P, A, "-pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows -3")
    assert rc != 0
    assert setup_again(P, ksp, pc, A, "-pc_factor_hipmi355x_trisolve fused") == 0 and solve_plan(P, pc) == (1, 1, 1)


def test_the_point_type_refuses_fused_as_any_unknown_value(P):
    """AIJ operators are untouched: their parser knows syncfree, level and sweeps:<k>"""
    ai, aj, aa = P.gen_poisson7(4, 3, 3)
    A = P.Mat.from_csr(ai, aj, aa)
    rcs = [bilu_pc(P, A, "-pc_factor_hipmi355x_trisolve " + v)[2] for v in ("fused", "no_such_route", "level")]
    assert rcs[0] == rcs[1] != 0 and rcs[2] == 0


def test_right_preconditioned_gmres_takes_the_level_route_s_iterations(P):
    bs = 3
    bcsr = pb.spd_blocks(4, 4, 3)[1]
    for levels in (0, 1):
        opts = "-pc_type ilu -pc_factor_levels %d" % levels
        level = gmres_right(P, bcsr, bs, opts)
        fused = gmres_right(P, bcsr, bs, opts + " -pc_factor_hipmi355x_trisolve fused")
        mixed = gmres_right(P, bcsr, bs, opts + " -pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows 2")
        assert level[1] > 0 and level[0] > 0
        assert fused == level and mixed == level          # iterations, reason and both residual norms: the same bits went in
