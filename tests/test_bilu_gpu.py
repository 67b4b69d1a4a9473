"""Block ILU(k) on the device: the level-scheduled block triangular solves of csrc/bilu.hip through the C ABI against bilu_ref bit
for bit, and the plug-in's route from -pc_type ilu on a MATSEQBAIJHIPMI355X operator down to them (host/bilu.c).

x and ba live between guard bands of a marker; every comparison of a solution is on bit patterns.  The reference is checked on its own,
without a GPU, by test_bilu_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import bilu_ref as br
import problems as pb
from ilufactor import MARK, bits
from test_bilu_cpu import zero_pivot_case
from test_ilu_device_factor_gpu import numeric_info, setup_again
from test_ilu_factor_specials_gpu import Guarded
from test_ilu_sweeps_gpu import V, apply
from test_kernels_gpu import dev, rnd  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu
INVALID, ERR_SUP, ERR_ZRPVT, ERR_WRONGSTATE = 1, 56, 71, 73
BLOCK_SIZES = [2, 3, 4, 5, 7]


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


# ---------------------------------------------------------------- 1. the kernels through the C ABI
class BlockFactor:
    """a factor on the device: the layout, ba between guard bands, and the block rows of every level of L and U"""

    def __init__(self, dev, bs, layout, ba):
        self.dev, self.bs, self.lay = dev, bs, [_i32(a) for a in layout[:3]]
        self.ba = np.ascontiguousarray(ba, dtype=np.float64)
        self.d = [dev.put(a) for a in self.lay]
        self.gba = Guarded(dev, self.ba.size)
        self.gba.put(self.ba)
        self.L, self.U = br.level_rows(self.lay)
        self.dL, self.dU = [dev.put(r) for r in self.L], [dev.put(r) for r in self.U]

    def lower(self, l, db, dx):
        return self.dev.k.mi355x_bilu_lower_level(self.dev.h, self.L[l].size, self.dL[l], self.bs, self.d[0], self.d[1], self.gba.ptr, db, dx)

    def upper(self, l, dx):
        return self.dev.k.mi355x_bilu_upper_level(self.dev.h, self.U[l].size, self.dU[l], self.bs, self.d[1], self.gba.ptr, self.d[2], dx)

    def solve(self, b, alias=False, what=""):
        """lower then upper over all levels; x between guard bands, pre-filled with the marker (b itself when it aliases x)"""
        gx = Guarded(self.dev, b.size)
        if alias:
            gx.put(b)
        db = gx.ptr if alias else self.dev.put(b)
        for l in range(len(self.L)):
            self.dev.chk(self.lower(l, db, gx.ptr))
        for l in range(len(self.U)):
            self.dev.chk(self.upper(l, gx.ptr))
        x = gx.get(what + ": x")
        self.unchanged(what)
        if not alias:
            assert np.array_equal(bits(self.dev.get(db, b.size)), bits(b)), what + ": b was written"
        gx.free()
        return x

    def unchanged(self, what):
        assert np.array_equal(bits(self.gba.get(what + ": ba")), bits(self.ba)), what + ": ba was written"
        for p, a in zip(self.d, self.lay):
            assert np.array_equal(self.dev.get(p, a.size, np.int32), a), what + ": an index array was written"


def factor_of(bs, bcsr, levels=0):
    bi, bj, ba = bcsr
    lay = br.symbolic(bi, bj, levels)
    f, z = br.numeric(bs, bi, bj, ba, lay)
    assert z == -1
    return lay, f


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_lower_then_upper_over_all_levels_equals_the_reference(dev, bs):
    lay, f = factor_of(bs, pb.elasticity_like(3, 3, 2, dof=bs)[1])
    b = rnd(18 * bs, 40 + bs)
    F = BlockFactor(dev, bs, lay, f)
    assert len(F.L) > 1 and len(F.U) > 1
    x = F.solve(b, what="bs %d" % bs)
    assert np.array_equal(bits(x), bits(br.apply(bs, lay, f, b)))


@pytest.mark.parametrize("bs", [3, 5])
def test_one_level_of_more_rows_than_a_workgroup_covers(dev, bs):
    """300 uncoupled block rows: one level of 300 groups of 4 (bs = 3) or 8 (bs = 5) lanes, 5 or 10 workgroups, the last one partly idle"""
    bcsr = br.independent_blocks(300, bs)
    lay, f = factor_of(bs, bcsr)
    F = BlockFactor(dev, bs, lay, f)
    assert [r.size for r in F.L] == [300] and [r.size for r in F.U] == [300]
    b = rnd(300 * bs, 50 + bs)
    assert np.array_equal(bits(F.solve(b, what="300 rows, bs %d" % bs)), bits(br.apply(bs, lay, f, b)))


def test_levels_of_one_block_row(dev):
    """the block-tridiagonal chain of 70 block rows: 70 + 70 launches of one group each"""
    bs = 3
    lay, f = factor_of(bs, br.block_tridiag(70, bs))
    F = BlockFactor(dev, bs, lay, f)
    assert [r.size for r in F.L] == [1] * 70 and [r.size for r in F.U] == [1] * 70
    b = rnd(70 * bs, 60)
    assert np.array_equal(bits(F.solve(b, what="chain")), bits(br.apply(bs, lay, f, b)))


def test_an_empty_level_launches_nothing_and_b_may_alias_x(dev):
    bs = 4
    lay, f = factor_of(bs, pb.elasticity_like(3, 3, 2, dof=bs)[1])
    F = BlockFactor(dev, bs, lay, f)
    b = rnd(18 * bs, 70)
    gx = Guarded(dev, b.size)
    dev.chk(dev.k.mi355x_bilu_lower_level(dev.h, 0, F.dL[0], bs, F.d[0], F.d[1], F.gba.ptr, gx.ptr, gx.ptr))
    dev.chk(dev.k.mi355x_bilu_upper_level(dev.h, 0, F.dU[0], bs, F.d[1], F.gba.ptr, F.d[2], gx.ptr))
    dev.chk(dev.k.mi355x_bilu_lower_level(dev.h, -3, None, bs, None, None, None, None, None))
    dev.sync()
    assert (bits(gx.get("nrows = 0")) == bits(np.array([MARK]))[0]).all()
    F.unchanged("nrows = 0")
    assert np.array_equal(bits(F.solve(b, alias=True, what="aliased")), bits(F.solve(b, what="separate")))


def test_nan_and_inf_in_one_block_stay_where_the_reference_puts_them(dev):
    """two uncoupled chains of four block rows; a NaN and an Inf in block row 1 of the right-hand side.  Where the reference has a NaN the
    device has one (payloads differ between processors and are not compared), every other value carries the reference's bits, and the
    second chain's rows carry the bits of the solve without specials."""
    bs = 3
    bi, bj, ba = br.block_tridiag(8, bs)
    keep = np.array([not ((i, int(j)) in ((3, 4), (4, 3))) for i in range(8) for j in bj[bi[i]:bi[i + 1]]])
    bj2 = bj[keep]; ba2 = ba.reshape(-1, bs * bs)[keep].ravel()
    bi2 = _i32(np.concatenate(([0], np.cumsum([int(keep[bi[i]:bi[i + 1]].sum()) for i in range(8)]))))
    lay, f = factor_of(bs, (bi2, bj2, ba2))
    F = BlockFactor(dev, bs, lay, f)
    b = rnd(8 * bs, 80)
    clean = F.solve(b, what="clean")
    assert np.array_equal(bits(clean), bits(br.apply(bs, lay, f, b)))
    bsp = b.copy(); bsp[bs * 1 + 0] = np.nan; bsp[bs * 1 + 2] = np.inf
    ref = br.apply(bs, lay, f, bsp)
    x = F.solve(bsp, what="specials")
    assert np.isnan(ref[:4 * bs]).any() and np.isfinite(ref[4 * bs:]).all()
    assert np.array_equal(np.isnan(x), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(x[ok]), bits(ref[ok]))
    assert np.array_equal(bits(x[4 * bs:]), bits(clean[4 * bs:]))


@pytest.mark.parametrize("bs", [1, 8])
def test_a_block_size_outside_2_to_7_is_refused_with_nothing_written(dev, bs):
    lay, f = factor_of(3, br.block_tridiag(4, 3))
    F = BlockFactor(dev, 3, lay, f)
    gx = Guarded(dev, 12 * 8)
    assert dev.k.mi355x_bilu_lower_level(dev.h, F.L[0].size, F.dL[0], bs, F.d[0], F.d[1], F.gba.ptr, gx.ptr, gx.ptr) == INVALID
    assert dev.k.mi355x_bilu_upper_level(dev.h, F.U[0].size, F.dU[0], bs, F.d[1], F.gba.ptr, F.d[2], gx.ptr) == INVALID
    dev.sync()
    assert (bits(gx.get("bad bs")) == bits(np.array([MARK]))[0]).all()
    F.unchanged("bad bs")


# ---------------------------------------------------------------- 2. the plug-in
def bilu_pc(P, A, opts, pctype="ilu"):
    """a KSP over A whose PC is configured from the options and set up: (ksp, pc, PCSetUp's code)"""
    L = P.lib()
    pc = C.c_void_p()
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc))
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type preonly -pc_type %s %s" % (pctype, opts)).encode())
    rc = L.raw("KSPSetFromOptions")(k.h)
    rc = rc or L.raw("PCSetUp")(pc)
    L.PetscOptionsClear()
    return k, pc, rc


def bilu_info(P, pc):
    v = [C.c_int(-1) for _ in range(4)]
    P.lib().PCBILUGetInfo_HIPMI355X(pc, *[C.byref(a) for a in v])
    return tuple(a.value for a in v)


def ref_info(bs, lay):
    L, U = br.level_rows(lay)
    return bs, len(L), len(U), int(lay[2][0]) + 1


def dominant(bs):
    """elasticity_like(3, 3, 2) with 30 I added to every diagonal block (a preconditioner's operator rather than pure noise)"""
    bi, bj, ba = pb.elasticity_like(3, 3, 2, dof=bs)[1]
    ba = ba.copy().reshape(-1, bs * bs)
    for i in range(bi.size - 1):
        ba[int(bi[i]) + list(bj[bi[i]:bi[i + 1]]).index(i)] += (30.0 * np.eye(bs)).ravel()
    return bi, bj, ba.ravel()


@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("bs", [3, 4])
def test_pc_type_ilu_on_a_baij_operator_gives_the_reference_bits(P, bs, levels):
    """the test that fails without the feature: the set-up ended in "Matrix format seqbaijhipmi355x does not have a solver package petsc"."""
    L = P.lib()
    bi, bj, ba = dominant(bs)
    A = P.Mat.from_bsr(bs, bi, bj, ba)
    lay, f = factor_of(bs, (bi, bj, ba), levels)
    b = rnd(18 * bs, 90 + bs)
    ksp, pc, rc = bilu_pc(P, A, "-pc_factor_levels %d" % levels)
    assert rc == 0
    vb, vx = V(P, b), V(P, np.zeros(b.size))
    ksp.solve(vb, vx)
    assert ksp.reason > 0
    assert np.array_equal(bits(vx.array()), bits(br.apply(bs, lay, f, b)))
    assert bilu_info(P, pc) == ref_info(bs, lay)
    assert numeric_info(P, pc) == (0, 1, 1)
    # new values on the same pattern: the numeric pass and the upload only
    L.MatScale(A.h, 1.75)
    assert setup_again(P, ksp, pc, A, "-pc_factor_levels %d" % levels) == 0
    assert numeric_info(P, pc) == (0, 1, 2) and bilu_info(P, pc) == ref_info(bs, lay)
    f2, z = br.numeric(bs, bi, bj, 1.75 * ba, lay)
    assert z == -1 and np.array_equal(bits(apply(P, pc, b)), bits(br.apply(bs, lay, f2, b)))
    # nothing changed: nothing redone
    assert setup_again(P, ksp, pc, A, "") == 0 and numeric_info(P, pc) == (0, 1, 2)
    if levels == 0:                                              # another level of fill on the same objects: a new pattern pass
        L.PCFactorSetLevels(pc, 1)
        assert setup_again(P, ksp, pc, A, "") == 0 and numeric_info(P, pc) == (0, 2, 3)
        lay1 = br.symbolic(bi, bj, 1)
        assert bilu_info(P, pc) == ref_info(bs, lay1)
        assert np.array_equal(bits(apply(P, pc, b)), bits(br.apply(bs, lay1, br.numeric(bs, bi, bj, 1.75 * ba, lay1)[0], b)))


GMRES_C = 2.0    # twice the measured gap of 1.0000, see the docstring below


def gmres_right(P, bcsr, bs, pc_opts, rtol=1e-8):
    """-ksp_type gmres -ksp_pc_side right <pc_opts> -ksp_rtol rtol on the BAIJ form: (iterations, reason, recurrence residual, x, b)"""
    L = P.lib()
    bi, bj, ba = bcsr
    A = P.Mat.from_bsr(bs, bi, bj, ba)
    n = (bi.size - 1) * bs
    Ad = br.dense_of(bs, bi, bj, ba)
    b = Ad @ (np.sin(0.37 * np.arange(n)) + 1.5)
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type gmres -ksp_pc_side right %s -ksp_rtol %g" % (pc_opts, rtol)).encode())
    k.set_from_options()
    vb, vx = V(P, b), V(P, np.zeros(n))
    k.solve(vb, vx)
    L.PetscOptionsClear()
    x = vx.array()
    return k.its, k.reason, k.rnorm, float(np.linalg.norm(b - Ad @ x)), float(np.linalg.norm(b))


def test_right_preconditioned_gmres_converges_in_the_true_residual(P):
    """-ksp_type gmres -ksp_pc_side right -pc_type ilu -ksp_rtol 1e-8 on spd_blocks(4, 4, 3) stored as BAIJ.  With right preconditioning
    the tested norm is the true residual's, so ||b - A x||2 <= c rtol ||b||2 with c = twice the gap between the recurrence's residual
    norm and the true one that the same solve shows with -pc_type pbjacobi.  Measured on an MI355X: pbjacobi 8 iterations,
    recurrence 1.055741e-04 against true 1.055741e-04, a gap of 1.0000, so c = 2.0 (block ILU(0): 3 iterations, ILU(1): 2, both with a
    gap of 1.0000; ||b||2 = 3.255447e+04)."""
    bs = 3
    bcsr = pb.spd_blocks(4, 4, 3)[1]
    its, reason, rnorm, true, bnorm = gmres_right(P, bcsr, bs, "-pc_type pbjacobi")
    print("pbjacobi: %d iterations, recurrence residual %.6e, true residual %.6e, gap %.4f, ||b|| %.6e" % (its, rnorm, true, true / rnorm, bnorm))
    assert reason > 0
    runs = [gmres_right(P, bcsr, bs, "-pc_type ilu -pc_factor_levels %d" % levels) for levels in (0, 1)]
    for levels, (its, reason, rnorm, true, bnorm) in enumerate(runs):
        print("block ILU(%d): %d iterations, recurrence residual %.6e, true residual %.6e, gap %.4f" % (levels, its, rnorm, true, true / rnorm))
    for its, reason, rnorm, true, bnorm in runs:
        assert reason > 0
        assert true <= GMRES_C * 1e-8 * bnorm


@pytest.mark.parametrize("opts,pctype", [("", "icc"), ("-pc_factor_shift_type nonzero", "ilu"), ("-pc_factor_hipmi355x_numeric device", "ilu"),
                                         ("-pc_factor_hipmi355x_trisolve syncfree", "ilu")])
def test_what_the_block_route_does_not_offer_is_err_sup(P, opts, pctype):
    bs = 3
    A = P.Mat.from_bsr(bs, *dominant(bs))
    ksp, pc, rc = bilu_pc(P, A, opts, pctype=pctype)
    assert rc == ERR_SUP
    # the same PC sets up once the option is gone (nothing was left half done); ICC stays refused
    if pctype == "ilu":
        assert setup_again(P, ksp, pc, A, "") == 0 and numeric_info(P, pc) == (0, 1, 1)


def test_zero_pivot_and_missing_diagonal_block(P):
    bs = 3
    bi, bj, ba, row = zero_pivot_case(bs)
    ksp, pc, rc = bilu_pc(P, P.Mat.from_bsr(bs, bi, bj, ba), "")
    assert rc == ERR_ZRPVT
    assert ("row %d" % row) in P.lib()._h.PetscGetLastErrorMessage().decode(errors="replace")
    tbi, tbj, tba = br.block_tridiag(4, bs)
    keep = np.array([not (i == 2 and int(j) == 2) for i in range(4) for j in tbj[tbi[i]:tbi[i + 1]]])
    bi2 = _i32(np.concatenate(([0], np.cumsum([int(keep[tbi[i]:tbi[i + 1]].sum()) for i in range(4)]))))
    ksp, pc, rc = bilu_pc(P, P.Mat.from_bsr(bs, bi2, tbj[keep], tba.reshape(-1, bs * bs)[keep].ravel()), "")
    assert rc == ERR_WRONGSTATE
