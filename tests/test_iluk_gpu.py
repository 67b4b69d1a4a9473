"""ILU(k) on the device: the numeric factorisation on a pattern with fill (csrc/ilu_factor.hip, mi355x_ilu0_factor_create_fill) against
iluk_ref.reference_pass bit for bit, and the plug-in's route from -pc_factor_levels / PCFactorSetLevels down to it (host/ilu.c).

The factor carries the sequential loop's BITS on its level-of-fill pattern, so every comparison of a factor or of an application is on
bit patterns; ba lives between guard bands of a marker and is pre-filled with it.  The reference and the shapes are checked on their
own, without a GPU, by test_iluk_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import ilufactor as ilf
import iluk_ref as ik
import orc
import problems as pb
from ilufactor import MARK, ZP, bits
from test_ilu_device_factor_gpu import numeric_info, setup_again
from test_ilu_factor_specials_gpu import Guarded, _by_rule, _i32, _same_bits, _untouched
from test_ilu_sweeps_gpu import V, apply, perturbed
from test_kernels_gpu import dev, rnd  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu
INVALID, ERR_SUP = 1, 56
DEVICE, HOST = "-pc_factor_hipmi355x_numeric device", "-pc_factor_hipmi355x_numeric host"


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


# ---------------------------------------------------------------- 1. the kernel through the C ABI
def _create_fill(dev, ai, aj, layout, blk=None):
    n = ai.size - 1
    _, nlev, levptr, rows = ik.levels_L(layout)
    keep = [_i32(a) for a in (ai, aj, layout[0], layout[1], layout[2], levptr, rows)] + [None if blk is None else _i32(blk)]
    ctx = C.c_void_p()
    rc = dev.k.mi355x_ilu0_factor_create_fill(dev.h, n, *[a.ctypes.data for a in keep[:5]], nlev, keep[5].ctypes.data, keep[6].ctypes.data,
                                              1 if blk is None else len(blk) - 1, None if blk is None else keep[7].ctypes.data, C.byref(ctx))
    return rc, ctx, nlev


class FillFactor:
    """the context of A's pattern and a factor layout that contains it, A on the device, ba (bdiag[0] + 2 doubles) between guard bands
    and pre-filled with the marker"""

    def __init__(self, dev, ai, aj, aa, layout, blk=None):
        self.dev, self.ai, self.aj, self.aa = dev, _i32(ai), _i32(aj), np.ascontiguousarray(aa, dtype=np.float64)
        self.n, self.nza = self.ai.size - 1, int(self.ai[-1])
        self.nz = int(layout[2][0]) + 1 if self.n else 0
        self.nblk = 1 if blk is None else len(blk) - 1
        rc, self.ctx, nlev = _create_fill(dev, self.ai, self.aj, layout, blk)
        dev.chk(rc)
        self.dai, self.daj, self.daa = dev.put(self.ai), dev.put(np.concatenate((self.aj, [0])).astype(np.int32)), dev.put(np.concatenate((self.aa, [0.0])))
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
        assert np.array_equal(self.dev.get(self.dai, self.n + 1, np.int32), self.ai) and np.array_equal(self.dev.get(self.daj, self.nza, np.int32), self.aj), what
        assert np.array_equal(bits(self.dev.get(self.daa, self.nza)), bits(self.aa)), "%s: A's values were modified" % what
        return ba


def _every(ba):
    every = np.ones(ba.size, dtype=bool); every[-1] = False
    return every


def _clean(dev, name, levels):
    """the shape factored once on the device: the reference's bits, nothing else written; returns the lanes per row"""
    ai, aj, aa = ik.shape(name)
    lay = ik.layout_of(name, levels)
    ref, rfrow = ik.clean_factor(name, levels)
    what = "%s, %d levels" % (name, levels)
    with FillFactor(dev, ai, aj, aa, lay) as F:
        assert F.lanes == ik.lanes_of(lay), what
        frow, fabs_ = F.run()
        assert frow[0] == rfrow[0] == -1 and fabs_[0] == 0.0, what
        ba = F.values(what)
        _same_bits(ba, ref, _every(ba), what)
        # nothing pending: a second pass reports success and touches nothing
        F.ba.put(np.full(ba.size, MARK))
        assert F.run()[0][0] == -1
        _untouched(F.values(what + ", second pass"), np.ones(ba.size, dtype=bool), what + ", second pass")
        print("%s: n = %d, widest row of A %d, of the factor %d, %d lanes" % (what, ai.size - 1, int(np.diff(ai).max()), ik.widest(lay), F.lanes))
        return F.lanes


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", ["lap2d", "p7"])
def test_register_rows_wider_than_as_rows(dev, name, levels):
    """A's rows need 8 lanes, the factor's 16 or 32"""
    ai, _, _ = ik.shape(name)
    assert ilf.lanes_of(ai) == 8
    lanes = _clean(dev, name, levels)
    assert lanes in (8, 16, 32) and lanes == ik.lanes_of(ik.layout_of(name, levels))
    if name == "p7":
        assert lanes == (16 if levels == 1 else 32)


@pytest.mark.parametrize("name", ["fill_wide", "a_wide", "uchunk_fill", "ex10", "random"])
def test_factor_rows_wider_than_a_wavefront_and_chunk_edges(dev, name):
    """fill_wide: A's rows all fit a wavefront, fill makes factor rows wider than 64 (in L and in U).  a_wide: A's rows are wider than
    64 already.  uchunk_fill: U(k) of exactly 64, 65 and 128 entries after fill.  ex10, random: the patterns of the symbolic tests."""
    ai, _, _ = ik.shape(name)
    lanes = _clean(dev, name, 1)
    if name == "fill_wide":
        assert np.diff(ai).max() <= ik.WAVE and ik.widest(ik.layout_of(name, 1)) > ik.WAVE and lanes == 64
    if name == "a_wide":
        assert np.diff(ai).max() > ik.WAVE and lanes == 64
    if name == "uchunk_fill":
        lay = ik.layout_of(name, 1)
        assert [int(lay[2][k] - lay[2][k + 1] - 1) for k in (3, 4, 5)] == [64, 65, 128]
        _clean(dev, name, 2)


def test_zero_fill_layout_through_the_fill_kernel_is_ilu0(dev):
    """levels = 0: the factor's pattern is A's; the fill kernel gives the bits of the ILU(0) kernel's reference"""
    for name in ("p7", "a_wide"):
        ai, aj, aa = ik.shape(name)
        _clean(dev, name, 0)
        assert np.array_equal(bits(ik.clean_factor(name, 0)[0][:-1]), bits(orc.ilu0_factor(ai, aj, aa)[3][:-1]))


def test_a_fill_entry_that_stays_zero_is_skipped_and_one_that_does_not_is_a_multiplier(dev):
    ai, aj, aa = ik.skipped_fill_case()
    lay = ik.symbolic(ai, aj, 1)
    ref = ik.reference_pass(ai, aj, aa, None, [0.0], ZP, [1], layout=lay)[0]
    with FillFactor(dev, ai, aj, aa, lay) as F:
        assert F.lanes == 8
        assert F.run()[0][0] == -1
        ba = F.values("skipped fill")
        _same_bits(ba, ref, _every(ba), "skipped fill")
        rows = ik.factor_rows(lay)
        for i, c in ((2, 1), (3, 1)):                          # the untouched fill entries: +0.0, not the -0.0 of 0.0 * (1 / -4)
            q = rows[i][1][list(rows[i][0]).index(c)]
            assert bits(ba[q:q + 1])[0] == 0


def test_blocks_over_three_passes_on_a_fill_pattern(dev):
    """iluk_ref.blocks_case: blocks that pass at once, after one shift, after two.  After pass 1 the finished blocks' slots are
    overwritten with the marker on the device and stay that way; the fill slots of a block that runs again carry the reference's
    bits of THAT pass, not what the pass before left there.  Every pass: failed_row, failed_abs and ba as the reference."""
    c = ik.blocks_case()
    ai, aj, blk, lay = c["ai"], c["aj"], c["blk"], c["layout"]
    with FillFactor(dev, ai, aj, c["aa"], lay, blk=blk) as F:
        for ps, (shifts, ref, rfrow, rfabs, _) in enumerate(c["passes"]):
            what = "40 blocks with fill, pass %d" % (ps + 1)
            frow, fabs_ = F.run(shifts)
            assert np.array_equal(frow, rfrow), what
            assert np.array_equal(bits(fabs_), bits(rfabs)), what
            ba = F.values(what)
            if ps == 0:
                ba[c["finished1"]] = MARK
                F.ba.put(ba)
            _untouched(ba, c["finished1"], what)
            _same_bits(ba, ref, ik.compared_slots(lay, blk, rfrow) & ~c["finished1"], what)
        assert (frow == -1).all()


@pytest.mark.parametrize("special", [np.nan, np.inf, -np.inf])
def test_a_special_in_one_entry_of_a_follows_the_rule(dev, special):
    """zeropivot = 0: no pivot fails; the factor is compared under ilufactor.rule_violations"""
    ai, aj, aa = ik.shape("p7")
    lay = ik.layout_of("p7", 1)
    r = 47
    q = int(ai[r + 1]) - 1                                     # its last entry: strict upper
    assert aj[q] > r
    aap = aa.copy(); aap[q] = special
    ref, rfrow, _, _ = ik.reference_pass(ai, aj, aap, None, [0.0], 0.0, [1], layout=lay)
    assert rfrow[0] == -1 and not np.isfinite(ref[:-1]).all()
    with FillFactor(dev, ai, aj, aap, lay) as F:
        frow, _ = F.run(zeropivot=0.0)
        assert frow[0] == -1
        ba = F.values("special %r" % special)
        _by_rule(ba, ref, _every(ba), "special %r" % special)


def test_no_row_and_one_row(dev):
    lay = ik.symbolic(np.array([0, 1], np.int32), np.zeros(1, np.int32), 2)
    with FillFactor(dev, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([-4.0]), lay) as F:
        assert F.lanes == 1 and F.run()[0][0] == -1
        assert np.array_equal(bits(F.values("n = 1")[:1]), bits(np.array([-0.25])))
    ctx, frow = C.c_void_p(), np.full(1, -7, np.int32)
    zero, shift = np.zeros(1, np.int32), np.zeros(1)
    dev.chk(dev.k.mi355x_ilu0_factor_create_fill(dev.h, 0, zero.ctypes.data, None, None, None, None, 0, None, None, 1, None, C.byref(ctx)))
    dev.chk(dev.k.mi355x_ilu0_factor_reset(ctx))
    dev.chk(dev.k.mi355x_ilu0_factor_run(dev.h, ctx, None, None, None, ZP, shift.ctypes.data, None, frow.ctypes.data, None))
    assert frow[0] == -1
    dev.chk(dev.k.mi355x_ilu0_factor_destroy(ctx))


def test_create_fill_refuses_a_factor_pattern_that_lacks_an_entry_of_a(dev):
    ai, aj, aa = ik.shape("lap2d")
    lay = ik.layout_of("lap2d", 1)
    rc, ctx, _ = _create_fill(dev, _i32(ai), _i32(aj), lay)
    assert rc == 0 and ctx.value
    dev.chk(dev.k.mi355x_ilu0_factor_destroy(ctx))
    full = ik.dense_pattern(lay)
    for r, c in ((40, int(np.flatnonzero(~full[40, :40])[0])), (10, int(np.flatnonzero(~full[10, 11:])[-1]) + 11)):
        pat = ik.pattern_of(ai, aj)
        pat[r] = sorted(pat[r] + [c])
        ai2, aj2, _ = ilf._values(pat, 1)
        rc, ctx, _ = _create_fill(dev, ai2, aj2, lay)
        assert rc == INVALID and not ctx.value, (r, c)
    aj2 = _i32(aj).copy(); aj2[ai[20]], aj2[ai[20] + 1] = aj[ai[20] + 1], aj[ai[20]]      # A's row not sorted
    rc, ctx, _ = _create_fill(dev, _i32(ai), aj2, lay)
    assert rc == INVALID and not ctx.value


# ---------------------------------------------------------------- 2. the plug-in
def iluk_pc(P, A, opts, pctype="ilu"):
    """a KSP over A whose PC is configured from the options (-pc_type, -pc_factor_levels, ...) and set up: (ksp, pc, PCSetUp's code)"""
    L = P.lib()
    pc = C.c_void_p()
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc))
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-pc_type %s %s" % (pctype, opts)).encode())
    rc = L.raw("PCSetFromOptions")(pc)
    rc = rc or L.raw("PCSetUp")(pc)
    L.PetscOptionsClear()
    return k, pc, rc


def fill_info(P, pc):
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    P.lib().PCILUGetFill_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def ref_factor(ai, aj, aa, levels):
    """(bi, bj, bdiag, ba) of the reference, the form orc.ilu0_solve takes"""
    lay = ik.symbolic(ai, aj, levels)
    ba, frow, _, _ = ik.reference_pass(ai, aj, aa, None, [0.0], ZP, [1], layout=lay)
    assert frow[0] == -1
    return lay[0], lay[1], lay[2], ba


def csr_cases(P):
    return [("lap2d", perturbed(pb.lap2d(9, 7))), ("p7", perturbed(P.gen_poisson7(7, 6, 5)))]


def test_pc_factor_levels_sets_up(P):
    """error 56 before ILU(k) existed"""
    ai, aj, aa = perturbed(pb.lap2d(9, 7))
    A = P.Mat.from_csr(ai, aj, aa)
    ksp, pc, rc = iluk_pc(P, A, "-pc_factor_levels 1")
    assert rc == 0
    lay = ik.symbolic(ai, aj, 1)
    assert fill_info(P, pc) == (1, int(lay[2][0]) + 1, int(ai[-1]))
    ksp0, pc0, rc = iluk_pc(P, A, "")
    assert rc == 0 and fill_info(P, pc0) == (0, int(ai[-1]), int(ai[-1]))


@pytest.mark.parametrize("where", [HOST, DEVICE])
@pytest.mark.parametrize("levels", [1, 2])
def test_every_trisolve_mode_applies_the_reference_factor_bit_for_bit(P, where, levels):
    for name, (ai, aj, aa) in csr_cases(P):
        n = ai.size - 1
        f = ref_factor(ai, aj, aa, levels)
        A = P.Mat.from_csr(ai, aj, aa)
        b = rnd(n, 500 + levels)
        ref = orc.ilu0_solve(f, b)
        base = "-pc_factor_levels %d %s" % (levels, where)
        ksp, pc, rc = iluk_pc(P, A, base)
        assert rc == 0, (name, where)
        nl, nu = C.c_int(), C.c_int(); P.lib().PCILUGetLevels_HIPMI355X(pc, C.byref(nl), C.byref(nu))
        assert nl.value == ik.levels_L(f)[1]
        assert fill_info(P, pc) == (levels, int(f[2][0]) + 1, int(ai[-1]))
        assert numeric_info(P, pc) == ((1 if where == DEVICE else 0), 1, 1)
        assert np.array_equal(bits(apply(P, pc, b)), bits(ref)), (name, where, "default")
        k = max(nl.value, nu.value)
        for tri in ("level", "syncfree", "sweeps:%d" % k):
            ksp, pc, rc = iluk_pc(P, A, base + " -pc_factor_hipmi355x_trisolve " + tri)
            assert rc == 0, (name, where, tri)
            assert np.array_equal(bits(apply(P, pc, b)), bits(ref)), (name, where, tri)
        ksp, pc, rc = iluk_pc(P, A, base + " -pc_factor_hipmi355x_trisolve sweeps:2")
        assert rc == 0
        x2 = apply(P, pc, b)
        assert np.isfinite(x2).all() and not np.array_equal(bits(x2), bits(ref)), (name, where, "sweeps:2")


def test_host_and_device_factor_are_bit_identical(P):
    """the factor itself, read back through the factored matrix's solves of unit vectors would cost n applications: the two routes
    are compared on several right-hand sides instead, in the level mode (one lane per row, column order), and both against the
    reference, whose bits they carry"""
    for name, (ai, aj, aa) in csr_cases(P):
        n = ai.size - 1
        A = P.Mat.from_csr(ai, aj, aa)
        f = ref_factor(ai, aj, aa, 2)
        pcs = [iluk_pc(P, A, "-pc_factor_levels 2 -pc_factor_hipmi355x_trisolve level " + w) for w in (HOST, DEVICE)]
        assert pcs[0][2] == 0 and pcs[1][2] == 0
        for rep in range(3):
            b = rnd(n, 520 + rep)
            xh, xd = apply(P, pcs[0][1], b), apply(P, pcs[1][1], b)
            assert np.array_equal(bits(xh), bits(xd)) and np.array_equal(bits(xd), bits(orc.ilu0_solve(f, b))), (name, rep)


def test_a_second_set_up_runs_the_numeric_kernels_only_and_a_new_level_rebuilds(P):
    L = P.lib()
    ai, aj, aa = perturbed(P.gen_poisson7(7, 6, 5))
    n = ai.size - 1
    A = P.Mat.from_csr(ai, aj, aa)
    opts = "-pc_factor_levels 1 " + DEVICE
    ksp, pc, rc = iluk_pc(P, A, opts)
    assert rc == 0 and numeric_info(P, pc) == (1, 1, 1)
    b = rnd(n, 530)
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(ref_factor(ai, aj, aa, 1), b)))
    L.MatScale(A.h, 1.75)
    assert setup_again(P, ksp, pc, A, opts) == 0 and numeric_info(P, pc) == (1, 1, 2)
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(ref_factor(ai, aj, 1.75 * aa, 1), b)))
    L.PCFactorSetLevels(pc, 1)                                 # the level it has: nothing to redo
    assert setup_again(P, ksp, pc, A, opts) == 0 and numeric_info(P, pc) == (1, 1, 2)
    L.PCFactorSetLevels(pc, 2)
    assert setup_again(P, ksp, pc, A, DEVICE) == 0
    assert numeric_info(P, pc) == (1, 2, 3)
    f2 = ref_factor(ai, aj, 1.75 * aa, 2)
    assert fill_info(P, pc) == (2, int(f2[2][0]) + 1, int(ai[-1]))
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(f2, b)))
    L.PCFactorSetLevels(pc, 0)                                 # back to zero fill on the same objects: the ILU(0) kernel, the oracle's bits
    assert setup_again(P, ksp, pc, A, DEVICE) == 0 and numeric_info(P, pc) == (1, 3, 4)
    assert fill_info(P, pc) == (0, int(ai[-1]), int(ai[-1]))
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, 1.75 * aa), b)))


@pytest.mark.parametrize("where", ["host", "device"])
def test_block_jacobi_with_three_ilu1_blocks(P, where):
    import scipy.sparse as sp
    L = P.lib()
    blocks = [perturbed(pb.lap2d(5, 4)), perturbed(pb.lap2d(4, 5)), perturbed(pb.lap2d(5, 4))]
    T = sp.block_diag([sp.csr_matrix((a, j, i)) for i, j, a in blocks]).tolil()
    T[19, 20] = T[20, 19] = 0.25; T[39, 40] = T[40, 39] = 0.25      # couplings between the blocks (dropped by block Jacobi)
    T = T.tocsr(); T.sort_indices()
    A = P.Mat.from_csr(T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy())
    b = np.cos(0.3 * np.arange(60)) + 0.2
    pc = C.c_void_p()
    ksp = P.KSP(comm=L.COMM_SELF); ksp.set_operators(A); L.KSPGetPC(ksp.h, C.byref(pc)); L.PCSetType(pc, b"bjacobi")
    L.PetscOptionsClear(); L.PetscOptionsInsertString(("-pc_bjacobi_blocks 3 -sub_pc_type ilu -sub_pc_factor_levels 1 -sub_pc_factor_hipmi355x_numeric " + where).encode())
    assert L.raw("PCSetUp")(pc) == 0
    x = apply(P, pc, b)                                         # (block Jacobi sets its block solver up at the first application)
    L.PetscOptionsClear()
    nloc, first, sub, spc = C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
    L.PCBJacobiGetSubKSP(pc, C.byref(nloc), C.byref(first), C.byref(sub))
    L.KSPGetPC(C.cast(sub, C.POINTER(C.c_void_p))[0], C.byref(spc))
    assert numeric_info(P, spc)[0] == (1 if where == "device" else 0)
    refs = [ref_factor(i.astype(np.int32), j.astype(np.int32), a, 1) for i, j, a in blocks]
    assert fill_info(P, spc) == (1, sum(int(f[2][0]) + 1 for f in refs), sum(int(i[-1]) for i, _, _ in blocks))
    ref = np.concatenate([orc.ilu0_solve(f, b[20 * s:20 * s + 20]) for s, f in enumerate(refs)])
    assert np.array_equal(bits(x), bits(ref))


def test_icc_with_levels_is_still_refused(P):
    ai, aj, aa = pb.lap2d(9, 7)
    A = P.Mat.from_csr(ai, aj, aa)
    ksp, pc, rc = iluk_pc(P, A, "-pc_factor_levels 1", pctype="icc")
    assert rc == ERR_SUP
    ksp, pc, rc = iluk_pc(P, A, "-pc_factor_levels 0", pctype="icc")
    assert rc == 0


def test_gmres_takes_fewer_iterations_with_more_fill(P):
    """GMRES(30) on lap2d(31, 31), rtol 1e-8: ILU(1) strictly fewer iterations than ILU(0), ILU(2) no more than ILU(1).  All three
    stop on their own preconditioned residual norm, so the ILU(k) error against the direct solution is allowed 10 x the measured
    error of the ILU(0) solve."""
    L = P.lib()
    ai, aj, aa = pb.lap2d(31, 31)
    n = ai.size - 1
    u = np.sin(0.37 * np.arange(n)) + 1.5
    b = orc.spmv(ai, aj, aa, u)
    Ad = np.zeros((n, n)); Ad[np.repeat(np.arange(n), np.diff(ai)), aj] = aa
    direct = np.linalg.solve(Ad, b)
    A = P.Mat.from_csr(ai, aj, aa)
    its, err = {}, {}
    for levels in (0, 1, 2):
        k = P.KSP(comm=L.COMM_SELF); k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type gmres -ksp_gmres_restart 30 -pc_type ilu -pc_factor_levels %d" % levels).encode())
        k.set_tolerances(rtol=1e-8)
        k.set_from_options()
        vb, vx = V(P, b), V(P, np.zeros(n))
        k.solve(vb, vx)
        L.PetscOptionsClear()
        assert k.reason > 0
        pc = C.c_void_p(); L.KSPGetPC(k.h, C.byref(pc))
        assert fill_info(P, pc)[0] == levels
        its[levels] = k.its
        err[levels] = float(np.linalg.norm(vx.array() - direct) / np.linalg.norm(direct))
    print("GMRES(30) lap2d(31,31) rtol 1e-8: iterations %r, relative error against the direct solution %r" % (its, err))
    assert its[1] < its[0] and its[2] <= its[1]
    assert err[1] <= 10.0 * err[0] and err[2] <= 10.0 * err[0]
