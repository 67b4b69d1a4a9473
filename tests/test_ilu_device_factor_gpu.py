"""-pc_factor_hipmi355x_numeric device: the numeric ILU(0) on the device, one launch per dependency level of L (csrc/ilu_factor.hip,
mi355x_ilu0_factor_*), and the plug-in's route over it (host/ilu.c).

Every row's arithmetic is the sequential loop's (MatLUFactorNumeric_SeqAIJ: multipliers in column order, product rounded before the
subtraction, pivots stored inverted, MatPivotCheck_nz's restarts), so the factor carries the reference's BITS: the tests compare bit
patterns, never to a tolerance.  The reference everywhere is the oracle's restatement (orc.ilu0_factor / ilu0_factor_shift /
ilu0_solve)."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
import problems as pb
from test_ilu_sweeps_gpu import V, apply, block_diagonal, ilu_pc, levels_of, p7_31, perturbed, strict_triangles
from test_kernels_gpu import bits, dev, rnd  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARG_WRONG, ZRPVT = 62, 71
DEVICE = "-pc_factor_hipmi355x_numeric device"


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def numeric_info(P, pc):
    """(on_device, symbolic_builds, numeric_runs)"""
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    P.lib().PCILUGetNumeric_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def shift_count(P, pc):
    ns = C.c_int(-1)
    P.lib().PCILUGetShiftCount_HIPMI355X(pc, C.byref(ns))
    return ns.value


def setup_again(P, ksp, pc, A, opts):
    L = P.lib()
    ksp.set_operators(A)
    L.PetscOptionsClear()
    if opts:
        L.PetscOptionsInsertString(opts.encode())
    rc = L.raw("PCSetUp")(pc)
    L.PetscOptionsClear()
    return rc


# ---------------------------------------------------------------- 1. the kernel through the C ABI
def symbolic(ai, aj, aa):
    """the factor's layout (the oracle's own symbolic arrays) and the rows sorted by dependency level of L"""
    n = ai.size - 1
    bi, bj, bd, _ = orc.ilu0_factor(ai, aj, aa) if n else (np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([-1], np.int32), None)
    lev = np.zeros(n, np.int64)
    for i in range(n):
        cols = bj[bi[i]:bi[i + 1]]
        lev[i] = lev[cols].max() + 1 if cols.size else 0
    nlev = int(lev.max()) + 1 if n else 0
    rows = np.argsort(lev, kind="stable").astype(np.int32)
    levptr = np.zeros(nlev + 1, np.int32)
    levptr[1:] = np.cumsum(np.bincount(lev, minlength=nlev)) if n else 0
    return bi, bj, bd, nlev, levptr, rows


def device_factor(dev, ai, aj, aa, blk=None, shifts=None, zeropivot=100.0 * 2.220446049250313e-16, passes=1):
    """ba read back after `passes` calls of mi355x_ilu0_factor_run, the per-block outcome of the last one and (lanes, levels)"""
    k = dev.k
    n, nz = ai.size - 1, int(ai[-1])
    bi, bj, bd, nlev, levptr, rows = symbolic(ai, aj, aa)
    nblk = 1 if blk is None else len(blk) - 1
    ctx = C.c_void_p()
    I32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    keep = [I32(bi), I32(bj), I32(bd), I32(levptr), I32(rows), I32(blk if blk is not None else [0, n])]
    dev.chk(k.mi355x_ilu0_factor_create(dev.h, n, *[a.ctypes.data for a in keep[:3]], nlev, keep[3].ctypes.data, keep[4].ctypes.data,
                                        nblk, keep[5].ctypes.data if blk is not None else None, C.byref(ctx)))
    dai, daj, daa, dba = dev.put(I32(ai)), dev.put(I32(aj)), dev.put(aa), dev.put(np.zeros(nz + 1))
    sh = np.zeros(nblk) if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64)
    frow, fabs_ = np.full(nblk, -7, np.int32), np.full(nblk, -7.0)
    dev.chk(k.mi355x_ilu0_factor_reset(ctx))
    for _ in range(passes):
        dev.chk(k.mi355x_ilu0_factor_run(dev.h, ctx, dai, daj, daa, zeropivot, sh.ctypes.data, dba, frow.ctypes.data, fabs_.ctypes.data))
    ba = dev.get(dba, nz + 1)
    lanes, nl = C.c_int(), C.c_int()
    dev.chk(k.mi355x_ilu0_factor_info(ctx, C.byref(lanes), C.byref(nl)))
    assert nl.value == nlev
    dev.chk(k.mi355x_ilu0_factor_destroy(ctx))
    for p in (dai, daj, daa, dba):
        dev.free(p)
    return ba, frow, fabs_, (lanes.value, nl.value)


def random_pattern(n, seed, wide=()):
    """non-symmetric random pattern with a full diagonal, diagonally dominant values; rows in `wide` get > 64 entries, a few rows one"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=min(1.0, 5.0 / n), random_state=int(rng.integers(1 << 30)), data_rvs=rng.standard_normal).tolil()
    for r in wide:
        cols = rng.choice(n, size=min(n, int(rng.integers(70, 150))), replace=False)
        R[r, cols] = rng.standard_normal(cols.size)
    for r in range(0, n, 37):
        R[r, :] = 0.0                                       # rows of one entry (the diagonal)
    R = R.tocsr(); R.eliminate_zeros()
    A = (R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() + 1.0)).tocsr(); A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def test_kernel_factor_is_the_oracles_bit_for_bit(dev):
    cases = [("lap2d", perturbed(pb.lap2d(9, 7))), ("p7 small", perturbed(orc_p7(7, 6, 5))), ("p7 31 levels", perturbed(orc_p7(12, 11, 10))),
             ("ex10", pb.ex10_elasticity()[0]), ("random", random_pattern(700, 1)), ("random, rows wider than a wavefront", random_pattern(900, 2, wide=(5, 450, 451, 899))),
             ("all rows wide", random_pattern(200, 3, wide=range(200)))]
    seen_lanes = set()
    for name, (ai, aj, aa) in cases:
        ai, aj = ai.astype(np.int32), aj.astype(np.int32)
        ref = orc.ilu0_factor(ai, aj, aa)[3]
        ba, frow, fabs_, (lanes, nlev) = device_factor(dev, ai, aj, aa)
        width = int(np.diff(ai).max())
        print("%s: n=%d widest row %d lanes %d levels %d" % (name, ai.size - 1, width, lanes, nlev))
        assert lanes == min(64, 1 << (width - 1).bit_length())
        assert frow[0] == -1, name
        assert np.array_equal(bits(ba), bits(ref)), name
        seen_lanes.add(lanes)
        if "wide" in name:
            assert width > 64 and np.diff(ai).min() == 1
    assert {8, 64} <= seen_lanes
    # a second pass over a finished factorisation has no pending block: nothing is touched; n = 1 and n = 0
    ai, aj, aa = perturbed(pb.lap2d(9, 7))
    ba2 = device_factor(dev, ai, aj, aa, passes=2)[0]
    assert np.array_equal(bits(ba2), bits(orc.ilu0_factor(ai, aj, aa)[3]))
    one = (np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([-4.0]))
    ba, frow, _, info = device_factor(dev, *one)
    assert frow[0] == -1 and np.array_equal(bits(ba), bits(np.array([-0.25, 0.0]))) and info[0] == 1
    ba, frow, _, _ = device_factor(dev, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert ba.size == 1 and ba[0] == 0.0 and frow[0] == -1


def orc_p7(nx, ny, nz):
    from petsc_dev_amd import petsc as P
    return P.gen_poisson7(nx, ny, nz)


def test_kernel_reports_the_failing_pivot_per_block_and_takes_the_shift(dev):
    """tridiag(1, 1, 1) has a zero pivot in row 1 (MatPivotCheck_nz); as the second of three independent blocks only that block
    fails, stays pending and is factored again with its shift while the finished blocks are left alone; the result is the oracle's
    factor of every block with its own shift"""
    import scipy.sparse as sp
    T = sp.block_diag([sp.diags([-np.ones(19), 4.0 * np.ones(20), -np.ones(19)], [-1, 0, 1]), sp.diags([np.ones(19), np.ones(20), np.ones(19)], [-1, 0, 1]),
                       sp.diags([-np.ones(19), 3.0 * np.ones(20), -np.ones(19)], [-1, 0, 1])]).tocsr(); T.sort_indices()
    ai, aj, aa = T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()
    blk = [0, 20, 40, 60]
    ba, frow, fabs_, _ = device_factor(dev, ai, aj, aa, blk=blk)
    assert list(frow) == [-1, 21, -1] and fabs_[1] == 0.0
    (fb, nshift) = orc.ilu0_factor_shift(ai[20:41] - ai[20], aj[ai[20]:ai[40]] - 20, aa[ai[20]:ai[40]])
    assert nshift >= 1
    # the plug-in's loop through the C ABI: shiftamount, then twice that, ... until the block passes
    k = dev.k
    bi, bj, bd, nlev, levptr, rows = symbolic(ai, aj, aa)
    I32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    keep = [I32(bi), I32(bj), I32(bd), I32(levptr), I32(rows), I32(blk)]
    ctx = C.c_void_p()
    dev.chk(k.mi355x_ilu0_factor_create(dev.h, 60, *[a.ctypes.data for a in keep[:3]], nlev, keep[3].ctypes.data, keep[4].ctypes.data, 3, keep[5].ctypes.data, C.byref(ctx)))
    dai, daj, daa, dba = dev.put(ai), dev.put(aj), dev.put(aa), dev.put(np.zeros(int(ai[-1]) + 1))
    sh, cnt = np.zeros(3), np.zeros(3, int)
    frow, fabs_ = np.zeros(3, np.int32), np.zeros(3)
    amount = 100.0 * 2.220446049250313e-16
    for _ in range(82):
        dev.chk(k.mi355x_ilu0_factor_run(dev.h, ctx, dai, daj, daa, amount, sh.ctypes.data, dba, frow.ctypes.data, fabs_.ctypes.data))
        if not (frow >= 0).any():
            break
        for b in np.nonzero(frow >= 0)[0]:
            sh[b] = sh[b] * 2.0 if cnt[b] else amount
            cnt[b] += 1
    assert list(cnt) == [0, nshift, 0]
    ba = dev.get(dba, int(ai[-1]) + 1)
    # the whole matrix factored by the oracle with the middle block's shift on the middle block's diagonal
    aas = aa.copy()
    rowsof = np.repeat(np.arange(60), np.diff(ai))
    aas[(aj == rowsof) & (rowsof >= 20) & (rowsof < 40)] += sh[1]
    assert np.array_equal(bits(ba), bits(orc.ilu0_factor(ai, aj, aas)[3]))
    # the sweep form's arrays from the factor on the device: the negated strict triangles and the inverted pivots
    f = (bi, bj, bd, ba)
    (iL, jL, aL), (iU, jU, aU), dinv = strict_triangles(f)
    diU, daL, daU, ddinv = dev.put(iU), dev.put(np.zeros(aL.size)), dev.put(np.zeros(aU.size)), dev.put(np.zeros(60))
    dev.chk(k.mi355x_ilu0_factor_to_sweeps(dev.h, ctx, diU, dba, daL, daU, ddinv))
    assert np.array_equal(bits(dev.get(daL, aL.size)), bits(aL)) and np.array_equal(bits(dev.get(daU, aU.size)), bits(aU))
    assert np.array_equal(bits(dev.get(ddinv, 60)), bits(dinv))
    # the context's device copies of the layout
    ptrs = [C.c_void_p() for _ in range(4)]
    dev.chk(k.mi355x_ilu0_factor_arrays(ctx, *[C.byref(p) for p in ptrs]))
    assert np.array_equal(dev.get(ptrs[0], 61, np.int32), bi) and np.array_equal(dev.get(ptrs[2], 61, np.int32), bd)
    assert np.array_equal(dev.get(ptrs[1], int(ai[-1]), np.int32), bj[:-1]) and np.array_equal(dev.get(ptrs[3], 60, np.int32), rows)
    dev.chk(k.mi355x_ilu0_factor_destroy(ctx))
    for p in (dai, daj, daa, dba, diU, daL, daU, ddinv):
        dev.free(p)
    # a layout that does not hold together is refused before anything runs on it
    bad = keep[1].copy(); bad[0] = 99
    assert k.mi355x_ilu0_factor_create(dev.h, 60, keep[0].ctypes.data, bad.ctypes.data, keep[2].ctypes.data, nlev, keep[3].ctypes.data, keep[4].ctypes.data, 3, keep[5].ctypes.data, C.byref(ctx)) == 1
    assert not ctx.value


# ---------------------------------------------------------------- 2. through PCSetUp, every consumer of the factor
@pytest.mark.parametrize("mode", ["syncfree", "level", "sweeps"])
def test_pcsetup_on_the_device_applies_with_the_oracles_bits(P, mode):
    for csr in (pb.lap2d(9, 7), P.gen_poisson7(7, 6, 5), P.gen_poisson7(12, 11, 10), random_pattern(700, 1)):
        ai, aj, aa = perturbed(csr)
        n = ai.size - 1
        A = P.Mat.from_csr(ai, aj, aa)
        nl, nu = levels_of(P, A)
        tri = "-pc_factor_hipmi355x_trisolve " + (mode if mode != "sweeps" else "sweeps:%d" % max(max(nl, nu) - 1, 1))
        ksp, pc, rc = ilu_pc(P, A, DEVICE + " " + tri)
        assert rc == 0
        assert numeric_info(P, pc) == (1, 1, 1)
        f = orc.ilu0_factor(ai, aj, aa)
        for rep in range(3):
            b = rnd(n, 300 + rep)
            assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(f, b))), (n, mode, rep)
        l2, u2 = C.c_int(), C.c_int(); P.lib().PCILUGetLevels_HIPMI355X(pc, C.byref(l2), C.byref(u2))
        assert (l2.value, u2.value) == (nl, nu) and shift_count(P, pc) == 0
        ksp0, pc0, rc = ilu_pc(P, A, tri)                       # the default stays the host route
        assert rc == 0 and numeric_info(P, pc0) == (0, 1, 1)
        assert np.array_equal(bits(apply(P, pc0, b)), bits(orc.ilu0_solve(f, b)))


def test_pcsetup_of_an_empty_matrix_succeeds_on_both_routes(P):
    """n = 0: the operator's device arrays hold nothing; the device route lets it through as the host route does"""
    ai, aj, aa = np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)
    A = P.Mat.from_csr(ai, aj, aa)
    ksp0, pc0, rc0 = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve level")
    assert rc0 == 0 and numeric_info(P, pc0)[0] == 0
    ksp, pc, rc = ilu_pc(P, A, DEVICE + " -pc_factor_hipmi355x_trisolve level")
    assert rc == 0 and numeric_info(P, pc) == (1, 1, 1)
    assert apply(P, pc, np.zeros(0)).size == 0


# ---------------------------------------------------------------- 3. shifts
def test_restarts_with_a_shifted_diagonal_as_the_oracle(P):
    import scipy.sparse as sp
    L = P.lib()
    T = sp.diags([np.ones(299), np.ones(300), np.ones(299)], [-1, 0, 1]).tocsr(); T.sort_indices()      # zero pivots: shifts
    ai, aj, aa = T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()
    f, ns_o = orc.ilu0_factor_shift(ai, aj, aa)
    assert ns_o >= 1
    for tri in ("syncfree", "level"):
        A = P.Mat.from_csr(ai, aj, aa)
        ksp, pc, rc = ilu_pc(P, A, DEVICE + " -pc_factor_hipmi355x_trisolve " + tri)
        assert rc == 0 and numeric_info(P, pc)[0] == 1
        assert shift_count(P, pc) == ns_o
        b = rnd(300, 11)
        assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(f, b)))
    # without the shift the set-up fails (zero pivot); the default shift on the same objects then succeeds
    A = P.Mat.from_csr(ai, aj, aa)
    pc = C.c_void_p()
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc)); L.PCSetType(pc, b"ilu")
    L.PetscOptionsClear(); L.PetscOptionsInsertString((DEVICE + " -pc_factor_shift_type none").encode())
    rc0 = L.raw("PCSetFromOptions")(pc)
    rc = L.raw("PCSetUp")(pc)
    assert rc0 == 0 and rc != 0
    L.PetscOptionsClear(); L.PetscOptionsInsertString((DEVICE + " -pc_factor_shift_type nonzero").encode())
    assert L.raw("PCSetFromOptions")(pc) == 0 and L.raw("PCSetUp")(pc) == 0
    L.PetscOptionsClear()
    assert shift_count(P, pc) == ns_o and numeric_info(P, pc)[0] == 1
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(f, b)))


# ---------------------------------------------------------------- 4. independent blocks
def test_block_jacobi_blocks_one_of_them_shifted_same_bits_as_the_host_route(P):
    import scipy.sparse as sp
    L = P.lib()
    T = sp.block_diag([sp.diags([-np.ones(19), 4.0 * np.ones(20), -np.ones(19)], [-1, 0, 1]), sp.diags([np.ones(19), np.ones(20), np.ones(19)], [-1, 0, 1]),
                       sp.diags([-np.ones(19), 3.0 * np.ones(20), -np.ones(19)], [-1, 0, 1])]).tolil()
    T[19, 20] = T[20, 19] = 0.25; T[39, 40] = T[40, 39] = 0.25      # couplings between the blocks (dropped by block Jacobi)
    T = T.tocsr(); T.sort_indices()
    ai, aj, aa = T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()
    A = P.Mat.from_csr(ai, aj, aa)
    b = np.cos(0.3 * np.arange(60)) + 0.2
    out = {}
    for where in ("host", "device"):
        pc = C.c_void_p()
        ksp = P.KSP(comm=L.COMM_SELF); ksp.set_operators(A); L.KSPGetPC(ksp.h, C.byref(pc)); L.PCSetType(pc, b"bjacobi")
        L.PetscOptionsClear(); L.PetscOptionsInsertString(("-pc_bjacobi_blocks 3 -sub_pc_type ilu -sub_pc_factor_hipmi355x_numeric " + where).encode())
        assert L.raw("PCSetUp")(pc) == 0
        out[where] = apply(P, pc, b)                           # (block Jacobi sets its block solver up at the first application)
        L.PetscOptionsClear()
        nloc, first, sub, spc = C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
        L.PCBJacobiGetSubKSP(pc, C.byref(nloc), C.byref(first), C.byref(sub))
        L.KSPGetPC(C.cast(sub, C.POINTER(C.c_void_p))[0], C.byref(spc))
        assert numeric_info(P, spc)[0] == (1 if where == "device" else 0)
        out[where + " shifts"] = shift_count(P, spc)
    assert out["device shifts"] == out["host shifts"] >= 1
    assert np.array_equal(bits(out["device"]), bits(out["host"]))


# ---------------------------------------------------------------- 5. re-factorisation
@pytest.mark.parametrize("tri", ["syncfree", "level", "sweeps:30"])
def test_refactorisation_runs_the_numeric_kernels_only(P, tri):
    L = P.lib()
    ai, aj, aa = p7_31(P)
    n = ai.size - 1
    opts = DEVICE + " -pc_factor_hipmi355x_trisolve " + tri
    A = P.Mat.from_csr(ai, aj, aa)
    ksp, pc, rc = ilu_pc(P, A, opts)
    assert rc == 0 and numeric_info(P, pc) == (1, 1, 1)
    b = rnd(n, 40)
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa), b)))
    # unchanged operator state: nothing runs
    assert setup_again(P, ksp, pc, A, opts) == 0 and numeric_info(P, pc) == (1, 1, 1)
    # values changed on the device copy (rows scaled, then the whole matrix): what the next factorisation uses
    dl = 1.0 + 0.3 * np.cos(np.arange(n))
    vl = V(P, dl)
    L.MatDiagonalScale(A.h, vl.h, None)
    L.MatScale(A.h, 1.75)
    aa2 = 1.75 * (aa * np.repeat(dl, np.diff(ai)))
    assert setup_again(P, ksp, pc, A, opts) == 0
    assert numeric_info(P, pc) == (1, 1, 2)
    f2 = orc.ilu0_factor(ai, aj, aa2)
    for rep in range(2):
        b = rnd(n, 41 + rep)
        x = apply(P, pc, b)
        assert np.array_equal(bits(x), bits(orc.ilu0_solve(f2, b)))
    assert not np.array_equal(bits(x), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa), b)))
    # new values through the host copy (MatZeroEntries + MatSetValues) on the same pattern
    aa3 = aa * (1.0 + 0.04 * np.cos(0.7 * np.arange(aa.size)))
    L.MatZeroEntries(A.h)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(ai))
    for r, c, v in zip(rows, aj, aa3):
        L.MatSetValues(A.h, 1, C.byref(C.c_int(int(r))), 1, C.byref(C.c_int(int(c))), C.byref(C.c_double(float(v))), P.ADD_VALUES)
    L.MatAssemblyBegin(A.h, P.MAT_FINAL_ASSEMBLY); L.MatAssemblyEnd(A.h, P.MAT_FINAL_ASSEMBLY)
    assert setup_again(P, ksp, pc, A, opts) == 0 and numeric_info(P, pc) == (1, 1, 3)
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa3), b)))
    # another pattern (same size: the factored matrix keeps its dimensions): rebuilt, and correct
    bi_, bj_, ba_ = perturbed(P.gen_poisson7(10, 12, 11))
    assert bi_.size == ai.size and not np.array_equal(bi_, ai)
    B = P.Mat.from_csr(bi_, bj_, ba_)
    assert setup_again(P, ksp, pc, B, opts.replace("sweeps:30", "sweeps:40")) == 0
    assert numeric_info(P, pc) == (1, 2, 4)
    b = rnd(bi_.size - 1, 44)
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(orc.ilu0_factor(bi_, bj_, ba_), b)))
    # back to the host route on the same objects
    L.MatScale(B.h, 0.5)
    assert setup_again(P, ksp, pc, B, "-pc_factor_hipmi355x_trisolve " + tri.replace("30", "40")) == 0 and numeric_info(P, pc)[0] == 0
    assert np.array_equal(bits(apply(P, pc, b)), bits(orc.ilu0_solve(orc.ilu0_factor(bi_, bj_, 0.5 * ba_), b)))


# ---------------------------------------------------------------- 6. goldens
def test_goldens_ex2_and_ex5_print_the_same_lines_with_the_option(P):
    L = P.lib()
    ai, aj, aa = pb.lap2d(5, 5)
    u = np.ones(25)
    b = orc.spmv(ai, aj, aa, u)
    gold = pb.parse_monitor(os.path.join(G, "ksp_tutorials", "ex2_1.out"))[0]
    A = P.Mat.from_csr(ai, aj, aa)
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A)
    L.PetscOptionsClear(); L.PetscOptionsInsertString(("-ksp_gmres_cgs_refinement_type refine_always " + DEVICE).encode())
    k.set_tolerances(rtol=1e-2 / 36, abstol=1e-50)
    k.set_from_options(); k.record_history()
    vb, vx = V(P, b), V(P, np.zeros(25))
    k.solve(vb, vx)
    L.PetscOptionsClear()
    pb.check_monitor(k.history(), gold)
    assert k.its == 4 and "%.5g" % np.linalg.norm(vx.array() - u) in ("0.0003927", "0.00039270")
    pc = C.c_void_p(); L.KSPGetPC(k.h, C.byref(pc))
    assert numeric_info(P, pc) == (1, 1, 1)
    # ex5: two solves with ONE KSP, the second after MatZeroEntries + re-assembly into the same pattern.  The golden run is
    # GMRES + Jacobi (the option is inert there: same lines); with ILU(0) the device route repeats the host route's history bit for bit
    solves = pb.parse_monitor(os.path.join(G, "ksp_tutorials", "ex5_1.out"))
    hist = {}
    for pcopts in ("-pc_type jacobi " + DEVICE, "-pc_type ilu", "-pc_type ilu " + DEVICE):
        (ai, aj, aa), u = pb.ex5_tutorial(1, False)
        A = P.Mat.from_csr(ai, aj, aa)
        vu = V(P, u); vb = vu.duplicate(); vx = vu.duplicate()
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type gmres -ksp_gmres_cgs_refinement_type refine_always " + pcopts).encode())
        k.set_from_options()
        hist[pcopts] = []
        for second in (False, True):
            if second:
                (ai2, aj2, aa2), _ = pb.ex5_tutorial(1, True)
                L.MatZeroEntries(A.h)
                rows = np.repeat(np.arange(ai2.size - 1, dtype=np.int32), np.diff(ai2))
                for r, c, v in zip(rows, aj2, aa2):
                    L.MatSetValues(A.h, 1, C.byref(C.c_int(int(r))), 1, C.byref(C.c_int(int(c))), C.byref(C.c_double(float(v))), P.ADD_VALUES)
                L.MatAssemblyBegin(A.h, P.MAT_FINAL_ASSEMBLY); L.MatAssemblyEnd(A.h, P.MAT_FINAL_ASSEMBLY)
                k.set_operators(A)
            A.mult(vu, vb)
            k.record_history()
            k.solve(vb, vx)
            if "jacobi" in pcopts:
                pb.check_monitor(k.history(), solves[1 if second else 0])
            hist[pcopts].append(np.array(k.history()))
            assert np.linalg.norm(vx.array() - u) < 1e-4 * np.linalg.norm(u)
        L.PetscOptionsClear()
        if "ilu" in pcopts:
            pc = C.c_void_p(); L.KSPGetPC(k.h, C.byref(pc))
            assert numeric_info(P, pc) == ((1, 1, 2) if DEVICE in pcopts else (0, 2, 2))
    for a, b_ in zip(hist["-pc_type ilu"], hist["-pc_type ilu " + DEVICE]):
        assert np.array_equal(bits(a), bits(b_))


# ---------------------------------------------------------------- 7. bad option value
@pytest.mark.parametrize("value", ["gpu", "Device", "1", "hostt"])
def test_any_other_value_is_refused(P, value):
    ai, aj, aa = pb.lap2d(9, 7)
    A = P.Mat.from_csr(ai, aj, aa)
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_numeric " + value)
    assert rc == ARG_WRONG
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_numeric host")
    assert rc == 0 and numeric_info(P, pc)[0] == 0
