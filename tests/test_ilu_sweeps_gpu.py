"""-pc_factor_hipmi355x_trisolve sweeps:<k>: ILU(0) applied by k Jacobi sweeps per triangular solve (host/ilu.c) and the kernel
form behind the upper sweep, mi355x_spmv_csr_add_scaled (z = d .* (y + A x)); the lower sweep is mi355x_spmv_csr_add on the negated
strict lower triangle.

What the tests lean on: a row of dependency level l is final from sweep l on, so k >= levels - 1 sweeps ARE the solve -- and
bit for bit where a row is summed by one lane (s = b_i; s = s + (-l_ij) y_j in column order is MatSolve_SeqAIJ_NaturalOrdering's
loop).  Fewer sweeps give an approximate application that gets closer with every sweep.  The reference everywhere is the oracle's
restatement of the reference routines (orc.ilu0_factor / orc.ilu0_solve)."""
import ctypes as C

import numpy as np
import pytest

import orc
import problems as pb
from sweeps_ref import ref_add_scaled, strict_triangles  # noqa: F401 (the restatements; other test modules take them from here)
from test_kernels_gpu import bits, dev, make_plan, random_csr, rnd  # noqa: F401 (dev: fixture)

pytestmark = pytest.mark.gpu
ARG_WRONG, ARG_IDN = 62, 61


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def V(P, a):
    return P.Vec.from_array(a, comm=P.lib().COMM_SELF)


def perturbed(csr):
    """the value perturbation of test_ilu0_apply_bitexact_and_golden"""
    ai, aj, aa = csr
    return ai, aj, aa * (1.0 + 0.05 * np.sin(np.arange(aa.size)))


def p7_31(P):
    """gen_poisson7(12, 11, 10), perturbed: 31 + 31 dependency levels"""
    return perturbed(P.gen_poisson7(12, 11, 10))


def ilu_pc(P, A, opts, pctype=b"ilu"):
    """a KSP over A whose PC is set up under the given options; (ksp, pc, PCSetUp's return code)"""
    L = P.lib()
    pc = C.c_void_p()
    k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc)); L.PCSetType(pc, pctype)
    L.PetscOptionsClear()
    if opts:
        L.PetscOptionsInsertString(opts.encode())
    rc = L.raw("PCSetUp")(pc)
    L.PetscOptionsClear()
    return k, pc, rc


def levels_of(P, A):
    """(nlevL, nlevU) from a default (exact) set-up"""
    L = P.lib()
    k, pc, rc = ilu_pc(P, A, "")
    assert rc == 0
    nl, nu = C.c_int(), C.c_int()
    L.PCILUGetLevels_HIPMI355X(pc, C.byref(nl), C.byref(nu))
    return nl.value, nu.value


def apply(P, pc, b):
    L = P.lib()
    vb, vx = V(P, b), V(P, np.zeros(b.size))
    assert L.raw("PCApply")(pc, vb.h, vx.h) == 0
    return vx.array()


# ---------------------------------------------------------------- 1. enough sweeps are the exact solve
def test_enough_sweeps_are_the_exact_solve_bit_for_bit(P):
    L = P.lib()
    for which, csr in enumerate((pb.lap2d(9, 7), P.gen_poisson7(7, 6, 5), P.gen_poisson7(12, 11, 10))):
        ai, aj, aa = perturbed(csr)
        n = ai.size - 1
        A = P.Mat.from_csr(ai, aj, aa)
        nl, nu = levels_of(P, A)
        k = max(nl, nu) - 1
        ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:%d" % k)
        assert rc == 0
        f = orc.ilu0_factor(ai, aj, aa)
        vb, vx = V(P, np.zeros(n)), V(P, np.zeros(n))
        for rep in range(4):                                   # several right-hand sides in a row: the work vectors carry nothing over
            b = rnd(n, 77 + rep); vb.set_array(b)
            assert L.raw("PCApply")(pc, vb.h, vx.h) == 0
            assert np.array_equal(bits(vx.array()), bits(orc.ilu0_solve(f, b))), (n, k, rep)
        got = C.c_int(-1); L.PCILUGetSweeps_HIPMI355X(pc, C.byref(got))
        assert got.value == k
        # the other getters keep answering: the levels of the analysis, "not sync-free, nothing gave up", no node plans
        l2, u2 = C.c_int(), C.c_int(); L.PCILUGetLevels_HIPMI355X(pc, C.byref(l2), C.byref(u2))
        assert (l2.value, u2.value) == (nl, nu)
        sf, ab = C.c_int(-1), C.c_int(-1); L.PCILUGetSolver_HIPMI355X(pc, C.byref(sf), C.byref(ab))
        assert (sf.value, ab.value) == (0, 0)
        if which == 2:
            assert (nl, nu) == (31, 31)
            # one sweep short: the rows of the last level are not final yet (3.9e-12 relative with sequential sums on the CPU)
            ksp1, pc1, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:%d" % (k - 1))
            assert rc == 0
            b = rnd(n, 77)
            x1, ref = apply(P, pc1, b), orc.ilu0_solve(f, b)
            assert not np.array_equal(bits(x1), bits(ref))
            assert np.linalg.norm(x1 - ref) <= 1e-9 * np.linalg.norm(ref)
            L.PCILUGetSweeps_HIPMI355X(pc1, C.byref(got)); assert got.value == k - 1
    # a factor that solves exactly reports 0 sweeps
    ksp0, pc0, rc = ilu_pc(P, A, "")
    got = C.c_int(-1); L.PCILUGetSweeps_HIPMI355X(pc0, C.byref(got))
    assert rc == 0 and got.value == 0


# ---------------------------------------------------------------- 2. the kernel form through the C ABI
def put_csr(dev, ai, aj, aa):
    """device CSR with the 16 bytes of slack past the value and index arrays that the row-block kernels' paired loads ask for"""
    return dev.put(ai), dev.put(np.concatenate([aj, np.zeros(4, np.int32)])), dev.put(np.concatenate([aa, np.zeros(2)]))


def run_add_scaled(dev, ai, aj, aa, x, y, d, alias):
    k = dev.k
    dai, daj, daa = put_csr(dev, ai, aj, aa)
    dx, dy, dd = dev.put(x), dev.put(y), dev.put(d)
    dz = dy if alias else dev.put(np.full(y.size, 7.0))
    plan = make_plan(dev, ai)
    dev.chk(k.mi355x_spmv_csr_add_scaled(dev.h, plan, dai, daj, daa, dx, dy, dd, dz))
    z = dev.get(dz, y.size)
    if not alias:
        assert np.array_equal(bits(dev.get(dy, y.size)), bits(y))       # the input is left alone
        dev.free(dz)
    dev.chk(k.mi355x_spmv_plan_destroy(plan))
    for p in (dai, daj, daa, dx, dy, dd):
        dev.free(p)
    return z


@pytest.mark.parametrize("alias", [False, True])
def test_add_scaled_short_rows_bit_for_bit(dev, alias):
    """rows of 0..16 nonzeros, empty rows among them, rectangular: one lane per row in column order"""
    ai, aj, aa = random_csr(3001, 2000, lambda rng, m: rng.integers(0, 17, m), 160)
    assert np.any(np.diff(ai) == 0)
    x, y, d = rnd(2000, 161), rnd(3001, 162), rnd(3001, 163)
    got = run_add_scaled(dev, ai, aj, aa, x, y, d, alias)
    assert np.array_equal(bits(got), bits(ref_add_scaled(ai, aj, aa, x, y, d)))
    assert np.array_equal(bits(got), bits(d * orc.spmv_add(ai, aj, aa, x, y)))     # = MatMultAdd, then VecPointwiseMult
    # only empty rows, and no rows at all
    ai0 = np.zeros(301, np.int32); e = np.zeros(0)
    got = run_add_scaled(dev, ai0, np.zeros(0, np.int32), e, x, y[:300], d[:300], alias)
    assert np.array_equal(bits(got), bits(d[:300] * y[:300]))
    assert run_add_scaled(dev, np.zeros(1, np.int32), np.zeros(0, np.int32), e, x, e, e, alias).size == 0


@pytest.mark.parametrize("alias", [False, True])
def test_add_scaled_long_rows_within_the_long_row_bound(dev, alias):
    """log-normal row lengths, rows longer than the LDS stage (a whole workgroup each) and empty rows: the lane tree's bound,
    1e-12 * sum |a_ij x_j| per row; empty rows exactly d .* y"""
    def rl(rng, m):
        l = np.clip(np.exp(rng.normal(np.log(60), 0.6, m)), 3, 400)
        l[::97] = 3000
        l[5::50] = 0
        return l
    ai, aj, aa = random_csr(1500, 6000, rl, 164)
    x, y, d = rnd(6000, 165), rnd(1500, 166), rnd(1500, 167)
    got = run_add_scaled(dev, ai, aj, aa, x, y, d, alias)
    ref = ref_add_scaled(ai, aj, aa, x, y, d)
    scale = np.zeros(1500)
    np.add.at(scale, np.repeat(np.arange(1500), np.diff(ai)), np.abs(aa * x[aj]))
    empty = np.diff(ai) == 0
    assert empty.any() and np.array_equal(bits(got[empty]), bits(ref[empty]))
    err = np.abs(got - ref)
    print("long rows: max |err| / sum|a x| = %.3g" % np.max(err[~empty] / scale[~empty]))
    assert np.all(err[~empty] <= 1e-12 * scale[~empty])


def test_sweep_steps_on_the_strict_triangles_of_a_factor(dev):
    """the two steps on the triangles of a real factor: one step each equals numpy bit for bit (the add form on the strict lower
    triangle, the new form on the strict upper one), and levels - 1 steps of each, driven through the C ABI alone, are
    MatSolve_SeqAIJ_NaturalOrdering bit for bit"""
    k = dev.k
    ai, aj, aa = perturbed(pb.lap2d(9, 7))
    n = ai.size - 1
    f = orc.ilu0_factor(ai, aj, aa)
    (iL, jL, aL), (iU, jU, aU), dinv = strict_triangles(f)
    assert np.all(jL < np.repeat(np.arange(n), np.diff(iL))) and np.all(jU > np.repeat(np.arange(n), np.diff(iU)))
    b = rnd(n, 170)
    dL, dU = put_csr(dev, iL, jL, aL), put_csr(dev, iU, jU, aU)
    pL, pU = make_plan(dev, iL), make_plan(dev, iU)
    db, dd, w = dev.put(b), dev.put(dinv), [dev.put(np.zeros(n)) for _ in range(3)]
    dev.chk(k.mi355x_spmv_csr_add(dev.h, pL, *dL, db, db, w[0]))
    y1 = dev.get(w[0], n)
    assert np.array_equal(bits(y1), bits(ref_add_scaled(iL, jL, aL, b, b)))
    dev.chk(k.mi355x_spmv_csr_add_scaled(dev.h, pU, *dU, db, w[0], dd, w[1]))
    assert np.array_equal(bits(dev.get(w[1], n)), bits(ref_add_scaled(iU, jU, aU, b, y1, dinv)))
    nsw = n                                                    # >= levels - 1 for any pattern
    prev = db
    for j in range(nsw):
        dev.chk(k.mi355x_spmv_csr_add(dev.h, pL, *dL, prev, db, w[j & 1])); prev = w[j & 1]
    yk, cur = prev, w[2]
    spare = w[nsw & 1]
    dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, dd, yk, cur))
    for j in range(nsw):
        out = spare if cur is w[2] else w[2]
        dev.chk(k.mi355x_spmv_csr_add_scaled(dev.h, pU, *dU, cur, yk, dd, out)); cur = out
    assert np.array_equal(bits(dev.get(cur, n)), bits(orc.ilu0_solve(f, b)))
    for p in (pL, pU):
        dev.chk(k.mi355x_spmv_plan_destroy(p))
    for p in (*dL, *dU, db, dd, *w):
        dev.free(p)


# ---------------------------------------------------------------- 3. convergence towards the exact application
def test_every_sweep_brings_the_application_closer_to_the_solve(P):
    """relative distance from the oracle's solve over k = 1, 2, 4, 8 on the 31-level matrix: strictly decreasing (sequential sums
    on the CPU give 0.31, 0.15, 0.038, 0.0027)"""
    ai, aj, aa = p7_31(P)
    n = ai.size - 1
    A = P.Mat.from_csr(ai, aj, aa)
    b = rnd(n, 77)
    ref = orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa), b)
    dist = []
    for k in (1, 2, 4, 8):
        ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:%d" % k)
        assert rc == 0
        dist.append(np.linalg.norm(apply(P, pc, b) - ref) / np.linalg.norm(ref))
    print("relative distance from the exact application, k = 1, 2, 4, 8:", " ".join("%.3g" % v for v in dist))
    assert all(dist[i + 1] < dist[i] for i in range(3)) and dist[0] < 1.0 and dist[3] > 0.0


# ---------------------------------------------------------------- 4. as a preconditioner
def test_gmres_with_three_sweeps_is_close_to_exact_ilu_and_far_from_jacobi(P):
    """GMRES(30), b = A 1, rtol 1e-8 on the 31-level matrix (CPU: 19 / 18 / 53 iterations for sweeps:3 / exact ILU(0) / Jacobi).
    its(sweeps:3) < its(Jacobi); its(sweeps:3) <= its(exact) + 4 -- one iteration of drift from the device's reduction order
    plus the sweep count's own cost of one, not tuned.  x agrees with 1 as in the existing ILU solve tests at this rtol."""
    L = P.lib()
    ai, aj, aa = p7_31(P)
    n = ai.size - 1
    u = np.ones(n)
    b = orc.spmv(ai, aj, aa, u)
    A = P.Mat.from_csr(ai, aj, aa)
    its = {}
    for name, opts in (("sweeps:3", "-pc_type ilu -pc_factor_hipmi355x_trisolve sweeps:3"), ("exact", "-pc_type ilu"), ("jacobi", "-pc_type jacobi")):
        k = P.KSP(comm=L.COMM_SELF); k.set_operators(A)
        L.PetscOptionsClear(); L.PetscOptionsInsertString(("-ksp_type gmreshipmi355x -ksp_gmres_restart 30 " + opts).encode())
        k.set_tolerances(rtol=1e-8); k.set_from_options()
        vb, vx = V(P, b), V(P, np.zeros(n))
        k.solve(vb, vx)
        L.PetscOptionsClear()
        assert k.reason == 2, (name, k.reason)
        its[name] = k.its
        if name == "sweeps:3":
            pc = C.c_void_p(); L.KSPGetPC(k.h, C.byref(pc))
            got = C.c_int(-1); L.PCILUGetSweeps_HIPMI355X(pc, C.byref(got)); assert got.value == 3
            x = vx.array()
    print("GMRES(30) iterations:", its)
    assert its["sweeps:3"] < its["jacobi"]
    assert its["sweeps:3"] <= its["exact"] + 4
    assert np.linalg.norm(x - u) <= 1e-6 * np.linalg.norm(u)


# ---------------------------------------------------------------- 5. long rows and nodes
def test_three_dof_matrix_with_inodes_long_rows_and_no_node_plans(P):
    """the small FEM generator (3 dof per node, rows of the triangles too long for one lane each): k >= levels - 1 sweeps agree
    with the natural-ordering solve to 1e-13 relative, the project's tolerance where rows are summed by a lane tree; the
    sweep form builds no node plans"""
    L = P.lib()
    ai, aj, aa = pb.gen_fem3(7, 6, 5)
    n = ai.size - 1
    assert orc.check_inode(ai, aj)[0] > 0
    A = P.Mat.from_csr(ai, aj, aa)
    nl, nu = levels_of(P, A)
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:%d" % (max(nl, nu) - 1))
    assert rc == 0
    nn, a, b_ = C.c_int(-1), C.c_int(), C.c_int(); L.PCILUGetNodeInfo_HIPMI355X(pc, C.byref(nn), C.byref(a), C.byref(b_))
    assert nn.value == 0
    f = orc.ilu0_factor(ai, aj, aa)
    for rep in range(2):
        b = rnd(n, 90 + rep)
        x, ref = apply(P, pc, b), orc.ilu0_solve(f, b)
        rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
        print("fem3 n=%d levels %d/%d: relative distance from the natural-ordering solve %.3g" % (n, nl, nu, rel))
        assert rel <= 1e-13
        assert np.array_equal(bits(apply(P, pc, b)), bits(x))                 # deterministic


# ---------------------------------------------------------------- 6. block Jacobi and re-factorisation
def block_diagonal(ai, aj, aa, nblk):
    """the matrix block Jacobi with nblk equal blocks factors: couplings between blocks dropped"""
    n = ai.size - 1
    assert n % nblk == 0
    rows = np.repeat(np.arange(n), np.diff(ai))
    keep = (rows // (n // nblk)) == (aj // (n // nblk))
    bi = np.zeros(n + 1, np.int32); np.add.at(bi, rows[keep] + 1, 1)
    return np.cumsum(bi).astype(np.int32), aj[keep].copy(), aa[keep].copy()


def test_block_jacobi_and_a_second_factorisation_with_new_values(P):
    """four local blocks factored as one block-diagonal matrix ("MatFactorSetIndependentBlocks_C"); the option under the sub-PC's
    prefix.  Block Jacobi sets its block solver up at the first application, so the options stay in place until after it."""
    L = P.lib()
    ai, aj, aa = p7_31(P)
    n = ai.size - 1
    A = P.Mat.from_csr(ai, aj, aa)
    nl, nu = levels_of(P, A)                                   # a block's dependencies are a subset of the whole matrix's
    k = max(nl, nu) - 1
    base = "-pc_bjacobi_blocks 4 -sub_pc_type ilu"

    def bjacobi(opts, b, ksp=None, pc=None):
        """set up (again, when ksp and pc are given) under the options and apply once"""
        if ksp is None:
            pc = C.c_void_p()
            ksp = P.KSP(comm=L.COMM_SELF); L.KSPGetPC(ksp.h, C.byref(pc)); L.PCSetType(pc, b"bjacobi")
        ksp.set_operators(A)
        L.PetscOptionsClear(); L.PetscOptionsInsertString(opts.encode())
        assert L.raw("PCSetUp")(pc) == 0
        x = apply(P, pc, b)
        L.PetscOptionsClear()
        return ksp, pc, x

    def sub_sweeps(pc):
        nloc, first, sub = C.c_int(), C.c_int(), C.c_void_p()
        L.PCBJacobiGetSubKSP(pc, C.byref(nloc), C.byref(first), C.byref(sub))
        spc, got = C.c_void_p(), C.c_int(-1)
        L.KSPGetPC(C.cast(sub, C.POINTER(C.c_void_p))[0], C.byref(spc))
        L.PCILUGetSweeps_HIPMI355X(spc, C.byref(got))
        return nloc.value, got.value

    b = rnd(n, 120)
    ks, pcs, xs = bjacobi(base + " -sub_pc_factor_hipmi355x_trisolve sweeps:%d" % k, b)
    ke, pce, xe = bjacobi(base, b)
    assert sub_sweeps(pcs) == (4, k) and sub_sweeps(pce) == (4, 0)
    assert np.array_equal(bits(xs), bits(xe))
    di, dj, da = block_diagonal(ai, aj, aa, 4)
    assert np.array_equal(bits(xs), bits(orc.ilu0_solve(orc.ilu0_factor(di, dj, da), b)))
    # new values in the same pattern (rows scaled on the device), the operators announced again, a second set-up
    dl = 1.0 + 0.3 * np.cos(np.arange(n))
    vl = V(P, dl)
    L.MatDiagonalScale(A.h, vl.h, None)
    aa2 = aa * np.repeat(dl, np.diff(ai))
    di, dj, da2 = block_diagonal(ai, aj, aa2, 4)
    f2 = orc.ilu0_factor(di, dj, da2)
    ks, pcs, x2 = bjacobi(base + " -sub_pc_factor_hipmi355x_trisolve sweeps:%d" % k, b, ks, pcs)
    assert sub_sweeps(pcs) == (4, k)
    assert np.array_equal(bits(x2), bits(orc.ilu0_solve(f2, b))) and not np.array_equal(bits(x2), bits(xs))
    b = rnd(n, 121)
    assert np.array_equal(bits(apply(P, pcs, b)), bits(orc.ilu0_solve(f2, b)))
    # the same for a plain PCILU: second numeric factorisation, values only
    A1 = P.Mat.from_csr(ai, aj, aa)
    k1, pc1, rc = ilu_pc(P, A1, "-pc_factor_hipmi355x_trisolve sweeps:%d" % k)
    assert rc == 0
    assert np.array_equal(bits(apply(P, pc1, b)), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa), b)))
    L.MatDiagonalScale(A1.h, vl.h, None)
    k1.set_operators(A1)
    L.PetscOptionsClear(); L.PetscOptionsInsertString(("-pc_factor_hipmi355x_trisolve sweeps:%d" % k).encode())
    assert L.raw("PCSetUp")(pc1) == 0
    L.PetscOptionsClear()
    assert np.array_equal(bits(apply(P, pc1, b)), bits(orc.ilu0_solve(orc.ilu0_factor(ai, aj, aa2), b)))
    got = C.c_int(-1); L.PCILUGetSweeps_HIPMI355X(pc1, C.byref(got)); assert got.value == k


# ---------------------------------------------------------------- 7. bad arguments
@pytest.mark.parametrize("mode", ["sweeps", "sweeps:", "sweeps:0", "sweeps:x", "sweeps:-2", "sweeps:3x", "sweep:3"])
def test_a_missing_or_malformed_sweep_count_is_refused(P, mode):
    ai, aj, aa = pb.lap2d(9, 7)
    A = P.Mat.from_csr(ai, aj, aa)
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve " + mode)
    assert rc == ARG_WRONG
    ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:1")      # (and the well-formed one is taken)
    assert rc == 0


# ---------------------------------------------------------------- 8. b == x
def test_input_and_result_in_one_vector(P):
    """The sweep form's iterates live in work vectors: b is read by the lower sweeps only and x is written after them, so one
    vector may be both.  PCApply itself refuses identical vectors here exactly as the reference's does (precon.c:380, and
    MatSolve, matrix.c:3205) -- that contract is not this option's to change, so PCApply(pc, v, v) stays error 61 and the
    in-place application is reached through PCILUApplyInPlace_HIPMI355X, which hands ONE vector to the same routine as b and x."""
    L = P.lib()
    ai, aj, aa = p7_31(P)
    n = ai.size - 1
    A = P.Mat.from_csr(ai, aj, aa)
    f = orc.ilu0_factor(ai, aj, aa)
    for k in (30, 3, 4):                                        # exact; odd and even counts (the result alternates between buffers)
        ksp, pc, rc = ilu_pc(P, A, "-pc_factor_hipmi355x_trisolve sweeps:%d" % k)
        assert rc == 0
        b = rnd(n, 130 + k)
        want = apply(P, pc, b)                                  # two vectors
        v = V(P, b)
        L.PCILUApplyInPlace_HIPMI355X(pc, v.h)
        assert np.array_equal(bits(v.array()), bits(want))
        if k == 30:
            assert np.array_equal(bits(want), bits(orc.ilu0_solve(f, b)))
        assert L.raw("PCApply")(pc, v.h, v.h) == ARG_IDN
    ksp, pc, rc = ilu_pc(P, A, "")                              # the exact solves are not offered in place
    assert rc == 0 and L.raw("PCILUApplyInPlace_HIPMI355X")(pc, v.h) == 56
