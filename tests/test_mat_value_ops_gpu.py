"""MatShift / MatAXPY / MatCopy on the device copy of AIJ matrices: host and device copies updated side by side, no
re-upload, the derived forms following by a gather.  Expected values are computed in numpy (`cur[diag] += a` and
`cur[xtoy] += a * xa` are separate ufuncs: two roundings); comparisons are bit for bit unless said otherwise.  The last grid runs
every operator that updates values in place (MatScale, MatZeroEntries, MatDiagonalScale and the zero-rows pair included) through the
three states of the device copy."""
import ctypes as C

import numpy as np
import pytest

import orc
import problems as pb
import vecspecials as vs
from gpu import Dev, ksp_type_for
from test_mat_value_ops_cpu import drop_entries, host_values, host_pattern

pytestmark = pytest.mark.gpu
ARG_WRONG, ERR_SUP = 62, 56


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def V(P, a):
    return P.Vec.from_array(a, comm=P.lib().COMM_SELF)


def uploads(P, A):
    n = C.c_int(-1)
    P.lib().MatHIPMI355XGetUploadCount(A.h, C.byref(n))
    return n.value


def tcounts(P, A):
    b, r = C.c_int(-1), C.c_int(-1)
    P.lib().MatHIPMI355XGetTransposeCounts(A.h, C.byref(b), C.byref(r))
    return b.value, r.value


def vpatterns(P, A):
    n = C.c_int(-1)
    P.lib().MatHIPMI355XGetValuePatterns(A.h, C.byref(n))
    return n.value


class Case:
    """Y (the matrix updated), Z (Y's pattern, other values) and X (a subset of the pattern) with the numpy side of every update"""

    def __init__(self, ai, aj, aa, exact=True):
        self.ai, self.aj, self.aa, self.exact = ai, aj, aa, exact
        self.n = ai.size - 1
        rows = np.repeat(np.arange(self.n), np.diff(ai))
        self.diag = np.flatnonzero(rows == aj)
        assert self.diag.size == self.n
        self.za = np.cos(np.arange(aa.size)) - 0.3
        self.xi, self.xj, self.xa, self.xtoy = drop_entries(ai, aj, aa)
        self.x = np.cos(0.3 * np.arange(self.n))

    def mats(self, P):
        return P.Mat.from_csr(self.ai, self.aj, self.aa), P.Mat.from_csr(self.ai, self.aj, self.za), P.Mat.from_csr(self.xi, self.xj, self.xa)

    def apply(self, P, op, Y, Z, X, cur):
        """one update of Y through the library and of cur in numpy"""
        cur = cur.copy()
        if op == "shift":
            Y.shift(0.37); cur[self.diag] += 0.37
        elif op == "same":
            Y.axpy(-1.3, Z, P.SAME_NONZERO_PATTERN); cur = cur + (-1.3) * self.za
        elif op == "self":                                   # X == Y is allowed: on the device an in-place vec_axpy(x = y)
            Y.axpy(0.7, Y, P.SAME_NONZERO_PATTERN); cur = cur + 0.7 * cur
        elif op == "subset":
            Y.axpy(0.25, X, P.SUBSET_NONZERO_PATTERN); cur[self.xtoy] += 0.25 * self.xa
        elif op == "different":
            Y.axpy(0.25, X, P.DIFFERENT_NONZERO_PATTERN); cur[self.xtoy] += 0.25 * self.xa
        elif op == "copy":
            Z.copy(Y, P.SAME_NONZERO_PATTERN); cur = self.za.copy()
        elif op == "copy_basic":
            X.copy(Y, P.DIFFERENT_NONZERO_PATTERN); cur = np.zeros(cur.size); cur[self.xtoy] += 1.0 * self.xa
        else:
            raise AssertionError(op)
        return cur

    def check(self, P, A, vals, vx, vy, what, transpose=True):
        L = P.lib()
        A.mult(vx, vy)
        if self.exact:
            assert np.array_equal(bits(vy.array()), bits(orc.matmult(self.ai, self.aj, vals, self.x)[0])), what
        else:
            # a form whose row sums take another order than the reference's (the blocked companion of rows longer than 16): the bits
            # of a matrix assembled from the same values and sent to the device, and the reference to the bound of a sum of
            # `width` terms in any order, width * eps * sum |a_ij x_j|
            got = vy.array().copy()
            F = P.Mat.from_csr(self.ai, self.aj, vals)
            F.mult(vx, vy)
            assert np.array_equal(bits(got), bits(vy.array())), what
            F.destroy()
            width = int(np.diff(self.ai).max())
            bound = width * 2.220446049250313e-16 * orc.matmult(self.ai, self.aj, np.abs(vals), np.abs(self.x))[0]
            assert np.all(np.abs(got - orc.matmult(self.ai, self.aj, vals, self.x)[0]) <= bound), what
        L.MatGetDiagonal(A.h, vy.h)
        assert np.array_equal(bits(vy.array()), bits(orc.get_diagonal(self.ai, self.aj, vals))), what
        if transpose:
            L.MatMultTranspose(A.h, vx.h, vy.h)
            assert np.allclose(vy.array(), orc.spmv_t(self.ai, self.aj, vals, self.x, self.n), rtol=0, atol=1e-12), what
        assert np.array_equal(bits(host_values(P, A, vals.size)), bits(vals)), what + ": host copy"


OPS = ("shift", "same", "self", "subset", "different", "copy", "copy_basic")


def perturbed(csr):
    ai, aj, aa = csr
    return ai.astype(np.int32), aj.astype(np.int32), aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))


@pytest.fixture(scope="module")
def cases():
    return {"lap2d": Case(*perturbed(pb.lap2d(23, 19))), "p7": Case(*perturbed(orc.gen_p7(11, 9, 7)))}


@pytest.mark.parametrize("name", ["lap2d", "p7"])
def test_each_update_used_first_and_not(P, cases, name):
    """1. every operation after the matrix has been used on the device (device-side update: no upload) and before (host update, one
    upload at the first use)"""
    c = cases[name]
    L = P.lib()
    assert c.n in (437, 693)
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))
    for op in OPS:
        for used_first in (True, False):
            Y, Z, X = c.mats(P)
            what = "%s %s used_first=%s" % (name, op, used_first)
            if used_first:
                Y.mult(vx, vy); L.MatMultTranspose(Y.h, vx.h, vy.h)
                if op == "copy":
                    Z.mult(vx, vy)
            cur = c.apply(P, op, Y, Z, X, c.aa)
            c.check(P, Y, cur, vx, vy, what)
            assert uploads(P, Y) == 1, "%s: Y's values crossed %d times" % (what, uploads(P, Y))
            if used_first:
                assert tcounts(P, Y) == (1, 1), what
                src = {"same": Z, "copy": Z, "subset": X, "different": X, "copy_basic": X}.get(op)
                if src is not None:
                    assert uploads(P, src) == 1, "%s: the source is read on the device: one use" % what
            for o in (Y, Z, X):
                o.destroy()


def run_sequence(P, c, opts, vx, vy, transpose=True, before=None, between=None):
    """all updates on one matrix after a first use; the products' bits after every update"""
    L = P.lib()
    L.PetscOptionsClear()
    if opts:
        L.PetscOptionsInsertString(opts.encode())
    try:
        Y, Z, X = c.mats(P)
        Y.mult(vx, vy)
        if transpose:
            L.MatMultTranspose(Y.h, vx.h, vy.h)
        if before:
            before(Y)
        cur, out = c.aa, []
        for op in OPS:
            cur = c.apply(P, op, Y, Z, X, cur)
            if between:
                between(Y, op)
            c.check(P, Y, cur, vx, vy, "%s after %s" % (opts, op), transpose)
            Y.mult(vx, vy)
            out.append(vy.array().copy())
        return Y, out
    finally:
        L.PetscOptionsClear()


def test_update_on_device_0_is_the_route_through_an_upload(P, cases):
    """2. -mat_hipmi355x_update_on_device 0: the same product bits, one upload per update"""
    c = cases["p7"]
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))
    Y1, on = run_sequence(P, c, "", vx, vy)
    Y0, off = run_sequence(P, c, "-mat_hipmi355x_update_on_device 0", vx, vy)
    for a, b in zip(on, off):
        assert np.array_equal(bits(a), bits(b))
    assert uploads(P, Y1) == 1
    assert uploads(P, Y0) == 1 + len(OPS)
    assert tcounts(P, Y1) == (1, len(OPS))


def test_derived_forms_follow(P, cases):
    """3. the column-tiled layout, the blocked companion and the value-pattern dictionary after device-side updates"""
    L = P.lib()
    c = cases["p7"]
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))

    def tiled(Y):
        s, r = C.c_int(), C.c_int()
        L.MatHIPMI355XGetTiledInfo(Y.h, C.byref(s), C.byref(r))
        assert s.value + r.value == c.aj.size, "the column-tiled layout was not taken"
    Y, _ = run_sequence(P, c, "-mat_hipmi355x_tiled 1 -mat_hipmi355x_index_compression 0", vx, vy, before=tiled)
    assert uploads(P, Y) == 1 and tcounts(P, Y) == (1, len(OPS))
    # a 3-dof matrix through its blocked companion
    (ai, aj, aa), _ = pb.elasticity_like(6, 5, 4)
    cb = Case(ai.astype(np.int32), aj.astype(np.int32), aa, exact=False)
    assert cb.n == 360
    bx, by = V(P, cb.x), V(P, np.zeros(cb.n))

    def blocked(Y):
        bs, nb = C.c_int(), C.c_int()
        L.MatHIPMI355XGetBlockedInfo(Y.h, C.byref(bs), C.byref(nb))
        assert bs.value == 3 and nb.value * 9 == cb.aj.size
    Y, _ = run_sequence(P, cb, "-mat_hipmi355x_blocked 1", bx, by, before=blocked)
    assert uploads(P, Y) == 1
    assert tcounts(P, Y) == (0, 0)           # the companion's block transpose is a gather form of its own: no scalar transpose is ever built
    # constant coefficients: the dictionary describes the old values and is dropped by the update
    cc = Case(*[np.ascontiguousarray(a) for a in orc.gen_p7(11, 9, 7)])

    def has_dictionary(Y):
        assert vpatterns(P, Y) == 27

    def dropped(Y, op):
        assert vpatterns(P, Y) == 0, op
    Y, _ = run_sequence(P, cc, "", vx, vy, before=has_dictionary, between=dropped)
    assert uploads(P, Y) == 1 and tcounts(P, Y) == (1, len(OPS))


SPECIAL_ALPHAS = [0.0, -0.0, np.inf, -np.inf, np.nan, 4.9406564584124654e-324, -2.5e-310]


def test_ieee_specials_and_guard_bands(P, dev, cases):
    """4. alpha in {+-0, +-inf, NaN, denormal}, values holding +-inf, NaN and -0; the kernels through the C ABI on guarded value arrays
    (both alignments), then the operators: a == 0 leaves Y's bits alone with SAME and does the arithmetic with SUBSET"""
    c = cases["lap2d"]
    k = dev.k
    nz = c.aj.size
    dai, daj = dev.put(c.ai), dev.put(c.aj)
    dmap = dev.put(c.xtoy)
    dmiss = dev.put(np.array([77], np.int32))
    with np.errstate(all="ignore"):
        for rot, alpha in enumerate(SPECIAL_ALPHAS + [0.37]):
            for off in (0, 1):
                ya = vs.special_vector(nz, 1, vs.SHARE, rot)
                xa = vs.special_vector(c.xa.size, 2, vs.SHARE, rot)
                gy = vs.guarded(dev, ya, off, tag=1)
                dev.chk(k.mi355x_csr_shift(dev.h, c.n, dai, daj, alpha, gy.ptr, dmiss))
                ref = ya.copy(); ref[c.diag] = ref[c.diag] + alpha
                vs.same(gy.get(), ref, "shift alpha=%r" % alpha)
                assert dev.get(dmiss, 1, np.int32)[0] == 0
                gx = vs.guarded(dev, xa, 1 - off, tag=2)
                dev.chk(k.mi355x_csr_axpy_map(dev.h, xa.size, dmap, alpha, gx.ptr, gy.ptr))
                ref[c.xtoy] = ref[c.xtoy] + alpha * xa
                vs.same(gy.get(), ref, "axpy_map alpha=%r" % alpha)
                dev.chk(k.mi355x_csr_axpy_map(dev.h, 0, dmap, alpha, gx.ptr, gy.ptr))      # nzx = 0
                dev.chk(k.mi355x_csr_axpy_map(dev.h, 1, dmap, 2.0, gx.ptr, gy.ptr))        # one entry: the rest of the workgroup idle
                ref[c.xtoy[0]] = ref[c.xtoy[0]] + 2.0 * xa[0]
                vs.same(gy.get(), ref, "axpy_map of one entry")
                vs.guards_intact(gy, gx, names=["ya", "xa"])
                gy.free(); gx.free()
    # rows without a diagonal entry are counted and not touched: X's pattern lacks some
    xrows = np.repeat(np.arange(c.n), np.diff(c.xi))
    missing = c.n - int(np.sum(xrows == c.xj))
    assert missing > 3
    dxi, dxj = dev.put(c.xi), dev.put(c.xj)
    gx = vs.guarded(dev, c.xa, 1, tag=3)
    dev.chk(k.mi355x_csr_shift(dev.h, c.n, dxi, dxj, 1.5, gx.ptr, dmiss))
    ref = c.xa.copy(); ref[xrows == c.xj] += 1.5
    vs.same(gx.get(), ref, "shift with missing diagonals")
    assert dev.get(dmiss, 1, np.int32)[0] == missing
    vs.guards_intact(gx)
    # the operators
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))
    with np.errstate(all="ignore"):
        for rot, alpha in enumerate(SPECIAL_ALPHAS):
            ya = vs.special_vector(nz, 3, vs.SHARE, rot); za = vs.special_vector(nz, 4, vs.SHARE, rot); xa = vs.special_vector(c.xa.size, 5, vs.SHARE, rot)
            Y = P.Mat.from_csr(c.ai, c.aj, ya); Z = P.Mat.from_csr(c.ai, c.aj, za); X = P.Mat.from_csr(c.xi, c.xj, xa)
            Y.mult(vx, vy)
            cur = ya.copy()
            Y.shift(alpha); cur[c.diag] = cur[c.diag] + alpha
            Y.axpy(alpha, Z, P.SAME_NONZERO_PATTERN)
            if alpha != 0.0:
                cur = cur + alpha * za
            Y.axpy(alpha, X, P.SUBSET_NONZERO_PATTERN); cur[c.xtoy] = cur[c.xtoy] + alpha * xa
            vs.same(host_values(P, Y, nz), cur, "host copy, alpha=%r" % alpha)
            L = P.lib()
            L.MatGetDiagonal(Y.h, vy.h)
            vs.same(vy.array(), cur[c.diag], "device diagonal, alpha=%r" % alpha)
            assert uploads(P, Y) == 1
            for o in (Y, Z, X):
                o.destroy()
    # a == 0: SAME leaves the bits (-0 stays -0), SUBSET adds 0 * x
    ya = vs.special_vector(nz, 6, vs.SHARE); xa = vs.special_vector(c.xa.size, 7, vs.SHARE)
    Y = P.Mat.from_csr(c.ai, c.aj, ya); Z = P.Mat.from_csr(c.ai, c.aj, np.full(nz, np.inf)); X = P.Mat.from_csr(c.xi, c.xj, xa)
    Y.mult(vx, vy)
    Y.axpy(0.0, Z, P.SAME_NONZERO_PATTERN)
    assert np.array_equal(bits(host_values(P, Y, nz)), bits(ya))
    with np.errstate(all="ignore"):
        Y.axpy(0.0, X, P.SUBSET_NONZERO_PATTERN)
        cur = ya.copy(); cur[c.xtoy] = cur[c.xtoy] + 0.0 * xa
    vs.same(host_values(P, Y, nz), cur, "SUBSET with a == 0")
    assert vs.differing(cur, ya).any()
    P.lib().MatGetDiagonal(Y.h, vy.h)
    vs.same(vy.array(), cur[c.diag], "SUBSET with a == 0 on the device")
    assert uploads(P, Y) == 1


def test_errors_and_fallbacks(P, cases):
    """5. refused claims leave Y alone on host and device; a missing diagonal entry and BAIJ take the host route"""
    L = P.lib()
    c = cases["lap2d"]
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))
    Y, Z, X = c.mats(P)
    Y.mult(vx, vy); X.mult(vx, vy)
    ref_y = vy.array().copy()
    for call, code in ((lambda: Y.axpy(1.0, X, P.SAME_NONZERO_PATTERN), ARG_WRONG), (lambda: X.axpy(1.0, Y, P.SUBSET_NONZERO_PATTERN), ARG_WRONG),
                       (lambda: X.axpy(1.0, Y, P.DIFFERENT_NONZERO_PATTERN), ERR_SUP), (lambda: Y.copy(X, P.DIFFERENT_NONZERO_PATTERN), ARG_WRONG)):
        with pytest.raises(P.PetscError) as e:
            call()
        assert e.value.code == code, str(e.value)
    assert np.array_equal(bits(host_values(P, X, c.xa.size)), bits(c.xa))
    X.mult(vx, vy)
    assert np.array_equal(bits(vy.array()), bits(ref_y)) and uploads(P, X) == 1 and uploads(P, Y) == 1
    # MatShift on a matrix some rows of which lack the diagonal entry: the reference's loop of MatSetValues, the entries inserted
    X.shift(2.5)
    gi, gj = host_pattern(P, X)
    import scipy.sparse as sp
    S = sp.csr_matrix((c.xa, c.xj, c.xi), shape=(c.n, c.n)) + sp.csr_matrix((np.full(c.n, 2.5), (np.arange(c.n), np.arange(c.n))), shape=(c.n, c.n))
    S.sort_indices()
    assert np.array_equal(gi, S.indptr) and np.array_equal(gj, S.indices)
    assert np.array_equal(bits(host_values(P, X, S.data.size)), bits(S.data))
    X.mult(vx, vy)
    assert np.array_equal(bits(vy.array()), bits(orc.matmult(S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data, c.x)[0]))
    X.shift(-1.0)                                           # every row has its entry now: the device route
    X.mult(vx, vy)
    d = S.data.copy(); rows = np.repeat(np.arange(c.n), np.diff(S.indptr)); d[rows == S.indices] += -1.0
    assert np.array_equal(bits(vy.array()), bits(orc.matmult(S.indptr.astype(np.int32), S.indices.astype(np.int32), d, c.x)[0]))
    assert uploads(P, X) == 2
    # BAIJ bs = 3
    bs = 3
    bi, bj, _ = pb.lap2d(6, 5)
    nb = bj.size
    ba = np.cos(0.1 * np.arange(nb * bs * bs)); bb = np.sin(0.2 * np.arange(nb * bs * bs))
    A = P.Mat.from_bsr(bs, bi, bj, ba); B = P.Mat.from_bsr(bs, bi, bj, bb)
    xb = np.cos(0.3 * np.arange(30 * bs)); bx, by = V(P, xb), V(P, np.zeros(30 * bs))
    A.mult(bx, by)
    brow = np.repeat(np.arange(bi.size - 1), np.diff(bi))
    cur = ba.copy()
    A.shift(0.75)
    for k in np.flatnonzero(brow == bj):
        for q in range(bs):
            cur[k * bs * bs + q * bs + q] += 0.75
    A.axpy(-0.3, B, P.SAME_NONZERO_PATTERN); cur = cur + (-0.3) * bb
    # the BCSR kernel sums a row in its own order: the bits of a matrix built from the same values, and the reference to the bound of
    # a sum of (blocks per row) * bs terms in any order
    F = P.Mat.from_bsr(bs, bi, bj, cur)
    F.mult(bx, by)
    fresh = by.array().copy()
    bound = int(np.diff(bi).max()) * bs * 2.220446049250313e-16 * orc.spmv_bsr(bs, bi, bj, np.abs(cur), np.abs(xb))
    assert np.all(np.abs(fresh - orc.spmv_bsr(bs, bi, bj, cur, xb)) <= bound)
    A.mult(bx, by)
    assert np.array_equal(bits(by.array()), bits(fresh))
    assert np.array_equal(bits(host_values(P, A, cur.size)), bits(cur))
    A.copy(B, P.SAME_NONZERO_PATTERN)
    B.mult(bx, by)
    assert np.array_equal(bits(by.array()), bits(fresh))


def test_mpiaij_on_one_rank(P, cases):
    """6. MPIAIJ on one rank: the operators go through the blocks; MatMult equals the sequential matrix's after the same updates.
    (Two staged ranks with differing garrays: the host copies in tests/test_mat_value_ops_cpu.py; the multi-rank GPU launcher starts
    torch.distributed.run with a script of its own and is not used here.)"""
    c = cases["p7"]
    L = P.lib()
    vx, vy = V(P, c.x), V(P, np.zeros(c.n))
    mk = lambda i, j, a: P.Mat.from_csr_mpi(i, j, a, c.n, c.n, c.n, comm=L.COMM_SELF)   # noqa: E731
    for used_first in (True, False):
        Y, Z, X = mk(c.ai, c.aj, c.aa), mk(c.ai, c.aj, c.za), mk(c.xi, c.xj, c.xa)
        if used_first:
            Y.mult(vx, vy)
        cur = c.aa
        for op in OPS:
            cur = c.apply(P, op, Y, Z, X, cur)
            Y.mult(vx, vy)
            assert np.array_equal(bits(vy.array()), bits(orc.matmult(c.ai, c.aj, cur, c.x)[0])), (op, used_first)
        Ad = C.c_void_p()
        L.MatMPIAIJGetSeqAIJ(Y.h, C.byref(Ad), None, None)
        assert uploads(P, P.Mat(Ad, own=False)) == 1


def test_mpiaij_two_staged_ranks(built):
    """6. two ranks sharing the GPU over the host-staged transport (the launcher of tests/test_multirank_gpu.py): shift, SAME, SUBSET
    with X's garray shorter than Y's, copy; MatMult bit for bit the split of the sequential result on every rank"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(root, "tests", "tools", "mat_value_ops_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    for k in range(2):
        m = re.search(r"rank %d/2: MatShift, MatAXPY SAME / SUBSET, MatCopy of MPIAIJ then MatMult bitexact=True garray lengths X (\d+) Y (\d+)" % k, out)
        assert m, out[-3000:]
        assert 0 < int(m.group(1)) < int(m.group(2)), "the run wants X's garray shorter than Y's: %s" % m.group(0)


class Tri70:
    """a 70-row tridiagonal whose row 66 has only its diagonal: two row blocks of a 64-wide wavefront, the second partly idle"""
    n, lone, listed = 70, 66, np.array([2, 63, 64, 66], np.int32)

    def __init__(self):
        cols = [[r] if r == self.lone else [c for c in (r - 1, r, r + 1) if 0 <= c < self.n] for r in range(self.n)]
        self.ai = np.concatenate([[0], np.cumsum([len(q) for q in cols])]).astype(np.int32)
        self.aj = np.concatenate(cols).astype(np.int32)
        self.rows = np.repeat(np.arange(self.n), np.diff(self.ai))
        self.diag = np.flatnonzero(self.rows == self.aj)
        nz = self.aj.size
        self.aa = 2.0 + np.sin(np.arange(nz))
        self.za = np.cos(np.arange(nz)) - 0.3
        self.xa = 0.5 + 0.01 * np.arange(self.n)                        # X: the diagonal alone, a subset of the pattern
        self.x, self.l, self.r = np.cos(0.3 * np.arange(self.n)), 1.0 + 0.1 * np.cos(np.arange(self.n)), 1.0 + 0.1 * np.sin(np.arange(self.n))

    def apply(self, P, op, Y, Z, X, cur):
        """one update of Y through the library and of cur in numpy"""
        L = P.lib()
        cur = cur.copy()
        in_list = np.isin(self.rows, self.listed)
        if op == "scale":
            L.MatScale(Y.h, -0.37); cur = -0.37 * cur
        elif op == "zero_entries":
            L.MatZeroEntries(Y.h); cur = np.zeros(cur.size)
        elif op == "diagonal_scale":
            vl, vr = V(P, self.l), V(P, self.r)
            L.MatDiagonalScale(Y.h, vl.h, vr.h); cur = (cur * self.l[self.rows]) * self.r[self.aj]
        elif op == "shift":
            Y.shift(0.37); cur[self.diag] += 0.37
        elif op == "axpy_same":
            Y.axpy(-1.3, Z, P.SAME_NONZERO_PATTERN); cur = cur + (-1.3) * self.za
        elif op == "axpy_subset":
            Y.axpy(0.25, X, P.SUBSET_NONZERO_PATTERN); cur[self.diag] += 0.25 * self.xa
        elif op == "copy":
            Z.copy(Y, P.SAME_NONZERO_PATTERN); cur = self.za.copy()
        elif op in ("zero_rows", "zero_rows_columns"):
            if op == "zero_rows":
                Y.zero_rows(self.listed, 2.0)
            else:
                Y.zero_rows_columns(self.listed, 2.0); cur[np.isin(self.aj, self.listed)] = 0.0
            cur[in_list] = 0.0; cur[self.diag[self.listed]] = 2.0
        else:
            raise AssertionError(op)
        return cur


VALUE_UPDATES = ("scale", "zero_entries", "diagonal_scale", "shift", "axpy_same", "axpy_subset", "copy", "zero_rows", "zero_rows_columns")
ASK_THE_OPTION = ("shift", "axpy_same", "axpy_subset", "copy", "zero_rows", "zero_rows_columns")


@pytest.mark.parametrize("state", ["current", "host_newer", "option_0"])
@pytest.mark.parametrize("op", VALUE_UPDATES)
def test_the_device_step_of_every_value_update(P, op, state):
    """8. every operator that updates the values in place, in three states of the device copy: current (the update runs on it: no
    upload), the host copy newer (MatSetValues and an assembly since the last use: the host copy alone is updated and the next use
    sends it -- but MatCopy, which asks for the target's device arrays, not for its values, overwrites them there), and
    -mat_hipmi355x_update_on_device 0 under the matrix's prefix (the operators that ask the option update the host copy alone)"""
    L = P.lib()
    t = Tri70()
    vx, vy = V(P, t.x), V(P, np.zeros(t.n))
    L.PetscOptionsClear()
    try:
        Y, Z, X = P.Mat.from_csr(t.ai, t.aj, t.aa), P.Mat.from_csr(t.ai, t.aj, t.za), P.Mat.from_csr(np.arange(t.n + 1, dtype=np.int32), np.arange(t.n, dtype=np.int32), t.xa)
        Y.set_option(P.MAT_KEEP_NONZERO_PATTERN)
        if state == "option_0":
            L.MatSetOptionsPrefix(Y.h, b"vu_")
            L.PetscOptionsSetValue(b"-vu_mat_hipmi355x_update_on_device", b"0")
            L.MatSetFromOptions(Y.h)
        Y.mult(vx, vy)
        cur = t.aa.copy()
        if state == "host_newer":
            i, v = np.array([3], np.int32), np.array([7.25])
            L.MatSetValues(Y.h, 1, i.ctypes.data, 1, i.ctypes.data, v.ctypes.data, P.INSERT_VALUES)
            L.MatAssemblyBegin(Y.h, P.MAT_FINAL_ASSEMBLY); L.MatAssemblyEnd(Y.h, P.MAT_FINAL_ASSEMBLY)
            cur[t.diag[3]] = 7.25
        assert uploads(P, Y) == 1
        cur = t.apply(P, op, Y, Z, X, cur)
        assert uploads(P, Y) == 1, "the update itself sends nothing"
        assert np.array_equal(bits(host_values(P, Y, cur.size)), bits(cur)), "host copy"
        Y.mult(vx, vy)
        assert np.array_equal(bits(vy.array()), bits(orc.matmult(t.ai, t.aj, cur, t.x)[0]))
        on_device = {"current": True, "host_newer": op == "copy", "option_0": op not in ASK_THE_OPTION}[state]
        assert uploads(P, Y) == (1 if on_device else 2)
    finally:
        L.PetscOptionsClear()


@pytest.mark.parametrize("tri", ["", "-pc_factor_hipmi355x_trisolve sweeps:3"])
def test_the_time_stepping_loop(P, cases, tri):
    """7. A <- M, A += dt K, A += sigma I, refactor on the device, solve: four steps equal to a freshly assembled matrix each, with A's
    values never crossing again"""
    L = P.lib()
    c = cases["p7"]
    opts = "-ksp_type %s -pc_type ilu -pc_factor_hipmi355x_numeric device -ksp_rtol 1e-10 %s" % (ksp_type_for("gmres"), tri)
    b = np.sin(0.1 * np.arange(c.n)) + 1.0

    def solver(A):
        k = P.KSP(comm=L.COMM_SELF)
        L.KSPSetOperators(k.h, A.h, A.h, P.SAME_NONZERO_PATTERN)
        L.PetscOptionsClear(); L.PetscOptionsInsertString(opts.encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.record_history()
        return k

    def solve(k):
        vb, vx = V(P, b), V(P, np.zeros(c.n))
        L.PetscOptionsInsertString(opts.encode())
        try:
            k.solve(vb, vx)
        finally:
            L.PetscOptionsClear()
        return vx.array().copy(), k.history()

    M, K = P.Mat.from_csr(c.ai, c.aj, c.aa), P.Mat.from_csr(c.xi, c.xj, c.xa)
    A = P.Mat.from_csr(c.ai, c.aj, c.za)
    k = solver(A)
    vx0, vy0 = V(P, c.x), V(P, np.zeros(c.n))
    A.mult(vx0, vy0)                                        # the first use
    up0 = uploads(P, A)
    assert up0 == 1
    for step, (dt, sigma) in enumerate(((0.01, 0.5), (0.02, 0.25), (0.005, 1.0), (0.04, 0.125))):
        M.copy(A, P.SAME_NONZERO_PATTERN)
        A.axpy(dt, K, P.SUBSET_NONZERO_PATTERN)
        A.shift(sigma)
        cur = c.aa.copy(); cur[c.xtoy] += dt * c.xa; cur[c.diag] += sigma
        L.KSPSetOperators(k.h, A.h, A.h, P.SAME_NONZERO_PATTERN)
        x1, h1 = solve(k)
        F = P.Mat.from_csr(c.ai, c.aj, cur)
        kf = solver(F)
        x2, h2 = solve(kf)
        print("step %d: %d iterations, |x| %.6e" % (step, k.its, np.linalg.norm(x1)))
        assert h1.size == h2.size and h1.size > 2, (step, h1.size, h2.size)
        assert np.array_equal(bits(h1), bits(h2)), step
        assert np.array_equal(bits(x1), bits(x2)), step
        kf.destroy(); F.destroy()
    assert uploads(P, A) == up0
    pc = C.c_void_p()
    L.KSPGetPC(k.h, C.byref(pc))
    dev_, sym, num = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.PCILUGetNumeric_HIPMI355X(pc, C.byref(dev_), C.byref(sym), C.byref(num))
    print("numeric on device %d, symbolic builds %d, numeric runs %d" % (dev_.value, sym.value, num.value))
    assert dev_.value == 1 and sym.value == 1
    assert num.value == 4
