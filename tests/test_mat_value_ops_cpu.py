"""MatShift / MatAXPY / MatCopy without a GPU: the host-only map builder mi355x_csr_subset_map against a numpy dictionary lookup,
the declaration / export pairs of the new names, and the host copy of the three operators (a matrix that was never used on the
device takes the host route alone: these need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
import problems as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME, SUBSET, DIFFERENT = 2, 1, 0


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def subset_map(k, xi, xj, yi, yj, xcols=None, ycols=None):
    xi, xj, yi, yj = i32(xi), i32(xj), i32(yi), i32(yj)
    xcols = None if xcols is None else i32(xcols)
    ycols = None if ycols is None else i32(ycols)
    out = np.full(max(xj.size, 1), -7, np.int32)
    bad = C.c_int(-99)
    rc = k.mi355x_csr_subset_map(xi.size - 1, ptr(xi), ptr(xj), ptr(xcols), ptr(yi), ptr(yj), ptr(ycols), ptr(out), C.byref(bad))
    return rc, out[:xj.size], bad.value


def lookup(xi, xj, yi, yj, xcols=None, ycols=None):
    """xtoy by a dictionary of Y's (row, global column) -> position; (None, row) for the first row with an entry Y lacks"""
    pos = {}
    for r in range(len(yi) - 1):
        for q in range(yi[r], yi[r + 1]):
            pos[(r, int(yj[q] if ycols is None else ycols[yj[q]]))] = q
    out = []
    for r in range(len(xi) - 1):
        for q in range(xi[r], xi[r + 1]):
            key = (r, int(xj[q] if xcols is None else xcols[xj[q]]))
            if key not in pos:
                return None, r
            out.append(pos[key])
    return np.array(out, np.int32), -1


def drop_entries(ai, aj, aa, seed=3, empty_rows=(5, 6, 100), diag_only=17, frac=1.0 / 3.0):
    """X from Y: about a third of the entries dropped, every entry of some rows, everything but the diagonal of one row"""
    rng = np.random.default_rng(seed)
    m = ai.size - 1
    rows = np.repeat(np.arange(m), np.diff(ai))
    keep = rng.random(aj.size) >= frac
    keep[np.isin(rows, empty_rows)] = False
    keep[rows == diag_only] = aj[rows == diag_only] == diag_only
    xi = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
    return xi, aj[keep].copy(), (0.5 + np.cos(np.arange(int(keep.sum())))) * 1.7, np.flatnonzero(keep).astype(np.int32)


@pytest.mark.parametrize("threads", [1, 8])
def test_csr_subset_map_against_a_dictionary_lookup(built, monkeypatch, threads):
    monkeypatch.setenv("MI355X_HOST_THREADS", str(threads))
    k = built.load_kernels()
    ai, aj, aa = orc.gen_p7(11, 9, 7)
    # an identical pattern: the identity
    rc, m_, bad = subset_map(k, ai, aj, ai, aj)
    assert rc == 0 and bad == -1 and np.array_equal(m_, np.arange(aj.size))
    # a proper subset with empty rows and a diagonal-only row
    xi, xj, _, kept = drop_entries(ai, aj, aa)
    assert xi[6] == xi[5] and xi[18] - xi[17] == 1 and 0.5 < xj.size / aj.size < 0.8
    rc, m_, bad = subset_map(k, xi, xj, ai, aj)
    ref, _ = lookup(xi, xj, ai, aj)
    assert rc == 0 and bad == -1 and np.array_equal(m_, ref) and np.array_equal(m_, kept)
    # m = 0 and m = 1
    rc, m_, bad = subset_map(k, [0], [], [0], [])
    assert rc == 0 and bad == -1
    rc, m_, bad = subset_map(k, [0, 2], [0, 3], [0, 4], [0, 1, 3, 4])
    assert rc == 0 and list(m_) == [0, 2]
    rc, m_, bad = subset_map(k, [0, 0], [], [0, 1], [0])
    assert rc == 0 and m_.size == 0
    # column translations that reorder nothing but differ in length: X's garray has 4 columns, Y's 6
    xg, yg = [3, 10, 40, 41], [3, 7, 10, 12, 40, 41]
    xi2, xj2 = [0, 2, 2, 4, 5], [0, 2, 1, 3, 0]
    yi2, yj2 = [0, 3, 4, 7, 9], [0, 1, 4, 2, 2, 3, 5, 0, 5]
    rc, m_, bad = subset_map(k, xi2, xj2, yi2, yj2, xg, yg)
    ref, _ = lookup(xi2, xj2, yi2, yj2, xg, yg)
    assert rc == 0 and bad == -1 and np.array_equal(m_, ref) and list(m_) == [0, 2, 4, 6, 7]
    # one side translated only
    rc, m_, bad = subset_map(k, xi2, [3, 40, 10, 41, 3], yi2, yj2, None, yg)
    assert rc == 0 and list(m_) == [0, 2, 4, 6, 7]
    # not a subset: the error and the first bad row, whichever chunk finds it
    for row in (0, 250, 692):
        yj_less = np.delete(aj, ai[row] + 1)
        yi_less = ai.copy(); yi_less[row + 1:] -= 1
        rc, m_, bad = subset_map(k, ai, aj, yi_less, yj_less)
        assert rc != 0 and bad == row == lookup(ai, aj, yi_less, yj_less)[1]
    yj_less = np.delete(aj, [ai[40] + 1, ai[600]])
    yi_less = ai.copy(); yi_less[41:] -= 1; yi_less[601:] -= 1
    rc, m_, bad = subset_map(k, ai, aj, yi_less, yj_less)
    assert rc != 0 and bad == 40
    rc, m_, bad = subset_map(k, xi2, xj2, yi2, yj2, [3, 10, 40, 42], yg)       # a global column Y lacks, in rows 2 and 3
    assert rc != 0 and bad == 2


def test_csr_subset_map_on_host_threads_from_200000_entries(built, monkeypatch):
    """without the override the rows are split from 200 000 entries of X: the same map as one thread's"""
    k = built.load_kernels()
    ai, aj, aa = orc.gen_p7(40, 32, 25)
    assert aj.size > 200000
    xi, xj, _, kept = drop_entries(ai, aj, aa, frac=0.03)
    assert xj.size > 200000
    monkeypatch.setenv("MI355X_HOST_THREADS", "1")
    rc1, m1, _ = subset_map(k, xi, xj, ai, aj)
    monkeypatch.delenv("MI355X_HOST_THREADS")
    rc2, m2, _ = subset_map(k, xi, xj, ai, aj)
    assert rc1 == 0 and rc2 == 0 and np.array_equal(m1, kept) and np.array_equal(m2, kept)


def test_new_names_are_declared_and_exported(built):
    kh = open(os.path.join(ROOT, "include", "mi355x_kernels.h")).read()
    mini = open(os.path.join(ROOT, "include", "petscmini.h")).read()
    from petsc_dev_amd._lib import KERNEL_API
    k = built.load_kernels()
    for n in ("mi355x_csr_shift", "mi355x_csr_axpy_map", "mi355x_csr_subset_map"):
        assert re.search(r"\bint\s+%s\s*\(" % n, kh), n
        assert hasattr(k, n), n
        assert n in KERNEL_API
    harness = built.load_harness()
    for n in ("MatShift", "MatAXPY", "MatAYPX", "MatCopy"):
        assert re.search(r"PetscErrorCode\s+%s\s*\(" % n, mini), n
        assert hasattr(harness, n), n
    impl = open(os.path.join(ROOT, "petsc-dev_amd", "harness", "petscimpl.h")).read()
    for slot, sig in (("shift", r"\(Mat,\s*PetscScalar\)"), ("axpy", r"\(Mat,\s*PetscScalar,\s*Mat,\s*MatStructure\)"), ("copy", r"\(Mat,\s*Mat,\s*MatStructure\)")):
        assert re.search(r"PetscErrorCode\s*\(\*%s\)%s;" % (slot, sig), impl), slot
    for frag in ("aijhipmi355x_ctor.h", "mpiaijhipmi355x_ctor.h"):
        t = open(os.path.join(ROOT, "integration", "petsc-3.3", frag)).read()
        for slot in ("shift", "axpy", "copy"):
            assert re.search(r"B->ops->%s\s*=" % slot, t), (frag, slot)


# ---------------------------------------------------------------------------------------------------- the host copy
@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def host_values(P, A, nvals):
    m, pa = C.c_int(), C.c_void_p()
    P.lib().MatSeqAIJGetArrays(A.h, C.byref(m), None, None, C.byref(pa))
    return np.ctypeslib.as_array(C.cast(pa, C.POINTER(C.c_double)), (max(nvals, 1),))[:nvals].copy()


def host_pattern(P, A):
    m, pi_, pj = C.c_int(), C.c_void_p(), C.c_void_p()
    P.lib().MatSeqAIJGetArrays(A.h, C.byref(m), C.byref(pi_), C.byref(pj), None)
    ai = np.ctypeslib.as_array(C.cast(pi_, C.POINTER(C.c_int)), (m.value + 1,)).copy()
    aj = np.ctypeslib.as_array(C.cast(pj, C.POINTER(C.c_int)), (max(int(ai[-1]), 1),))[:ai[-1]].copy()
    return ai, aj


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_host_copy_of_shift_axpy_copy(P):
    L = P.lib()
    ai, aj, aa = orc.gen_p7(11, 9, 7)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    diag = np.flatnonzero(rows == aj)
    xi, xj, xa, xtoy = drop_entries(ai, aj, aa)
    Y = P.Mat.from_csr(ai, aj, aa); X = P.Mat.from_csr(xi, xj, xa); Z = P.Mat.from_csr(ai, aj, np.cos(np.arange(aa.size)))
    cur = aa.copy()
    Y.shift(0.37); cur[diag] += 0.37
    assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(cur))
    Y.axpy(-1.3, Z, P.SAME_NONZERO_PATTERN); cur = cur + (-1.3) * np.cos(np.arange(aa.size))
    assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(cur))
    Y.axpy(0.7, Y, P.SAME_NONZERO_PATTERN); cur = cur + 0.7 * cur
    assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(cur))
    for str_ in (P.SUBSET_NONZERO_PATTERN, P.DIFFERENT_NONZERO_PATTERN):
        Y.axpy(0.25, X, str_); cur[xtoy] += 0.25 * xa
        assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(cur))
    L.MatAYPX(Y.h, 0.5, X.h, P.SUBSET_NONZERO_PATTERN); cur = 0.5 * cur; cur[xtoy] += 1.0 * xa
    assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(cur))
    Y.copy(Z, P.SAME_NONZERO_PATTERN)
    assert np.array_equal(bits(host_values(P, Z, aa.size)), bits(cur))
    X.copy(Z, P.DIFFERENT_NONZERO_PATTERN)                       # MatCopy_Basic: zero, then X's entries
    ref = np.zeros(aa.size); ref[xtoy] += 1.0 * xa
    assert np.array_equal(bits(host_values(P, Z, aa.size)), bits(ref))
    X.copy(Z, P.SAME_NONZERO_PATTERN)                            # a SAME claim for unequal patterns: handled the same way
    assert np.array_equal(bits(host_values(P, Z, aa.size)), bits(ref))
    Y.copy(Y, P.SAME_NONZERO_PATTERN)
    # errors leave Y alone
    before = host_values(P, Y, aa.size)
    for call, code in ((lambda: Y.axpy(1.0, X, P.SAME_NONZERO_PATTERN), 62), (lambda: X.axpy(1.0, Y, P.SUBSET_NONZERO_PATTERN), 62),
                       (lambda: X.axpy(1.0, Y, P.DIFFERENT_NONZERO_PATTERN), 56), (lambda: Y.copy(X, P.SAME_NONZERO_PATTERN), 62)):
        with pytest.raises(P.PetscError) as e:
            call()
        assert e.value.code == code, str(e.value)
    with pytest.raises(P.PetscError) as e:
        X.axpy(1.0, Y, P.SUBSET_NONZERO_PATTERN)
    assert "row 0" in str(e.value)
    assert np.array_equal(bits(host_values(P, Y, aa.size)), bits(before)) and np.array_equal(bits(host_values(P, X, xa.size)), bits(xa))
    W = P.Mat.from_csr(*pb.lap2d(5, 4))
    with pytest.raises(P.PetscError) as e:
        Y.axpy(1.0, W, P.SAME_NONZERO_PATTERN)
    assert e.value.code == 60


def test_shift_inserts_a_missing_diagonal_entry(P):
    ai, aj, aa = pb.lap2d(7, 5)
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    keep = ~((rows == aj) & np.isin(rows, (0, 9, n - 1)))
    xi = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    A = P.Mat.from_csr(xi, aj[keep], aa[keep])
    A.shift(2.5)
    gi, gj = host_pattern(P, A)
    assert np.array_equal(gi, ai) and np.array_equal(gj, aj)
    ref = np.where(rows == aj, np.where(np.isin(rows, (0, 9, n - 1)), 2.5, aa + 2.5), aa)
    assert np.array_equal(bits(host_values(P, A, aa.size)), bits(ref))
    A.shift(-1.0)                                               # now every row has its entry
    ref = np.where(rows == aj, ref + -1.0, ref)
    assert np.array_equal(bits(host_values(P, A, aa.size)), bits(ref))


def test_baij_takes_the_host_route(P):
    bs = 3
    bi, bj, _ = pb.lap2d(6, 5)
    nb = bj.size
    ba = np.cos(0.1 * np.arange(nb * bs * bs)); bb = np.sin(0.2 * np.arange(nb * bs * bs))
    A = P.Mat.from_bsr(bs, bi, bj, ba); B = P.Mat.from_bsr(bs, bi, bj, bb)
    brow = np.repeat(np.arange(bi.size - 1), np.diff(bi))
    cur = ba.copy()
    A.shift(0.75)
    for k in np.flatnonzero(brow == bj):
        for q in range(bs):
            cur[k * bs * bs + q * bs + q] += 0.75
    assert np.array_equal(bits(host_values(P, A, ba.size)), bits(cur))
    A.axpy(-0.3, B, P.SAME_NONZERO_PATTERN); cur = cur + (-0.3) * bb
    assert np.array_equal(bits(host_values(P, A, ba.size)), bits(cur))
    A.copy(B, P.SAME_NONZERO_PATTERN)
    assert np.array_equal(bits(host_values(P, B, ba.size)), bits(cur))
    with pytest.raises(P.PetscError) as e:
        A.axpy(1.0, B, P.SUBSET_NONZERO_PATTERN)
    assert e.value.code == 56


@pytest.mark.parametrize("size", [1, 2, 3])
def test_mpiaij_host_copy_through_both_blocks(P, size):
    """shift, SAME, SUBSET and copy of MPIAIJ matrices on ranks staged as threads: X's off-diagonal block keeps fewer columns than Y's,
    so the two garrays differ; every rank's blocks hold what the split of the updated global values gives"""
    from fakempi import FakeWorld
    L = P.lib()
    nx, ny, nz = 5, 4, 9
    ai, aj, aa = orc.gen_p7(nx, ny, nz)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    N = ai.size - 1
    rows = np.repeat(np.arange(N), np.diff(ai))
    za = np.cos(np.arange(aa.size))
    xi, xj, xa, xtoy = drop_entries(ai, aj, aa, empty_rows=(5, 6, 100), diag_only=17, frac=0.5)
    ranges = np.array([nx * ny * ((nz * r) // size) for r in range(size + 1)], dtype=np.int32)
    cur = aa.copy()
    cur[rows == aj] += 0.37
    cur = cur + (-1.3) * za
    cur[xtoy] += 0.25 * xa
    cpy = np.zeros(aa.size); cpy[xtoy] += 1.0 * xa

    def local(comm, i_, j_, a_, rs, re_):
        return P.Mat.from_csr_mpi((i_[rs:re_ + 1] - i_[rs]).astype(np.int32), j_[i_[rs]:i_[re_]].copy(), a_[i_[rs]:i_[re_]].copy(), re_ - rs, N, N, comm=comm)

    def blocks(A):
        Ad, Ao, g = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.MatMPIAIJGetSeqAIJ(A.h, C.byref(Ad), C.byref(Ao), C.byref(g))
        out = []
        for blk in (Ad, Ao):
            bi, _ = host_pattern(P, P.Mat(blk, own=False))
            out.append(host_values(P, P.Mat(blk, own=False), int(bi[-1])))
        ec = C.c_int(); L.MatMPIAIJGetScatter(A.h, None, None, C.byref(ec))
        return out[0], out[1], ec.value

    def work(rank, comm):
        rs, re_ = int(ranges[rank]), int(ranges[rank + 1])
        Y = local(comm, ai, aj, aa, rs, re_); Z = local(comm, ai, aj, za, rs, re_); X = local(comm, xi, xj, xa, rs, re_); W = local(comm, ai, aj, za, rs, re_)
        Y.shift(0.37)
        Y.axpy(-1.3, Z, P.SAME_NONZERO_PATTERN)
        Y.axpy(0.25, X, P.SUBSET_NONZERO_PATTERN)
        Y.copy(Z, P.SAME_NONZERO_PATTERN)
        X.copy(W, P.DIFFERENT_NONZERO_PATTERN)
        codes = []
        for call in (lambda: Y.axpy(1.0, X, P.SAME_NONZERO_PATTERN), lambda: X.axpy(1.0, Y, P.SUBSET_NONZERO_PATTERN)):
            try:
                call(); codes.append(0)
            except P.PetscError as e:
                codes.append(e.code)
        return blocks(Y), blocks(Z), blocks(W), blocks(X), codes

    got = FakeWorld(size).run(work)
    for r in range(size):
        rs, re_ = int(ranges[r]), int(ranges[r + 1])
        ref = {k: orc.mpiaij_split(rs, re_, rs, re_, ai, aj, v) for k, v in (("cur", cur), ("cpy", cpy))}
        refx = orc.mpiaij_split(rs, re_, rs, re_, xi, xj, xa)
        (yd, yo, yec), (zd, zo, _), (wd, wo, _), (xd, xo, xec), codes = got[r]
        assert np.array_equal(bits(yd), bits(ref["cur"]["ad_a"])) and np.array_equal(bits(yo), bits(ref["cur"]["bo_a"])), r
        assert np.array_equal(bits(zd), bits(ref["cur"]["ad_a"])) and np.array_equal(bits(zo), bits(ref["cur"]["bo_a"])), r
        assert np.array_equal(bits(wd), bits(ref["cpy"]["ad_a"])) and np.array_equal(bits(wo), bits(ref["cpy"]["bo_a"])), r
        assert np.array_equal(bits(xd), bits(refx["ad_a"])) and np.array_equal(bits(xo), bits(refx["bo_a"])), r    # the refused updates changed nothing
        assert codes == [62, 62], codes
        if size > 1:
            assert xec < yec, "the test wants differing garrays (%d, %d)" % (xec, yec)
