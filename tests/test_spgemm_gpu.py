"""Sparse matrix products on the device: the numeric kernel of csrc/spgemm.hip through the C ABI, and MatMatMult / MatTranspose /
MatPtAP of the plug-in, against the restatement of the contract in tests/spgemm_ref.py.  Every comparison is on bit patterns; where
the reference is NaN a NaN is asked for.  ca lives between guard bands of a marker and is pre-filled with a NaN of a payload of its
own; the arrays of A, B and C's pattern are read back: the kernel writes the ci[m] slots of ca and nothing else."""
import ctypes as C

import numpy as np
import pytest

import orc
import spgemm_ref as sg
from gpu import Dev
from specials import SPECIALS, bits
from test_spgemm_cpu import p7_and_p, raises, same_csr

pytestmark = pytest.mark.gpu
ERR_SUP, ARG_WRONG = 56, 62
BAND = 64
MARK = -1.2345e300
PREFILL = np.array([0x7FF8DEAD00000001], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.free_all()


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture()
def opts(P):
    L = P.lib()

    def set_(route=None):
        L.PetscOptionsClear()
        if route:
            L.PetscOptionsSetValue(b"-mat_hipmi355x_product", route.encode())
    set_()
    yield set_
    L.PetscOptionsClear()


def geometry(dev):
    lds, block = C.c_int(), C.c_int()
    dev.chk(dev.k.mi355x_spgemm_geometry(C.byref(lds), C.byref(block)))
    return lds.value, block.value


def same_values(got, ref, what=""):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaNs at %s, reference at %s" % (what, np.flatnonzero(np.isnan(got))[:8], np.flatnonzero(nan)[:8])
    d = np.flatnonzero(~nan & (bits(got) != bits(ref)))
    assert d.size == 0, "%s: bits differ at %s: %r, reference %r" % (what, d[:8], got[d[:8]], ref[d[:8]])


def device_product(dev, A, B, k, n, runs=2):
    """C = A B by the kernel: (ci, cj, ca, lanes, nwindowed); the guard bands, the pre-fill, the inputs and a second run checked on the way"""
    m = A[0].size - 1
    ci, cj = sg.symbolic(A[0], A[1], B[0], B[1])
    nz = int(ci[-1])
    host = [np.ascontiguousarray(a) for a in (A[0], A[1], A[2], B[0], B[1], B[2], ci, cj)]
    d = [dev.put(a) for a in host]
    plan = C.c_void_p()
    dev.chk(dev.k.mi355x_spgemm_plan_create(dev.h, m, k, n, *[host[q].ctypes.data for q in (0, 1, 3, 4, 6, 7)], C.byref(plan)))
    lanes, nwin, ws = C.c_int(), C.c_int(), C.c_size_t()
    dev.chk(dev.k.mi355x_spgemm_plan_info(plan, C.byref(lanes), C.byref(nwin), C.byref(ws)))
    assert ws.value >= 4
    outs = []
    for _ in range(runs):
        full = np.full(nz + 2 * BAND, MARK); full[BAND:BAND + nz] = PREFILL
        base = dev.put(full)
        dev.chk(dev.k.mi355x_spgemm_numeric(dev.h, plan, *d, C.c_void_p(base.value + 8 * BAND)))
        back = dev.get(base, nz + 2 * BAND)
        mark = bits(np.array([MARK]))[0]
        assert (bits(back[:BAND]) == mark).all() and (bits(back[BAND + nz:]) == mark).all(), "a guard band was written"
        ca = back[BAND:BAND + nz]
        assert not (bits(ca) == bits(np.array([PREFILL]))[0]).any(), "a slot of ca was not written"
        outs.append(ca)
        dev.free(base)
    for a, p in zip(host, d):
        assert np.array_equal(dev.get(p, a.size, a.dtype).view(np.uint8), a.view(np.uint8)), "an input array changed"
        dev.free(p)
    assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs), "two runs differ"
    dev.chk(dev.k.mi355x_spgemm_plan_destroy(plan))
    return ci, cj, outs[0], lanes.value, nwin.value


def check_product(dev, A, B, k, n, lanes=None, nwindowed=None, what=""):
    ci, cj, ca, ln, nw = device_product(dev, A, B, k, n)
    same_values(ca, sg.numeric(A[0], A[1], A[2], B[0], B[1], B[2], ci, cj), what)
    if lanes is not None:
        assert ln == lanes, (what, ln, lanes)
    if nwindowed is not None:
        assert nw == nwindowed, (what, nw, nwindowed)
    return ci, cj, ca


# ---------------------------------------------------------------------------------------------------- the kernel through the C ABI
@pytest.mark.parametrize("seed", [5, 6])
def test_random_rectangular(dev, seed):
    A, B = sg.rect_pair(seed)
    check_product(dev, A, B, 53, 41, lanes=8, nwindowed=0)


def test_order_sensitive_case(dev):
    A, B = sg.order_sensitive_pair()
    fwd, rev = sg.matmult(A, B), sg.matmult(A, B, reverse=True)
    assert np.any(bits(fwd[2]) != bits(rev[2]))
    same_values(device_product(dev, A, B, 3, 4)[2], fwd[2])


@pytest.mark.parametrize("W,blen", [(8, 5), (16, 12), (32, 25), (64, 50), (64, 90)])
def test_lane_widths(dev, W, blen):
    """every B row has blen entries, so that is the mean length the plan sees: the smallest width >= it, 64 at most; more than one
    workgroup (300 rows), a row count that fills no wavefront"""
    rng = np.random.default_rng(W + blen)
    A = sg.random_csr(301, 150, rng.integers(0, 7, 301), 40 + W)
    B = sg.random_csr(150, 333, np.full(150, blen), 41 + W)
    check_product(dev, A, B, 150, 333, lanes=W, what="W=%d" % W)


@pytest.mark.parametrize("W", [8, 16, 32, 64])
def test_strided_loop_over_long_b_rows(dev, W):
    """B rows of W + 1 and 2 W + 3 entries among rows of W - 2: the mean stays below W, the two rows take two and three rounds of the lanes"""
    rng = np.random.default_rng(90 + W)
    lb = np.full(120, W - 2); lb[5] = W + 1; lb[17] = 2 * W + 3
    B = sg.random_csr(120, 400, lb, 50 + W)
    A = list(sg.random_csr(130, 120, rng.integers(1, 6, 130), 51 + W))
    A[1] = A[1].copy()
    for i, c in ((0, 5), (1, 17), (64, 5), (65, 17), (129, 17)):           # rows that name the long B rows, first entry of the row
        row = A[1][A[0][i]:A[0][i + 1]]
        if c not in row:
            row[0] = c; row.sort()
            assert np.all(np.diff(row) > 0)
    check_product(dev, tuple(A), B, 120, 400, lanes=W, what="W=%d" % W)


@pytest.mark.parametrize("short_b", [False, True])
def test_rows_around_the_lds_budget_and_windows(dev, short_b):
    """C rows of budget - 1, budget, budget + 1 and 2 budget + 5 entries among ordinary ones: the last two run in column windows.
    long B rows (64 lanes): a C row is the union of an even-column and an odd-column B row that overlap in a few columns;
    short B rows (8 lanes): a C row is the union of many B rows of 8 columns, neighbours overlapping in two"""
    budget, _ = geometry(dev)
    want = [budget - 1, budget, budget + 1, 2 * budget + 5]
    n = 2 * budget + 40
    brows, arows = [], []
    for L in want:
        if not short_b:
            even = np.arange(0, L, 2); odd = np.union1d(np.arange(1, L, 2), [0, 4, L - 1 - (L - 1) % 2])
            arows.append([len(brows), len(brows) + 1]); brows += [even + 7, odd + 7]
        else:
            names = []
            for s in range(0, L, 6):
                names.append(len(brows)); brows.append(np.arange(s, min(s + 8, L)) + 7)
            arows.append(names)
    nspecial = len(brows)
    rng = np.random.default_rng(3)
    blen, per_a = (6, 3) if short_b else (60, 1)                 # the ordinary rows: what keeps the mean B-row length at 8 or at 64 lanes
    for _ in range(30):
        brows.append(np.sort(rng.choice(n, size=blen, replace=False)))
    k = len(brows)
    order = rng.permutation(k)                                   # B's rows shuffled, so that A's columns are not sorted by construction alone
    inv = np.argsort(order)
    bi = np.concatenate(([0], np.cumsum([brows[r].size for r in order]))).astype(np.int32)
    bj = np.concatenate([brows[r] for r in order]).astype(np.int32)
    B = (bi, bj, rng.standard_normal(bj.size))
    alist = []
    for i in range(70):
        alist.append(np.sort(inv[np.array(arows[(i - 10) // 15])]) if i in (10, 25, 40, 55) else np.sort(inv[nspecial + rng.choice(30, size=per_a, replace=False)]))
    ai = np.concatenate(([0], np.cumsum([r.size for r in alist]))).astype(np.int32)
    aj = np.concatenate(alist).astype(np.int32)
    A = (ai, aj, rng.standard_normal(aj.size))
    ci, cj, ca = check_product(dev, A, B, k, n, lanes=8 if short_b else 64, nwindowed=2)
    assert [int(ci[i + 1] - ci[i]) for i in (10, 25, 40, 55)] == want


def test_ieee_specials_and_containment(dev):
    """NaN, +-Inf, -0.0 and denormals inside A and B: NaNs exactly where the reference has them, every other bit equal; a stored 0.0
    in A against an Inf in B is a NaN; an entry of C none of whose products involves a changed operand keeps the clean run's bits"""
    rng = np.random.default_rng(77)
    A = sg.random_csr(150, 140, rng.integers(0, 8, 150), 70)
    B = sg.random_csr(140, 160, rng.integers(0, 8, 140), 71)
    ci, cj, clean = check_product(dev, A, B, 140, 160)
    kinds = np.concatenate((SPECIALS, [-0.0, 0.0, 5e-324, -1e-310, 2.2e-308]))
    aa, ba = A[2].copy(), B[2].copy()
    pa = rng.choice(aa.size, size=24, replace=False); pb_ = rng.choice(ba.size, size=24, replace=False)
    aa[pa] = kinds[np.arange(24) % kinds.size]; ba[pb_] = kinds[(np.arange(24) + 3) % kinds.size]
    # a stored 0.0 in A against +Inf in B: the first entry of a row of A that names a non-empty B row
    i0 = next(i for i in range(150) if A[0][i + 1] > A[0][i] and B[0][A[1][A[0][i]] + 1] > B[0][A[1][A[0][i]]])
    t0 = int(A[0][i0]); q0 = int(B[0][A[1][t0]])
    aa[t0] = 0.0; ba[q0] = np.inf
    pa, pb_ = np.append(pa, t0), np.append(pb_, q0)
    As, Bs = (A[0], A[1], aa), (B[0], B[1], ba)
    ci2, cj2, got = check_product(dev, As, Bs, 140, 160, what="specials")
    slot = int(ci[i0] + np.searchsorted(cj[ci[i0]:ci[i0 + 1]], B[1][q0]))
    assert np.isnan(got[slot]), "0.0 * Inf"
    ia, ib = np.zeros(aa.size), np.zeros(ba.size)
    ia[pa] = 1.0; ib[pb_] = 1.0
    touched = (sg.numeric(A[0], A[1], ia, B[0], B[1], np.ones(ba.size), ci, cj) + sg.numeric(A[0], A[1], np.ones(aa.size), B[0], B[1], ib, ci, cj)) > 0
    assert touched.any() and (~touched).sum() > touched.sum()
    leak = ~touched & (bits(got) != bits(clean))
    assert not leak.any(), "entries %s have no changed operand and changed" % np.flatnonzero(leak)[:8]


def test_plan_create_refuses_bad_patterns(dev):
    A, B = sg.rect_pair()
    ci, cj = sg.symbolic(A[0], A[1], B[0], B[1])
    plan = C.c_void_p()

    def create(aj=A[1], bj=B[1], cj_=cj, k=53):
        arrs = [np.ascontiguousarray(a) for a in (A[0], aj, B[0], bj, ci, cj_)]
        return dev.k.mi355x_spgemm_plan_create(dev.h, 37, k, 41, *[a.ctypes.data for a in arrs], C.byref(plan))
    bad = A[1].copy(); bad[0] = 53
    assert create(aj=bad) != 0 and not plan.value
    bad = B[1].copy(); bad[1] = bad[0]
    assert create(bj=bad) != 0
    bad = cj.copy(); bad[-1] = 41
    assert create(cj_=bad) != 0
    assert create() == 0 and plan.value
    dev.chk(dev.k.mi355x_spgemm_plan_destroy(plan))


# ---------------------------------------------------------------------------------------------------- the plug-in
def upload_count(P, A):
    up = C.c_int()
    P.lib().MatHIPMI355XGetUploadCount(A.h, C.byref(up))
    return up.value


def test_device_and_host_routes_agree(P, opts):
    A, B = sg.rect_pair()
    Ap, Pc = p7_and_p(np.random.default_rng(1).standard_normal(512))
    res = {}
    for route in ("device", "host"):
        opts(route)
        Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
        Cm, Tm = Am.matmult(Bm), Am.transpose()
        Gm = P.Mat.from_csr(*Ap).ptap(P.Mat.from_csr(*Pc, ncols=64))
        want = (1, 1, 0) if route == "device" else (1, 0, 1)
        assert Cm.product_counts() == want and Tm.product_counts() == want and Gm.product_counts() == want
        res[route] = (Cm.csr(), Tm.csr(), Gm.csr())
    for d, h, ref in zip(res["device"], res["host"], (sg.matmult(A, B), sg.transpose(A, 53), sg.ptap(Ap, Pc, 64))):
        same_csr(d, h)
        same_csr(d, ref)


def square_pair():
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 4, 60)
    A = list(sg.random_csr(60, 60, lens, 13))
    rows = [np.union1d(A[1][A[0][i]:A[0][i + 1]], [i]) for i in range(60)]      # a stored diagonal, for MatShift
    ai = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int32)
    aj = np.concatenate(rows).astype(np.int32)
    return (ai, aj, rng.standard_normal(aj.size)), sg.random_csr(60, 41, rng.integers(0, 4, 60), 14)


def test_matmult_reuse_after_device_side_value_changes(P, opts):
    opts("device")
    A, B = square_pair()
    Am, Bm = P.Mat.from_csr(*A), P.Mat.from_csr(*B, ncols=41)
    Cm = Am.matmult(Bm)
    same_csr(Cm.csr(), sg.matmult(A, B))
    ups = upload_count(P, Am), upload_count(P, Bm)
    P.lib().MatScale(Am.h, 1.75)
    Am.shift(-0.375)
    A2 = (A[0], A[1], Am.csr()[2])
    assert np.any(bits(A2[2]) != bits(A[2]))
    assert Am.matmult(Bm, reuse=Cm) is Cm
    same_csr(Cm.csr(), sg.matmult(A2, B))
    assert (upload_count(P, Am), upload_count(P, Bm)) == ups, "an operand changed on the device is not sent again"
    assert Cm.product_counts() == (1, 2, 0) and upload_count(P, Cm) == 1


def test_matmult_with_the_product(P, opts):
    """C's device values, its plan and its host copy agree: MatMult on short rows carries the oracle's bits"""
    opts("device")
    A, B = square_pair()
    Cm = P.Mat.from_csr(*A).matmult(P.Mat.from_csr(*B, ncols=41))
    ref = sg.matmult(A, B)
    assert ref[0][-1] <= 16 * 60
    x = np.random.default_rng(2).standard_normal(41)
    vx = P.Vec.from_array(x, comm=P.lib().COMM_SELF); vy = P.Vec.create(60, comm=P.lib().COMM_SELF)
    Cm.mult(vx, vy)
    assert np.array_equal(bits(vy.array()), bits(orc.spmv(ref[0], ref[1], ref[2], x)))
    assert upload_count(P, Cm) == 1


def test_transpose_and_its_reuse(P, opts):
    opts("device")
    A, _ = sg.rect_pair(6)
    Am = P.Mat.from_csr(*A, ncols=53)
    Tm = Am.transpose()
    same_csr(Tm.csr(), orc.csr_transpose(A[0], A[1], A[2], 53))
    ups = upload_count(P, Am)
    P.lib().MatScale(Am.h, -2.5)
    A2 = (A[0], A[1], Am.csr()[2])
    Am.transpose(reuse=Tm)
    same_csr(Tm.csr(), orc.csr_transpose(A2[0], A2[1], A2[2], 53))
    assert Tm.product_counts() == (1, 2, 0) and upload_count(P, Am) == ups and upload_count(P, Tm) == 1
    x = np.random.default_rng(4).standard_normal(37)                         # T's device copy multiplies as A^T
    vx = P.Vec.from_array(x, comm=P.lib().COMM_SELF); vy = P.Vec.create(53, comm=P.lib().COMM_SELF)
    Tm.mult(vx, vy)
    t = sg.transpose(A2, 53)
    assert np.array_equal(bits(vy.array()), bits(orc.spmv(t[0], t[1], t[2], x)))


def test_ptap_poisson_aggregation(P, opts):
    opts("device")
    A, Pc = p7_and_p()
    Am, Pm = P.Mat.from_csr(*A), P.Mat.from_csr(*Pc, ncols=64)
    Cm = Am.ptap(Pm)
    same_csr(Cm.csr(), sg.ptap(A, Pc, 64))
    ci, cj, ca = Cm.csr()
    dense = np.zeros((64, 64)); dense[np.repeat(np.arange(64), np.diff(ci)), cj] = ca
    ref = sg.ptap(A, Pc, 64)
    dref = np.zeros((64, 64)); dref[np.repeat(np.arange(64), np.diff(ref[0])), ref[1]] = ref[2]
    assert np.array_equal(dense, dense.T) and np.array_equal(dense.sum(axis=1), dref.sum(axis=1))
    ups = upload_count(P, Am), upload_count(P, Pm)
    Am.shift(0.5)
    A2 = (A[0], A[1], Am.csr()[2])
    Am.ptap(Pm, reuse=Cm)
    same_csr(Cm.csr(), sg.ptap(A2, Pc, 64))
    assert Cm.product_counts() == (1, 2, 0) and (upload_count(P, Am), upload_count(P, Pm)) == ups


def test_ptap_random_weights(P, opts):
    opts("device")
    A, Pc = p7_and_p(np.random.default_rng(17).standard_normal(512))
    A = (A[0], A[1], A[2] * (1.0 + 0.01 * np.cos(np.arange(A[2].size))))
    Cm = P.Mat.from_csr(*A).ptap(P.Mat.from_csr(*Pc, ncols=64))
    same_csr(Cm.csr(), sg.ptap(A, Pc, 64))
    assert Cm.product_counts() == (1, 1, 0)


def test_unsupported_operands_and_foreign_results(P, opts):
    opts("device")
    bs = P.Mat.from_bsr(2, np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.arange(8.0))
    mp = P.Mat.from_csr_mpi(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4), 4)
    for X in (bs, mp):
        raises(P, ERR_SUP, lambda: X.matmult(X))
        raises(P, ERR_SUP, lambda: X.transpose())
        raises(P, ERR_SUP, lambda: X.ptap(X))
    A, B = sg.rect_pair()
    Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
    Cm = Am.matmult(Bm)
    raises(P, ARG_WRONG, lambda: Am.matmult(Bm, reuse=Bm))
    raises(P, ARG_WRONG, lambda: Am.transpose(reuse=Cm))
    A2m = P.Mat.from_csr(*A, ncols=53)
    raises(P, ARG_WRONG, lambda: A2m.matmult(Bm, reuse=Cm))
    # an operand whose pattern was uploaded anew since the symbolic pass
    P.lib().PetscOptionsSetValue(b"-mat_hipmi355x_index_compression", b"0")
    P.lib().MatSetFromOptions(Am.h)
    raises(P, ARG_WRONG, lambda: Am.matmult(Bm, reuse=Cm))
