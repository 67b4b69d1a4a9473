"""Sparse matrix products without a GPU: the host symbolic pass of csrc/spgemm.hip, the host route of MatMatMult / MatTranspose /
MatPtAP (-mat_hipmi355x_product host) against the restatement of the contract in tests/spgemm_ref.py, the error codes and the reuse
counts.  Every comparison of values is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import orc
import spgemm_ref as sg
from spgemm_ref import bits

ERR_SUP, ARG_SIZ, ARG_WRONG = 56, 60, 62


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture()
def host_route(P):
    L = P.lib()
    L.PetscOptionsClear()
    L.PetscOptionsSetValue(b"-mat_hipmi355x_product", b"host")
    yield L
    L.PetscOptionsClear()


def raises(P, code, call):
    with pytest.raises(P.PetscError) as e:
        call()
    assert e.value.code == code, str(e.value)


def symbolic_lib(k, A, B, n, nthreads):
    m = A[0].size - 1
    ci = np.full(m + 1, -7, np.int32)
    args = (m, n, A[0].ctypes.data, A[1].ctypes.data, B[0].ctypes.data, B[1].ctypes.data)
    assert k.mi355x_spgemm_symbolic_host(*args, ci.ctypes.data, None, nthreads) == 0
    cj = np.full(max(int(ci[-1]), 1), -7, np.int32)
    assert k.mi355x_spgemm_symbolic_host(*args, ci.ctypes.data, cj.ctypes.data, nthreads) == 0
    return ci, cj[:ci[-1]]


def same_csr(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "pattern differs"
    d = np.flatnonzero(bits(got[2]) != bits(ref[2]))
    assert d.size == 0, "values differ at %s: %r, reference %r" % (d[:8], got[2][d[:8]], ref[2][d[:8]])


# ---------------------------------------------------------------------------------------------------- symbolic pass
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_symbolic_host_gives_the_union_patterns(built, seed):
    k = built.load_kernels()
    A, B = sg.rect_pair(seed)
    ci_ref, cj_ref = sg.symbolic(A[0], A[1], B[0], B[1])
    lens = np.diff(ci_ref)
    assert lens[3] == 0 and lens[20] == 0 and lens[11] == 0 and lens[25] == 0 and lens.max() > 9      # empty for each of the three reasons; real unions
    outs = [symbolic_lib(k, A, B, 41, nth) for nth in (1, 2, 5, 37)]
    for ci, cj in outs:
        assert np.array_equal(ci, ci_ref) and np.array_equal(cj, cj_ref)


def test_symbolic_host_many_threads_on_a_larger_product(built):
    k = built.load_kernels()
    rng = np.random.default_rng(3)
    A = sg.random_csr(3000, 2500, rng.integers(0, 12, 3000), 31)
    B = sg.random_csr(2500, 2700, rng.integers(0, 12, 2500), 32)
    one = symbolic_lib(k, A, B, 2700, 1)
    many = symbolic_lib(k, A, B, 2700, 7)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    rows = [0, 1, 777, 1500, 2999]
    for i in rows:                                             # the reference on a sample of rows (the full restatement is the test above)
        cols = [B[1][B[0][r]:B[0][r + 1]] for r in A[1][A[0][i]:A[0][i + 1]]]
        ref = np.unique(np.concatenate(cols)) if cols else np.zeros(0, np.int32)
        assert np.array_equal(one[1][one[0][i]:one[0][i + 1]], ref)


def test_symbolic_host_empty_matrix_and_bad_arguments(built):
    k = built.load_kernels()
    ci = np.full(1, -7, np.int32)
    assert k.mi355x_spgemm_symbolic_host(0, 5, None, None, None, None, ci.ctypes.data, None, 1) == 0 and ci[0] == 0
    assert k.mi355x_spgemm_symbolic_host(3, 5, None, None, None, None, ci.ctypes.data, None, 1) != 0
    assert k.mi355x_spgemm_symbolic_host(-1, 5, None, None, None, None, ci.ctypes.data, None, 1) != 0
    lds, block = C.c_int(), C.c_int()
    assert k.mi355x_spgemm_geometry(C.byref(lds), C.byref(block)) == 0 and lds.value >= 8 and block.value % 64 == 0


# ---------------------------------------------------------------------------------------------------- host route == the restatement
def test_host_route_matmult_transpose(P, host_route):
    A, B = sg.rect_pair()
    Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
    Cm = Am.matmult(Bm)
    same_csr(Cm.csr(), sg.matmult(A, B))
    assert Cm.local_size() == (37, 41) and Cm.product_counts() == (1, 0, 1)
    Tm = Am.transpose()
    same_csr(Tm.csr(), sg.transpose(A, 53))
    same_csr(Tm.csr(), orc.csr_transpose(A[0], A[1], A[2], 53))
    assert Tm.local_size() == (53, 37) and Tm.product_counts() == (1, 0, 1)


def test_host_route_symbolic_then_numeric(P, host_route):
    A, B = sg.rect_pair(8)
    Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
    Cm = P.Mat()
    host_route.MatMatMultSymbolic(Am.h, Bm.h, float(P.PETSC_DEFAULT), C.byref(Cm.h))
    ref = sg.matmult(A, B)
    got = Cm.csr()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[2].any() and Cm.product_counts() == (1, 0, 0)
    host_route.MatMatMultNumeric(Am.h, Bm.h, Cm.h)
    same_csr(Cm.csr(), ref)


def p7_and_p(weights=None):
    A = orc.gen_p7(8, 8, 8)
    return A, sg.aggregation_p(8, 8, 8, weights)


def test_host_route_ptap_poisson_aggregation(P, host_route):
    A, Pc = p7_and_p()
    Am, Pm = P.Mat.from_csr(*A), P.Mat.from_csr(*Pc, ncols=64)
    Cm = Am.ptap(Pm)
    ref = sg.ptap(A, Pc, 64)
    same_csr(Cm.csr(), ref)
    assert Cm.local_size() == (64, 64)
    ci, cj, ca = Cm.csr()                                      # small integers: exact, so symmetric and with the fine operator's sums
    dense = np.zeros((64, 64)); dense[np.repeat(np.arange(64), np.diff(ci)), cj] = ca
    assert np.array_equal(dense, dense.T) and dense.sum() == A[2].sum() and np.all(np.diag(dense) > 0)
    Am.shift(0.5)
    A2 = (A[0], A[1], Am.csr()[2])
    assert Am.ptap(Pm, reuse=Cm) is Cm
    same_csr(Cm.csr(), sg.ptap(A2, Pc, 64))
    assert Cm.product_counts() == (1, 0, 2)


def test_host_route_ptap_random_weights(P, host_route):
    w = np.random.default_rng(17).standard_normal(512)
    A, Pc = p7_and_p(w)
    A = (A[0], A[1], A[2] * (1.0 + 0.01 * np.cos(np.arange(A[2].size))))
    Cm = P.Mat.from_csr(*A).ptap(P.Mat.from_csr(*Pc, ncols=64))
    same_csr(Cm.csr(), sg.ptap(A, Pc, 64))


def test_order_of_the_sum_is_the_sequential_loops(P, host_route):
    A, B = sg.order_sensitive_pair()
    fwd, rev = sg.matmult(A, B), sg.matmult(A, B, reverse=True)
    assert np.any(bits(fwd[2]) != bits(rev[2])), "the case does not tell the two orders apart"
    same_csr(P.Mat.from_csr(*A, ncols=3).matmult(P.Mat.from_csr(*B, ncols=4)).csr(), fwd)


def test_specials_nothing_is_skipped(P, host_route):
    A = (np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([0.0, 2.0, -0.0]))
    B = (np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([np.inf, 1.0, -np.inf]))
    got = P.Mat.from_csr(*A, ncols=2).matmult(P.Mat.from_csr(*B, ncols=2)).csr()
    same_csr((got[0], got[1], np.where(np.isnan(got[2]), 0.0, got[2])), (np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([0.0, -np.inf, 0.0])))
    assert np.array_equal(np.isnan(got[2]), [True, False, True])          # 0.0 * Inf and -0.0 * -Inf


# ---------------------------------------------------------------------------------------------------- reuse, errors
def test_reuse_counts_and_value_changes(P, host_route):
    A, B = sg.rect_pair(9)
    Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
    Cm, Tm = Am.matmult(Bm), Am.transpose()
    for k in range(2, 5):
        host_route.MatScale(Am.h, 1.0 + 0.25 * k)
        A = (A[0], A[1], Am.csr()[2])
        Am.matmult(Bm, reuse=Cm); Am.transpose(reuse=Tm)
        same_csr(Cm.csr(), sg.matmult(A, B)); same_csr(Tm.csr(), sg.transpose(A, 53))
        assert Cm.product_counts() == (1, 0, k) and Tm.product_counts() == (1, 0, k)


def test_error_codes(P, host_route):
    A, B = sg.rect_pair()
    Am, Bm = P.Mat.from_csr(*A, ncols=53), P.Mat.from_csr(*B, ncols=41)
    raises(P, ARG_SIZ, lambda: Bm.matmult(Am))                              # 53 x 41 times 37 x 53
    raises(P, ARG_SIZ, lambda: Am.ptap(Bm))                                 # A is not square
    sq = sg.random_csr(53, 53, np.full(53, 3), 4)
    Sm = P.Mat.from_csr(*sq)
    raises(P, ARG_SIZ, lambda: Sm.ptap(P.Mat.from_csr(*A, ncols=53)))       # P has 37 rows
    Cm = Am.matmult(Bm)
    raises(P, ARG_WRONG, lambda: Am.matmult(Bm, reuse=Bm))                  # a matrix no product made
    raises(P, ARG_WRONG, lambda: Sm.matmult(Bm, reuse=Cm))                  # other operands
    raises(P, ARG_WRONG, lambda: Am.transpose(reuse=Cm))                    # the result of another operation
    raises(P, ARG_WRONG, lambda: Sm.ptap(Bm, reuse=Cm))
    raises(P, ARG_WRONG, lambda: P.Mat.from_csr(*A, ncols=53).matmult(Bm, reuse=Cm))   # an equal matrix is not the operand
    bs = P.Mat.from_bsr(2, np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.arange(8.0))
    raises(P, ERR_SUP, lambda: bs.matmult(bs))
    raises(P, ERR_SUP, lambda: bs.transpose())
    raises(P, ERR_SUP, lambda: bs.ptap(bs))
    sq4 = P.Mat.from_csr(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4))
    raises(P, ERR_SUP, lambda: sq4.matmult(bs))                             # operands of different types
    mp = P.Mat.from_csr_mpi(np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4), 4)
    raises(P, ERR_SUP, lambda: mp.matmult(mp))
    raises(P, ERR_SUP, lambda: mp.transpose())
    raises(P, ERR_SUP, lambda: mp.ptap(mp))
    raises(P, ARG_WRONG, lambda: (host_route.PetscOptionsSetValue(b"-mat_hipmi355x_product", b"gpu"), Am.matmult(Bm)))
