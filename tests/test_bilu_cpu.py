"""Block ILU(k) without a GPU: the host numeric factorisation of csrc/bilu.hip (mi355x_bilu_numeric_host) against the restatement in
tests/bilu_ref.py bit for bit, that restatement pinned against the point reference (iluk_ref) on a matrix of scaled identity blocks and
against numpy's dense solve on a block-tridiagonal matrix, and the error paths of the host routines."""
import ctypes as C

import numpy as np
import pytest

import bilu_ref as br
import iluk_ref as ik
import problems as pb
from iluk_ref import bits

INVALID = 1                                     # hipErrorInvalidValue
MARK = -7.25
BLOCK_SIZES = [2, 3, 4, 5, 7]


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def numeric_lib(k, bs, ai, aj, aa, layout, fill=MARK):
    """(rc, ba, zero-pivot row) of the library routine on a ba pre-filled with a marker"""
    ai, aj, aa = _i32(ai), _i32(aj), np.ascontiguousarray(aa, dtype=np.float64)
    bi, bj, bd = (_i32(a) for a in layout[:3])
    mbs = ai.size - 1
    ba = np.full((int(bd[0]) + 2) * bs * bs, fill)
    z = C.c_int(-9)
    rc = k.mi355x_bilu_numeric_host(mbs, bs, ai.ctypes.data, aj.ctypes.data, aa.ctypes.data, bi.ctypes.data, bj.ctypes.data, bd.ctypes.data,
                                    ba.ctypes.data, C.byref(z))
    return rc, ba, z.value


def cases(bs):
    return [("elasticity_like(3,3,2)", pb.elasticity_like(3, 3, 2, dof=bs)[1]), ("block tridiagonal, 9 rows", br.block_tridiag(9, bs))]


# ---------------------------------------------------------------- 1. the host routine against the reference
@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_host_numeric_equals_the_reference_bit_for_bit(built, bs, levels):
    k = built.load_kernels()
    for name, (ai, aj, aa) in cases(bs):
        lay = br.symbolic(ai, aj, levels)
        ref, zref = br.numeric(bs, ai, aj, aa, lay)
        rc, ba, z = numeric_lib(k, bs, ai, aj, aa, lay)
        nv = (int(lay[2][0]) + 1) * bs * bs
        assert rc == 0 and z == -1 and zref == -1, (name, rc, z, zref)
        assert np.array_equal(bits(ba[:nv]), bits(ref[:nv])), name
        assert (ba[nv:] == MARK).all(), "%s: the block past the last one was written" % name
        if levels and name.startswith("elasticity"):
            assert int(lay[2][0]) + 1 > int(ai[-1]), "no fill at level 1?"


# ---------------------------------------------------------------- 2. the reference pinned without trusting itself
@pytest.mark.parametrize("levels", [0, 1])
@pytest.mark.parametrize("bs", [2, 3, 5])
def test_scaled_identity_blocks_give_the_point_factor(bs, levels):
    """blocks a_ij I_bs on the node pattern of lap2d(4, 3): the block factor's blocks are f_ij I_bs with f the point factor's values --
    every extra term of a block product is an exact zero, so a wrong summation order or a wrong operand shows"""
    ai, aj, aa = pb.lap2d(4, 3)
    aa = aa * (1.0 + 0.05 * np.sin(np.arange(aa.size)))
    lay = ik.symbolic(ai, aj, levels)
    f, frow, _, _ = ik.reference_pass(ai, aj, aa, None, [0.0], 0.0, [1], layout=lay)
    assert frow[0] == -1
    eye = np.eye(bs).ravel()
    ba, z = br.numeric(bs, ai, aj, np.concatenate([a * eye for a in aa]), lay[:3])
    assert z == -1
    nzb = int(lay[2][0]) + 1
    blocks = ba[:nzb * bs * bs].reshape(nzb, bs, bs)
    off = ~np.eye(bs, dtype=bool)
    for q in range(nzb):
        assert (np.diag(blocks[q]) == f[q]).all(), (q, blocks[q], f[q])          # == on values: a -0.0 from 0 * x does not count
        assert (blocks[q][off] == 0.0).all(), (q, blocks[q])


# ---------------------------------------------------------------- 3. block tridiagonal: ILU(0) is the complete LU
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_block_tridiagonal_solve_is_as_good_as_a_dense_solve(bs):
    """Residual ||b - A x||inf / (||A||inf ||x||inf) of the reference's application against numpy.linalg.solve's on the expanded matrix: a
    factor of 16 over numpy's value is allowed (pivoting inside blocks only is weaker than full partial pivoting; the diagonal blocks
    are dominant, so it is stable), never an absolute number."""
    bi, bj, ba = br.block_tridiag(9, bs)
    lay = br.symbolic(bi, bj, 0)
    f, z = br.numeric(bs, bi, bj, ba, lay)
    assert z == -1
    A = br.dense_of(bs, bi, bj, ba)
    b = np.cos(0.7 * np.arange(9 * bs)) + 0.3
    x = br.apply(bs, lay, f, b)
    xn = np.linalg.solve(A, b)

    def res(v):
        return float(np.abs(b - A @ v).max() / (np.abs(A).sum(1).max() * np.abs(v).max()))
    print("bs = %d: scaled residual of the block ILU(0) solve %.3e, of numpy.linalg.solve %.3e" % (bs, res(x), res(xn)))
    assert res(x) <= 16.0 * max(res(xn), np.finfo(float).eps / 16.0)


# ---------------------------------------------------------------- 4. error paths
def zero_pivot_case(bs=3):
    """four block rows: 0 and 1 a random dominant pair; row 2 = [I, U], row 3 = [L, L U + S] with small integers, S = diag(2, 0, 3):
    the elimination leaves exactly S in the last diagonal block, whose second pivot is zero -> scalar row 3 bs + 1"""
    rng = np.random.default_rng(5)
    t = br.block_tridiag(2, bs)
    L = rng.integers(-3, 4, (bs, bs)).astype(float); U = rng.integers(-3, 4, (bs, bs)).astype(float)
    S = np.zeros((bs, bs)); S[0, 0] = 2.0; S[2, 2] = 3.0
    bi = np.array([0, 2, 4, 6, 8], np.int32)
    bj = np.array([0, 1, 0, 1, 2, 3, 2, 3], np.int32)
    cm = lambda B: np.ascontiguousarray(B.T).ravel()          # noqa: E731 (column-major)
    ba = np.concatenate([t[2], cm(np.eye(bs)), cm(U), cm(L), cm(L @ U + S)])
    return bi, bj, ba, 3 * bs + 1


def test_zero_pivot_reports_the_scalar_row_and_keeps_the_rows_before_it(built):
    k = built.load_kernels()
    bs = 3
    bi, bj, ba, row = zero_pivot_case(bs)
    lay = br.symbolic(bi, bj, 0)
    ref, zref = br.numeric(bs, bi, bj, ba, lay)
    assert zref == row
    rc, got, z = numeric_lib(k, bs, bi, bj, ba, lay)
    assert rc != 0 and z == row
    before = np.zeros((int(lay[2][0]) + 2), dtype=bool)
    for i in range(3):                                           # every slot of the block rows 0 .. 2
        before[lay[0][i]:lay[0][i + 1]] = True
        before[lay[2][i + 1] + 1:lay[2][i] + 1] = True
    m = np.repeat(before, bs * bs)
    assert np.array_equal(bits(got[m]), bits(ref[m]))


def test_documented_errors(built):
    k = built.load_kernels()
    bi, bj, ba = br.block_tridiag(4, 2)
    lay = br.symbolic(bi, bj, 0)
    for bs in (1, 8):                                            # block sizes this route does not serve: nothing written
        vals = np.ones(bj.size * bs * bs)
        rc, got, z = numeric_lib(k, bs, bi, bj, vals, lay)
        assert rc == INVALID and (got == MARK).all() and z == -1
    # a missing diagonal block and negative levels: the symbolic pass refuses, naming the row
    bi2, bj2 = [0], []
    for i in range(4):
        bj2 += [int(c) for c in bj[bi[i]:bi[i + 1]] if not (i == 2 and c == 2)]           # block row 2 loses its diagonal
        bi2.append(len(bj2))
    bi2, bj2 = _i32(bi2), _i32(bj2)
    obi, obd, bad = np.zeros(5, np.int32), np.zeros(5, np.int32), C.c_int(-9)
    assert k.mi355x_iluk_symbolic_host(4, bi2.ctypes.data, bj2.ctypes.data, 0, obi.ctypes.data, obd.ctypes.data, None, None, C.byref(bad)) == INVALID
    assert bad.value == 2
    assert k.mi355x_iluk_symbolic_host(4, bi.ctypes.data, bj.ctypes.data, -1, obi.ctypes.data, obd.ctypes.data, None, None, C.byref(bad)) == INVALID
    # a block of A that the factor's pattern lacks
    dense_i = np.arange(0, 17, 4, dtype=np.int32); dense_j = np.tile(np.arange(4, dtype=np.int32), 4)
    rc, got, z = numeric_lib(k, 2, dense_i, dense_j, np.ones(16 * 4), lay)
    assert rc == INVALID and z == -1


def test_new_symbols_are_exported_declared_and_bound(built):
    import os
    import subprocess
    from petsc_dev_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["nm", "-D", "--defined-only", built.kernels_lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "include", "mi355x_kernels.h")).read()
    for name in ("mi355x_bilu_lower_level", "mi355x_bilu_upper_level", "mi355x_bilu_numeric_host"):
        assert (" T " + name) in out and name in header and name in _lib.KERNEL_API, name
    host = subprocess.run(["nm", "-D", "--defined-only", built.host_lib_path()], capture_output=True, text=True, check=True).stdout
    assert " T PCBILUGetInfo_HIPMI355X" in host and "PCBILUGetInfo_HIPMI355X" in open(os.path.join(root, "include", "petschipmi355x.h")).read()
