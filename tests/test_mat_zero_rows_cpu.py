"""MatZeroRows / MatZeroRowsColumns / MatSetOption without a GPU: the declarations, slots and exports of the new names, the wrappers'
argument errors, and the host copy of a matrix that was never used on the device (it takes the host route alone).  The numpy side of both
operations lives here and serves the GPU tests too: a plain loop per row, so the order of the right-hand-side correction and its two
roundings are the contract's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
import problems as pb
from test_mat_value_ops_cpu import bits, host_pattern, host_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SUP, ARG_SIZ, ARG_IDN, ARG_WRONG, ARG_OUTOFRANGE, ARG_WRONGSTATE = 56, 60, 61, 62, 63, 73


# ---------------------------------------------------------------------------------------------------- the contract in numpy
def ref_zero_rows(ai, aj, aa, rows, diag, x=None, b=None):
    """MatZeroRows with MAT_KEEP_NONZERO_PATTERN: every stored entry of a listed row +0.0, then diag on its diagonal when diag != 0"""
    aa = np.array(aa, dtype=np.float64)
    b = None if b is None else np.array(b, dtype=np.float64)
    diag = np.float64(diag)
    with np.errstate(all="ignore"):
        for r in sorted(set(int(r) for r in rows)):
            for k in range(ai[r], ai[r + 1]):
                aa[k] = diag if (diag != 0 and aj[k] == r) else 0.0
            if b is not None:
                b[r] = diag * x[r]
    return aa, b


def ref_zero_rows_columns(ai, aj, aa, rows, diag, x=None, b=None):
    """MatZeroRowsColumns: in every row that is not listed, in stored order, an entry in a listed column gives b[i] = b[i] - a_ij * x[col]
    (product, then difference: two roundings) and becomes +0.0; then the listed rows as above"""
    aa = np.array(aa, dtype=np.float64)
    b = None if b is None else np.array(b, dtype=np.float64)
    n = len(ai) - 1
    listed = np.zeros(n, bool)
    listed[np.asarray(rows, dtype=np.int64)] = True
    with np.errstate(all="ignore"):
        for i in range(n):
            if listed[i]:
                continue
            for k in range(ai[i], ai[i + 1]):
                if listed[aj[k]]:
                    if b is not None:
                        p = np.float64(aa[k]) * np.float64(x[aj[k]])
                        b[i] = np.float64(b[i]) - p
                    aa[k] = 0.0
    return ref_zero_rows(ai, aj, aa, rows, diag, x, b)


def ref_zero_rows_new_pattern(ai, aj, aa, rows, diag):
    """MatZeroRows in its default mode: a listed row keeps (r, r) = diag when diag != 0 and nothing otherwise"""
    n = len(ai) - 1
    listed = np.zeros(n, bool)
    listed[np.asarray(rows, dtype=np.int64)] = True
    ni, nj, na = [0], [], []
    for r in range(n):
        if listed[r]:
            if diag != 0:
                nj.append(r); na.append(diag)
        else:
            nj.extend(aj[ai[r]:ai[r + 1]]); na.extend(aa[ai[r]:ai[r + 1]])
        ni.append(len(nj))
    return np.array(ni, np.int32), np.array(nj, np.int32), np.array(na, np.float64)


def arrow(n=300, empty=7):
    """first row and first column dense (row 0 is longer than a lane group and than a wavefront), a diagonal, and one row -- `empty` --
    with nothing beside its diagonal entry"""
    ai, aj, aa = [0], [], []
    for r in range(n):
        cols = list(range(n)) if r == 0 else ([r] if r == empty else [0, r])
        aj.extend(cols)
        aa.extend(2.0 + np.cos(1.3 * r + 0.7 * c) for c in cols)
        ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64)


def perturbed(csr):
    ai, aj, aa = csr
    return ai.astype(np.int32), aj.astype(np.int32), aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


# ---------------------------------------------------------------------------------------------------- names
def test_new_names_are_declared_and_exported(built):
    mini = open(os.path.join(ROOT, "include", "petscmini.h")).read()
    harness = built.load_harness()
    for n in ("MatZeroRows", "MatZeroRowsColumns", "MatSetOption"):
        assert re.search(r"PetscErrorCode\s+%s\s*\(" % n, mini), n
        assert hasattr(harness, n), n
    assert re.search(r"\bMAT_KEEP_NONZERO_PATTERN\b", mini) and re.search(r"\}\s*MatOption\s*;", mini)
    impl = open(os.path.join(ROOT, "petsc-dev_amd", "harness", "petscimpl.h")).read()
    zr = r"\(Mat,\s*PetscInt,\s*const PetscInt\s*\[\],\s*PetscScalar,\s*Vec,\s*Vec\)"
    for slot, sig in (("zerorows", zr), ("zerorowscolumns", zr), ("setoption", r"\(Mat,\s*MatOption,\s*PetscBool\)")):
        assert re.search(r"PetscErrorCode\s*\(\*%s\)%s;" % (slot, sig), impl), slot
    for frag in ("aijhipmi355x_ctor.h", "mpiaijhipmi355x_ctor.h"):
        t = open(os.path.join(ROOT, "integration", "petsc-3.3", frag)).read()
        for slot in ("zerorows", "zerorowscolumns"):
            assert re.search(r"B->ops->%s\s*=" % slot, t), (frag, slot)
    kh = open(os.path.join(ROOT, "include", "mi355x_kernels.h")).read()
    from petsc_dev_amd._lib import KERNEL_API
    k = built.load_kernels()
    for n in ("mi355x_csr_zero_rows", "mi355x_csr_zero_columns"):
        assert re.search(r"\bint\s+%s\s*\(" % n, kh), n
        assert hasattr(k, n), n
        assert n in KERNEL_API
    ph = open(os.path.join(ROOT, "include", "petschipmi355x.h")).read()
    assert re.search(r"PetscErrorCode\s+MatHIPMI355XGetZeroRowsCounts\s*\(", ph)
    built.load_kernels()
    assert hasattr(C.CDLL(built.host_lib_path()), "MatHIPMI355XGetZeroRowsCounts")


# ---------------------------------------------------------------------------------------------------- the wrappers' errors
def raises(P, code, call):
    with pytest.raises(P.PetscError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("op", ["zero_rows", "zero_rows_columns"])
def test_argument_errors(P, op):
    L = P.lib()
    ai, aj, aa = perturbed(pb.lap2d(7, 5))
    n = ai.size - 1
    for keep in (False, True):
        A = P.Mat.from_csr(ai, aj, aa)
        A.set_option(P.MAT_KEEP_NONZERO_PATTERN, keep)
        A.set_option(2, True)                               # MAT_SYMMETRIC: declared, accepted, without effect
        f = getattr(A, op)
        x, b = P.Vec.create(n, comm=L.COMM_SELF), P.Vec.create(n, comm=L.COMM_SELF)
        raises(P, ARG_WRONG, lambda: f([1, 2], 1.0, x=x))   # x without b
        raises(P, ARG_WRONG, lambda: f([1, 2], 1.0, b=b))
        raises(P, ARG_IDN, lambda: f([1, 2], 1.0, x=x, b=x))
        short = P.Vec.create(n - 1, comm=L.COMM_SELF)
        raises(P, ARG_SIZ, lambda: f([1, 2], 1.0, x=x, b=short))
        for bad in ([0, n], [-1], [3, 2 * n, 1]):
            raises(P, ARG_OUTOFRANGE, lambda: f(bad, 1.0))
        assert np.array_equal(bits(host_values(P, A, aa.size)), bits(aa)), "an error must leave the values alone"
        gi, gj = host_pattern(P, A)
        assert np.array_equal(gi, ai) and np.array_equal(gj, aj)
        raises(P, ARG_OUTOFRANGE, lambda: L.MatSetOption(A.h, 1000, 1))
        # an unassembled matrix
        i0, v = np.array([0], np.int32), np.array([1.0])
        L.MatSetValues(A.h, 1, i0.ctypes.data_as(C.c_void_p), 1, i0.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), P.INSERT_VALUES)
        raises(P, ARG_WRONGSTATE, lambda: f([1], 1.0))
        A.destroy()


def test_missing_diagonal_and_shapes(P):
    ai, aj, aa = perturbed(pb.lap2d(7, 5))
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    keep = ~((rows == aj) & (rows == 9))
    xi = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    A = P.Mat.from_csr(xi, aj[keep], aa[keep])
    A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
    # the whole matrix is asked (MatMissingDiagonal), not the listed rows alone; diag == 0 and -0.0 do not ask
    assert "row 9" in raises(P, ARG_WRONGSTATE, lambda: A.zero_rows([1, 2], 1.0))
    assert "row 9" in raises(P, ARG_WRONGSTATE, lambda: A.zero_rows_columns([1, 2], 2.5))
    assert np.array_equal(bits(host_values(P, A, int(keep.sum()))), bits(aa[keep]))
    A.zero_rows([1, 2], -0.0)
    ref, _ = ref_zero_rows(xi, aj[keep], aa[keep], [1, 2], -0.0)
    assert np.array_equal(bits(host_values(P, A, ref.size)), bits(ref))
    # not square
    ri = np.array([0, 2, 3, 5], np.int32); rj = np.array([0, 3, 1, 2, 4], np.int32); ra = np.arange(1.0, 6.0)
    R = P.Mat.from_csr(ri, rj, ra, ncols=5)
    raises(P, ARG_SIZ, lambda: R.zero_rows_columns([0], 0.0))
    for k in (False, True):
        R.set_option(P.MAT_KEEP_NONZERO_PATTERN, k)
        raises(P, ERR_SUP, lambda: R.zero_rows([0], 1.0))
    assert np.array_equal(bits(host_values(P, R, 5)), bits(ra))
    R.zero_rows([2, 0], 0.0)                                # the option is set: the pattern stays
    assert np.array_equal(bits(host_values(P, R, 5)), bits(np.array([0.0, 0.0, 3.0, 0.0, 0.0])))
    # BAIJ
    bi, bj, _ = pb.lap2d(3, 2)
    B = P.Mat.from_bsr(2, bi, bj, np.ones(bj.size * 4))
    raises(P, ERR_SUP, lambda: B.zero_rows([0], 1.0))
    raises(P, ERR_SUP, lambda: B.zero_rows_columns([0], 1.0))


# ---------------------------------------------------------------------------------------------------- the host copy
LISTS = {"empty": lambda n: [], "first": lambda n: [0], "last": lambda n: [n - 1], "straddle": lambda n: [255, 256],
         "all": lambda n: list(range(n)), "dups": lambda n: [5, 17, 5, n - 1, 17, 5, 0]}


@pytest.mark.parametrize("name", ["lap2d", "arrow"])
def test_host_copy(P, name):
    ai, aj, aa = perturbed(pb.lap2d(23, 19)) if name == "lap2d" else arrow()
    n = ai.size - 1
    for lname, mk in LISTS.items():
        rows = mk(n)
        for diag in (0.0, 1.0, 2.5):
            A = P.Mat.from_csr(ai, aj, aa)
            A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
            A.zero_rows(rows, diag)
            ref, _ = ref_zero_rows(ai, aj, aa, rows, diag)
            assert np.array_equal(bits(host_values(P, A, aa.size)), bits(ref)), (name, lname, diag)
            D = P.Mat(C.c_void_p(), own=True)
            P.lib().MatDuplicate(A.h, 1, C.byref(D.h))      # the option goes along: the copy keeps its pattern too
            D.zero_rows([1], 0.0)
            assert np.array_equal(host_pattern(P, D)[0], ai)
            B = P.Mat.from_csr(ai, aj, aa)                  # MatZeroRowsColumns keeps the pattern without the option
            B.zero_rows_columns(rows, diag)
            ref, _ = ref_zero_rows_columns(ai, aj, aa, rows, diag)
            assert np.array_equal(bits(host_values(P, B, aa.size)), bits(ref)), (name, lname, diag)
            gi, gj = host_pattern(P, B)
            assert np.array_equal(gi, ai) and np.array_equal(gj, aj)
            E = P.Mat.from_csr(ai, aj, aa)                  # the default: the pattern shrinks
            E.zero_rows(rows, diag)
            ni, nj, na = ref_zero_rows_new_pattern(ai, aj, aa, rows, diag)
            gi, gj = host_pattern(P, E)
            assert np.array_equal(gi, ni) and np.array_equal(gj, nj), (name, lname, diag)
            assert np.array_equal(bits(host_values(P, E, na.size)), bits(na)), (name, lname, diag)
            for o in (A, B, D, E):
                o.destroy()


def test_default_mode_inserts_the_diagonal_of_an_empty_row(P):
    """a listed row without any slot gets one (MatSetValues of the reference's loop); a row whose only entry is off the diagonal has it
    replaced"""
    ai = np.array([0, 2, 2, 3, 5], np.int32); aj = np.array([0, 1, 3, 0, 3], np.int32); aa = np.arange(1.0, 6.0)
    A = P.Mat.from_csr(ai, aj, aa)
    A.zero_rows([1, 2], 7.0)
    gi, gj = host_pattern(P, A)
    assert list(gi) == [0, 2, 3, 4, 6] and list(gj) == [0, 1, 1, 2, 0, 3]
    assert list(host_values(P, A, 6)) == [1.0, 2.0, 7.0, 7.0, 4.0, 5.0]
    A.zero_rows([0, 1], 0.0)
    gi, gj = host_pattern(P, A)
    assert list(gi) == [0, 0, 0, 1, 3] and list(gj) == [2, 0, 3]
