"""The launch plan of the fused-level block solves without a GPU: mi355x_bilu_chain_plan_host (csrc/bilu.hip) against a restatement of
its rule on seeded random lists of level sizes, the properties the plan has by that rule, its error codes, and the export of the three
new entry points."""
import ctypes as C

import numpy as np
import pytest

INVALID = 1                                     # hipErrorInvalidValue
MARK = -77


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def plan_ref(sizes, max_rows):
    """[(l0, l1, fused)]: every maximal run of levels of at most max_rows rows is one fused segment, every other level stands alone"""
    segs = []
    for l, n in enumerate(sizes):
        narrow = max_rows > 0 and n <= max_rows
        if narrow and segs and segs[-1][2] and segs[-1][1] == l:
            segs[-1] = (segs[-1][0], l + 1, 1)
        else:
            segs.append((l, l + 1, 1 if narrow else 0))
    return segs


def plan_lib(k, sizes, max_rows):
    """(rc, [(l0, l1, fused)]) of the library; the slots behind the plan keep their marker"""
    nlev = len(sizes)
    levptr = _i32(np.concatenate(([0], np.cumsum(sizes, dtype=np.int64))))
    seg_ptr, seg_fused, nseg = np.full(nlev + 3, MARK, np.int32), np.full(nlev + 2, MARK, np.int32), C.c_int(MARK)
    rc = k.mi355x_bilu_chain_plan_host(nlev, levptr.ctypes.data, max_rows, seg_ptr.ctypes.data, seg_fused.ctypes.data, C.byref(nseg))
    ns = nseg.value
    if rc == 0:
        assert 0 <= ns <= nlev
        if nlev:
            assert (seg_ptr[ns + 1:] == MARK).all() and (seg_fused[ns:] == MARK).all()
        else:
            assert (seg_ptr == MARK).all() and (seg_fused == MARK).all()
    return rc, [(int(seg_ptr[s]), int(seg_ptr[s + 1]), int(seg_fused[s])) for s in range(ns)] if rc == 0 else None


def random_cases():
    rng = np.random.default_rng(20)
    for max_rows in (1, 2, 3, 256, 1024):
        pool = [0, 1, 2, max_rows - 1, max_rows, max_rows + 1, 10 * max_rows]
        for nlev in list(range(0, 12)) + [int(v) for v in rng.integers(12, 201, size=12)] + [200]:
            yield max_rows, [int(pool[j]) for j in rng.integers(0, len(pool), size=nlev)]


def test_the_plan_equals_its_restatement_and_has_its_properties(built):
    k = built.load_kernels()
    seen_mixed = 0
    for max_rows, sizes in random_cases():
        rc, segs = plan_lib(k, sizes, max_rows)
        assert rc == 0
        assert segs == plan_ref(sizes, max_rows), (max_rows, sizes)
        nlev = len(sizes)
        # the segments partition [0, nlev) in order
        assert [s[0] for s in segs] == ([0] + [s[1] for s in segs[:-1]] if segs else [])
        assert (segs[-1][1] if segs else 0) == nlev and all(l0 < l1 for l0, l1, _ in segs)
        for q, (l0, l1, fused) in enumerate(segs):
            if fused:
                assert all(sizes[l] <= max_rows for l in range(l0, l1))                 # only narrow levels ...
                assert l0 == 0 or sizes[l0 - 1] > max_rows                              # ... and maximal on both sides
                assert l1 == nlev or sizes[l1] > max_rows
            else:
                assert l1 == l0 + 1 and sizes[l0] > max_rows                            # a wide level stands alone
        seen_mixed += len({f for _, _, f in segs}) == 2
    assert seen_mixed > 20


@pytest.mark.parametrize("max_rows", [0, -1, -1000])
def test_no_level_is_narrow_without_a_positive_bound(built, max_rows):
    k = built.load_kernels()
    for sizes in ([], [0], [0, 0, 3, 1, 0], [5] * 40):
        rc, segs = plan_lib(k, sizes, max_rows)
        assert rc == 0 and segs == [(l, l + 1, 0) for l in range(len(sizes))]


def test_no_levels_no_segments_and_one_run_is_one_segment(built):
    k = built.load_kernels()
    nseg = C.c_int(MARK)
    assert k.mi355x_bilu_chain_plan_host(0, None, 256, None, None, C.byref(nseg)) == 0 and nseg.value == 0
    assert plan_lib(k, [], 256) == (0, [])
    assert plan_lib(k, [3], 256) == (0, [(0, 1, 1)])
    assert plan_lib(k, [300], 256) == (0, [(0, 1, 0)])
    assert plan_lib(k, [1, 0, 256, 7], 256) == (0, [(0, 4, 1)])
    assert plan_lib(k, [1, 257, 0, 2, 300, 300, 9], 256) == (0, [(0, 1, 1), (1, 2, 0), (2, 4, 1), (4, 5, 0), (5, 6, 0), (6, 7, 1)])


def test_documented_errors(built):
    k = built.load_kernels()
    good = _i32([0, 2, 5, 5, 9])
    sp, sf, nseg = np.full(5, MARK, np.int32), np.full(4, MARK, np.int32), C.c_int(MARK)

    def call(nlev, levptr, a=sp, b=sf, n=nseg):
        return k.mi355x_bilu_chain_plan_host(nlev, None if levptr is None else levptr.ctypes.data, 4, None if a is None else a.ctypes.data,
                                             None if b is None else b.ctypes.data, None if n is None else C.byref(n))
    assert call(4, good) == 0 and nseg.value == 1
    assert call(4, None) == INVALID and nseg.value == 0                    # NULL levptr with levels to plan
    assert call(4, _i32([0, 2, 1, 5, 9])) == INVALID                       # decreasing
    assert call(4, _i32([0, 2, 5, 5, 4])) == INVALID
    assert call(-1, good) == INVALID
    assert call(4, good, a=None) == INVALID and call(4, good, b=None) == INVALID and call(4, good, n=None) == INVALID
    sp[:] = MARK; sf[:] = MARK
    assert call(4, _i32([0, 2, 1, 5, 9])) == INVALID and (sp == MARK).all() and (sf == MARK).all()      # refused before anything is written


def test_new_symbols_are_exported_declared_and_bound(built):
    import os
    import subprocess
    from petsc_dev_amd import _lib
    from petsc_dev_amd import petsc as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["nm", "-D", "--defined-only", built.kernels_lib_path()], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "include", "mi355x_kernels.h")).read()
    for name in ("mi355x_bilu_lower_chain", "mi355x_bilu_upper_chain", "mi355x_bilu_chain_plan_host"):
        assert (" T " + name) in out and name in header and name in _lib.KERNEL_API, name
    host = subprocess.run(["nm", "-D", "--defined-only", built.host_lib_path()], capture_output=True, text=True, check=True).stdout
    assert " T PCBILUGetSolvePlan_HIPMI355X" in host
    assert "PCBILUGetSolvePlan_HIPMI355X" in open(os.path.join(root, "include", "petschipmi355x.h")).read()
    assert "PCBILUGetSolvePlan_HIPMI355X" in open(P.__file__).read()
