"""Run-coded row patterns, the host side (no GPU): the descriptors mi355x_spmv_pattern_runs_host builds from the rows' words -- the
routine the analysis in mi355x_spmv_plan_compress_indices calls -- against the runs recomputed in numpy from (ai, aj, block cuts):
run starts, table starts, first nonzeros, lengths, unused runs, and the fallback for a block of more than four runs."""
import ctypes as C

import numpy as np
import pytest

import pattern_runs as pr


def host_runs(k, cuts, ai, prow, pattab):
    nb = cuts.size - 1
    rowblk = np.ascontiguousarray(np.stack((cuts, ai[cuts]), axis=1), dtype=np.int32)      # {first row, first nonzero} per block
    runs = np.full(8 * nb, 0xDEADBEEF, dtype=np.uint32)
    ncoded = C.c_int(-1)
    rc = k.mi355x_spmv_pattern_runs_host(nb, rowblk.ctypes.data, prow.ctypes.data, pattab.ctypes.data, runs.ctypes.data, C.byref(ncoded))
    assert rc == 0
    return runs.reshape(nb, pr.RUNS, 2), ncoded.value


@pytest.mark.parametrize("name", pr.MATRICES)
def test_run_descriptors_equal_the_runs_recomputed_from_the_pattern(built, name):
    k = built.load_kernels()
    ai, aj, _, _ = pr.matrix(name)
    cuts = pr.block_cuts(ai)
    prow, pattab, start_of = pr.row_words(ai, aj, cuts)
    ref = pr.runs_reference(ai, aj, cuts)
    got, ncoded = host_runs(k, cuts, ai, prow, pattab)
    assert ncoded == sum(r is not None for r in ref)
    for b, runs in enumerate(ref):
        n = 0 if runs is None else len(runs)
        for i, (first, key, nz0) in enumerate(runs or []):
            w, rn = int(got[b, i, 0]), int(got[b, i, 1])
            assert (rn & 0xffff, w & 0xffff, w >> 16, rn >> 16) == (first, start_of[key], nz0, len(key)), (name, b, i)
        assert np.all(got[b, n:, 0] == 0) and np.all(got[b, n:, 1] == pr.RUN_NONE), (name, b)      # unused runs: no lane reaches their first row
        assert runs is None or runs[0][0] == 0                                                   # a coded block's first run starts at row 0
    # what each shape is there for
    nb = cuts.size - 1
    expect = {"p7_256_2_2": (4, 4), "p7_300_3_2": (8, 8), "p7_8_8_8": (2, 0), "stack": (6, 3), "stack_empty": (6, 3), "lap257": (2, 2), "lap256": (1, 1)}
    assert (nb, ncoded) == expect[name]
    if name == "p7_256_2_2":
        assert all(len(r) == 3 for r in ref)                             # a block is one grid line: first row, interior, last row
    if name == "p7_300_3_2":
        # lines of 300 rows cut every 256: a block holds the start of a line, a line's end and the next one's start, or interior rows only
        assert [len(r) for r in ref] == [2, 4, 4, 4, 4, 4, 1, 2] and cuts[-1] - cuts[-2] == 8
    if name == "stack":
        assert [None if r is None else len(r) for r in ref] == [2, 2, 3, None, None, None]
    if name == "stack_empty":
        assert [None if r is None else [len(key) for _, key, _ in r] for r in ref[:3]] == [[2, 3, 0, 3], [3, 0, 3, 2], [0, 3, 0]]
    if name == "lap257":
        assert cuts.tolist() == [0, 256, 257]


def test_run_descriptors_refuse_missing_arrays(built):
    k = built.load_kernels()
    assert k.mi355x_spmv_pattern_runs_host(1, None, None, None, None, None) != 0
    assert k.mi355x_spmv_pattern_runs_host(-1, None, None, None, None, None) != 0
    n = C.c_int(7)
    assert k.mi355x_spmv_pattern_runs_host(0, None, None, None, None, C.byref(n)) == 0 and n.value == 0
