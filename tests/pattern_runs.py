"""Host side of the run-coded row patterns' tests (test_spmv_pattern_runs_cpu.py, test_spmv_pattern_runs_gpu.py): the matrices, and
a few lines of numpy that recompute a row block's runs of equal patterns from (ai, aj, block cuts) alone.

The constants restate petsc-dev_amd/csrc/spmv_csr.hip: a row block is <= 256 rows and <= 2046 nonzeros (mi355x_spmv_plan_create),
a block's descriptor holds <= 4 runs, 8 words: per run {row word of its first row, first row in the block : 16 | length : 16},
a row word is {table start : 16 (low), first nonzero in the block : 16}, unused runs are {0, 0xffff}."""
import numpy as np

import orc

BLOCK_ROWS, BLOCK_CAP, RUNS, RUN_NONE = 256, 2046, 4, 0xffff


def lap1d_stack(lines, empty=()):
    """block-diagonal stack of 1-D 3-point Laplacians, one per line length in `lines`; the rows in `empty` keep no entry (their
    columns stay referenced by the neighbouring rows).  Values: random, mixed signs."""
    m = int(np.sum(lines))
    empty = set(int(r) for r in empty)
    ai, aj, lo = [0], [], 0
    for n in lines:
        for i in range(n):
            if lo + i not in empty:
                aj.extend(lo + j for j in (i - 1, i, i + 1) if 0 <= j < n)
            ai.append(len(aj))
        lo += n
    ai, aj = np.array(ai, dtype=np.int32), np.array(aj, dtype=np.int32)
    rng = np.random.default_rng(m + len(empty))
    return ai, aj, rng.standard_normal(aj.size) * 10.0 ** rng.integers(-2, 3, aj.size), m


STACK = [512] + [256] + 2 * [128] + 4 * [64] + 8 * [32]            # row blocks of 2, 2, 3, 6, 12, 24 runs
# zero-length patterns: inside a run-coded block (first, interior, EMPTY, interior), (interior, EMPTY, interior, last), at both ends
# of one (EMPTY, interior, EMPTY), and in blocks that keep their row words; some columns (101, 102, ...) are then referenced by no row
STACK_EMPTY = [100, 101, 102, 103, 300, 512, 513, 767, 896, 897, 898, 1100, 1279]


def matrix(name):
    """-> (ai, aj, aa, number of columns)"""
    if name.startswith("p7_"):
        ai, aj, aa = orc.gen_p7(*[int(t) for t in name.split("_")[1:]])
        return ai, aj, aa, ai.size - 1
    if name == "stack":
        return lap1d_stack(STACK)
    if name == "stack_empty":
        return lap1d_stack(STACK, STACK_EMPTY)
    if name == "lap257":                                            # a last block of one row
        return lap1d_stack([257])
    assert name == "lap256", name                                   # one block of exactly 256 rows
    return lap1d_stack([256])


MATRICES = ["p7_256_2_2", "p7_300_3_2", "p7_8_8_8", "stack", "stack_empty", "lap257", "lap256"]


def mixed(n, seed):
    """random values with mixed signs and magnitudes"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)


def block_cuts(ai):
    """first rows of the row blocks, as mi355x_spmv_plan_create cuts them (no row here is longer than a block)"""
    m, cuts, r = ai.size - 1, [0], 0
    while r < m:
        start = r
        while r < m and r - start < BLOCK_ROWS and ai[r + 1] - ai[start] <= BLOCK_CAP:
            r += 1
        assert r > start
        cuts.append(r)
    return np.array(cuts, dtype=np.int32)


def row_keys(ai, aj):
    """per row: its offsets col - row as a tuple (the row's pattern)"""
    return [tuple(int(c) - r for c in aj[ai[r]:ai[r + 1]]) for r in range(ai.size - 1)]


def runs_reference(ai, aj, cuts):
    """per row block: None when its rows form more than RUNS runs, else [(first row in the block, pattern, first nonzero in the
    block), ...] of its maximal runs of consecutive rows with one pattern"""
    keys = row_keys(ai, aj)
    out = []
    for b in range(cuts.size - 1):
        r0, r1 = int(cuts[b]), int(cuts[b + 1])
        starts = [r for r in range(r0, r1) if r == r0 or keys[r] != keys[r - 1]]
        out.append(None if len(starts) > RUNS else [(r - r0, keys[r], int(ai[r] - ai[r0])) for r in starts])
    return out


def row_words(ai, aj, cuts):
    """the analysis' inputs to the run coding, rebuilt here: the pattern table {length, offsets ...} in order of first appearance
    and the rows' words; -> (prow, pattab, {pattern: table start})"""
    keys = row_keys(ai, aj)
    start_of, tab = {}, []
    prow = np.zeros(ai.size - 1, dtype=np.uint32)
    blk = np.searchsorted(cuts, np.arange(ai.size - 1), side="right") - 1
    for r, key in enumerate(keys):
        if key not in start_of:
            start_of[key] = len(tab)
            tab.extend((len(key),) + key)
        prow[r] = start_of[key] | (int(ai[r] - ai[cuts[blk[r]]]) << 16)
    assert len(tab) <= 512
    return prow, np.array(tab, dtype=np.int32), start_of
