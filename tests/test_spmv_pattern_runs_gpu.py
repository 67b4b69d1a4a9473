"""Run-coded row patterns (spmv_csr_rowblock_pat_kernel with a block's runs of equal patterns instead of its rows' words): every
case multiplies three times -- runs on, runs off (the per-row-word path of the SAME plan), the oracle -- and compares bit for bit:
these are short rows summed by one lane in column order.  ADD = 0, ADD = 1 (non-zero yin) and the DOT instance, whose finished p'w
must carry the same bits on both paths.  tests/pattern_runs.py holds the matrices and says what each is there for;
test_spmv_pattern_runs_cpu.py checks the descriptors themselves."""
import ctypes as C

import numpy as np
import pytest

import orc
import pattern_runs as pr
from test_kernels_gpu import assert_bitexact, bits, dev  # noqa: F401 (dev: fixture)
from test_spmv_specials_gpu import Csr, check_dot

pytestmark = pytest.mark.gpu

# nblocks, nblocks_run_coded (test_spmv_pattern_runs_cpu.py derives them from the patterns)
BLOCKS = {"p7_256_2_2": (4, 4), "p7_300_3_2": (8, 8), "p7_8_8_8": (2, 0), "stack": (6, 3), "stack_empty": (6, 3), "lap257": (2, 2), "lap256": (1, 1)}


def use_runs(dev, csr, on):
    n = C.c_int(-1)
    dev.chk(dev.k.mi355x_spmv_plan_use_pattern_runs(csr.plan, on, C.byref(n)))
    return n.value


def rowpat(dev, name):
    ai, aj, aa, n = pr.matrix(name)
    csr = Csr(dev, ai, aj, aa, int(aj[0]), n, form="rowpat")
    assert csr.info()[0] == BLOCKS[name][0]
    assert use_runs(dev, csr, -1) == BLOCKS[name][1]
    return csr, (ai, aj, aa, n)


@pytest.mark.parametrize("name", pr.MATRICES)
def test_runs_on_runs_off_and_the_oracle_agree_bit_for_bit(dev, name):
    csr, (ai, aj, aa, n) = rowpat(dev, name)
    nb, ncoded = BLOCKS[name]
    if name == "p7_8_8_8":
        assert ncoded == 0                       # 32 lines per block: the whole matrix keeps its row words
    if name.startswith("stack"):
        assert 0 < ncoded < nb                   # both kinds of block in one launch
    x, y0 = pr.mixed(n, 1), pr.mixed(ai.size - 1, 2)
    dx = dev.put(x)
    refs = {"mult": orc.spmv(ai, aj, aa, x), "add": orc.spmv_add(ai, aj, aa, x, y0)}
    refs["dot"] = refs["mult"]
    for mode in ("mult", "add", "dot"):
        out = {}
        for on in (1, 0):
            use_runs(dev, csr, on)
            out[on] = csr.run(mode, dx, y0)
        assert_bitexact(out[1][0], refs[mode])
        assert_bitexact(out[0][0], refs[mode])
        if mode == "dot":
            assert bits(np.float64(out[1][1])) == bits(np.float64(out[0][1])), "p'w differs between the paths: %r, %r" % (out[1][1], out[0][1])
            check_dot(out[1][1], x, out[1][0], "%s runs on" % name)
    dev.free(dx)
    csr.free()


def test_runs_with_the_inode_summation_order(dev):
    """pairsum (two products at a time, MatMult_SeqAIJ_Inode's order) on rows of up to 6 entries, blocks of 1 to 4 runs"""
    csr, (ai, aj, aa, n) = rowpat(dev, "p7_300_3_2")
    csr.pairsum(1)
    x = pr.mixed(n, 3)
    dx = dev.put(x)
    ref = orc.spmv_inode(ai, aj, aa, x)
    assert not np.array_equal(bits(ref), bits(orc.spmv(ai, aj, aa, x)))          # the two orders do differ here
    for on in (1, 0):
        use_runs(dev, csr, on)
        assert_bitexact(csr.run("mult", dx)[0], ref)
    dev.free(dx)
    csr.free()


def test_runs_containment(dev):
    """y between bands of NaN, x followed by NaN and NaN in every column no row references (rows emptied together with their
    neighbours leave such columns inside the run-coded blocks): nothing outside y changes, no NaN reaches y, y is the oracle's"""
    G = 16
    csr, (ai, aj, aa, n) = rowpat(dev, "stack_empty")
    m = ai.size - 1
    x = pr.mixed(n + 64, 4)
    ref_mult, y0 = orc.spmv(ai, aj, aa, x[:n].copy()), pr.mixed(m, 5)
    ref_add = orc.spmv_add(ai, aj, aa, x[:n].copy(), y0)
    unref = np.setdiff1d(np.arange(n), aj)
    assert unref.size >= 3 and np.any(unref < 256) and np.any(unref >= 768)        # inside a run-coded block and inside one that is not
    x[unref] = np.nan
    x[n:] = np.nan
    dx = dev.put(x)
    for on in (1, 0):
        use_runs(dev, csr, on)
        for mode, ref in (("mult", ref_mult), ("add", ref_add)):
            h = np.full(m + 2 * G, np.nan)
            h[G:G + m] = y0 if mode == "add" else -1e300
            before = bits(h).copy()
            dy = dev.put(h)
            p = C.c_void_p(dy.value + 8 * G)
            if mode == "mult":
                dev.chk(dev.k.mi355x_spmv_csr(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, p))
            else:
                dev.chk(dev.k.mi355x_spmv_csr_add(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, p, p))
            got = dev.get(dy, m + 2 * G)
            dev.free(dy)
            assert np.array_equal(bits(got)[:G], before[:G]) and np.array_equal(bits(got)[G + m:], before[G + m:]), "written outside y"
            assert not np.any(np.isnan(got[G:G + m])), np.flatnonzero(np.isnan(got[G:G + m]))
            assert_bitexact(got[G:G + m], ref)
    assert np.array_equal(bits(dev.get(dx, n + 64)), bits(x))
    dev.free(dx)
    csr.free()


def test_workspace_counts_the_run_descriptors(dev):
    """mi355x_spmv_plan_info: 32 bytes per row block on top of the block table once the analysis has run"""
    ai, aj, aa, n = pr.matrix("stack")
    csr = Csr(dev, ai, aj, aa, 0, n, form="rowpat")
    nb, ws = C.c_int(), C.c_size_t()
    dev.chk(dev.k.mi355x_spmv_plan_info(csr.plan, C.byref(nb), None, C.byref(ws)))
    assert ws.value == 8 * (nb.value + 1) + 32 * nb.value
    csr.free()
