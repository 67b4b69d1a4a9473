"""Compressed-row plans (mi355x_spmv_plan_create with rows_host != NULL): row r of the plan is row rows[r] of y, every other
row of y is not touched.  Every multi-rank product runs its off-diagonal block through such a plan (host/mpiaijhip.c).  The
kernel's three look-ups of rows[] -- a long row, a block of only empty rows, the normal path -- each have a shape here
(specials.cprow_case), in every output mode, pair stream and scalar stream, both summation orders; the oracle multiplies the
matrix expanded to all m rows."""
import ctypes as C

import numpy as np
import pytest

import specials as sp
from test_kernels_gpu import assert_bitexact, dev  # noqa: F401 (dev: fixture)
from test_spmv_specials_gpu import Csr, Guarded, containment_rounds, marker

pytestmark = pytest.mark.gpu


def cprow_plan(dev, c, scalar=False):
    return Csr(dev, c["cai"], c["aj"], c["aa"], sp.C_SLACK, c["n"], form="scalar" if scalar else "plain", rows=c["rows"], m_out=c["m"])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_compressed_rows_every_mode_and_unlisted_rows_untouched(dev, k):
    """listed rows: the oracle on the expanded matrix, bit for bit on the one-lane shapes (1, 4, 5), within 1e-12 * (sum|a x| [+ |y0|])
    [* |d|] on the 81-entry rows and the long rows (2, 3); every unlisted row keeps the bits it held before the call (a marker
    that differs per row) in every mode; shape 6 (no listed row): nblocks == 0, every call returns 0 and touches nothing"""
    c = sp.cprow_case(k)
    csr = cprow_plan(dev, c, scalar=k == 4)
    assert csr.info() == (c["rb"].size - 1, c["nlong"])
    if k == 1:                 # the first row block holds only empty listed rows, more empty ones are scattered behind it
        assert c["cai"][256] == 0 and np.sum(np.diff(c["cai"])[300:] == 0) > 10
    if k == 3:
        assert c["nlong"] == 2 and np.diff(c["cai"])[-1] == 2500
    if k == 6:
        assert csr.info() == (0, 0)
    assert c["one_lane"][c["rows"]].all() == (k in (1, 4, 5, 6))
    A = (c["ai"], c["aj"], c["aa"], c["n"])
    containment_rounds(dev, csr, A, c["x"], c["y0"], c["d"], c["Ps"] if k in (1, 3) else [], c["one_lane"],
                       (0, 1) if k in (1, 4) else (0,), unlisted=~c["listed"], what="cprow shape %d" % k)
    csr.free()


def test_compressed_row_plans_refuse_the_derived_forms(dev):
    """index compression, value patterns and row grouping do not apply to a compressed-row plan: each returns 0 and leaves the
    plan as it was (is_compressed, nvpat, ngroups 0), the product afterwards carries the bits of the product before; no x'y
    by-product: dot_available 0, mi355x_spmv_csr_dot returns 801 (hipErrorNotSupported) and writes nothing"""
    k = dev.k
    c = sp.cprow_case(1)
    csr = cprow_plan(dev, c)
    dx = dev.put(c["x"])
    before, _ = csr.run("add", dx, c["y0"], c["d"], zfill=c["y0"])
    cai, aj, aa = c["cai"], c["aj"], c["aa"]
    nt, nv, ng = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert k.mi355x_spmv_plan_compress_indices(dev.h, csr.plan, cai.ctypes.data, aj.ctypes.data) == 0
    k.mi355x_spmv_plan_is_compressed(csr.plan, C.byref(nt))
    assert k.mi355x_spmv_plan_value_patterns(dev.h, csr.plan, cai.ctypes.data, aj.ctypes.data, aa.ctypes.data, C.byref(nv)) == 0
    ns = np.ones(cai.size - 1, dtype=np.int32)
    assert k.mi355x_spmv_plan_group_rows(dev.h, csr.plan, cai.ctypes.data, aj.ctypes.data, ns.size, ns.ctypes.data) == 0
    k.mi355x_spmv_plan_group_info(csr.plan, C.byref(ng), None, None)
    assert (nt.value, nv.value, ng.value) == (0, 0, 0)
    dev.chk(k.mi355x_spmv_plan_use_value_patterns(csr.plan, -1, C.byref(nv)))
    assert nv.value == 0
    after, _ = csr.run("add", dx, c["y0"], c["d"], zfill=c["y0"])
    assert_bitexact(after, before)
    yes = C.c_int(-1)
    dev.chk(k.mi355x_spmv_plan_dot_available(csr.plan, csr.daa, C.byref(yes)))
    assert yes.value == 0
    out = Guarded(dev, marker(c["m"]))
    assert k.mi355x_spmv_csr_dot(dev.h, csr.plan, csr.dai, csr.daj, csr.daa, dx, out.p) == 801
    dev.sync()
    assert_bitexact(out.get(), marker(c["m"]))
    out.free()
    dev.free(dx)
    csr.free()
