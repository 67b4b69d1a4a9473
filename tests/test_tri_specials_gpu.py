"""Triangular solves (csrc/trisolve.hip) against the plain loops on data that is not tame: containment of NaN / +-Inf along the
dependency graph (Part A), IEEE specials inside the arithmetic -- signed zeros, 0.0 * Inf, overflow, subnormals, NaN as a solution
VALUE next to the sentinel that means "not computed yet" -- (Part B), and nothing stale from one application to the next, sync-free
and level by level in any order (Part C).  Every case runs on every kernel family: row plans (host and device build route), the
library's default for narrow shapes (single-row node plans on the split-role kernels), node plans split-role / one wavefront /
block columns; each with mi355x_trisolve_apply and mi355x_trisolve_apply_levels; by_level = 0, where bit-exactness is claimed.

Comparison rule: where the reference is finite (+-0.0 and subnormals included) or +-Inf the same bits, where it is NaN a NaN.
References: tri.tri_reference_apply / tri.tri_node_reference_apply; the machinery (trispecials.py) is checked on its own, without a
GPU, by test_tri_specials_cpu.py.  No case feeds the sentinel's bit pattern or tries to produce it."""
import ctypes as C

import numpy as np
import pytest

import trispecials as ts
from test_kernels_gpu import dev  # noqa: F401 (fixture)
from trispecials import bits

pytestmark = pytest.mark.gpu

MARK = -7.25e300            # pre-fill of y
ROW_FAMILIES = ["rows-host", "rows-device", "default"]
NODE_FORMS = {"mixed": ["split", "onewave"], "fixed3": ["blockcols"]}


def _p(a):
    return a.ctypes.data if a is not None else None


class Plans:
    """the plan pair of factor f on one kernel family (the environment is read when the plan is created), two device vectors"""

    def __init__(self, dev, f, family, monkeypatch):
        k = dev.k
        self.dev, self.f, self.family, self.n = dev, f, family, f["n"]
        monkeypatch.setenv("MI355X_TRISOLVE_BUILD", "device" if family == "rows-device" else "host")
        monkeypatch.delenv("MI355X_TRISOLVE_ONE_XCD", raising=False)
        if family in ("rows-host", "rows-device", "onewave"):
            monkeypatch.setenv("MI355X_TRISOLVE_SPLIT", "0")
        else:
            monkeypatch.delenv("MI355X_TRISOLVE_SPLIT", raising=False)
        self.lo, self.up = C.c_void_p(), C.c_void_p()
        if ts.is_nodes(f):
            rc = k.mi355x_trisolve_plan_create_nodes_pair(dev.h, f["n"], f["nstart"].size - 1, _p(f["nstart"]), 0, 1 if family == "blockcols" else 0,
                                                          f["nlev"], _p(f["lev"]), _p(f["rp"]), _p(f["rl"]), f["nlevu"], _p(f["levu"]), _p(f["rpu"]), _p(f["rlu"]),
                                                          _p(f["cj"]), _p(f["cv"]), _p(f["dinv"]), C.byref(self.lo), C.byref(self.up))
        else:
            rc = k.mi355x_trisolve_plan_create_pair(dev.h, f["n"], 0, f["nlev"], _p(f["lev"]), _p(f["rp"]), _p(f["rl"]), _p(f["cj"]), _p(f["cv"]),
                                                    f["nlevu"], _p(f["levu"]), _p(f["rpu"]), _p(f["rlu"]), _p(f["cju"]), _p(f["cvu"]), _p(f["dinv"]),
                                                    _p(f["rscale"]), C.byref(self.lo), C.byref(self.up))
        assert rc == 0 and self.lo.value and self.up.value, "plan creation returned %d (%s)" % (rc, family)
        self.db, self.dy = dev.alloc(8 * self.n), dev.alloc(8 * self.n)
        # the family is the one asked for: mi355x_trisolve_debug_get serves row plans and refuses node plans
        nb = C.c_size_t(0)
        is_row_plan = k.mi355x_trisolve_debug_get(self.lo, 0, None, C.c_size_t(0), C.byref(nb)) == 0
        assert is_row_plan == (family in ("rows-host", "rows-device")), "family %s asked for, the library built %s plans" % (
            family, "row" if is_row_plan else "node")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.k.mi355x_trisolve_plan_destroy(self.lo); self.dev.k.mi355x_trisolve_plan_destroy(self.up)
        self.dev.free(self.db); self.dev.free(self.dy)

    def apply(self, b, levels, what):
        """one application: returns 0, no abort on either plan, b unchanged; y pre-filled with the marker"""
        dev, k = self.dev, self.dev.k
        b = np.ascontiguousarray(b)
        dev.chk(k.mi355x_memcpy_h2d(dev.h, self.db, b.ctypes.data, b.nbytes))
        dev.chk(k.mi355x_vec_set(dev.h, self.n, MARK, self.dy))
        rc = (k.mi355x_trisolve_apply_levels if levels else k.mi355x_trisolve_apply)(dev.h, self.lo, self.up, self.db, self.dy)
        assert rc == 0, "%s: the application returned %d" % (what, rc)
        got = dev.get(self.dy, self.n)
        flag = C.c_int(-1)
        for pl in (self.lo, self.up):
            dev.chk(k.mi355x_trisolve_aborted(pl, C.byref(flag)))
            assert flag.value == 0, "%s: an abort was reported" % what
        back = dev.get(self.db, self.n)
        assert np.array_equal(bits(back), bits(b)), "%s: the right-hand side was modified" % what
        return got

    def row_at_position_0(self, plan):
        """row plans: position -> row, entry 0 (mi355x_trisolve_debug_get, which = 2); None for node plans, which it refuses"""
        out = np.full(((self.n + 63) // 64) * 64, -5, dtype=np.int32)
        nb = C.c_size_t(0)
        rc = self.dev.k.mi355x_trisolve_debug_get(plan, 2, out.ctypes.data, C.c_size_t(out.nbytes), C.byref(nb))
        return int(out[0]) if rc == 0 and nb.value == out.nbytes else None


def _families(name):
    if name in ts.NODE_FACTORS:
        return NODE_FORMS[name]
    return ROW_FAMILIES if ts.base_factor(name)["n"] >= 64 else ROW_FAMILIES[:2]       # below 64 rows the default IS the row plan


A_PARAMS = [pytest.param(name, config, fam, id="%s-%s-%s" % (name, config, fam)) for name, config in ts.part_a_cases() for fam in _families(name)]


@pytest.mark.parametrize("name,config,family", A_PARAMS)
def test_poison_stays_inside_what_it_can_reach(dev, name, config, family, monkeypatch):
    """Part A.  b poisoned with NaN, +Inf, -Inf at the rows S of every round: rows S cannot reach through L's and then U's
    dependency graph keep the bits of the clean run, rows it can reach follow the reference of the poisoned b by the comparison
    rule.  Row factors unscaled and with rscale.  Row plans: the row the plan holds at position 0 is the one the host derived."""
    c = ts.part_a_case(name, config)
    assert c["kept"] and c["rounds"]
    for scaled in ((True,) if ts.is_nodes(c["f"]) else (False, True)):
        f = c["f"] if scaled else ts.unscaled(c["f"])
        ref_clean, rounds = ts.part_a_refs(name, config, scaled)
        where = "%s, %s, family %s, %s" % (name, config, family, "scaled" if scaled and not ts.is_nodes(f) else "unscaled")
        with Plans(dev, f, family, monkeypatch) as P:
            if family in ("rows-host", "rows-device"):
                t = ts.targets(f)
                assert P.row_at_position_0(P.lo) == t["L.pos0"] and P.row_at_position_0(P.up) == t["U.pos0"], where
            for levels in (False, True):
                w = "%s, levels = %s" % (where, levels)
                clean = P.apply(c["b"], levels, w)
                ts.check_rule(clean, ref_clean, np.ones(f["n"], dtype=bool), w + ", clean")
                for j, ((S, reach), (bp, ref)) in enumerate(zip(c["rounds"], rounds)):
                    ts.check_containment(clean, P.apply(bp, levels, w), ref, reach, "%s, round %d (%d poisoned rows)" % (w, j, S.size))


def _b_cases():
    out = []
    for name in ts.special_tables():
        out += [pytest.param(name, fam, id="%s-%s" % (name, fam)) for fam in ROW_FAMILIES]
    return out + [pytest.param("node_table", fam, id="node_table-%s" % fam) for fam in ("split", "onewave")] + [
        pytest.param("block_node_table", "blockcols", id="block_node_table-blockcols")]


@pytest.mark.parametrize("name,family", _b_cases())
def test_specials_inside_the_arithmetic(dev, name, family, monkeypatch):
    """Part B.  The hand-built factors of trispecials.special_tables / node_table (two and three slices of positions): signed
    zeros, an entry 0.0 against Inf / NaN / a finite value, Inf - Inf, overflow from finite operands, Inf * dinv, rscale * Inf,
    dinv of 0.0 / +-Inf / NaN, subnormal b / entry / dinv / product / sum, a NaN in b through a chain of 77 rows; node plans (a
    table of nodes of 1..5 rows, one of 3 rows throughout for block columns): the same kinds in a shared column, a coupling and the
    inverted diagonals, a NaN in slot 0 of w that no list names, and the pair of columns whose sum overflows only when
    the two products are added to each other first.  Three applications each way: the NaN values must not be taken for the
    sentinel (no abort, the result NaN exactly where the reference is)."""
    t = ts.node_table() if name == "node_table" else ts.block_node_table() if name == "block_node_table" else ts.special_tables()[name]
    f, b = t["f"], t["b"]
    ref = ts.reference(f, b)
    rows = np.ones(f["n"], dtype=bool)
    with Plans(dev, f, family, monkeypatch) as P:
        for levels in (False, True, False):
            what = "%s, family %s, levels = %s" % (name, family, levels)
            got = P.apply(b, levels, what)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN in rows %s, reference %s" % (
                what, np.flatnonzero(np.isnan(got))[:12], np.flatnonzero(np.isnan(ref))[:12])
            ts.check_rule(got, ref, rows, what)


C_PARAMS = [pytest.param(name, fam, id="%s-%s" % (name, fam)) for name in ts.C_FACTORS for fam in _families(name)]


@pytest.mark.parametrize("name,family", C_PARAMS)
def test_nothing_stale_between_applications(dev, name, family, monkeypatch):
    """Part C.  On one plan pair: clean b0, poisoned b, clean b1, all-NaN b, clean b2 -- sync-free, then level by level, then the two
    forms alternating application by application (starting with each).  Every clean application is its own reference bit for bit:
    a slot not returned to the sentinel, or a NaN left in w, shows up only here."""
    f, seq = ts.part_c_case(name)
    orders = [[False] * 5, [True] * 5, [False, True, False, True, False], [True, False, True, False, True]]
    with Plans(dev, f, family, monkeypatch) as P:
        for o, order in enumerate(orders):
            for j, ((b, ref), levels) in enumerate(zip(seq, order)):
                what = "%s, family %s, sequence %d (levels = %s), application %d" % (name, family, o, order, j)
                got = P.apply(b, levels, what)
                if ref is not None:
                    assert np.array_equal(bits(got), bits(ref)), "%s: %d of %d rows differ from the reference, first %s" % (
                        what, int((bits(got) != bits(ref)).sum()), f["n"], np.flatnonzero(bits(got) != bits(ref))[:8])
                elif j == 3:
                    assert np.isnan(got).all(), what
