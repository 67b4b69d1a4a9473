"""The helper and the inputs of test_vec_specials_gpu.py checked with the oracle alone, so that a GPU pass means something:
the comparator rejects what it must, the special vectors hold every kind at every structural position, the chosen inputs tell
every special branch of the reference from the general form, the reference outputs are mostly finite and still hold every
IEEE class, and the oracle's device-order reductions give the sequential oracle's class on special data."""
import numpy as np
import pytest

import orc
import vecspecials as vs
from vecspecials import INF, NAN, KINDS, K, same

B_SIZES = [3, 513, 1025, 4097]          # Parts B and C of the GPU module
ROTS = range(K)


def input_sets(case, kinds=KINDS):
    for n in B_SIZES:
        for rot in range(kinds.size):
            yield n, rot, vs.operands(case, n, rot, kinds=kinds)


def test_same_rejects_and_accepts_what_it_must():
    with pytest.raises(AssertionError, match="1 of 3 entries differ, first at 1: 0x8000000000000000"):
        same(np.array([1.0, -0.0, 2.0]), np.array([1.0, 0.0, 2.0]))
    with pytest.raises(AssertionError):
        same(np.array([vs.MIN_SUB]), np.array([0.0]))
    with pytest.raises(AssertionError):
        same(np.array([NAN]), np.array([INF]))
    with pytest.raises(AssertionError):
        same(np.array([INF]), np.array([-INF]))
    with pytest.raises(AssertionError):
        same(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))
    payload = np.array([0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000123], dtype=np.uint64).view(np.float64)
    same(payload, np.array([NAN, NAN, NAN]))
    same(np.array([-0.0, vs.MIN_SUB, INF]), np.array([-0.0, vs.MIN_SUB, INF]))
    assert vs.is_same(payload, payload[::-1]) and not vs.is_same(np.array([0.0]), np.array([-0.0]))


def test_special_vector_holds_every_kind_at_every_structural_position():
    for n in B_SIZES + [2, 4096, 8193]:
        pos = vs.structural_positions(n)
        assert pos[0] == 0 and n - 1 in pos and len(pos) == min(n, 3) and all((p >> 1) >= (n >> 1) - 1 for p in pos[1:])
        seen = {p: set() for p in pos}
        for rot in ROTS:
            x = vs.special_vector(n, 11, vs.SHARE, rot)
            for p in pos:
                seen[p].add(int(vs.bits(x[p:p + 1])[0]))
        for p in pos:
            assert seen[p] == {int(b) for b in vs.bits(KINDS)}, (n, p)
    x = vs.special_vector(100001, 3, vs.SHARE)
    b = vs.bits(x)
    share = np.isin(b, vs.bits(KINDS)).mean()
    assert abs(share - vs.SHARE) < 0.01
    assert all((b == kb).sum() >= 500 for kb in vs.bits(KINDS))          # every kind, signed zeros and the smallest subnormal apart
    x2 = vs.special_vector(100001, 3, vs.SHARE)
    assert not np.array_equal(vs.bits(x), vs.bits(vs.special_vector(100001, 3, vs.SHARE, 1)))     # another rotation, other positions
    assert np.array_equal(vs.bits(x), vs.bits(x2))                         # a pure function of its arguments
    f = vs.special_vector(4097, 5, vs.SHARE, kinds=vs.FINITE_KINDS)
    assert np.all(np.isfinite(f)) and (vs.bits(f) == vs.bits(np.array([-0.0]))[0]).any()


def test_guard_layout():
    """the layout `Guarded` gives: >= 2 guard doubles on each side, the view 0 or 8 bytes off a 16-byte boundary; and
    guard_damage names exactly the guard doubles that changed"""
    for n in (1, 2, 513):
        for off in (0, 1):
            front, back = 2 + off, 3 - off
            assert front >= 2 and back >= 2 and (8 * front) % 16 == 8 * off
            whole = np.empty(front + n + back); vs.bits(whole)[:] = vs.GUARD
            whole[front:front + n] = NAN                                 # data NaN with another payload is not a guard
            assert vs.guard_damage(whole, front, n) == []
            whole[front + n] = 1.0; whole[front - 1] = NAN
            assert vs.guard_damage(whole, front, n) == [-1, n]
    assert np.isnan(np.array([vs.GUARD | np.uint64(255)]).view(np.float64)[0]) and not (int(vs.GUARD) >> 51) & 1    # a signalling NaN


ALL_CASES = vs.ELEMENTWISE + [vs.MAXPY_SPECIAL, vs.SCALE_RNORM] + vs.FUSED
BRANCH_CASES = [(c, t) for c in ALL_CASES for t in c.tuples]


def test_case_tables_cover_the_tuples_of_the_issue():
    by = {c.name: c for c in ALL_CASES}
    for name in ("axpy", "aypx", "waxpy"):
        assert len(by[name].tuples) == 7 and sum(np.isnan(t[0]) for t in by[name].tuples) == 1
    assert len(by["scale"].tuples) == 6 and len(by["axpby"].tuples) == 16
    assert {(t[0] == 1.0, t[2] == 1.0, t[2] == 0.0) for t in by["axpbypcz"].tuples} >= {(True, False, False), (False, True, False), (False, False, True), (False, False, False), (True, False, True)}
    assert [t[0] for t in by["cg_update"].tuples] == [0.0, -0.0, 0.731] and np.signbit(by["cg_update"].tuples[1][0])
    assert len(vs.guard_band_cases()) == len({c.name for c in vs.guard_band_cases()})


@pytest.mark.parametrize("case,t", BRANCH_CASES, ids=["%s%r" % (c.name, t) for c, t in BRANCH_CASES])
def test_inputs_distinguish_every_branch(case, t):
    """For a tuple that selects a special branch the reference's result differs, under `same`, from the result of the form a
    kernel without that branch would compute -- on every input set the GPU module uses; and the forms the sources call
    bit-identical (alpha = +-1, beta = 1, gamma = 1) are: the general arithmetic equals the reference there."""
    special = 0
    told = dict.fromkeys(B_SIZES, 0)
    for n, rot, v in input_sets(case):
        with np.errstate(all="ignore"):
            ref, _ = case.ref(t, v)
            wrong = case.wrong(t, v)
        if wrong is None:
            continue
        special += 1
        told[n] += any(not vs.is_same(ref[name], wrong[name]) for name in wrong)
    if special:       # three elements cannot tell every branch at every rotation: there one rotation at least must, above that every one
        assert told[3] >= 1 and all(told[n] == K for n in B_SIZES[1:]), "the inputs cannot tell the branch: %r of %d" % (told, K)
    expect_special = {"axpy": t and t[0] == 0.0, "aypx": t and t[0] == 0.0, "waxpy": t and t[0] == 0.0, "scale": t and t[0] == 0.0,
                      "axpby": len(t) == 2 and (t[0] == 0.0 or t[1] == 0.0), "axpbypcz": len(t) == 3 and t[2] == 0.0,
                      "cg_update": t and t[0] == 0.0, "cg_update_nod": t and t[0] == 0.0, "aypx_dev": t and t[0] == 0.0,
                      "bcgs_update": len(t) == 2 and t[1] == 0.0, "maxpy3": True, "scale_rnorm_dev": t and np.isinf(t[0])}
    assert (special > 0) == bool(expect_special.get(case.name, False)), "special-branch tuples without a wrong form (or the reverse)"


def test_forms_the_sources_call_bit_identical_are():
    """x + 1 * y and x + (-1) * y carry the bits of x + y and x - y, 1 * x those of x: why alpha = +-1, beta = 1 and gamma = 1
    need no device branch of their own"""
    by = {c.name: c for c in vs.ELEMENTWISE}
    general = {"axpy": lambda t, v: v["y"] + t[0] * v["x"], "aypx": lambda t, v: v["x"] + t[0] * v["y"], "waxpy": lambda t, v: v["y"] + t[0] * v["x"],
               "axpby": lambda t, v: t[0] * v["x"] + t[1] * v["y"], "axpbypcz": lambda t, v: t[0] * v["x"] + t[1] * v["y"] + t[2] * v["z"]}
    n_checked = 0
    for name, g in general.items():
        c = by[name]
        for t in c.tuples:
            if any(s == 0.0 for s in t) or not any(abs(s) == 1.0 for s in t):
                continue
            for n, rot, v in input_sets(c):
                with np.errstate(all="ignore"):
                    ref, _ = c.ref(t, v)
                    same(list(ref.values())[0], g(t, v), "%s%r n = %d" % (name, t, n))
            n_checked += 1
    assert n_checked >= 10


CLASSES = ("nan", "+inf", "-inf", "-0.0", "subnormal")
# Output classes a case cannot produce, whatever its inputs, and cases whose outputs cannot be half finite -- by the arithmetic:
#   alpha = Inf / NaN: y + alpha * x is non-finite wherever x != 0 resp. everywhere; Inf * x is never -0.0 or subnormal
#   set writes one value; scale by 0 and axpby(0, 0) set +0.0; axpby(0, 1), axpby(0, b) and scale keep / scale y alone
#   jacobi_invert: 1 / x is +-Inf only for x = +-0, which gives 1 instead
#   reciprocal: zeros stay, so no Inf (1 / subnormal overflows: +-Inf do occur), -0.0 stays -0.0
CANNOT = {
    ("axpy", INF): ("-0.0", "subnormal", "half"), ("aypx", INF): ("-0.0", "subnormal", "half"), ("waxpy", INF): ("-0.0", "subnormal", "half"),
    ("scale", INF): ("-0.0", "subnormal", "half"),
    ("axpy", "nan"): ("+inf", "-inf", "-0.0", "subnormal", "half"), ("aypx", "nan"): ("+inf", "-inf", "-0.0", "subnormal", "half"),
    ("waxpy", "nan"): ("+inf", "-inf", "-0.0", "subnormal", "half"),
    ("scale", 0.0): CLASSES, ("axpby", 0.0, 0.0): CLASSES, ("set",): CLASSES + ("half",),
    ("jacobi_invert",): ("+inf", "-inf"),
}


def _cannot(case, t):
    key = (case.name,) + tuple("nan" if np.isnan(s) else float(s) for s in t)
    return CANNOT.get(key, CANNOT.get((case.name,), ()))


ELEMENT_CASES = [(c, t) for c in vs.ELEMENTWISE + [vs.MAXPY_SPECIAL] for t in c.tuples]


@pytest.mark.parametrize("case,t", ELEMENT_CASES, ids=["%s%r" % (c.name, t) for c, t in ELEMENT_CASES])
def test_reference_outputs_are_mostly_finite_and_hold_every_class(case, t):
    """A condition on the inputs, not a measurement: over the input sets of a case at least half of the reference output
    entries are finite, and NaN, +Inf, -Inf, -0.0 and a subnormal each occur -- except where the arithmetic of the case
    cannot produce them (CANNOT, with the reasons)."""
    count = dict.fromkeys(CLASSES, 0)
    finite = total = 0
    for n, rot, v in input_sets(case):
        with np.errstate(all="ignore"):
            ref, _ = case.ref(t, v)
        for o in ref.values():
            count["nan"] += int(np.isnan(o).sum()); count["+inf"] += int((o == INF).sum()); count["-inf"] += int((o == -INF).sum())
            count["-0.0"] += int((vs.bits(o) == np.uint64(1) << np.uint64(63)).sum())
            count["subnormal"] += int(((o != 0.0) & (np.abs(o) < vs.DBL_MIN)).sum())
            finite += int(np.isfinite(o).sum()); total += o.size
    cannot = _cannot(case, t)
    if "half" not in cannot:
        assert 2 * finite >= total, (finite, total)
    for c in CLASSES:
        if c not in cannot:
            assert count[c] >= 1, "no %s in the reference output: %r" % (c, count)


def test_divide_reciprocal_and_jacobi_inputs_hold_the_named_edges():
    by = {c.name: c for c in vs.ELEMENTWISE}
    seen = dict.fromkeys(["0/0", "x/0", "x/inf", "subnormal quotient", "recip +-0 stay", "1/huge subnormal", "jacobi -0 -> 1", "jacobi inf -> 0"], 0)
    for n, rot, v in input_sets(by["pointwise_divide"]):
        x, y = v["x"], v["y"]
        with np.errstate(all="ignore"):
            w = by["pointwise_divide"].ref((), v)[0]["w"]
        seen["0/0"] += int(((x == 0) & (y == 0) & np.isnan(w)).sum())
        seen["x/0"] += int((np.isfinite(x) & (x != 0) & (y == 0) & np.isinf(w)).sum())
        seen["x/inf"] += int((np.isfinite(x) & np.isinf(y) & (w == 0)).sum())
        seen["subnormal quotient"] += int(((w != 0) & (np.abs(w) < vs.DBL_MIN)).sum())
    for n, rot, v in input_sets(by["reciprocal"]):
        x = v["x"]; r = by["reciprocal"].ref((), v)[0]["x"]
        z = x == 0
        assert np.array_equal(vs.bits(x[z]), vs.bits(r[z]))
        seen["recip +-0 stay"] += int(np.signbit(r[z]).sum() and (~np.signbit(r[z])).sum())
        seen["1/huge subnormal"] += int(((np.abs(x) == vs.DBL_MAX) & (r != 0) & (np.abs(r) < vs.DBL_MIN)).sum())
    for n, rot, v in input_sets(by["jacobi_invert"]):
        d = v["d"]; r = by["jacobi_invert"].ref((), v)[0]["d"]
        m0 = vs.bits(d) == np.uint64(1) << np.uint64(63)
        assert np.all(r[m0] == 1.0) and np.all(r[np.isinf(d)] == 0.0)
        seen["jacobi -0 -> 1"] += int(m0.sum()); seen["jacobi inf -> 0"] += int(np.isinf(d).sum())
    assert all(seen.values()), seen


def test_maxpy_zero_coefficient_meets_inf_and_nan_columns():
    c = vs.MAXPY_SPECIAL
    for t in c.tuples:
        j = [i for i in range(3) if t[i] == 0.0][0]
        for n, rot, v in input_sets(c):
            col = v["y%d" % j]
            bad = ~np.isfinite(col)
            assert bad.any() or n == 3
            assert np.all(np.isnan(c.ref(t, v)[0]["x"][bad]))             # 0 * Inf, 0 * NaN: the reference does not skip zeros


# ------------------------------------------------------------------------------------------------------ reductions (Part D)
reduction_positions = vs.reduction_positions
D_SIZES = [3, 4097, 8193, (1 << 21) + 1]
PLACEMENTS = [("nan", (NAN,)), ("+inf", (INF,)), ("-inf", (-INF,)), ("nan", (INF, -INF))]


def test_reduction_positions_are_where_they_claim():
    for n in D_SIZES:
        grid = vs.reduction_grid(n)
        pos = reduction_positions(n)
        assert all(0 <= p < n for p in pos.values())
        assert ((pos["mid_wg0"] >> 1) // 256) % grid == 0
        if n > 3:
            assert ((pos["last_wg"] >> 1) // 256) % grid == grid - 1
    assert ((reduction_positions(D_SIZES[-1])["wg>=256"] >> 1) // 256) % 512 == 300


@pytest.mark.parametrize("n", D_SIZES)
def test_device_order_reductions_give_the_sequential_class_on_special_data(n):
    """orc.device_reduction_order() on the vectors of Part D: the class (finite, NaN, +Inf, -Inf) of every reduction equals the
    sequential oracle's, for a single special at every structural position, for +Inf with -Inf, and for the special vectors;
    finite vectors of signed zeros and subnormals stay finite in both orders"""
    base = {name: np.random.default_rng(31 + j).standard_normal(n) for j, name in enumerate(["x", "y", "s", "t"] + ["y%d" % j for j in range(5)])}
    base["x"] = np.abs(base["x"]); base["y"] = np.abs(base["y"]); base["s"] = np.abs(base["s"]); base["t"] = np.abs(base["t"])
    for j in range(5):
        base["y%d" % j] = np.abs(base["y%d" % j])                       # positive terms: Inf * y keeps the sign of Inf in every sum
    pos = list(reduction_positions(n).values())
    vecs = []
    for want, vals in PLACEMENTS:
        for i, p in enumerate(pos):
            v = {k_: a.copy() for k_, a in base.items()}
            for name in ("x", "t"):
                v[name][p] = vals[0]
                if len(vals) > 1:
                    v[name][pos[(i + 1) % len(pos)] if pos[(i + 1) % len(pos)] != p else (p + 1) % n] = vals[1]
            vecs.append(v)
    if n > (1 << 20):
        vecs = vecs[:1]                                                   # the largest size: one placement, the oracle being slow
    finite_ones = []
    for rot in ((0, 4, 9) if n < (1 << 20) else (4,)):                    # the vectors the GPU module uses
        vecs.append(vs.reduction_vectors(n, rot, KINDS))
        finite_ones.append(vs.reduction_vectors(n, rot, vs.FINITE_KINDS))
    for v in finite_ones:
        for case in vs.REDUCTIONS:
            for order in (0, 1):
                with orc.device_reduction_order() if order else np.errstate(all="ignore"):
                    assert all(np.isfinite(vs.sum_value(s)[0]) for s in case.ref((), v)[1]), case.name
    for v in vecs:
        for case in vs.REDUCTIONS:
            _, sums = case.ref((), v)
            seq = [vs.sum_value(s)[0] for s in sums]
            with orc.device_reduction_order():
                dev = [vs.sum_value(s)[0] for s in sums]
            assert [vs.klass(a) for a in seq] == [vs.klass(a) for a in dev], case.name
    allneg0 = np.full(n, -0.0)
    assert vs.bits(np.array([orc.vec_norm(allneg0, 3)]))[0] == 0
    big = base["x"].copy(); big[n // 2] = 1e200
    with orc.device_reduction_order():
        assert orc.vec_dot(big, big) == INF                              # x * x overflows: +Inf, not NaN
