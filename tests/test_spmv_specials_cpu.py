"""The machinery the SpMV containment / special-value tests rest on (tests/specials.py), checked without a GPU: the host
row-block recovery, the hit computation, the rule that the class of a row (NaN, +Inf, -Inf, finite) does not depend on the
order of its sum, that every round of poisoned columns is informative, and the hand-stated expectations of the special-value
matrices against the oracle's loops."""
import numpy as np
import pytest

import orc
import specials as sp

CSR_SHAPES = sorted({s for _, s in sp.CSR_FORMS})


def ptr(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int32)


def test_row_block_recovery_restates_the_plan_rule():
    """at most 256 rows, at most 2046 nonzeros, a longer row alone: each split on its own, then the greedy property on the shapes in use"""
    rb, nlong = sp.row_blocks(ptr(np.full(600, 10)))                 # 204 rows of 10 fill 2040 <= 2046, a 205th does not fit
    assert rb.tolist() == [0, 204, 408, 600] and nlong == 0
    rb, nlong = sp.row_blocks(ptr(np.ones(1000, dtype=int)))         # the 256-row split
    assert rb.tolist() == [0, 256, 512, 768, 1000] and nlong == 0
    rb, nlong = sp.row_blocks(ptr(np.zeros(700, dtype=int)))         # rows without entries count as rows
    assert rb.tolist() == [0, 256, 512, 700] and nlong == 0
    rb, nlong = sp.row_blocks(ptr([3, 2047, 3, 2046, 1]))            # 2047 > cap: alone and long; 2046 fills a block by itself: neither the 3 before nor the 1 after fits with it
    assert rb.tolist() == [0, 1, 2, 3, 4, 5] and nlong == 1
    rb, nlong = sp.row_blocks(ptr([]))
    assert rb.tolist() == [0] and nlong == 0
    pointers = [sp.csr_case(s)["ai"] for s in CSR_SHAPES] + [sp.cprow_case(k)["cai"] for k in range(1, 7)] + \
        [(sp.bsr_case(bs)["ai"].astype(np.int64) * bs * bs) for bs in (3, 4, 5)]
    for ai in pointers:
        rb, nlong = sp.row_blocks(ai)
        assert rb[0] == 0 and rb[-1] == ai.size - 1 and np.all(np.diff(rb) > 0)
        for b in range(rb.size - 1):
            r0, r1 = rb[b], rb[b + 1]
            nnz = ai[r1] - ai[r0]
            assert r1 - r0 <= sp.BLOCK_ROWS and (nnz <= sp.CAP or r1 - r0 == 1)
            if r1 < ai.size - 1 and nnz <= sp.CAP:                   # greedy: the next row did not fit
                assert r1 - r0 == sp.BLOCK_ROWS or ai[r1 + 1] - ai[r0] > sp.CAP
        assert nlong == int(np.sum(np.diff(ai) > sp.CAP))
    assert sp.csr_case("longrow")["nlong"] == 1 and sp.cprow_case(3)["nlong"] == 2 and sp.cprow_case(6)["rb"].size == 1
    assert not sp.csr_case("band81")["one_lane"].any() and sp.csr_case("p7")["one_lane"].all() and sp.csr_case("rand16")["one_lane"].all()
    ol = sp.csr_case("longrow")
    assert not ol["one_lane"][7] and ol["one_lane"].sum() == ol["m"] - 1


def test_unlisted_rows_of_the_compressed_row_cases_hold_a_marker_of_their_own():
    """the pre-fill of y in the add modes (cprow_case's y0) and of the other outputs (the GPU file's marker): one value per row"""
    from test_spmv_specials_gpu import marker
    assert np.unique(marker(sp.CPROW_M)).size == sp.CPROW_M
    for k in range(1, 7):
        c = sp.cprow_case(k)
        unlisted = ~c["listed"]
        assert unlisted.sum() == sp.CPROW_M - c["rows"].size and np.unique(c["y0"][unlisted]).size == unlisted.sum()
        assert np.all(np.abs(c["y0"][unlisted]) >= 1e200) and np.all(np.abs(c["y0"][c["rows"]]) < 1e3)


def test_hit_rows_against_sets():
    rng = np.random.default_rng(3)
    for _ in range(5):
        m, n = 40, 30
        lens = rng.integers(0, 6, m)
        ai = ptr(lens)
        aj = np.concatenate([np.sort(rng.choice(n, int(c), replace=False)) for c in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
        P = rng.choice(n, 4, replace=False)
        want = np.array([bool(set(aj[ai[r]:ai[r + 1]].tolist()) & set(P.tolist())) for r in range(m)])
        assert np.array_equal(sp.hit_rows(ai, aj, P, n), want)
    xp = sp.poison(np.zeros(9), [1, 4, 5, 7], shift=1)
    assert np.isposinf(xp[1]) and np.isneginf(xp[4]) and np.isnan(xp[5]) and np.isposinf(xp[7]) and np.count_nonzero(xp == 0.0) == 5
    xb = sp.poison(np.zeros(12), [0, 2, 3], stride=3)                # one point entry of every poisoned block column
    assert np.flatnonzero(xb != 0.0).tolist() == [0, 7, 11]


def all_rounds():
    for s in CSR_SHAPES:
        c = sp.csr_case(s)
        yield "csr " + s, c["ai"], c["aj"], c["aa"], c["n"], c["x"], c["y0"], c["Ps"], c["m"], 1, c["rb"]
    for k in (1, 3):
        c = sp.cprow_case(k)
        yield "cprow %d" % k, c["cai"], c["aj"], c["aa"], c["n"], c["x"], c["y0"][c["rows"]], c["Ps"], c["cai"].size - 1, 1, c["rb"]
    for bs in (3, 4, 5):
        c = sp.bsr_case(bs)
        yield "bsr %d" % bs, c["ai"], c["aj"], None, c["nbs"], c["x"], c["y0"], c["Ps"], c["mbs"], bs, c["rb"]


def test_every_round_is_informative():
    """every round holds c_slack, the first three also column 0 and column n - 1; hit is non-empty and at most half of the rows; the
    rounds differ; together they poison EVERY block target that fits the budget next to c_slack -- on these shapes all of them"""
    for what, ai, aj, _, n, _, _, Ps, m, _, rb in all_rounds():
        assert sp.MAX_ROUNDS >= len(Ps) >= sp.ROUNDS >= 3 and len({tuple(P.tolist()) for P in Ps}) == len(Ps), what
        for r, P in enumerate(Ps):
            hit = sp.hit_rows(ai, aj, P, n)
            assert 0 < hit.sum() <= m // 2, (what, int(hit.sum()), m)
            assert sp.C_SLACK in P and (r >= sp.ROUNDS or {0, n - 1} <= set(P.tolist())), what
        covered, fits, targets = sp.target_coverage(ai, aj, n, rb, Ps, budget=m // 2)
        print("%s: %d rounds, %d of %d block targets poisoned (%d fit the budget)" % (what, len(Ps), len(covered), len(targets), len(fits)))
        assert covered == fits == targets and len(targets) >= 4, what
    z = sp.csr_case("p7const_zeros")
    k = np.flatnonzero(z["aa"] == 0.0)
    assert k.size == 2 and np.signbit(z["aa"][k]).tolist() == [False, True] and all(set(z["aj"][k].tolist()) <= set(P.tolist()) for P in z["Ps"])


def test_class_of_a_row_does_not_depend_on_the_order_of_its_sum():
    """for every shape and round: the oracle's class of each row (A x and y0 + A x) equals the class of the long-double sum of
    the same products front to back and back to front (|a|, |x| <= 1e3: finite products cannot overflow)"""
    for what, ai, aj, aa, n, x, y0, Ps, m, bs, _ in all_rounds():
        if bs > 1:
            c = sp.bsr_case(bs)
            pai, paj, paa = c["pai"], c["paj"], c["paa"]
        else:
            pai, paj, paa = ai, aj, aa
        assert np.max(np.abs(paa)) <= 1e3 and np.max(np.abs(x)) <= 1e3
        for r, P in enumerate(Ps):
            xp = sp.poison(x, P, shift=r, stride=bs)
            assert np.sum(~np.isfinite(xp)) == P.size
            with np.errstate(all="ignore"):
                prod = paa * xp[paj]
                ref = orc.spmv_bsr(bs, ai, aj, c["aa"], xp) if bs > 1 else orc.spmv(ai, aj, aa, xp)
                ref_add = ref + y0 if bs > 1 else orc.spmv_add(ai, aj, aa, xp, y0)
            for got, start in ((ref, None), (ref_add, y0)):
                fwd, bwd = sp.row_class_two_orders(pai, prod, start)
                assert np.array_equal(fwd, bwd) and np.array_equal(sp.classify(got), fwd), (what, r)
            hit = np.repeat(sp.hit_rows(ai, aj, P, n), bs)
            assert np.all(sp.classify(ref)[~hit] == sp.FIN) and np.any(sp.classify(ref)[hit] != sp.FIN), (what, r)
            if bs == 1:                                              # the inode order has the same classes
                assert np.array_equal(sp.classify(orc.spmv_inode(ai, aj, aa, xp)), sp.classify(ref)), (what, r)


def test_check_containment_rejects_a_leak_a_wrong_class_and_a_wrong_bit():
    clean = np.array([1.0, 2.0, 3.0, 4.0]); hit = np.array([False, False, True, True])
    ref = np.array([1.0, 2.0, np.inf, np.nan]); exact = np.ones(4, dtype=bool); bound = np.ones(4)
    sp.check_containment(clean, np.array([1.0, 2.0, np.inf, np.nan]), ref, hit, exact, bound, "ok")
    for bad in ([1.0, np.nextafter(2.0, 3.0), np.inf, np.nan], [1.0, 2.0, np.nan, np.nan], [1.0, 2.0, np.inf, 7.0], [np.nan, 2.0, np.inf, np.nan]):
        with pytest.raises(AssertionError):
            sp.check_containment(clean, np.array(bad), ref, hit, exact, bound, "bad")
    ref2 = np.array([1.0, 2.0, 5.0, -0.0])
    sp.check_containment(clean, np.array([1.0, 2.0, 5.0, -0.0]), ref2, hit, exact, bound, "ok")
    with pytest.raises(AssertionError):                              # the sign of a zero is a bit
        sp.check_containment(clean, np.array([1.0, 2.0, 5.0, 0.0]), ref2, hit, exact, bound, "bad")
    sp.check_containment(clean, np.array([1.0, 2.0, 5.0 + 1e-13, 0.0]), ref2, hit, ~exact, bound, "within 1e-12")
    with pytest.raises(AssertionError):
        sp.check_containment(clean, np.array([1.0, 2.0, 5.0 + 1e-11, 0.0]), ref2, hit, ~exact, bound, "bad")


def test_special_value_expectations_equal_the_oracle():
    """the values stated by hand in specials.special_matrix / special_matrix_multilane, entry by entry against orc.spmv,
    orc.spmv_add, MatMult + VecPointwiseMult and the two-at-a-time loops"""
    s = sp.special_matrix()
    ai, aj, aa, x, y0, d = (s[k] for k in ("ai", "aj", "aa", "x", "y0", "d"))
    assert ai.size - 1 == 64 and sp.one_lane_rows(ai, sp.row_blocks(ai)[0]).all() and np.isnan(x[s["c_slack"]])
    assert set(s["expect"]) == (set(range(24)) - {21}) | {60, 61, 62}          # (row 21 is finite: the oracle alone)
    for pairsum in (0, 1):
        exp = dict(s["expect"])
        if pairsum:
            exp.update(s["expect_pair"])
        for col, mode in enumerate(("mult", "add", "scaled")):
            sp.assert_expected(sp.oracle(mode, pairsum, ai, aj, aa, x, y0, d), exp, col, "oracle %s pairsum %d" % (mode, pairsum))
    a, b = orc.spmv(ai, aj, aa, x), orc.spmv_inode(ai, aj, aa, x)
    differ = np.flatnonzero((sp.bits(a) != sp.bits(b)) & ~(np.isnan(a) & np.isnan(b)))
    assert 17 in differ and np.isfinite(a[17]) and np.isposinf(b[17])          # the two orders differ where stated
    nodes, ns = orc.check_inode(ai, aj)
    assert nodes > 0 and 4 in ns.tolist()                                        # the reference would group the rows 24..59
    t = sp.special_matrix_multilane()
    ai, aj, aa, x, y0, d = (t[k] for k in ("ai", "aj", "aa", "x", "y0", "d"))
    assert not sp.one_lane_rows(ai, sp.row_blocks(ai)[0]).any() and sp.row_blocks(ai)[0].tolist() == [0, 17]
    for col, mode in enumerate(("mult", "add", "scaled")):
        ref = sp.oracle(mode, 0, ai, aj, aa, x, y0, d)
        sp.assert_expected(ref, t["expect"], col, "oracle multilane %s" % mode)
    assert sp.bits(sp.oracle("add", 0, ai, aj, aa, x, y0, d))[8] == sp.bits(np.array([-0.0]))[0]   # the reference's order gives -0.0 where a tree may not
