"""The machinery of the triangular-solve containment / IEEE-special / re-arming tests (trispecials.py) checked against the
references alone, without a GPU: so that test_tri_specials_gpu.py cannot pass quietly by checking nothing.  What is asserted: the
references agree with an independent numpy float64 restatement (and the node reference with the oracle's inode routine); the
conditions of Part A (shares, targets, the list of dropped pairs); the stated results and classes of Part B; that no input carries
the sentinel's payload; that the shapes reach the features the kernels' paths depend on."""
import numpy as np
import pytest

import orc
import trispecials as ts
from trispecials import FIN, NAN, NINF, PINF, bits, classify, differing


def test_references_agree_with_a_numpy_restatement_and_the_inode_routine():
    for name in ts.NODE_FACTORS:
        f = ts.node_factor(name)
        b = ts.clean_b(f["n"], 3)
        ref = ts.reference(f, b)
        assert np.array_equal(bits(ref), bits(orc.ilu0_solve_inode(f["ilu"], f["ns"], b))), name      # the plain-Python restatement == the oracle
        assert not differing(ref, ts.numpy_reference(f, b)).any(), name
        for config in ("L", "U"):
            g = ts.one_sided(f, config)
            assert not differing(ts.reference(g, b), ts.numpy_reference(g, b)).any(), (name, config)
    for shape in ("n65", "chain", "empty_rows"):
        f = ts.row_factor(shape)
        for g in (f, ts.unscaled(f), ts.one_sided(f, "L"), ts.one_sided(f, "U")):
            b = ts.poison(ts.clean_b(f["n"], 4), np.array([1, f["n"] // 2, f["n"] - 2]))
            assert not differing(ts.reference(g, b), ts.numpy_reference(g, b)).any(), shape


@pytest.mark.parametrize("name", ts.A_SHAPES + ts.NODE_FACTORS)
def test_part_a_conditions_hold_from_the_graph_alone(name):
    """every (shape, configuration) pair is kept exactly when it is not in DROPPED; a kept pair's rounds each reach >= 5 % of the rows
    (>= 1 row for n <= 65) and leave >= 25 % untouched; the reach of a round is closed under both dependency graphs and holds S;
    the targets no round held are exactly UNREACHED; a poisoned reference differs from the clean one only inside the reach"""
    kept = []
    for config in ts.CONFIGS:
        c = ts.part_a_case(name, config)
        f, n = c["f"], c["f"]["n"]
        assert c["kept"] == ((name, config) not in ts.DROPPED), (name, config)
        if not c["kept"]:
            continue
        kept.append(config)
        assert ts.ROUNDS <= len(c["rounds"]) <= ts.MAX_ROUNDS
        assert c["unreached"] == ts.UNREACHED.get((name, config), []), (name, config, c["unreached"])
        assert sorted(c["held"] + c["unreached"]) == sorted(ts.targets(f))
        for S, reach in c["rounds"]:
            assert S.size and reach[S].all()
            assert reach.sum() >= (1 if n <= 65 else 0.05 * n) and (~reach).sum() >= 0.25 * n, (name, config, reach.sum(), n)
            assert np.array_equal(ts.reach_matrix(f, [int(S[0])])[:, 0] | reach, reach)
            # closed: a row outside names no row inside (U's graph; L's too where U adds nothing to what L reached)
            for rp, rl, cj in ((f["rpu"], f["rlu"], f["cju"]),) + (((f["rp"], f["rl"], f["cj"]),) if config != "both" else ()):
                for i in np.flatnonzero(~reach):
                    assert not reach[cj[rp[i]:rp[i] + rl[i]]].any()
    if name not in ("tiny", "n1"):
        assert "L" in kept and "U" in kept
    if name in ("n65", "chain", "mixed"):
        config = kept[0]
        c = ts.part_a_case(name, config)
        clean, rounds = ts.part_a_refs(name, config, True)
        for (S, reach), (bp, ref) in zip(c["rounds"], rounds):
            assert not (~reach & (bits(ref) != bits(clean))).any()
            assert (classify(ref[reach]) != FIN).any()


def test_part_a_targets_follow_the_layout_rule():
    """positions sorted by level, longer lists first: on n65 (levels of a few rows) the row at position 0 is the level-0 row with the
    longest list -- none has entries, so row 0 --, and the layout is a permutation of the rows; on the mixed node factor position 0
    holds node 0 and a level of 32 nodes or more would start on a slice boundary"""
    f = ts.row_factor("n65")
    lev, rl, r0, rL = ts.items(f, False)
    at = ts.layout(lev, rl, False)
    assert at.size == 128 and sorted(at[at >= 0].tolist()) == list(range(65)) and (at[65:] == -1).all()
    assert (np.diff(lev[at[:65]]) >= 0).all()
    for l in range(int(lev.max()) + 1):
        assert (np.diff(rl[at[:65]][lev[at[:65]] == l]) <= 0).all()
    assert ts.targets(f)["L.pos0"] == int(at[0]) == 0
    lev = np.array([0] * 40 + [1] * 40 + [2] * 3); ln = np.zeros(83, dtype=np.int32)
    at = ts.layout(lev, ln, True)
    assert at[39] == 39 and (at[40:64] == -1).all() and at[64] == 40 and at[104] == 80 and at.size == 128
    g = ts.node_factor("mixed")
    t = ts.targets(g)
    assert t["L.pos0"] == 0 and g["nstart"][-2] <= t["U.pos0"] <= g["n"] - 1 and t["node_last"] > t["node_first"]


def test_shapes_reach_every_feature():
    """slice boundaries (64 and 65 rows), sub-steps inside a slice, more batches than the LDS ring holds, rows of 0, 1, 7, 8 and 9
    entries, odd and even list lengths, padding positions in the last slice; node factors: nodes of every size 1..5"""
    lens = set()
    for shape in ts.A_SHAPES:
        f = ts.row_factor(shape)
        lens |= set(f["rl"].tolist()) | set(f["rlu"].tolist())
    assert {0, 1, 7, 8, 9} <= lens and any(l % 2 for l in lens if l > 9) and any(l % 2 == 0 for l in lens if l > 9)
    assert ts.row_factor("n64")["n"] == 64 and ts.row_factor("n65")["n"] == 65
    f = ts.row_factor("chain")
    lev, rl, _, _ = ts.items(f, False)
    at = ts.layout(lev, rl, False)
    assert len(set(lev[at[:64]].tolist())) > 1                     # sub-steps: a slice spans several levels
    assert ts.row_factor("longrow")["rl"].max() > 4 * ts.SPLIT_B1 * ts.split_ring_batches(1)      # more batches than the LDS ring holds, with a margin of 4
    for shape in ("n65", "ragged", "chain"):
        f = ts.row_factor(shape)
        assert f["n"] % 64                                         # padding positions (rowof = -1) in the last slice
    assert set(np.diff(ts.node_factor("mixed")["nstart"]).tolist()) == {1, 2, 3, 4, 5}
    assert set(np.diff(ts.node_factor("fixed3")["nstart"]).tolist()) == {3}
    for name in ts.NODE_FACTORS:
        f = ts.node_factor(name)
        sh = f["rl"][f["nstart"][:-1]]
        assert (sh % 2 == 1).any() and (sh % 2 == 0).any() and sh.max() >= 9


NODE_CLASSES = "NN" "-+-" "FFFFF" "FF" "FFF" "N+F" "-F" "NNFFF" "FF"      # nodes A .. I of trispecials.node_table, rows 16 .. 42
# sources S0 .. S7 and consumers a .. h of trispecials.block_node_table, rows 0 .. 47
BLOCK_CLASSES = "NNN" "FFF" "+++" "---" "FFF" "FFF" "FFF" "FFF" "NNN" "-+-" "NNN" "FFF" "FFF" "N+F" "+FF" "FFF"


def _named(f):
    """the rows some list of the factor names"""
    out = set()
    for rp, rl, cj in ((f["rp"], f["rl"], f["cj"]), (f["rpu"], f["rlu"], f["cju"])):
        for i in range(f["n"]):
            out |= set(cj[rp[i]:rp[i] + rl[i]].tolist())
    return out


def test_part_b_tables_state_their_classes():
    T = ts.special_tables()
    for name in ("arith_lower", "arith_upper", "arith_lower_scaled", "arith_upper_scaled"):      # position 0 of both plans: a NaN no list names
        f, t = T[name]["f"], ts.targets(T[name]["f"])
        assert t["L.pos0"] == t["U.pos0"] == 0 and np.isnan(T[name]["b"][0]) and 0 not in _named(f)
    for name, t in T.items():
        ref = ts.reference(t["f"], t["b"])
        assert t["f"]["n"] <= 130
        assert not differing(ref, ts.numpy_reference(t["f"], t["b"])).any(), name
        if t["expect"] is not None:
            assert not differing(ref, t["expect"]).any(), (name, np.flatnonzero(differing(ref, t["expect"])))
        else:
            assert np.array_equal(np.isnan(ref), t["nan_rows"]) and np.isfinite(ref[~t["nan_rows"]]).all()
    # the arithmetic table holds every kind it is about, and they do not cancel: stated per row by arith_table, counted here
    x = T["arith_lower_scaled"]["expect"]
    cl = classify(x)
    assert (cl == NAN).sum() >= 8 and (cl == PINF).sum() >= 4 and (cl == NINF).sum() >= 4
    assert (np.signbit(x) & (x == 0.0)).sum() >= 3 and ((x != 0.0) & (np.abs(x) < 2.2250738585072014e-308)).sum() >= 6
    for k in (47, 20):
        assert bits(x[k:k + 1])[0] == bits(np.array([-0.0]))[0]
    assert bits(T["arith_lower"]["expect"][41:42])[0] == bits(np.array([-0.0]))[0]       # +0.0 * dinv = -2: the sign follows dinv
    # the NaN of the chain travels through 77 rows, of 77 different levels: more than a slice
    f = T["nan_chain_lower"]["f"]
    assert np.isnan(T["nan_chain_lower"]["expect"]).sum() == 77 and len(set(f["lev"][3:80].tolist())) == 77
    # node table: the classes of the special nodes, everything else finite
    nt = ts.node_table()
    f, b = nt["f"], nt["b"]
    ref = ts.reference(f, b)
    assert not differing(ref, ts.numpy_reference(f, b)).any()
    code = {"N": NAN, "+": PINF, "-": NINF, "F": FIN}
    want = np.full(f["n"], FIN, dtype=np.int8)
    want[3], want[4], want[0] = PINF, NINF, NAN
    want[16:43] = [code[c] for c in NODE_CLASSES]
    assert np.array_equal(classify(ref), want)
    assert bits(ref[41:42])[0] == bits(np.array([0.0]))[0]            # the odd last column alone: +0.0
    t = ts.targets(f)
    assert t["L.pos0"] == t["U.pos0"] == 0 and np.isnan(b[0]) and 0 not in _named(f)     # slot 0 is NaN, no list names it
    assert {2, 3, 5} <= set(np.diff(f["nstart"]).tolist()) and f["nstart"].size - 1 > 64
    assert bits(ref[28:29])[0] == bits(np.array([-0.0]))[0] and 0.0 < ref[27] < 1e-310 and ref[26] == -(1e-160 * 1e-160)
    # row 18: the pair added first overflows (1e308 + 1e308), one product after the other stays finite -- the two orders differ
    r = nt["seq_row"]
    p0, p1 = 1e8 * 1e300, 1e8 * 1e300
    assert np.isfinite((b[r] - p0) - p1) and b[r] - (p0 + p1) == -np.inf and ref[r] == -np.inf
    # block columns: 43 nodes of 3 rows; the same kinds, the same two proofs
    bt = ts.block_node_table()
    f, b = bt["f"], bt["b"]
    ref = ts.reference(f, b)
    assert not differing(ref, ts.numpy_reference(f, b)).any()
    assert set(np.diff(f["nstart"]).tolist()) == {3} and f["n"] <= 130
    want = np.full(f["n"], FIN, dtype=np.int8)
    want[:48] = [code[c] for c in BLOCK_CLASSES]
    t = ts.targets(f)
    assert t["L.pos0"] == 0 and t["U.pos0"] in (0, 1, 2) and not {0, 1, 2} & _named(dict(f, rl=f["rl"] * 0 + np.repeat(f["rl"][f["nstart"][:-1]], 3), rlu=f["rlu"] * 0))
    assert np.array_equal(classify(ref), want)
    neg0, pos0 = bits(np.array([-0.0]))[0], bits(np.array([0.0]))[0]
    assert [int(v) for v in bits(ref[[13, 23, 33, 34, 45]])] == [neg0, neg0, neg0, pos0, pos0]
    assert ref[36] == -(1e-160 * 1e-160) and 0.0 < ref[37] < 1e-310 and ref[38] == 5e-324 and 0.0 < ref[41] < 1e-310
    r = bt["seq_row"]
    assert np.isfinite((b[r] - p0) - p1) and b[r] - (p0 + p1) == -np.inf and ref[r] == -np.inf
    for g in (f, nt["f"]):                                       # every shared list of the block table is a run of whole nodes
        sh = g["rl"][g["nstart"][:-1]]
        assert (sh % 2 == 1).any()
    for u in range(f["nstart"].size - 1):
        c = f["cj"][f["rp"][3 * u]:f["rp"][3 * u] + f["rl"][3 * u]]
        assert c.size % 3 == 0 and (c.reshape(-1, 3) == c.reshape(-1, 3)[:, :1] + np.arange(3)).all() and (c[::3] % 3 == 0).all() and (c >= 3).all()


def test_no_input_carries_the_sentinel_payload():
    """no right-hand side, factor value or reference result of any case is the sentinel, and no input NaN carries its payload with
    either sign, quiet or signalling"""
    def clean(a, what):
        u = bits(a[np.isnan(a)])
        assert not ((u & np.uint64(0x0007FFFFFFFFFFFF)) == np.uint64(ts.PAYLOAD & 0x0007FFFFFFFFFFFF)).any(), what
        assert not (bits(a) == np.uint64(ts.SENTINEL)).any(), what

    def factor(f, what):
        for key in ("cv", "cvu", "dinv", "rscale"):
            if f.get(key) is not None:
                clean(np.asarray(f[key]), what + " " + key)
    assert ts.SENTINEL & 0x0007FFFFFFFFFFFF == ts.PAYLOAD & 0x0007FFFFFFFFFFFF
    clean(ts.SPECIALS, "SPECIALS")
    for name, config in ts.part_a_cases():
        c = ts.part_a_case(name, config)
        factor(c["f"], name)
        clean(c["b"], name)
    for name, config in (("n65", "both"), ("chain", "U"), ("fixed3", "L")):
        cl, rounds = ts.part_a_refs(name, config, True)
        clean(cl, name)
        for bp, ref in rounds:
            clean(bp, name); clean(ref, name)
    for name, t in list(ts.special_tables().items()) + [("node_table", ts.node_table()), ("block_node_table", ts.block_node_table())]:
        factor(t["f"], name); clean(t["b"], name); clean(ts.reference(t["f"], t["b"]), name)
    for name in ts.C_FACTORS:
        f, seq = ts.part_c_case(name)
        for b, ref in seq:
            clean(b, name)
            if ref is not None:
                clean(ref, name)
                assert np.isfinite(ref).all()
