"""The machinery of the device ILU(0) factorisation's lane-width / IEEE-special / containment tests (ilufactor.py) checked
against the references alone, without a GPU: so that test_ilu_factor_specials_gpu.py cannot pass quietly by checking nothing.
What is asserted: reference_pass agrees with the oracle bit for bit on every shape (and with its restarts on a shape that needs
shifts); every shape has the features it is there for -- lane width, row-length edges, chunk positions 0 / 63 / 64, stored zeros,
wide rows naming wide rows --; the hand-built matrices have the stated classes; the containment and failure cases hold what
they promise."""
import numpy as np
import pytest

import ilufactor as ilf
import orc
from ilufactor import WAVE, ZP, bits


def _rows(ai, aj):
    n = ai.size - 1
    nzl = ilf.nzl_of(ai, aj)
    return n, np.diff(ai), nzl, ilf.levels(ai, aj)


@pytest.mark.parametrize("name", list(ilf.SHAPES))
def test_reference_pass_is_the_oracle_bit_for_bit_on_every_shape(name):
    ai, aj, aa = ilf.shape(name)
    bi, bj, bd, ba = orc.ilu0_factor(ai, aj, aa)
    lay = ilf.layout(ai, aj)
    assert np.array_equal(lay[0], bi) and np.array_equal(lay[1][:-1], bj[:-1]) and np.array_equal(lay[2], bd)
    assert orc.ilu0_factor_shift(ai, aj, aa)[1] == 0                          # passing pivots, zero shifts
    got, frow = ilf.clean_factor(name)
    assert frow[0] == -1 and np.array_equal(bits(got), bits(ba))
    assert np.isfinite(got).all() and ai.size - 1 <= 600
    assert ilf.levels(ai, aj).max() + 1 <= 200
    # the pending state: a block that is not pending is not touched
    again = ilf.reference_pass(ai, aj, aa, None, [0.0], ZP, [0], ba=np.full(ba.size, ilf.MARK))
    assert (again[0] == ilf.MARK).all() and again[1][0] == -1 and again[3][0] == 0


@pytest.mark.parametrize("name", ilf.LARGE_ZP_SHAPES)
def test_large_zeropivot_case_tells_a_pivot_inside_rs(name):
    ba, frow, inside = ilf.large_zeropivot_case(name)
    assert frow[0] == -1 and inside >= 10 and np.array_equal(bits(ba), bits(ilf.clean_factor(name)[0]))


def test_reference_pass_driven_by_the_doubling_loop_is_the_oracle_with_restarts():
    n = 20
    pattern = [[c for c in (i - 1, i, i + 1) if 0 <= c < n] for i in range(n)]
    ai = np.zeros(n + 1, np.int32); ai[1:] = np.cumsum([len(p) for p in pattern])
    aj = np.concatenate(pattern).astype(np.int32)
    aa = np.ones(aj.size)
    (_, _, _, ba), nshift = orc.ilu0_factor_shift(ai, aj, aa)
    assert nshift >= 1
    shift, count, pend, got = 0.0, 0, [1], None
    for _ in range(82):
        got, frow, fabs_, pend = ilf.reference_pass(ai, aj, aa, None, [shift], ZP, pend, got)
        if frow[0] < 0:
            break
        assert pend[0] == 1 and fabs_[0] >= 0.0
        shift = shift * 2.0 if count else ZP
        count += 1
    assert count == nshift and pend[0] == 0 and np.array_equal(bits(got), bits(ba))


@pytest.mark.parametrize("name", ilf.LANE_SHAPES)
def test_lane_width_shapes_have_their_rows_and_levels(name):
    ai, aj, _ = ilf.shape(name)
    n, ln, nzl, lev = _rows(ai, aj)
    W, wide = ilf.SHAPES[name]
    assert ilf.lanes_of(ai) == W and not wide and ln.max() <= W
    per_level = np.bincount(lev)
    assert per_level.max() > ilf.BLOCK // W                                   # a level of more than one workgroup
    if name in ilf.ONE_LEVEL:
        assert nzl.max() == 0 and per_level.size == 1
    else:
        assert (per_level == 1).any()                                         # a level of a single row
    # rows of different lengths inside one wavefront (W = 64: one row per wavefront, inside one workgroup), in the order the level's
    # rows are launched
    order = np.argsort(lev, kind="stable")
    together = max(WAVE // W, 4 if W == WAVE else 0)
    if name != "diagonal":
        assert any(np.unique(ln[order[s:s + together]]).size > 1 for s in range(0, n, together))
    expect = {"diagonal": [1], "lower_bidiagonal": [1, 2], "upper_bidiagonal": [1, 2], "tridiagonal": [2, 3]}.get(name, [W, W // 2 + 1])
    assert set(expect) <= set(ln.tolist())
    if name == "lower_bidiagonal":
        assert set(nzl[ln == 2]) == {1}                                       # the diagonal in the last lane
    if name == "upper_bidiagonal":
        assert nzl.max() == 0
    if name == "tridiagonal":
        assert ln.max() == 3 and W == 4                                       # an idle lane in every row
    if name.startswith("rows"):
        full = ln == W
        assert (full & (nzl == 0)).any() and (full & (nzl == W - 1)).any()    # rowlen == W with the diagonal in lane 0 and in the last lane
        assert (ln == 1).any()
    if name == "rows64":
        assert {33, 63, 64} <= set(ln.tolist()) and ln.max() == 64 and (nzl[ln == 64] == 63).any()


def test_wide_shape_has_the_row_length_edges():
    ai, aj, _ = ilf.shape("wide")
    n, ln, nzl, lev = _rows(ai, aj)
    assert ilf.lanes_of(ai) == 64
    wide = np.flatnonzero(ln > WAVE)
    assert {65, 128, 129, 150} <= set(ln[wide].tolist())
    have = set(zip(ln[wide].tolist(), nzl[wide].tolist()))
    assert {0, 63, 64, 65} <= {z for _, z in have} and sum(z == l - 1 for l, z in have) >= 3
    assert any(z % 64 == 0 and z > 0 and z == l - 1 for l, z in have)         # the diagonal last and at a multiple of 64
    assert (nzl[wide] >= 64).any()                                            # the multiplier's owner lane wraps
    names_wide = lambda i: np.isin(aj[ai[i]:ai[i] + nzl[i]], wide).any()      # noqa: E731
    assert sum(names_wide(i) for i in wide) >= 4                              # wide rows whose L columns name wide rows
    narrow = np.flatnonzero(ln <= 9)
    assert sum(names_wide(i) for i in narrow) >= 20                           # narrow rows whose L column names a wide row
    assert (np.bincount(lev) == 1).any() and np.bincount(lev).max() > 4 and (ln == 1).any()
    ai, aj, _ = ilf.shape("mini_wide")
    ln = np.diff(ai)
    assert ln.max() > WAVE and ai.size - 1 == 140


def test_uchunk_shape_shares_the_columns_at_the_chunk_edges():
    ai, aj, _ = ilf.shape("uchunk")
    n, ln, nzl, lev = _rows(ai, aj)
    nzu = ln - nzl - 1
    assert [int(nzu[k]) for k in (0, 1, 2)] == [64, 65, 128]
    seen = set()
    for i in range(3, n):
        cols = aj[ai[i]:ai[i + 1]]
        for k in cols[:nzl[i]]:
            if k > 2:
                continue
            assert ln[i] <= WAVE                                              # a register row
            uk = aj[ai[k] + 1:ai[k + 1]]
            shared = np.flatnonzero(np.isin(uk, cols))
            kind = lambda c: "L" if c < i else ("D" if c == i else "U")       # noqa: E731
            seen |= {(int(k), int(t), kind(uk[t])) for t in shared}
            assert shared.size < uk.size                                      # U(k) columns outside row i's pattern: discarded fill
            assert np.setdiff1d(cols[cols > k], uk).size                      # row-i columns beyond k that U(k) lacks
    pos = {(k, t) for k, t, _ in seen}
    assert {(0, 0), (0, 63), (1, 0), (1, 63), (1, 64), (2, 0), (2, 63), (2, 64), (2, 127)} <= pos
    assert {"L", "D", "U"} == {s for _, _, s in seen}
    assert sum(len({k for k in aj[ai[i]:ai[i] + nzl[i]] if k < 3}) == 3 for i in range(n)) == 1      # one row names all three


@pytest.mark.parametrize("name", ["zeros_narrow", "zeros_wide"])
def test_zero_shapes_take_the_skip(name):
    """stored +0.0 and -0.0 in L positions that the factor keeps with their sign, though the named row's inverted pivot is negative; a
    work value that is nonzero in A and exactly +0.0 in the factor; a stored zero in a U(k) that a later row reads"""
    ai, aj, aa = ilf.shape(name)
    n, ln, nzl, lev = _rows(ai, aj)
    ba = ilf.clean_factor(name)[0]
    bd, slot = ilf.layout(ai, aj)[2], ilf.slots(ai, aj)
    rows = np.repeat(np.arange(n), ln)
    isl = aj < rows
    kept = {"+0": 0, "-0": 0, "cancelled": 0}
    for q in np.flatnonzero(isl & (ba[slot] == 0.0)):
        assert ba[bd[aj[q]]] < 0.0                                            # w * pivot would be a zero of the other sign
        if aa[q] == 0.0:
            assert bits(ba[slot[q]:slot[q] + 1])[0] == bits(aa[q:q + 1])[0]
            kept[ilf.classify(aa[q])] += 1
        else:
            assert not np.signbit(ba[slot[q]])
            kept["cancelled"] += 1
    assert all(kept.values()), kept
    zero_u = np.flatnonzero(~isl & (aj != rows) & (aa == 0.0))
    assert zero_u.size and all(any(rows[q] in aj[ai[i]:ai[i] + nzl[i]] and aj[q] in aj[ai[i]:ai[i + 1]] for i in range(n)) for q in zero_u)
    if name == "zeros_wide":
        p = np.flatnonzero(isl & (ba[slot] == 0.0) & (rows == 100)) - ai[100]
        assert ln[100] > WAVE and (p >= 64).sum() >= 3 and (p < 64).sum() >= 2     # on both sides of the owner lane's wrap


@pytest.mark.parametrize("form", ilf.FORMS)
def test_hand_built_specials_have_the_stated_classes(form):
    m = ilf.specials_matrix(form)
    ai, aj, aa, blk = m["ai"], m["aj"], m["aa"], m["blk"]
    ln = np.diff(ai)
    ncore = int(m["first"][-1])
    assert ilf.lanes_of(ai) == {"narrow": 4, "reg64": 64, "wide": 64}[form]
    assert (ln[:ncore] > WAVE).all() if form == "wide" else ln.max() <= (4 if form == "narrow" else WAVE)
    seen = set()
    for which, zp in (("default", ZP), ("zero", 0.0)):
        ba, frow, fabs_, pend = ilf.reference_pass(ai, aj, aa, blk, m["shifts"], zp, np.ones(blk.size - 1, np.int32))
        efrow, efcls, cls = ilf.stated_classes(form, which)
        assert np.array_equal(frow, efrow), (form, which, frow, efrow)
        for b in np.flatnonzero(frow >= 0):
            assert ilf.classify(fabs_[b]) == efcls[b] and not np.signbit(fabs_[b])
        wrong = {s: (ilf.classify(ba[s]), c) for s, c in cls.items() if ilf.classify(ba[s]) != c}
        assert not wrong, (form, which, wrong)
        # every entry of every core row up to a failing row is stated
        stated = np.zeros(ba.size, dtype=bool); stated[list(cls)] = True
        core = ilf.compared_slots(ai, aj, blk, frow) & ilf.row_slots(ai, aj, np.arange(ai.size - 1) < ncore)
        for b in np.flatnonzero(frow >= 0):                                   # (a failing block: its rows before the failing row, in row order)
            later = np.zeros(ai.size - 1, dtype=bool); later[frow[b] + 1:blk[b + 1]] = True
            core &= ~ilf.row_slots(ai, aj, later)
        assert np.array_equal(stated, core), (form, which)
        seen |= set(cls.values())
    assert seen == {"nan", "+inf", "-inf", "+0", "-0", "sub", "fin"}
    assert ilf.special_cases()[0]["name"] == "nan_in_L" and len(ilf.special_cases()) >= 16


@pytest.mark.parametrize("form", ilf.FORMS)
def test_containment_conditions_hold_from_the_graph_alone(form):
    c = ilf.containment_case(form)
    ai, aj = c["ai"], c["aj"]
    n = ai.size - 1
    nzl = ilf.nzl_of(ai, aj)
    assert n <= 600 and len(c["rounds"]) == 3 and len({r for r, *_ in c["rounds"]}) == 3
    assert ilf.lanes_of(ai) == {"narrow": 8, "reg64": 64, "wide": 64}[form] and (np.diff(ai).max() > WAVE) == (form == "wide")
    # four independent sub-blocks: no entry leaves its quarter
    rows = np.repeat(np.arange(n), np.diff(ai))
    assert np.array_equal(rows // (n // 4), aj // (n // 4))
    for r, q, aap, ref, reach in c["rounds"]:
        assert rows[q] == r and aj[q] != r and not np.isfinite(aap[q]) and np.isfinite(np.delete(aap, q)).all()
        assert reach[r] and reach.sum() >= 2 and (~reach).sum() >= 0.25 * n
        for i in np.flatnonzero(~reach):                                      # closed: a row outside names no reached row
            assert not reach[aj[ai[i]:ai[i] + nzl[i]]].any()
        out = ilf.row_slots(ai, aj, ~reach)
        assert np.array_equal(bits(ref[out]), bits(c["clean"][out]))          # the reference itself is contained
        assert not np.isfinite(ref[ilf.row_slots(ai, aj, reach)]).all()
    assert np.isfinite(c["clean"]).all()


def test_failure_cases_fail_where_they_are_meant_to():
    forms, nonzero, negative = set(), 0, 0
    for name in ilf.FAIL_SHAPES:
        ai, aj, _ = ilf.shape(name)
        n, ln, nzl, lev = _rows(ai, aj)
        rows_ = ilf.failing_rows(name)
        assert lev[rows_[0]] == 0 and lev[rows_[1]] == lev.max() and (lev.max() == 0 or len(rows_) >= 2)
        for r in rows_:
            aa, ba, fabs_ = ilf.failing_case(name, r)                         # (asserts that row r, and no earlier row, fails)
            bd = ilf.layout(ai, aj)[2]
            assert bits(ba[bd[r]:bd[r] + 1])[0] == bits(np.array([fabs_]))[0] and fabs_ >= 0.0
            nonzero += fabs_ != 0.0
            negative += nzl[r] == 0 and aa[ai[r]] < 0.0
            forms.add((ilf.lanes_of(ai), "wide" if ln[r] > WAVE else "registers"))
    assert {(w, "registers") for w in (1, 2, 4, 8, 16, 32, 64)} | {(64, "wide")} <= forms
    assert nonzero >= 10 and negative >= 5
    ai, aj, _ = ilf.shape("wide")
    ln, lev = np.diff(ai), ilf.levels(ai, aj)
    got = {(bool(ln[r] > WAVE), bool(lev[r] > 0)) for r in ilf.failing_rows("wide")}
    assert got == {(True, False), (True, True), (False, False), (False, True)}


def test_block_passes_and_several_failing_rows():
    c = ilf.blocks_case()
    blk = c["blk"]
    assert blk.size - 1 == 40 and (np.diff(blk) == 0).sum() >= 8 and (np.diff(blk) == 1).sum() >= 16
    (s1, ba1, f1, a1, p1), (s2, ba2, f2, a2, p2), (s3, ba3, f3, a3, p3) = c["passes"]
    assert 0 < (f1 >= 0).sum() < 40 and 0 < (f2 >= 0).sum() < (f1 >= 0).sum() and (f3 >= 0).sum() == 0 and not p3.any()
    assert not s1.any() and np.unique(s2[f1 >= 0]).size == 3 and np.unique(s3[f2 >= 0]).size == (f2 >= 0).sum()
    assert np.array_equal(p1 != 0, f1 >= 0) and (f2[p1 == 0] == -1).all()
    fin = c["finished1"]
    assert fin.any() and all((ba[fin] == ilf.MARK).all() for ba in (ba1, ba2, ba3))
    assert np.isfinite(ba3).all() and not (ba3[~fin][:-1] == ilf.MARK).any()
    # each block's own shift: the oracle on every pending block alone, its shift on its diagonal
    ai, aj, aa = c["ai"], c["aj"], c["aa"]
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    aas = aa.copy(); aas[aj == rows] += np.repeat(s3, np.diff(blk))
    whole = orc.ilu0_factor(ai, aj, aas)[3]
    assert np.array_equal(bits(ba3[~fin]), bits(whole[~fin]))
    ai, aj, aa, absof, shift, ref = ilf.multi_fail_case()
    assert ilf.levels(ai, aj).max() == 0 and len(set(absof.values())) == len(absof) == 3
    for r in absof:                                                           # each of them fails on its own
        one = ilf.shape("upper_bidiagonal")[2].copy()
        d = ai[r] + ilf.nzl_of(ai, aj)[r]
        one[d] = aa[d]
        _, fr, fa, _ = ilf.reference_pass(ai, aj, one, None, [0.0], ZP, [1])
        assert fr[0] == r and fa[0] == absof[r]


def test_sweep_factors_hold_every_kind_in_every_part():
    assert {ilf.SHAPES[s][0] for s in ilf.SWEEP_SHAPES} == {1, 2, 4, 8, 16, 32, 64}
    for name in ilf.SWEEP_SHAPES:
        ai, aj, _ = ilf.shape(name)
        ba = ilf.sweep_factor(name)
        assert {ilf.classify(v) for v in ba} >= {"+0", "-0", "+inf", "-inf", "nan"}
    ai, aj, _ = ilf.shape("wide")
    ln, nzl = np.diff(ai), ilf.nzl_of(ai, aj)
    assert (ln - nzl - 1 == 0).any() and (ln - nzl - 1 > WAVE).any()          # rows without strict-upper entries, with more than lanes
    assert ilf.layout(*ilf.shape("diagonal")[:2])[0][-1] == 0                 # nzL = 0: no negate launch
