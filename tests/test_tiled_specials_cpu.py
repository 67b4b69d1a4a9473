"""The inputs and the reference of test_tiled_specials_gpu.py checked without a GPU (the library's host-only layout builder, the oracle
and tests/tiled.py), so that a GPU pass means something: every poisoned column is unreferenced and really read by a padding entry
(or lies beside real data), every hand-built row's expected value is what the layout's order gives and differs from what a kernel
without the special would give, every layout has the staged tiles, windows, padding and block counts its case relies on, and the
host replay of the layout agrees in class with the oracle on every row of every case."""
import numpy as np
import pytest

import tiled
import tiledspecials as ts
from tiledspecials import Layout, klass, padding
from vecspecials import NAN, differing, same


@pytest.fixture(scope="module")
def k(built):
    return built.load_kernels()


def classes_agree(L, x, yin=None, aa=None):
    y = L.replay(x, yin, aa=aa)
    L.against_oracle(y, x, yin, aa, "host replay")
    return y


def test_replay_is_tiled_apply_on_a_walk_done_once(k):
    case = ts.specials(k)
    L = Layout(k, "specials/split", *case["A"], case["n"], case["stage_min"]["split"])
    try:
        for yin in (None, case["yin"]):
            y = L.replay(case["x"], yin)
            with np.errstate(all="ignore"):
                same(y, tiled.apply(k, L.plan, L.m, L.aa, case["x"], yin), "replay against tiled.apply")
            # the parts: the remainder alone starts from yin as well; staged then remainder is the whole
            same(L.replay(case["x"], L.replay(case["x"], yin, which=1), which=2), y, "staged, then the remainder on top")
    finally:
        L.destroy()


def test_containment_columns_are_unreferenced_and_read_by_padding(k):
    c = ts.containment(k)
    g = tiled.geometry(k)
    L = Layout(k, "containment", *c["A"], c["n"], c["stage_min"])
    L2 = Layout(k, "containment/moved", *c["A2"], c["n"], c["stage_min"])
    try:
        pad = padding(k, L.plan)
        P = c["P"]
        assert 9e4 < L.aj.size < 1.3e5 and L.info["panels"] == 2
        assert L.info["staged"] > 0 and L.info["remainder"] > 0
        assert not np.isin(L.aj, P).any(), "a column of P is referenced"
        gathered = set(pad["staged"]) | set(pad["remainder"])
        assert all(int(q) in gathered or int(q) in c["listed"] for q in P)
        assert gathered <= set(P.tolist()), "every column a padding entry gathers is poisoned"
        assert len(pad["staged"]) > 10 and set(pad["remainder"]) == {0, 1 << ts.WIN}
        assert any(len(w) >= 2 for w in pad["windows"]), "a wavefront with remainder entries in two windows"
        last0 = (c["n"] - 1) // g["tw"] * g["tw"]
        assert last0 in pad["staged"] and pad["tiles"][-1][-1] == last0 // g["tw"] and len(pad["tiles"][-1]) > 1, "the short last tile is brought in by the loader"
        assert len(c["refs"]) == 3 and np.isin(c["refs"], L.aj).all() and len(c["neighbours"]) == 6
        # the heavy row: hundreds of entries in one tile, staged in its panel
        big, heavy = c["big"], c["heavy"]
        cols = L.aj[L.ai[big]:L.ai[big + 1]]
        assert ((cols // g["tw"]) == heavy).sum() >= 300
        assert heavy in pad["tiles"][int(np.searchsorted(L.prow, big, side="right")) - 1] and heavy * g["tw"] in P
        # the reference alone: poison at P changes no bit of it; the oracle agrees
        y = classes_agree(L, c["x"])
        for v in (NAN, np.inf, -np.inf):
            x = c["x"].copy(); x[P] = v
            same(L.replay(x), y, "host replay with P poisoned")
            same(L.oracle(x), L.oracle(c["x"]), "oracle with P poisoned")
        assert np.all(np.isfinite(y))
        # the moved columns: the poisoned rows have the classes the case states, among them the last row of a panel and the first of
        # the next; every other row keeps its bits
        y2 = classes_agree(L2, c["x_moved"])
        rows = np.array(sorted(c["expect_class"]))
        assert np.array_equal(klass(y2[rows]), [c["expect_class"][int(r)] for r in rows])
        (last, first), = L2.panel_edges()
        assert last in c["expect_class"] and first in c["expect_class"]
        other = np.setdiff1d(np.arange(L.m), rows)
        same(y2[other], y[other], "rows that reference no poisoned column")
        pad2 = padding(k, L2.plan)
        assert (1 << ts.WIN) in pad2["remainder"] and heavy * g["tw"] in pad2["staged"], "the moved columns are still padding's gather columns"
        yin = np.sin(np.arange(L.m) * 0.7)
        classes_agree(L2, c["x_moved"], yin)
    finally:
        L.destroy(); L2.destroy()


@pytest.mark.parametrize("placement", ["staged", "remainder", "split"])
def test_special_rows_have_their_stated_values_and_tell_the_wrong_kernel(k, placement):
    case = ts.specials(k)
    L = Layout(k, "specials/" + placement, *case["A"], case["n"], case["stage_min"][placement])
    try:
        assert (L.info["remainder"] == 0) == (placement == "staged") and (L.info["staged"] == 0) == (placement == "remainder")
        srow = np.array(case["srow"])
        if placement == "split":
            for row, spec in zip(srow, ts.SPECIAL_ROWS):
                if spec[1]:
                    assert (L.near[0] == row).sum() == len(spec[1]) and (L.far[0] == row).sum() == len(spec[2]) > 0, spec[0]
        for yin in (None, case["yin"]):
            rows, want, wrong = ts.special_expectation(case, yin is not None)
            y = classes_agree(L, case["x"], yin)
            same(y[rows], want, "the special rows' stated values (%s, %s)" % (placement, "yin" if yin is not None else "no yin"))
            assert differing(want, wrong).all(), [s[0] for s, d in zip(ts.SPECIAL_ROWS, differing(want, wrong)) if not d]
            assert np.all(np.isfinite(y[case["ordinary"]]))
        # every class occurs
        assert set(klass(L.replay(case["x"], case["yin"])).tolist()) == {0, 1, 3} and 2 in klass(L.replay(case["x"])).tolist()
    finally:
        L.destroy()


def test_boundary_layouts_contain_padding_in_both_kinds_of_run(k):
    g = tiled.geometry(k)
    for m in ts.boundary_sizes(k):
        case = ts.boundary(k, m)
        for stage_min in ts.BOUNDARY_STAGE_MIN:
            L = Layout(k, "boundary m=%d stage_min=%d" % (m, stage_min), *case["A"], case["n"], stage_min)
            try:
                pad = padding(k, L.plan)
                assert L.info["panels"] == -(-m // g["panel"]) and len(L.panel_edges()) == L.info["panels"] - 1
                if m == g["panel"]:
                    assert L.prow[1] - L.prow[0] == g["panel"], "a full panel: the spare accumulator sits right behind its last row"
                assert sum(pad["staged"].values()) > 0
                if stage_min > 1:
                    assert L.info["remainder"] > 0 and sum(pad["remainder"].values()) > 0
                else:
                    assert L.info["remainder"] == 0
                cols = np.array(sorted(set(pad["staged"]) | set(pad["remainder"])))
                assert np.isnan(case["x"][cols]).all() and not np.isin(L.aj, cols).any()
                assert np.all(np.diff(L.ai) >= 1), "the rows on both sides of a panel boundary hold entries"
                for yin in (None, case["yin"]):
                    assert np.all(np.isfinite(classes_agree(L, case["x"], yin)))
            finally:
                L.destroy()


def test_tail_layouts_stage_the_short_tile_first_second_and_third(k):
    g = tiled.geometry(k)
    for r in ts.tail_remainders(k):
        for depth in (1, 2, 3):
            case = ts.tail(k, r, depth)
            L = Layout(k, "tail r=%d depth=%d" % (r, depth), *case["A"], case["n"], 1)
            try:
                assert case["n"] % g["tw"] == r and padding(k, L.plan)["tiles"] == [list(range(3 - depth, 3))] and L.info["remainder"] == 0
                assert np.isin([case["n"] - 1, 2 * g["tw"]], L.aj).all() and (np.isin(case["n"] - 2, L.aj) or case["n"] - 2 < (3 - depth) * g["tw"])
                assert np.unique(case["x"]).size == case["n"]
                classes_agree(L, case["x"], case["yin"])
            finally:
                L.destroy()
    case = ts.unstaged_panel(k)
    L = Layout(k, "unstaged panel", *case["A"], case["n"], case["stage_min"])
    try:
        tiles = padding(k, L.plan)["tiles"]
        assert tiles == [[], [1]] and L.info["staged"] > 0 and L.info["remainder"] > 0
        classes_agree(L, case["x"], case["yin"])
    finally:
        L.destroy()


def test_window_layouts_skip_a_window_and_reach_every_block_count(k):
    w = 1 << ts.WIN
    case = ts.window_skip(k)
    L = Layout(k, "window skip", *case["A"], case["n"], case["stage_min"])
    try:
        pad = padding(k, L.plan)
        assert L.info["staged"] == 0 and [0, 2] in pad["windows"] and [0, 1, 2] in pad["windows"]
        assert np.isin([w - 1, w, w + 1], L.aj[L.ai[0]:L.ai[1]]).all()
        classes_agree(L, case["x"], case["yin"])
    finally:
        L.destroy()
    reached = []
    for count in ts.BLOCK_COUNTS:
        case = ts.window_blocks(k, count)
        L = Layout(k, "window blocks %d" % count, *case["A"], case["n"], case["stage_min"])
        try:
            pad = padding(k, L.plan)
            assert L.info["staged"] == 0 and pad["blocks"][0] == count and sum(pad["blocks"]) == count == L.info["blocks"]
            assert pad["windows"][0] == ([0, 1] if count > 1 else [1]) and np.isin([w, w + 1], L.aj).all() and (count == 1 or w - 1 in L.aj)
            reached.append(pad["blocks"][0])
            classes_agree(L, case["x"], case["yin"])
        finally:
            L.destroy()
    assert reached == ts.BLOCK_COUNTS and {1, 4, 5} <= set(reached)      # one block, 2 TL_FG and 2 TL_FG + 1 of the source's TL_FG = 2


def test_changed_values_hold_the_specials_at_known_positions(k):
    case = ts.specials(k)
    aa2, pos = ts.changed_values(case["A"][2], 5)
    assert np.isnan(aa2[pos[0]]) and aa2[pos[1]] == np.inf and aa2[pos[2]] == -np.inf and 0 < aa2[pos[3]] < 1e-320
    L = Layout(k, "specials/split", *case["A"], case["n"], case["stage_min"]["split"])
    try:
        y = classes_agree(L, case["x"], None, aa2)
        assert differing(y, L.replay(case["x"])).sum() >= 8
    finally:
        L.destroy()
