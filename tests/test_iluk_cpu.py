"""ILU(k) without a GPU: the host symbolic pass of csrc/ilu_factor.hip (mi355x_iluk_symbolic_host) against the restatement of the
level-of-fill rule in tests/iluk_ref.py, that restatement against an independent construction (complete LU by boolean elimination),
and the numeric reference (iluk_ref.reference_pass) against the oracle at zero fill and against A itself at full fill."""
import ctypes as C

import numpy as np
import pytest

import ilufactor as ilf
import iluk_ref as ik
import orc
from iluk_ref import bits

INVALID = 1                                     # hipErrorInvalidValue
SHAPES = ["lap2d", "p7", "ex10", "random"]
GUARD = 16


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def symbolic_lib(k, ai, aj, levels, with_levels=True):
    """the two calls; (rc, bad_row) on failure, else (bi, bj, bdiag, bjlev) -- bj / bjlev between guard bands that are checked"""
    ai, aj = _i32(ai), _i32(aj)
    n = ai.size - 1
    bi, bd, bad = np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int32), C.c_int(-9)
    rc = k.mi355x_iluk_symbolic_host(n, ai.ctypes.data, aj.ctypes.data, levels, bi.ctypes.data, bd.ctypes.data, None, None, C.byref(bad))
    if rc:
        return rc, bad.value
    assert bad.value == -1
    size = int(bd[0]) + 2
    bj, bl = np.full(size + GUARD, -7, np.int32), np.full(size + GUARD, -7, np.int32)
    bi2, bd2 = bi.copy(), bd.copy()
    rc = k.mi355x_iluk_symbolic_host(n, ai.ctypes.data, aj.ctypes.data, levels, bi2.ctypes.data, bd2.ctypes.data, bj.ctypes.data,
                                     bl.ctypes.data if with_levels else None, None)
    assert rc == 0 and np.array_equal(bi, bi2) and np.array_equal(bd, bd2)
    assert (bj[size - 1:] == -7).all() and (bl[size - 1:] == -7).all(), "the last slot or the guard band was written"
    if not with_levels:
        assert (bl == -7).all()
    return bi, bj[:size], bd, bl[:size]


def same_layout(got, ref, levels_too=True):
    nz = int(ref[2][0]) + 1
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]), "row pointers differ"
    assert np.array_equal(got[1][:nz], ref[1][:nz]), "columns differ"
    if levels_too:
        assert np.array_equal(got[3][:nz], ref[3][:nz]), "levels differ"


# ---------------------------------------------------------------- 1 / 2. the library against the restatement
@pytest.mark.parametrize("levels", [0, 1, 2, 3])
@pytest.mark.parametrize("name", SHAPES)
def test_symbolic_equals_the_restated_rule_array_for_array(built, name, levels):
    k = built.load_kernels()
    ai, aj, _ = ik.shape(name)
    ref = ik.layout_of(name, levels)
    got = symbolic_lib(k, ai, aj, levels)
    same_layout(got, ref)
    same_layout(symbolic_lib(k, ai, aj, levels, with_levels=False), ref, levels_too=False)
    nz = int(ref[2][0]) + 1
    assert got[3][:nz].max() <= levels and (got[3][:nz][ref[2][:-1]] == 0).all()
    if levels == 0:
        lay = ilf.layout(ai, aj)
        assert nz == int(ai[-1])
        same_layout(got, lay + (np.zeros(nz + 1, np.int32),))


def test_symbolic_of_nothing_and_of_one_row(built):
    k = built.load_kernels()
    bi, bj, bd, _ = symbolic_lib(k, np.zeros(1, np.int32), np.zeros(0, np.int32), 2)
    assert bi[0] == 0 and bd[0] == -1 and bj.size == 1
    bi, bj, bd, bl = symbolic_lib(k, np.array([0, 1], np.int32), np.zeros(1, np.int32), 3)
    assert list(bi) == [0, 0] and list(bd) == [0, -1] and bj[0] == 0 and bl[0] == 0


# ---------------------------------------------------------------- 3. the restatement against complete LU
@pytest.mark.parametrize("name", ["lap2d", "ex10", "random60"])
def test_enough_levels_give_the_pattern_of_complete_lu(built, name):
    """levels >= n keeps every fill entry; complete LU's pattern comes from boolean elimination of the dense pattern, which shares
    nothing with the level rule"""
    k = built.load_kernels()
    ai, aj, _ = ilf._values(ik.random_pattern(60, 9), 9) if name == "random60" else ik.shape(name)
    n = ai.size - 1
    full = ik.full_lu_pattern(ai, aj)
    for levels in (n, n + 5):
        ref = ik.symbolic(ai, aj, levels)
        assert np.array_equal(ik.dense_pattern(ref), full), name
        same_layout(symbolic_lib(k, ai, aj, levels), ref)
    assert full.sum() > ai[-1]                     # (there is fill to speak of)


# ---------------------------------------------------------------- 4. the counts grow until they stop
@pytest.mark.parametrize("name", SHAPES)
def test_entry_counts_grow_with_the_level_until_they_stop(built, name):
    k = built.load_kernels()
    ai, aj, _ = ik.shape(name)
    n = ai.size - 1
    # a level keeps every entry of the level before it; from n - 1 levels on nothing is added (a fill path visits a row once)
    counts, prev = [], None
    tried = list(range(0, 9)) + [n - 1, n, n + 5]
    for levels in tried:
        lay = symbolic_lib(k, ai, aj, levels)
        cur = ik.dense_pattern(lay)
        counts.append(int(lay[2][0]) + 1)
        assert int(cur.sum()) == counts[-1]
        if prev is not None:
            assert not (prev & ~cur).any(), "%d levels lost an entry that fewer levels hold" % levels
        prev = cur
    print(name, dict(zip(tried, counts)))
    assert counts[0] == int(ai[-1]) and all(b >= a for a, b in zip(counts, counts[1:]))
    assert counts[-1] == counts[-2] == counts[-3]
    if name != "ex10":                             # (ex10's rows are nearly full already)
        assert counts[1] > counts[0] and counts[2] > counts[1], counts


# ---------------------------------------------------------------- 5. errors
def test_every_error_names_its_row_and_writes_nothing(built):
    k = built.load_kernels()
    ai, aj, _ = ik.shape("lap2d")
    ai, aj = _i32(ai), _i32(aj)
    n = ai.size - 1
    assert symbolic_lib(k, ai, aj, -1) == (INVALID, -1)
    # an empty row
    r = 17
    keep = np.ones(aj.size, dtype=bool); keep[ai[r]:ai[r + 1]] = False
    ai2 = ai.copy(); ai2[r + 1:] -= ai[r + 1] - ai[r]
    assert symbolic_lib(k, ai2, aj[keep], 1) == (INVALID, r)
    # a missing diagonal
    r = 30
    d = int(ai[r] + np.flatnonzero(aj[ai[r]:ai[r + 1]] == r)[0])
    keep = np.ones(aj.size, dtype=bool); keep[d] = False
    ai2 = ai.copy(); ai2[r + 1:] -= 1
    assert symbolic_lib(k, ai2, aj[keep], 1) == (INVALID, r)
    # unsorted columns, a column twice, a column outside the matrix
    r = 44
    aj2 = aj.copy(); aj2[ai[r]], aj2[ai[r] + 1] = aj[ai[r] + 1], aj[ai[r]]
    assert symbolic_lib(k, ai, aj2, 2) == (INVALID, r)
    aj2 = aj.copy(); aj2[ai[r] + 1] = aj2[ai[r]]
    assert symbolic_lib(k, ai, aj2, 2) == (INVALID, r)
    aj2 = aj.copy(); aj2[ai[n] - 1] = n
    assert symbolic_lib(k, ai, aj2, 0) == (INVALID, n - 1)
    # the first row at fault is the one named
    aj2 = aj.copy(); aj2[ai[50]], aj2[ai[50] + 1] = aj[ai[50] + 1], aj[ai[50]]; aj2[ai[20]], aj2[ai[20] + 1] = aj[ai[20] + 1], aj[ai[20]]
    assert symbolic_lib(k, ai, aj2, 1) == (INVALID, 20)
    # a second call on arrays that are not the first call's: refused, the guard band of bj untouched
    bi, bj, bd, _ = symbolic_lib(k, ai, aj, 1)
    wrong = ik.layout_of("lap2d", 0)
    out = np.full(bj.size + GUARD, -7, np.int32)
    bi0, bd0 = wrong[0].copy(), wrong[2].copy()
    bad = C.c_int(-9)
    assert k.mi355x_iluk_symbolic_host(n, ai.ctypes.data, aj.ctypes.data, 1, bi0.ctypes.data, bd0.ctypes.data, out.ctypes.data, None, C.byref(bad)) == INVALID
    assert (out[int(wrong[2][0]) + 1:] == -7).all()
    # missing arrays
    assert k.mi355x_iluk_symbolic_host(n, ai.ctypes.data, aj.ctypes.data, 1, None, bd0.ctypes.data, None, None, None) == INVALID
    assert k.mi355x_iluk_symbolic_host(n, None, aj.ctypes.data, 1, bi0.ctypes.data, bd0.ctypes.data, None, None, None) == INVALID
    assert k.mi355x_iluk_symbolic_host(-1, ai.ctypes.data, aj.ctypes.data, 1, bi0.ctypes.data, bd0.ctypes.data, None, None, None) == INVALID


# ---------------------------------------------------------------- 6. the numeric reference
@pytest.mark.parametrize("name", SHAPES + ["fill_wide", "a_wide", "uchunk_fill"])
def test_reference_at_zero_fill_carries_the_oracles_bits(name):
    ai, aj, aa = ik.shape(name)
    ba, frow = ik.clean_factor(name, 0)
    bi, bj, bd, oba = orc.ilu0_factor(ai, aj, aa)
    lay = ik.layout_of(name, 0)
    assert np.array_equal(bi, lay[0]) and np.array_equal(bd, lay[2]) and np.array_equal(bj[:-1], lay[1][:-1])
    assert frow[0] == -1 and np.array_equal(bits(ba[:-1]), bits(oba[:-1]))
    same = ilf.reference_pass(ai, aj, aa, None, [0.0], ilf.ZP, [1])[0]
    assert np.array_equal(bits(ba), bits(same))


@pytest.mark.parametrize("name", ["lap2d", "ex10", "random60"])
def test_reference_at_full_fill_reproduces_a(name):
    """complete LU without pivoting: L U = A + E with |E| <= gamma_n |L||U| entry by entry (Higham, Accuracy and Stability of
    Numerical Algorithms, theorem 9.3), gamma_n = n u / (1 - n u), u = eps / 2.  The loop here rounds twice where the theorem's
    rounds once in two places (the multiplier is w * (1 / u_kk), and U's diagonal is read back as 1 / (1 / w)), which adds at most
    3 u; n eps = 2 n u covers gamma_(n + 3) for every n >= 4.  The bound is asked for row by row, summed over the row; the product
    L U is formed in extended precision so that forming it adds nothing to E."""
    ai, aj, aa = ilf._values(ik.random_pattern(60, 9), 9) if name == "random60" else ik.shape(name)
    n = ai.size - 1
    lay = ik.symbolic(ai, aj, n)
    ba, frow, _, pend = ik.reference_pass(ai, aj, aa, None, [0.0], ilf.ZP, [1], layout=lay)
    assert frow[0] == -1 and pend[0] == 0
    L, U = ik.dense_factors(lay, ba)
    A = np.zeros((n, n)); A[np.repeat(np.arange(n), np.diff(ai)), aj] = aa
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18
    E = np.abs(L.astype(ld) @ U.astype(ld) - A.astype(ld)).sum(axis=1)
    bound = n * ilf.EPS * (np.abs(L).astype(ld) @ np.abs(U).astype(ld)).sum(axis=1)
    print("%s: n = %d, largest row error / bound = %.3g" % (name, n, float((E / bound).max())))
    assert (E <= bound).all()


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", SHAPES + ["fill_wide", "a_wide", "uchunk_fill"])
def test_no_clean_case_reports_a_failing_row(name, levels):
    ba, frow = ik.clean_factor(name, levels)
    assert frow[0] == -1 and np.isfinite(ba).all()


# ---------------------------------------------------------------- the shapes hold what the GPU tests use them for
def test_the_shapes_reach_the_paths_they_are_there_for():
    seen = set()
    for name in ("lap2d", "p7"):
        ai, _, _ = ik.shape(name)
        assert ilf.lanes_of(ai) == 8
        for levels in (1, 2):
            seen.add(ik.lanes_of(ik.layout_of(name, levels)))
    assert {16, 32} <= seen, seen                                    # A's rows need 8 lanes, the factor's 16 or 32
    ai, _, _ = ik.shape("fill_wide")
    assert np.diff(ai).max() <= ik.WAVE and ik.widest(ik.layout_of("fill_wide", 1)) > ik.WAVE
    rows = ik.factor_rows(ik.layout_of("fill_wide", 1))
    assert max(r[2] for r in rows) > ik.WAVE and max(r[0].size - r[2] - 1 for r in rows) > ik.WAVE      # wide in L and wide in U
    ai, _, _ = ik.shape("a_wide")
    assert np.diff(ai).max() > ik.WAVE and ik.widest(ik.layout_of("a_wide", 1)) > np.diff(ai).max()
    ai, _, _ = ik.shape("uchunk_fill")
    lay0, lay1 = ik.layout_of("uchunk_fill", 0), ik.layout_of("uchunk_fill", 1)
    for k_, size in ik.UCHUNK_SIZES.items():
        assert lay1[2][k_] - lay1[2][k_ + 1] - 1 == size and lay0[2][k_] - lay0[2][k_ + 1] - 1 < size


def test_the_skipped_fill_case_is_what_it_says():
    ai, aj, aa = ik.skipped_fill_case()
    lay = ik.symbolic(ai, aj, 1)
    ba, frow, _, _ = ik.reference_pass(ai, aj, aa, None, [0.0], ilf.ZP, [1], layout=lay)
    rows = ik.factor_rows(lay)
    val = lambda i, c: ba[rows[i][1][list(rows[i][0]).index(c)]]      # noqa: E731
    lev = lambda i, c: lay[3][rows[i][1][list(rows[i][0]).index(c)]]   # noqa: E731
    assert frow[0] == -1
    assert lev(2, 1) == lev(3, 1) == lev(3, 2) == lev(2, 5) == lev(3, 5) == 1
    plus_zero = bits(np.array([0.0]))[0]
    assert bits(np.array([val(2, 1)]))[0] == plus_zero and bits(np.array([val(3, 1)]))[0] == plus_zero      # never touched: skipped
    assert 1.0 / val(1, 1) < 0.0                                                                            # (a multiplier formed anyway: -0.0)
    assert val(3, 2) == -0.5 / 2.5 and val(2, 5) == -0.5 and val(3, 5) == -0.5 - (-0.2 * -0.5)


def test_the_blocks_case_fails_shifts_and_passes():
    c = ik.blocks_case()
    p1, p2, p3 = [p[4] for p in c["passes"]]
    kinds = np.arange(ik.NBLOCKS) % 5
    assert (p1[kinds == 0] == 0).all() and (p1[kinds == 1] == 0).all() and (p1[kinds == 4] == 0).all()
    assert (p1[kinds == 2] == 1).all() and (p2[kinds == 2] == 0).all()          # one shift
    assert (p2[kinds == 3] == 1).all() and (p3 == 0).all()                      # two shifts
    assert int(c["layout"][2][0]) + 1 > int(c["ai"][-1])                        # a fill pattern
    # the failing row of a kind-3 block is its second row in passes 1 and 2
    for ps in (0, 1):
        fr = c["passes"][ps][2]
        assert all(fr[b] == c["blk"][b] + 1 for b in np.flatnonzero(kinds == 3))
