"""The coverage contract of the random re-set-up programs (tests/pcprog.py), checked from the programs alone, and the model against
plain NumPy.  No GPU."""
import numpy as np
import pytest

import iluk_ref as ik
import orc
import pcprog as pp


@pytest.fixture(scope="module")
def programs(built):
    return [pp.generate(i) for i in pp.SEEDS]


def test_same_index_same_program_and_show_lists_every_call(programs):
    for i in (0, 17, 45, len(pp.SEEDS) - 1):
        again = pp.generate(i)
        assert again["calls"] == programs[i]["calls"] and again["operator"] == programs[i]["operator"]
        lines = pp.show(programs[i]["calls"]).split("\n")
        assert len(lines) == len(programs[i]["calls"]) and all(c[0] + "(" in l for c, l in zip(programs[i]["calls"], lines))
    assert all(len(p["calls"]) <= pp.MAXCALLS for p in programs)
    assert {p["operator"] for p in programs} == set(pp.OPERATORS)


def test_the_pool(built):
    """full diagonal, diagonally dominant, O(1); A and B of one size and different patterns; the inode operator has three node levels"""
    for name in pp.OPERATORS + pp.ICC_OPERATORS:
        op = pp.operator(name)
        for ai, aj, aa in op.values():
            n = ai.size - 1
            rows = np.repeat(np.arange(n), np.diff(ai))
            d, off = np.zeros(n), np.zeros(n)
            d[rows[rows == aj]] = np.abs(aa[rows == aj]); np.add.at(off, rows[rows != aj], np.abs(aa[rows != aj]))
            # (dominant before the 5 % perturbation of the Poisson members)
            assert np.all(d * 1.05 >= off * 0.95) and np.all(d > 0) and np.abs(aa).max() < 100 and np.all(np.isfinite(aa))
    nodes, ns = orc.check_inode(*pp.operator("inode")["A"][:2])
    assert nodes == 3 and list(ns) == [3, 3, 3] and orc.check_inode(*pp.operator("inode")["B"][:2])[0] > 0
    assert all(orc.check_inode(*pp.operator(k)["A"][:2])[0] == 0 for k in ("p7", "lap2d", "nonsym"))
    for name in pp.ICC_OPERATORS:                       # symmetric, and positive definite by weak dominance with a positive diagonal
        for ai, aj, aa in pp.operator(name).values():
            D = _dense(ai, aj, aa, ai.size - 1)
            assert np.array_equal(D, D.T) and np.linalg.eigvalsh(D).min() > 0
    # with zero fill one lane sums every triangle row of every member, which is what the bits of enough sweeps rest on (Model.held_to_bits)
    assert all(pp.widest_triangle_row(ai, aj, 0) <= 16 for name in pp.OPERATORS for ai, aj, _ in pp.operator(name).values())


def test_every_call_kind_and_every_motif_occurs(programs):
    assert {c[0] for p in programs for c in p["calls"]} == set(pp.KINDS)
    assert {c[1] for p in programs for c in p["calls"] if c[0] == "load_values"} == {"shift_case", "failing_case", "clean"}
    assert {p["motif"][:4] for p in programs} == {t[:4] for t in pp.TABLE}
    want = {("mode", a, b, ch) for a in pp.MODES for b in pp.MODES for ch in pp.CHANGES} | {("route", a, b, ch) for a in pp.ROUTES for b in pp.ROUTES for ch in pp.CHANGES} \
        | {("crossing", x, None, None) for x in pp.CROSSINGS}
    assert {t[:4] for t in pp.TABLE} == want
    setups = [c for p in programs for c in p["calls"] if c[0] == "setup"]
    assert {c[1] for c in setups} == set(pp.ROUTES) and {c[3] for c in setups} == {None, "column", "level"} and {c[4] for c in setups} == {None, 0}
    assert {c[5] for c in setups} == {None, 1} and {c[6] for c in setups} == {0, 1, 2} and {c[2].split(":")[0] for c in setups} == set(pp.MODES)
    assert any(c[2] == "sweeps:2" for c in setups)
    assert 0 in {rc for p in programs for rc in p["rc"]} and pp.MISSING_DIAGONAL in {rc for p in programs for rc in p["rc"]}
    for p in programs:                                  # the motif is whole, behind a change that makes its first set-up run
        assert p["calls"][p["marks"][0] - 1][0] in pp.DEVICE_CHANGES and p["calls"][p["marks"][0]][0] in ("setup", "swap_operator", "load_values")
        assert p["marks"][1] - p["marks"][0] >= 5


def in_force(p):
    """(route, mode) of every set-up of a program that ran a factorisation and succeeded, in order"""
    m, out = pp.Model(p["operator"], p["index"]), []
    for c in p["calls"]:
        before = m.pc.num
        m.apply(c)
        if c[0] in ("setup", "setup_same") and m.pc.num > before:
            out.append((m.pc.cfg[0], m.pc.cfg[1].split(":")[0]))
    return out


def test_every_ordered_pair_of_modes_and_of_routes_occurs_twice(programs):
    modes, routes = {}, {}
    for p in programs:
        seq = in_force(p)
        for (r0, m0), (r1, m1) in zip(seq, seq[1:]):
            modes[(m0, m1)] = modes.get((m0, m1), 0) + 1
            routes[(r0, r1)] = routes.get((r0, r1), 0) + 1
    assert all(modes.get((a, b), 0) >= 2 for a in pp.MODES for b in pp.MODES), modes
    assert all(routes.get((a, b), 0) >= 2 for a in pp.ROUTES for b in pp.ROUTES), routes


def dense_rebuild(p):
    """the operators of a program rebuilt from the pool through dense NumPy alone: per operator a dense matrix and the mask of its
    stored entries, each call's plain formula applied to them"""
    base = pp.operator(p["operator"])
    n = base["A"][0].size - 1
    D = {k: _dense(*base[k], n) for k in ("A", "B")}
    S = {k: _dense(base[k][0], base[k][1], np.ones(base[k][2].size), n) > 0 for k in ("A", "B")}
    pool = lambda k, aa: _dense(base[k][0], base[k][1], aa, n)
    cur = back = "A"
    for c in p["calls"]:
        k = c[0]
        if k == "swap_operator": cur = back = c[1]
        elif k == "load_values" and c[1] == "failing_case": cur = "F"
        elif k == "load_values":
            cur = back
            D[cur] = pool(cur, base[cur][2]) * S[cur]
            if c[1] == "shift_case": D[cur][0, 0] = 0.0
        elif k == "matscale": D[cur] = c[1] * D[cur]
        elif k == "matdiagscale": D[cur] = pp.scaling(n, c[1], 0.3)[:, None] * D[cur] * (1.0 if c[2] is None else pp.scaling(n, c[2], 0.05)[None, :])
        elif k == "matshift": D[cur] = D[cur] + c[1] * np.eye(n)
        elif k == "mataxpy_same": D[cur] = D[cur] + c[1] * pool(cur, pp.new_values(base[cur][2], c[2])) * S[cur]
        elif k == "setvalues_same_pattern": D[cur] = pool(cur, pp.new_values(base[cur][2], c[1])) * S[cur]
        elif k in ("matzerorowscols", "matzerorows_default"):
            r = list(c[1])
            D[cur][r, :] = 0.0
            if k == "matzerorowscols": D[cur][:, r] = 0.0
            else: S[cur][r, :] = False; S[cur][r, r] = True
            D[cur][r, r] = c[2]
    return D, S


def test_the_models_operator_equals_a_rebuild_from_its_final_pattern_and_values(programs):
    """after every program, ILU and ICC alike: the model's pattern is the rebuilt mask exactly, its values the rebuilt dense matrix
    compressed to that pattern to rounding (the model rounds as the library does, the rebuild as NumPy's dense products do)"""
    for p in programs + [pp.generate_icc(i) for i in pp.ICC_SEEDS]:
        m = pp.replay(p)
        D, S = dense_rebuild(p)
        for k in ("A", "B"):
            ai, aj, aa = m.csr(k)
            n = ai.size - 1
            rows = np.repeat(np.arange(n), np.diff(ai))
            assert ai[0] == 0 and ai[-1] == aj.size == aa.size and all(np.all(np.diff(aj[ai[r]:ai[r + 1]]) > 0) for r in range(n))
            mask = np.zeros((n, n), bool); mask[rows, aj] = True
            assert np.array_equal(mask, S[k]), (p["index"], k)
            assert np.allclose(aa, D[k][rows, aj], rtol=1e-12, atol=1e-13) and not D[k][~S[k]].any(), (p["index"], k)
            assert np.array_equal(pp.operator(p["operator"])[k][1][m.M[k]["orig"]], aj)
            assert np.all(np.isfinite(aa)) and np.abs(aa).max() < 1e6
        for k in ("A", "B"):                            # the failing variants: the pool's pattern without (0, 0), never changed
            fi, fj, fa = m.csr("F" + k)
            bi, bj, ba = pp.operator(p["operator"])[k]
            assert fj.size == bj.size - 1 and 0 not in fj[:fi[1]] and np.array_equal(fa, ba[m.M["F" + k]["orig"]])


def test_the_models_changes_are_the_plain_formulas(built):
    m = pp.Model("nonsym", 0)
    ai, aj, aa = (a.copy() for a in m.csr())
    n = m.n
    D = lambda csr: _dense(*csr, n)
    A = D((ai, aj, aa))
    close = lambda u, v: np.allclose(u, v, rtol=1e-13, atol=1e-13)
    m.apply(("matscale", -0.75)); assert close(D(m.csr()), -0.75 * A)
    m.apply(("matshift", 1.25)); assert close(D(m.csr()), -0.75 * A + 1.25 * np.eye(n))
    m.apply(("mataxpy_same", 0.5, 7)); assert close(D(m.csr()), -0.75 * A + 1.25 * np.eye(n) + 0.5 * D((ai, aj, pp.new_values(aa, 7))))
    m.apply(("load_values", "clean")); assert np.array_equal(m.csr()[2], aa)
    m.apply(("matdiagscale", 3, 4)); assert close(D(m.csr()), pp.scaling(n, 3, 0.3)[:, None] * A * pp.scaling(n, 4, 0.05)[None, :])
    m.apply(("setvalues_same_pattern", 9)); assert close(m.csr()[2], pp.new_values(aa, 9))
    m.apply(("load_values", "clean"))
    rows = (2, 40)
    m.apply(("matzerorowscols", rows, 2.0))
    Z = A.copy(); Z[list(rows), :] = 0; Z[:, list(rows)] = 0; Z[list(rows), list(rows)] = 2.0
    assert close(D(m.csr()), Z) and m.M["A"]["serial"] == 0
    m.apply(("matzerorows_default", (5,), 1.5))
    Z[5, :] = 0; Z[5, 5] = 1.5
    assert close(D(m.csr()), Z) and m.M["A"]["serial"] == 1 and m.csr()[0][6] - m.csr()[0][5] == 1
    m.apply(("load_values", "shift_case")); assert m.csr()[2][m.csr()[0][0] + list(m.csr()[1][:m.csr()[0][1]]).index(0)] == 0.0
    assert np.all(np.isfinite(m.csr()[2]))
    m.apply(("load_values", "failing_case")); assert m.cur == "FA" and 0 not in m.csr()[1][:m.csr()[0][1]]
    assert m.setup(("host", "level", None, None, None, 0)) == pp.MISSING_DIAGONAL and m.setup(("device", "level", None, None, None, 1)) == pp.MISSING_DIAGONAL
    m.apply(("load_values", "clean")); assert m.cur == "A" and m.setup(("device", "level", None, None, None, 1)) == 0


def _dense(ai, aj, aa, n):
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(ai)), aj] = aa
    return A


def test_the_models_counters_follow_the_stated_rules(built):
    """unchanged state: nothing runs; the device route with the same pattern upload and the same levels: numeric only; anything else:
    symbolic again; the host route restates the reference's symbolic phase every time"""
    m = pp.Model("lap2d", 0)
    dev = lambda tri="syncfree", lv=0: ("device", tri, "column", None, None, lv)
    num = lambda: (m.pc.on_device, m.pc.sym, m.pc.num)
    assert m.setup(dev()) == 0 and num() == (1, 1, 1)
    assert m.setup(dev("level")) == 0 and num() == (1, 1, 1) and m.pc.cfg[1] == "syncfree"       # nothing ran: the old options stay in force
    m.apply(("matscale", 2.0)); assert m.setup(dev("level")) == 0 and num() == (1, 1, 2) and m.pc.cfg[1] == "level"
    m.apply(("setvalues_same_pattern", 1)); m.setup(dev()); assert num() == (1, 1, 3)
    m.apply(("matzerorows_default", (3,), 2.0)); m.setup(dev()); assert num() == (1, 2, 4)
    m.setup(dev(lv=1)); assert num() == (1, 3, 5)                                                  # new levels: symbolic again, values unchanged or not
    m.apply(("swap_operator", "B")); m.setup(dev(lv=1)); assert num() == (1, 4, 6)
    m.apply(("swap_operator", "A")); m.setup(dev(lv=1)); assert num() == (1, 5, 7)               # seen before, but not the last one
    m.apply(("matshift", 0.5)); m.setup(("host", "level", None, None, None, 1)); assert num() == (0, 6, 8)
    m.apply(("matshift", 0.5)); m.setup(dev(lv=1)); assert num() == (1, 7, 9)                    # the host route dropped the context
    m.apply(("load_values", "failing_case")); assert m.setup(dev(lv=1)) == pp.MISSING_DIAGONAL and num() == (0, 7, 9) and not m.pc.ok
    m.apply(("load_values", "clean")); assert m.setup(dev(lv=1)) == 0 and num() == (1, 8, 10) and m.pc.ok
    m.apply(("mark_aborted", 1)); assert m.solver() == (0, 1)
    m.apply(("matshift", 0.5)); m.setup(dev(lv=1)); assert m.solver() == (1, 1)                  # new plans; that one gave up is not forgotten


def test_the_models_iluk_with_every_level_is_the_dense_solve(built):
    """levels >= n on a 12-row matrix: the factor is complete, and the model's application is numpy.linalg.solve through the dense factors"""
    rng = np.random.default_rng(12)
    S = rng.random((12, 12)) < 0.3
    S |= S.T; S[np.arange(12), np.arange(12)] = True
    ri, rj = np.nonzero(S)
    ai = np.zeros(13, np.int32); np.add.at(ai, ri + 1, 1); ai = np.cumsum(ai).astype(np.int32)
    aj = rj.astype(np.int32)
    aa = rng.standard_normal(aj.size); aa[ri == rj] = 6.0
    f, ns = pp.reference_factor(ai, aj, aa, 12)
    assert ns == 0 and np.array_equal(ik.dense_pattern(f[:3]), ik.full_lu_pattern(ai, aj))
    Lm, Um = ik.dense_factors(f[:3], f[3])
    A = _dense(ai, aj, aa, 12)
    assert np.allclose(Lm @ Um, A, rtol=1e-13, atol=1e-13)
    b = pp.rhs(12, 3)
    x = orc.ilu0_solve(f, b)
    assert np.allclose(x, np.linalg.solve(Um, np.linalg.solve(Lm, b)), rtol=1e-12, atol=0) and np.allclose(A @ x, b, rtol=1e-12, atol=1e-12)
    # a few sweeps fewer than levels: the restatement approaches the solve; as many sweeps as levels: it is the solve
    f0, _ = pp.reference_factor(*pp.operator("lap2d")["A"], 0)
    b = pp.rhs(437, 4)
    ref = orc.ilu0_solve(f0, b)
    nl = max(pp.level_counts(*f0[:3]))
    assert nl == max(pp.pattern_levels(*pp.operator("lap2d")["A"][:2], 0))
    assert np.array_equal(pp.bits(pp.jacobi_sweeps(f0, b, nl)), pp.bits(ref))
    d = [np.linalg.norm(pp.jacobi_sweeps(f0, b, k) - ref) for k in (1, 2, 4)]
    assert d[0] > d[1] > d[2] > 0


def test_at_most_a_quarter_of_the_applications_are_held_to_the_bound_only(programs):
    flags = [b for p in programs for b in p["bound_only"]]
    assert len(flags) > 400 and sum(flags) <= len(flags) // 4 and sum(flags) > 0, (sum(flags), len(flags))
    assert all(p["bound_only"] and not all(p["bound_only"]) for p in programs)
    for p in programs:                                  # as many flags as application calls
        assert len(p["bound_only"]) == sum(c[0] in ("apply", "apply_in_place", "solve_preonly", "mark_aborted") for c in p["calls"])


def test_the_icc_programs_cover_their_motifs_and_the_model_is_the_oracle(built):
    progs = [pp.generate_icc(i) for i in pp.ICC_SEEDS]
    assert {p["motif"][:2] for p in progs} == {("change", ch) for ch in pp.CHANGES} | {("crossing", x) for x in pp.ICC_CROSSINGS}
    assert {p["operator"] for p in progs} == set(pp.ICC_OPERATORS) and all(len(p["calls"]) <= pp.MAXCALLS for p in progs)
    assert pp.generate_icc(pp.ICC_SEEDS[3])["calls"] == progs[3]["calls"]
    kinds = {c[0] for p in progs for c in p["calls"]}
    assert kinds >= set(pp.KINDS) - {"apply_in_place"} and "apply_in_place" not in kinds     # (no sweep form behind PCICC)
    assert all(c[1:] == pp.ICC_CFG and pp.options(c[1:], icc=True) == "" and pp.options(c[1:]) != "" for p in progs for c in p["calls"] if c[0] == "setup")
    assert not any(b for p in progs for b in p["bound_only"])                                 # column order throughout: bits
    assert {rc for p in progs for rc in p["rc"]} == {0, pp.MISSING_DIAGONAL}
    # the model's application is the oracle's factor and solve; the shift case takes a positive-definite shift, the clean values none
    m = pp.Model("icc_lap2d", pp.ICC_BASE)
    assert m.setup(pp.ICC_CFG) == 0
    b = pp.rhs(m.n, 1)
    f, ns = orc.icc0_factor(*m.csr())
    assert ns == 0 and np.array_equal(pp.bits(m.expected(b)), pp.bits(orc.icc0_solve(f, b))) and m.getters() == dict(info=pp.icc_levels(*m.csr()[:2]) + (0,))
    A = _dense(*m.csr(), m.n)
    assert np.linalg.norm(A @ m.expected(b) - b) < 0.5 * np.linalg.norm(b)                    # (a preconditioner of A)
    m.apply(("load_values", "shift_case")); assert m.setup(pp.ICC_CFG) == 0 and m.getters()["info"][2] >= 1
    m.apply(("load_values", "clean")); assert m.setup(pp.ICC_CFG) == 0 and m.getters()["info"][2] == 0
