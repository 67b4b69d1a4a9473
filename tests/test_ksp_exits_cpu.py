"""The table of tests/kspexits.py against the CPU oracle: every case ends with the (its, reason) it is named for, tiny and
replicated; every exit line of the three solvers and of KSPDefaultConverged is claimed; the BiCGStab and CG claims are checked
against restatements that name the line they leave through.  No GPU."""
import numpy as np
import pytest

import kspexits as kx

COMBOS = [(c.name, s, pc) for c in kx.CASES for s in kx.solvers_of(c) for pc in kx.pcs_of(c)]


@pytest.fixture(scope="module")
def runs(built):
    out = {}
    for name, s, pc in COMBOS:
        c = kx.BY_NAME[name]
        for size in ("tiny", "replicated"):
            out[name, s, pc, size] = kx.oracle(c, s, pc, size)
    return out


@pytest.mark.parametrize("name,solver,pc", COMBOS)
def test_case_ends_where_it_is_named_for(runs, name, solver, pc):
    c = kx.BY_NAME[name]
    e = kx.expected(c, solver, pc)
    x, h, its, reason = runs[name, solver, pc, "tiny"]
    assert (its, reason) == (e.its, e.reason)
    assert set(e.exits) <= set(kx.EXITS)
    # what tells the exits of one reason apart
    if "bcgs_tt_zero_s_zero" in e.exits:
        assert h.size == its + 1 and h[-1] == 0.0          # the oracle logs 0.0 there (the reference logs the old norm; the harness follows it)
    if "gmres_res_zero" in e.exits:
        assert h.size == 1 and h[0] == 0.0
    if "conv_nan" in e.exits:
        assert not np.isfinite(h[-1])
    if "conv_dtol" in e.exits:
        assert np.isfinite(h[-1]) and h[-1] >= c.tol["dtol"] * h[0]
    if reason in (kx.INDEF_MAT, kx.INDEF_PC):
        assert h.size == its                               # CG counts the refused iteration, which logged nothing
    if "bcgs_sv_zero" in e.exits or "bcgs_tt_zero_s_nonzero" in e.exits:
        assert h.size == its + 1                           # BiCGStab does not count it


@pytest.mark.parametrize("name,solver,pc", COMBOS)
def test_replicated_case_ends_the_same(runs, name, solver, pc):
    c = kx.BY_NAME[name]
    e = kx.expected(c, solver, pc)
    x, h, its, reason = runs[name, solver, pc, "replicated"]
    n = kx.matrix_of(c)[0].size - 1
    assert x.size == n * kx.copies_for(n) >= 4096 and kx.copies_for(n) & (kx.copies_for(n) - 1) == 0
    if (name, solver) in kx.ROUNDING:
        assert (its, reason) in kx.ROUNDING[name, solver]
    else:
        assert (its, reason) == (e.its, e.reason)
    if its == 0 or (solver == "cg" and its == 1 and reason in (kx.INDEF_MAT, kx.INDEF_PC)):     # the first step was refused: x is the guess
        x0 = np.zeros(n) if c.x0 is None else c.x0
        assert np.array_equal(kx.bits(x), kx.bits(np.tile(x0, kx.copies_for(n))))


@pytest.mark.parametrize("name,solver,pc", [t for t in COMBOS if t[1] in ("cg", "bcgs") and kx.BY_NAME[t[0]].x0 is None])
def test_named_line_against_the_restatement(name, solver, pc):
    c = kx.BY_NAME[name]
    e = kx.expected(c, solver, pc)
    ai, aj, aa = kx.matrix_of(c)
    line, its, reason = (kx.cg_exit if solver == "cg" else kx.bcgs_exit)(ai, aj, aa, c.b, c.tol, pc == "jacobi")
    assert line in e.exits
    if reason is None:
        assert e.error == kx.ERR_FP
    else:
        assert (its, reason) == (e.its, e.reason)
        assert (e.error == kx.ERR_PLIB) == (line == "bcgs_sv_zero")


def test_every_exit_is_claimed():
    claimed = set()
    for name, s, pc in COMBOS:
        claimed |= set(kx.expected(kx.BY_NAME[name], s, pc).exits)
    left_out = set(kx.EXITS) - claimed
    assert left_out <= set(kx.LEFT_OUT), sorted(left_out)
    assert len(kx.LEFT_OUT) <= 1 and set(kx.LEFT_OUT) <= {"bcgs_rho_zero"}
    assert claimed <= set(kx.EXITS)
