"""The table of tests/kspexits.py against the CPU oracle and the host models: every case ends with the (its, reason) it is named
for, tiny and replicated; every exit line of the eleven solvers, of KSPDefaultConverged and of KSPLSQRDefaultConverged is claimed; the
BiCGStab, CG, TFQMR, CGS, BiCG and MINRES claims are checked against restatements that name the line they leave through.  No GPU.

cg, gmres, bcgs run on the oracle (oracle/ksp_oracle.c), the eight types registered since on the models of tests/*_ref.py
(kspexits.model).  Neither raises.  What stands in for an error of the harness types:
  * bcgs_sv_zero (PETSC_ERR_PLIB): the oracle's DIVERGED_BREAKDOWN without counting the iteration;
  * cg_dot_not_finite, pipecg_dot_not_finite (PETSC_ERR_FP): the NaN goes on into the norm, DIVERGED_NAN at the next test
    (pipelined CG with the natural norm: at iteration 0, where res'u IS the norm);
  * the other seven of the eight have no error exit inside the solve: s == 0, dpi == 0, beta == 0 are reasons,
    and what they refuse they refuse at set-up (test_ksp_exits_gpu.py::test_refusals_at_set_up)."""
import numpy as np
import pytest

import kspexits as kx

COMBOS = [(c.name, s, pc) for c in kx.CASES for s in kx.solvers_of(c) for pc in kx.pcs_of(c, s)]
SEARCHED = {"tfqmr_s_zero_late", "cgs_s_zero_late", "bicg_dpi_zero_late", "bicg_beta_zero", "tfqmr_test_reason_half1", "bcgs_rho_zero"}


@pytest.fixture(scope="module")
def runs(built):
    out = {}
    for name, s, pc in COMBOS:
        c = kx.BY_NAME[name]
        for size in ("tiny", "replicated"):
            out[name, s, pc, size] = (kx.oracle if s in kx.SOLVERS else kx.model)(c, s, pc, size)
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
    if "conv_nan" in e.exits or "pipecg_dot_not_finite" in e.exits:
        assert not np.isfinite(h[-1])
    if "conv_dtol" in e.exits:
        assert np.isfinite(h[-1]) and h[-1] >= c.tol["dtol"] * h[0]
    if reason in (kx.INDEF_MAT, kx.INDEF_PC):
        assert h.size == its                               # CG and MINRES count the refused iteration, which logged nothing
    if "bcgs_sv_zero" in e.exits or "bcgs_tt_zero_s_nonzero" in e.exits:
        assert h.size == its + 1                           # BiCGStab does not count it
    # TFQMR: two entries per iteration entered; an exit after the first half step has logged one of them, and its stays
    if "tfqmr_test_reason_half1" in e.exits:
        assert h.size == 2 * its + 2
    if "tfqmr_test_reason_half2" in e.exits:
        assert h.size == 2 * its + 3
    if {"tfqmr_s_zero_first", "tfqmr_s_zero_late", "tfqmr_max_it"} & set(e.exits):
        assert h.size == 2 * its + 1
    for s in ("cgs", "bicg"):                              # a breakdown refuses the iteration it is found in
        if {s + "_s_zero_first", s + "_s_zero_late", s + "_dpi_zero_first", s + "_dpi_zero_late", s + "_beta_zero"} & set(e.exits):
            assert h.size == its + 1 and (its > 0) == any(t.endswith("_late") for t in e.exits)
    if "lsqr_atol_normal_start" in e.exits:
        assert h.size == 1 and h[0] > 0.0 and not x.any()
    if {"lsqr_happy_alpha", "lsqr_happy_beta"} & set(e.exits):
        assert its >= 1 and x.any()                        # the step that makes x exact was taken
    if "richardson_final_reason" in e.exits:
        assert its == c.tol["max_it"] and h.size == its + 1
    if {"chebychev_converged_its", "richardson_converged_its"} & set(e.exits):
        assert h.size == 0 and its == c.tol["max_it"]


def refused_at_once(solver, e):
    """the first step was refused: x is the guess"""
    if solver == "cg":
        return e.its == 0 or (e.its == 1 and e.reason in (kx.INDEF_MAT, kx.INDEF_PC))
    if kx.kind_of(solver) == "tfqmr":                      # its == 0 also after a half step of iteration 0, which has updated x
        return e.its == 0 and not any(t.startswith("tfqmr_test_reason") for t in e.exits)
    if kx.kind_of(solver) == "minres":
        return e.its == 0 or (e.its == 1 and e.reason == kx.INDEF_PC)
    if kx.kind_of(solver) == "chebychev":                  # its is 1 at the first checkpoint; the iterate there is p[k] = x + scale B r
        return False
    return e.its == 0


@pytest.mark.parametrize("name,solver,pc", COMBOS)
def test_replicated_case_ends_the_same(runs, name, solver, pc):
    c = kx.BY_NAME[name]
    e = kx.expected(c, solver, pc)
    x, h, its, reason = runs[name, solver, pc, "replicated"]
    n = kx.matrix_of(c)[0].size - 1
    assert x.size == kx.ncols_of(c, "replicated") and n * kx.copies_for(n) >= 4096 and kx.copies_for(n) & (kx.copies_for(n) - 1) == 0
    if (name, solver) in kx.ROUNDING:
        assert (its, reason) in kx.ROUNDING[name, solver]
    else:
        assert (its, reason) == (e.its, e.reason)
    if refused_at_once(solver, e) and (name, solver) not in kx.ROUNDING:
        x0 = np.zeros(kx.ncols_of(c)) if c.x0 is None else c.x0
        assert np.array_equal(kx.bits(x), kx.bits(np.tile(x0, kx.copies_for(n))))


@pytest.mark.parametrize("name,solver,pc", [t for t in COMBOS if t[1] in kx.EXIT_OF and kx.BY_NAME[t[0]].x0 is None])
def test_named_line_against_the_restatement(name, solver, pc):
    c = kx.BY_NAME[name]
    e = kx.expected(c, solver, pc)
    ai, aj, aa = kx.matrix_of(c)
    line, its, reason = kx.EXIT_OF[solver](ai, aj, aa, c.b, c.tol, pc == "jacobi")
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
    assert set(kx.LEFT_OUT) <= SEARCHED                    # only an exit a documented search did not reach may be left out
    assert not set(kx.LEFT_OUT) & claimed
    assert claimed <= set(kx.EXITS)
    for s in kx.MORE_SOLVERS:                              # every one of the eight has rows, tiny and replicated
        assert any(t[1] == s for t in COMBOS), s
