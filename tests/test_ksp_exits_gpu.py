"""Every way out of the registered Krylov types (cghipmi355x at -ksp_cg_fused 0..4, gmreshipmi355x and bcgshipmi355x at
-ksp_*_fused 0/1) against the plain harness types over the same device Vec / Mat types, on the table of tests/kspexits.py, tiny
(the one-lane tail) and replicated block-diagonally to >= 8192 rows (several workgroups).

Per case, solver, preconditioner, size and level:
  * error or reason: both return, or both raise the same PETSc error code (the plain type decides which);
  * where both return: x, the residual history, its and reason carry the plain type's bits (NaN compared as bits, tests/specials.py);
    the oracle replayed in the device's reduction order agrees where it returns the same kind of exit;
  * after an error or a refused step (INDEFINITE_MAT / _PC, BREAKDOWN, NULL, DIVERGED_NAN) x is the plain type's, bit for bit;
  * a second solve on the same KSP (a benign system of the same size) carries the bits of a fresh KSP.
Shapes: n = 2, 3, 8, 12 and 4^k copies of them.  Cost is launches, not bytes: about 0.1 - 2 s per test."""
import numpy as np
import pytest

import kspexits as kx
import vecspecials as vs
from gpu import PRODUCT_KSP

pytestmark = pytest.mark.gpu

LEVELS = {"cg": ["-ksp_cg_fused %d" % k for k in range(5)] + [""], "gmres": ["-ksp_gmres_fused 0", "-ksp_gmres_fused 1", ""],
          "bcgs": ["-ksp_bcgs_fused 0", "-ksp_bcgs_fused 1", ""]}
PAIRS = [(c.name, s) for c in kx.CASES for s in kx.solvers_of(c)]


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


class Run:
    """one KSP on one system; solve() returns ("ok", x, hist, its, reason) or ("error", code, x)"""

    def __init__(self, P, c, ksp_type, pc, opts, system):
        self.P, L = P, P.lib()
        ai, aj, aa, b, x0 = system
        self.n = b.size
        self.A = P.Mat.from_csr(ai, aj, aa, comm=L.COMM_SELF)
        self.k = P.KSP(comm=L.COMM_SELF)
        self.k.set_operators(self.A)
        text = "-ksp_type %s -pc_type %s -ksp_gmres_restart %d %s %s" % (ksp_type, pc, c.restart, "-ksp_pc_side right" if c.pc_right else "", opts)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(text.encode())
        self.k.set_tolerances(**c.tol)
        self.k.set_from_options()
        L.PetscOptionsClear()
        self.k.record_history()

    def solve(self, b, x0=None):
        P, L = self.P, self.P.lib()
        vb = P.Vec.from_array(b, comm=L.COMM_SELF)
        vx = P.Vec.from_array(np.zeros(b.size) if x0 is None else x0, comm=L.COMM_SELF)
        L.KSPSetInitialGuessNonzero(self.k.h, 0 if x0 is None else 1)
        try:
            self.k.solve(vb, vx)
        except P.PetscError as e:
            return ("error", e.code, vx.array())
        return ("ok", vx.array(), self.k.history(), self.k.its, self.k.reason)

    def second(self, Ab, b):
        """the same KSP on another matrix of the same size with the default tolerances"""
        self.A2 = self.P.Mat.from_csr(*Ab, comm=self.P.lib().COMM_SELF)
        self.k.set_operators(self.A2)
        self.k.set_tolerances(rtol=1e-5, abstol=1e-50, dtol=1e4, max_it=60)
        return self.solve(b)


def same(a, b):
    """tests/vecspecials.py's rule: any NaN equals any NaN (sign and payload of a NaN are not part of the contract), every other
    value bit for bit"""
    return a.shape == b.shape and not vs.differing(a, b).any()


def close_level4(a, b, h0, its, n):
    """-ksp_cg_fused 4 (the default) takes p'w from the SpMV pass, another summation tree (DESIGN, kspfused.c: "agrees with the other
    levels to rounding, not bit for bit"): where iterations were completed its history and x are compared to rounding -- a dot over
    n terms differs by at most n eps relative between two trees, the step length with it, over `its` iterations, times 8 for the
    growth through the recurrences of these well-conditioned systems -- and to 1e-9 relative, the bound of
    test_ksp_cg_fused_forms_are_bit_identical.  Non-finite entries by class."""
    if a.shape != b.shape:
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]):
        return False
    tol = 1e-9 * np.abs(b[fin]) + 8.0 * max(its, 1) * n * 2.220446049250313e-16 * h0
    return bool(np.all(np.abs(a[fin] - b[fin]) <= tol))


def describe(r):
    return r[:2] if r[0] == "error" else ("ok", r[3], r[4], r[2][-3:])


@pytest.fixture(scope="module")
def systems():
    memo = {}

    def get(name, size):
        if (name, size) not in memo:
            memo[name, size] = kx.system(kx.BY_NAME[name], size)
        return memo[name, size]
    return get


@pytest.mark.parametrize("name,solver", PAIRS)
def test_registered_type_leaves_like_the_plain_type(P, systems, name, solver):
    c = kx.BY_NAME[name]
    for pc in kx.pcs_of(c):
        e = kx.expected(c, solver, pc)
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            b, x0 = sysm[3], sysm[4]
            where = "%s %s %s %s" % (name, solver, pc, size)
            plain = Run(P, c, solver, pc, "", sysm).solve(b, x0)
            # the table: an error where it names one, with the code it names; a reason otherwise
            if e.error is not None:
                assert plain[0] == "error" and plain[1] == e.error, (where, describe(plain))
            else:
                assert plain[0] == "ok", (where, describe(plain))
                xo, ho, itso, ro = kx.oracle(c, solver, pc, size, device_order=True)
                if (name, solver) in kx.ROUNDING:
                    assert (plain[3], plain[4]) in kx.ROUNDING[name, solver], (where, describe(plain))
                else:
                    assert (plain[3], plain[4]) == (itso, ro) == (e.its, e.reason), (where, describe(plain), itso, ro)
                    keep = -1 if "bcgs_tt_zero_s_zero" in e.exits else None      # the oracle logs 0.0 there, the reference the old norm
                    assert np.array_equal(plain[2][:keep], ho[:keep], equal_nan=True), (where, plain[2], ho)     # NaN by position: the host's NaN has its own payload
                    assert np.array_equal(plain[1], xo, equal_nan=True), (where, plain[1][:8], xo[:8])
            for opts in LEVELS[solver]:
                got = Run(P, c, PRODUCT_KSP[solver], pc, opts, sysm).solve(b, x0)
                at = where + " [" + (opts or "default") + "]"
                assert got[0] == plain[0], (at, describe(got), describe(plain))
                if plain[0] == "error":
                    assert got[1] == plain[1], (at, describe(got), describe(plain))
                    if solver == "cg" and opts in ("-ksp_cg_fused 4", "") and e.its > 1 and not same(got[2], plain[2]):
                        # level 4 completed iterations in its own summation tree before the refused one: the iterate to rounding
                        fin = plain[2][np.isfinite(plain[2])]
                        assert close_level4(got[2], plain[2], float(np.max(np.abs(fin), initial=0.0)), e.its, b.size), (at, got[2][:8], plain[2][:8])
                        continue
                    assert same(got[2], plain[2]), (at, got[2][:8], plain[2][:8])        # x after the refused step
                    continue
                assert (got[3], got[4]) == (plain[3], plain[4]), (at, describe(got), describe(plain))
                stepped = solver == "cg" and opts in ("-ksp_cg_fused 4", "") and len(plain[2]) > 1       # level 4 and an update was made
                if stepped and not same(got[2], plain[2]):
                    xscale = float(np.max(np.abs(plain[1][np.isfinite(plain[1])]), initial=0.0))
                    assert close_level4(got[2], plain[2], plain[2][0], plain[3], b.size), (at, got[2], plain[2])
                    assert close_level4(got[1], plain[1], xscale, plain[3], b.size), (at, got[1][:8], plain[1][:8])
                    continue
                assert same(got[2], plain[2]), (at, got[2], plain[2])                     # history
                assert same(got[1], plain[1]), (at, got[1][:8], plain[1][:8])             # x: after a refused step as after any other


@pytest.mark.parametrize("name,solver", PAIRS)
def test_second_solve_on_the_same_ksp_carries_the_bits_of_a_fresh_one(P, systems, name, solver):
    c = kx.BY_NAME[name]
    for pc in kx.pcs_of(c):
        for size in ("tiny", "replicated"):
            sysm = systems(name, size)
            n = sysm[3].size
            nb = kx.matrix_of(c)[0].size - 1
            rows = kx.tridiag(nb, 1.0, 4.0, 1.0)
            benign = kx.Case("b", rows, np.arange(1.0, nb + 1), None, kx.DEFAULT_TOL, c.restart, c.pc_right, c.pcs, {}, False)
            Ab = kx.system(benign, size)
            assert Ab[3].size == n
            used = Run(P, c, PRODUCT_KSP[solver], pc, "", sysm)
            used.solve(sysm[3], sysm[4])
            again = used.second(Ab[:3], Ab[3])
            fresh = Run(P, c, PRODUCT_KSP[solver], pc, "", sysm).second(Ab[:3], Ab[3])
            where = "%s %s %s %s" % (name, solver, pc, size)
            assert again[0] == fresh[0] == "ok", (where, describe(again), describe(fresh))
            assert again[4] == fresh[4] and fresh[4] in (kx.RTOL, kx.ATOL) and again[3] == fresh[3] > 0, (where, describe(again), describe(fresh))
            assert same(again[2], fresh[2]) and same(again[1], fresh[1]), (where, again[2], fresh[2])
