"""Flexible GMRES and PCKSP without a GPU: the host model (tests/fgmres_ref.py) against numpy.linalg.solve and against a dense
right-preconditioned GMRES, the model at every way out of the cycle, and what the harness and the plug-in answer without touching a
device: the registered names, the refused left side, the restart setter's order, the inner solver's options prefix, the exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bicg_ref as br
import cheby_ref as cr
import fgmres_ref as fr
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PETSC_ERR_SUP, PETSC_ERR_ORDER, PETSC_ERR_ARG_WRONG = 56, 58, 62
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def problem(built):
    ai, aj, aa = br.convdiff(33, 31)
    return ai, aj, aa, np.sin(0.3 * np.arange(ai.size - 1)) + 0.5


def csr(rows):
    rows = np.asarray(rows, dtype=np.float64)
    ai, aj, aa = [0], [], []
    for r in rows:
        for c in np.flatnonzero(r):
            aj.append(c); aa.append(r[c])
        ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64)


# ------------------------------------------------------------------------------------------------ the model solves
@pytest.mark.parametrize("restart", [5, 20, 30])
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu", "variable"])
def test_model_solves_the_convection_diffusion_problem(problem, pc, restart):
    """rtol 1e-10 on the true residual; x within 1e-10 * cond(A) * 10 of numpy.linalg.solve relative to max |x| (|dx| / |x| <=
    cond |r| / |b|, the factor 10 for the max norm against the 2-norm on 1023 entries)"""
    ai, aj, aa, b = problem
    M = br.dense(ai, aj, aa)
    d = cr.jacobi(ai, aj, aa)
    if pc == "none":
        B = None
    elif pc == "jacobi":
        B = d
    elif pc == "ilu":
        f = orc.ilu0_factor(ai, aj, aa)
        B = lambda r: orc.ilu0_solve(f, np.ascontiguousarray(r))
    else:                                                       # a different operator at every call: 1..3 Richardson steps in turn
        calls = [0]

        def B(r):
            calls[0] += 1
            return cr.richardson(ai, aj, aa, r, pc=d, norm=cr.NONE, max_it=1 + calls[0] % 3)[0]
    x, hist, its, reason = fr.fgmres(ai, aj, aa, b, pc=B, restart=restart, rtol=1e-10, max_it=500)
    xs = np.linalg.solve(M, b)
    err = float(np.max(np.abs(x - xs)) / np.max(np.abs(xs)))
    true = float(np.linalg.norm(b - M @ x))
    bound = 10.0 * 1e-10 * np.linalg.cond(M)
    print(pc, restart, "its", its, "reason", reason, "error %.3e bound %.3e true residual %.3e history %.3e" % (err, bound, true, hist[-1]))
    assert reason == fr.CONVERGED_RTOL and 0 < its < 500
    assert hist[-1] <= 1e-10 * hist[0] and err <= bound


def dense_right_gmres(M, Bm, b, k):
    """the k-th iterate of right-preconditioned GMRES from a zero guess with dense numpy: Arnoldi on M Bm with two Gram-Schmidt passes,
    the small least-squares problem by numpy.linalg.lstsq, x = Bm V y"""
    n = b.size
    V = np.zeros((n, k + 1)); H = np.zeros((k + 1, k))
    beta = np.linalg.norm(b)
    V[:, 0] = b / beta
    for j in range(k):
        w = M @ (Bm @ V[:, j])
        for _ in range(2):
            h = V[:, :j + 1].T @ w
            w = w - V[:, :j + 1] @ h
            H[:j + 1, j] += h
        H[j + 1, j] = np.linalg.norm(w)
        V[:, j + 1] = w / H[j + 1, j]
    e1 = np.zeros(k + 1); e1[0] = beta
    y = np.linalg.lstsq(H, e1, rcond=None)[0]
    return Bm @ (V[:, :k] @ y)


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_fixed_linear_pc_gives_right_preconditioned_gmres(problem, pc):
    """with one linear operator as the preconditioner flexible GMRES IS right-preconditioned GMRES: the k-th iterates agree to rounding.
    Bound: 100 * eps * cond(A B) relative to max |x| -- the least-squares problem the iterate solves has the conditioning of the
    preconditioned operator, and 100 covers the at most 25 steps of accumulated rounding in two different orthogonalisations"""
    ai, aj, aa, b = problem
    M = br.dense(ai, aj, aa)
    d = cr.jacobi(ai, aj, aa)
    Bm = np.eye(b.size) if pc == "none" else np.diag(d)
    bound = 100.0 * EPS * np.linalg.cond(M @ Bm)
    for k in (1, 5, 12, 25):
        R = fr.fgmres(ai, aj, aa, b, pc=None if pc == "none" else d, restart=30, rtol=1e-30, max_it=k)
        xr = dense_right_gmres(M, Bm, b, k)
        err = float(np.max(np.abs(R.x - xr)) / np.max(np.abs(xr)))
        print(pc, k, "difference %.3e bound %.3e" % (err, bound))
        assert R.its == k and R.reason == fr.DIVERGED_ITS and err <= bound


# ------------------------------------------------------------------------------------------------ every way out of the model
def test_model_exits(problem):
    ai, aj, aa, b = problem
    n = b.size
    d = cr.jacobi(ai, aj, aa)
    R = fr.fgmres(ai, aj, aa, np.zeros(n), pc=d)                                    # a reason at the start of the cycle
    assert (R.its, R.reason, len(R.hist), R.monitor, R.cycles) == (0, fr.CONVERGED_ATOL, 1, [], [0]) and not R.x.any()
    R = fr.fgmres(ai, aj, aa, b, pc=d, dtol=1e-3, rtol=1e-30)
    assert (R.its, R.reason, len(R.hist), R.monitor) == (0, fr.DIVERGED_DTOL, 1, [])
    nb = b.copy(); nb[7] = np.nan                                                   # a NaN norm
    R = fr.fgmres(ai, aj, aa, nb, pc=d)
    assert (R.its, R.reason, len(R.hist), R.monitor) == (0, fr.DIVERGED_NAN, 1, []) and not R.x.any()
    # happy breakdown: the right-hand side is an eigenvector of a diagonal matrix
    dg = csr(np.diag(np.arange(1.0, 9.0)))
    e = np.zeros(8); e[2] = 2.0
    R = fr.fgmres(*dg, e)
    assert (R.its, R.reason, R.cycles) == (1, fr.CONVERGED_ATOL, [1]) and R.hist == [2.0, 0.0]
    assert R.monitor == [(0, 2.0), (1, 0.0)] and np.array_equal(R.x, e / 3.0)
    with pytest.raises(fr.HappyBreakdownWithoutConvergence):                        # ... which no test notices without a norm
        fr.fgmres(*dg, e, norm=fr.NONE, max_it=5)
    # a rotation of length 0 (DIVERGED_NULL) needs H(k,k) = 0 and H(k+1,k)^2 = 0 in a step that is not "happy", i.e. with H(k+1,k) = tt > 0.
    # No input reaches it: tt is the root of a sum of squares, so tt > 0 means a sum >= the smallest subnormal s, and sqrt(s)^2 rounds
    # back to s, not to 0.  The nearest miss -- H(0,0) = 0 and a new vector whose squares underflow -- has tt == 0 and is a happy breakdown:
    R = fr.fgmres(*csr([[0.0, 0.0], [1e-200, 0.0]]), np.array([2.0, 0.0]))
    assert (R.its, R.reason, R.cycles, R.hist) == (1, fr.CONVERGED_ATOL, [1], [2.0, 0.0]) and not R.x.any()
    tiny = np.sqrt(np.float64(5e-324))
    assert tiny > 0.0 and tiny * tiny > 0.0
    # H(k-1,k-1) == 0 in the update: A e1 = 0, so the one column is zero, the step is "happy" and y = 0
    R = fr.fgmres(*csr([[0.0, 1.0], [0.0, 0.0]]), np.array([1.0, 0.0]))
    assert (R.its, R.reason, R.cycles) == (1, fr.CONVERGED_ATOL, [1]) and not R.x.any()
    # restart, max_it inside a cycle and at a cycle boundary
    R = fr.fgmres(ai, aj, aa, b, pc=d, restart=5, rtol=1e-10)
    assert R.reason == fr.CONVERGED_RTOL and len(R.cycles) > 2 and set(R.cycles[:-1]) == {5} and len(R.hist) == R.its + len(R.cycles)
    R = fr.fgmres(ai, aj, aa, b, pc=d, restart=5, rtol=1e-30, max_it=7)
    assert (R.its, R.reason, R.cycles, len(R.hist)) == (7, fr.DIVERGED_ITS, [5, 2], 9) and R.monitor[-1][0] == 7
    R = fr.fgmres(ai, aj, aa, b, pc=d, restart=5, rtol=1e-30, max_it=10)
    assert (R.its, R.reason, R.cycles, len(R.hist)) == (10, fr.DIVERGED_ITS, [5, 5], 12)
    assert [m[0] for m in R.monitor] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10] and R.modify[5][:2] == (5, 0)
    assert fr.expected_step_counts(R, 5) == (8, 2)
    R = fr.fgmres(ai, aj, aa, b, pc=d, restart=5, norm=fr.NONE, max_it=6)
    assert (R.its, R.reason) == (6, fr.CONVERGED_ITS)


def test_pcksp_model_counts_inner_iterations(problem):
    ai, aj, aa, b = problem
    d = cr.jacobi(ai, aj, aa)

    def inner(r):
        x, hist, its, reason, _ = cr.richardson(ai, aj, aa, r, pc=d, norm=cr.PRECONDITIONED, max_it=3)
        return x, its
    B = fr.PCKSP(inner)
    R = fr.fgmres(ai, aj, aa, b, pc=B, rtol=1e-8, max_it=200)
    assert R.reason == fr.CONVERGED_RTOL and B.applications == R.its and B.total == 3 * R.its


# ------------------------------------------------------------------------------------------------ the harness and the plug-in, no device
def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_new_names_are_declared_and_exported(built):
    from petsc_dev_amd import _lib
    kernels = exported(built.kernels_lib_path())
    name = "mi355x_vec_scale_rnorm_dev_pmult"
    assert name in kernels and re.search(r"\bint\s+%s\s*\(" % name, header("mi355x_kernels.h")) and name in _lib.KERNEL_API
    assert len(_lib.KERNEL_API[name]) == 6
    harness = exported(built.harness_lib_path())
    for name in ("KSPCreate_FGMRES", "PCCreate_KSP", "PCKSPGetKSP", "PCKSPGetTotalIterations", "KSPFGMRESSetModifyPC", "KSPFGMRESModifyPCNoChange",
                 "KSPGetTolerances"):
        assert name in harness, name
    for name in ("PCKSPGetKSP", "PCKSPGetTotalIterations", "KSPFGMRESSetModifyPC", "KSPFGMRESModifyPCNoChange", "KSPGetTolerances"):
        assert re.search(r"\bPetscErrorCode\s+%s\s*\(" % name, header("petscmini.h")), name
    assert re.search(r'#define\s+KSPFGMRES\s+"fgmres"', header("petscmini.h")) and re.search(r'#define\s+PCKSP\s+"ksp"', header("petscmini.h"))
    plugin = exported(built.host_lib_path())
    for name in ("KSPCreate_FGMRESHIPMI355X", "VecFgmresOrthogNormalizePC_HIPMI355X"):
        assert name in plugin, name
    assert re.search(r'#define\s+KSPFGMRESHIPMI355X\s+"fgmreshipmi355x"', header("petschipmi355x.h"))
    fused = header("petsckrylovfused.h")
    assert fused.index("} VecLsqrFusedOps;") < fused.index("} VecFgmresFusedOps;") and '"VecFgmresFusedOps_C"' in fused
    body = fused[fused.index("typedef struct {", fused.index("} VecLsqrFusedOps;")):fused.index("} VecFgmresFusedOps;")]
    assert re.findall(r"\(\*(\w+)\)\(", body) == ["fgmres_orthog_normalize_pc"]


def test_types_are_registered_and_refuse_the_left_side(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*br.convdiff(5, 4))
    for t in ("fgmres", "fgmreshipmi355x"):
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_type(t)
        assert ksp.get_type() == t and ksp.fused_step_counts() == (0, 0)
        ksp.fgmres_set_modify_pc(lambda its, k, rn: None)           # answered by both types
        ksp.fgmres_set_modify_pc(None)
        ksp.set_operators(A)
        ksp.set_pc_type("none")
        L.KSPSetPCSide(ksp.h, 0)                                    # PC_LEFT
        with pytest.raises(P.PetscError) as e:
            L.KSPSetUp(ksp.h)
        assert e.value.code == PETSC_ERR_SUP, (t, e.value)
        for norm in ("none", "preconditioned"):                     # the left side and the preconditioned norm with no norm asked for either
            k2 = P.KSP(comm=L.COMM_SELF)
            k2.set_type(t); k2.set_operators(A); k2.set_pc_type("none")
            k2.set_norm_type(norm)
            if norm == "none":
                L.KSPSetPCSide(k2.h, 0)
            with pytest.raises(P.PetscError) as e:
                L.KSPSetUp(k2.h)
            assert e.value.code == PETSC_ERR_SUP, (t, norm, e.value)
    try:
        L.PetscOptionsInsertString(b"-ksp_type fgmres -ksp_gmres_restart 7")
        k3 = P.KSP(comm=L.COMM_SELF)
        k3.set_from_options()
        assert k3.get_type() == "fgmres"
    finally:
        L.PetscOptionsClear()


def test_restart_setter_after_set_up_is_out_of_order(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*br.convdiff(5, 4))
    for t in ("fgmres", "fgmreshipmi355x"):
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_type(t); ksp.set_operators(A); ksp.set_pc_type("none")
        L.KSPGMRESSetRestart(ksp.h, 12)
        L.KSPGMRESSetCGSRefinementType(ksp.h, 2)
        L.KSPSetUp(ksp.h)
        with pytest.raises(P.PetscError) as e:
            L.KSPGMRESSetRestart(ksp.h, 5)
        assert e.value.code == PETSC_ERR_ORDER, (t, e.value)


def test_pcksp_inner_solver_prefix_and_transpose(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    try:
        L.PetscOptionsInsertString(b"-ksp_ksp_max_it 3 -ksp_ksp_type richardson -o_ksp_ksp_max_it 4 -ksp_max_it 77")
        for prefix, want in ((None, 3), (b"o_", 4)):
            ksp = P.KSP(comm=L.COMM_SELF)
            if prefix:
                L.KSPSetOptionsPrefix(ksp.h, prefix)
            ksp.set_pc_type("ksp")
            pc = ksp.get_pc()
            assert not pc.apply_transpose_exists() and pc.ksp_total_iterations() == 0
            inner = pc.ksp_get_ksp()
            assert inner.h.value == pc.ksp_get_ksp().h.value            # created once
            inner.set_from_options()
            assert inner.get_tolerances()[3] == want
            if not prefix:
                assert inner.get_type() == "richardson"
            del inner                                                   # borrowed: the PC destroys it
        other = P.KSP(comm=L.COMM_SELF)
        other.set_pc_type("jacobi")
        for call in (other.get_pc().ksp_get_ksp, other.get_pc().ksp_total_iterations):
            with pytest.raises(P.PetscError) as e:
                call()
            assert e.value.code == PETSC_ERR_ARG_WRONG
    finally:
        L.PetscOptionsClear()


# ------------------------------------------------------------------------------------------------ what plain GMRES makes of a varying PC
def variable_bcgs(ai, aj, aa):
    return lambda r: orc.ksp_solve(ai, aj, aa, np.ascontiguousarray(r), ksp="bcgs", pc="jacobi", rtol=1e-2)[0]


def test_left_gmres_model_is_the_nullspace_model_with_a_fixed_pc(problem):
    ai, aj, aa, b = problem
    d = cr.jacobi(ai, aj, aa)
    import nullspace_ref as nr
    got = fr.gmres_left(ai, aj, aa, b, lambda r: r * d, rtol=1e-8)
    want = nr.gmres(ai, aj, aa, b, 1e-8, dinv=d)
    assert got[2:] == want[2:] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_gmres_claims_a_residual_it_does_not_have_fgmres_does_not(problem):
    """the preconditioner is BiCGStab + Jacobi to rtol 1e-2: another operator at every call.  Left-preconditioned GMRES stops with
    CONVERGED_RTOL on its recurrence's estimate.  With ONE linear B the true relative residual is at most cond(B) times the claimed one
    (|r| <= |B^-1| |B r|, |B b| <= |B| |b|), and B approximates A^-1, whose condition number is cond(A): a true relative residual above
    cond(A) * rtol is more than any such operator can hide.  Flexible GMRES with the same callable has a history that IS the true
    residual, to 100 eps cond(A) |b| (the bound of tests/test_fgmres_gpu.py).
    Measured on the CPU: GMRES claims 5.2e-09 and has 4.8e-03 (cond(A) * rtol = 2.2e-06); FGMRES claims and has 1.83e-09."""
    ai, aj, aa, b = problem
    b = np.cos(0.37 * np.arange(b.size)) + 0.25
    M = br.dense(ai, aj, aa)
    cond, nb = float(np.linalg.cond(M)), float(np.linalg.norm(b))
    B = variable_bcgs(ai, aj, aa)
    x, hist, its, reason = fr.gmres_left(ai, aj, aa, b, B, rtol=1e-8, max_it=300)
    claimed, true = hist[-1] / hist[0], float(np.linalg.norm(b - M @ x)) / nb
    print("gmres its %d reason %d claimed %.3e true %.3e cond * rtol %.3e" % (its, reason, claimed, true, cond * 1e-8))
    assert reason == fr.CONVERGED_RTOL and claimed <= 1e-8 and true > cond * 1e-8
    R = fr.fgmres(ai, aj, aa, b, pc=B, rtol=1e-8, max_it=300)
    true = float(np.linalg.norm(b - M @ R.x))
    print("fgmres its %d reason %d history %.6e true %.6e" % (R.its, R.reason, R.hist[-1], true))
    assert R.reason == fr.CONVERGED_RTOL and abs(true - R.hist[-1]) <= 100.0 * EPS * cond * nb
