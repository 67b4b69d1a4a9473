"""MINRES without a GPU: the new names are declared, exported and registered, the third fused-kernel table follows the second in the
header, and the host model the GPU tests compare against (tests/minres_ref.py: the two sweeps op by op through the oracle, iterated
with a host product) is the reference's sequence -- bit for bit a straight numpy transcription of it -- and solves the symmetric
indefinite problem it is for: P7(5,4,3) - 3.1 I, 60 rows, 6 negative eigenvalues."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cheby_ref as cr
import minres_ref as mr
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def shifted_p7(nx, ny, nz, sigma):
    """P7(nx, ny, nz) - sigma I in CSR"""
    ai, aj, aa = orc.gen_p7(nx, ny, nz)
    aa = aa.copy()
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    aa[rows == aj] -= sigma
    return ai, aj, aa


def dense(ai, aj, aa):
    n = ai.size - 1
    M = np.zeros((n, n))
    M[np.repeat(np.arange(n), np.diff(ai)), aj] = aa
    return M


def test_new_names_are_declared_and_exported(built):
    base = os.path.join(ROOT, "petsc-dev_amd")
    kernels = exported(built.kernels_lib_path())
    from petsc_dev_amd import _lib
    for name in ("mi355x_vec_minres_lanczos", "mi355x_vec_minres_update"):
        assert name in kernels and re.search(r"\bint\s+%s\s*\(" % name, header("mi355x_kernels.h")), name
        assert name in _lib.KERNEL_API, name
    plugin = exported(os.path.join(base, "host", "libpetschipmi355x.so"))
    for name in ("KSPCreate_MINRESHIPMI355X", "VecMinresLanczos_HIPMI355X", "VecMinresUpdate_HIPMI355X", "KSPHIPMI355XGetFusedStepCounts"):
        assert name in plugin, name
    assert "KSPCreate_MINRES" in exported(built.harness_lib_path())
    assert re.search(r'#define\s+KSPMINRESHIPMI355X\s+"minreshipmi355x"', header("petschipmi355x.h"))
    assert re.search(r'#define\s+KSPMINRES\s+"minres"', header("petscmini.h"))


def test_the_third_table_follows_the_second(built):
    fused = header("petsckrylovfused.h")
    assert 0 < fused.index("} VecKrylovFusedOps;") < fused.index("} VecPipelinedCGFusedOps;") < fused.index("} VecMinresFusedOps;")
    body = fused[fused.index("typedef struct {", fused.index("} VecPipelinedCGFusedOps;")):fused.index("} VecMinresFusedOps;")]
    assert re.findall(r"\(\*(\w+)\)\(", body) == ["minres_lanczos", "minres_update"]
    assert '"VecMinresFusedOps_C"' in fused


def test_both_types_are_registered(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    name = C.c_char_p()
    for t in ("minres", "minreshipmi355x"):
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_type(t)
        L.KSPGetType(ksp.h, C.byref(name))
        assert name.value.decode() == t
        assert ksp.fused_step_counts() == (0, 0)
    try:
        L.PetscOptionsInsertString(b"-ksp_type minreshipmi355x")
        k2 = P.KSP(comm=L.COMM_SELF)
        k2.set_from_options()
        L.KSPGetType(k2.h, C.byref(name))
        assert name.value.decode() == "minreshipmi355x"
    finally:
        L.PetscOptionsClear()


# ------------------------------------------------------------------------------------------------ the host model
def transcription(ai, aj, aa, b, d, max_it, rtol):
    """KSPSolve_MINRES of PETSc 3.3 written down line by line in numpy: nine vectors, the copies as copies; VecAXPY leaves y alone
    for alpha == 0; the two reductions through the oracle so that both sides add in the same order.  Zero guess, KSPDefaultConverged."""
    def axpy(y, a, x):
        return y if a == 0.0 else y + a * x

    n = b.size
    X = np.zeros(n)
    hist = []
    UOLD, VOLD, W, WOLD = (np.zeros(n) for _ in range(4))
    c = cold = 1.0
    s = sold = 0.0
    R = b.copy()
    Z = R * d if d is not None else R.copy()
    nrm = float(orc.vec_norm(Z, 1))
    dp = float(orc.vec_dot(R, Z))
    if dp < 1e-18:
        return X, np.array(hist), 0, -10
    beta = math.sqrt(abs(dp))
    eta = beta
    V = R * (1.0 / beta)
    U = Z * (1.0 / beta)
    rnorm = nrm
    hist.append(nrm)
    ttol = max(rtol * nrm, 1e-50)
    if nrm <= ttol:
        return X, np.array(hist), 0, 3 if nrm < 1e-50 else 2
    reason, its = 0, 0
    i = 0
    while i < max_it:
        its = i + 1
        R = orc.spmv(ai, aj, aa, U)
        alpha = float(orc.vec_dot(U, R))
        Z = R * d if d is not None else R.copy()
        R = axpy(R, -alpha, V); Z = axpy(Z, -alpha, U); R = axpy(R, -beta, VOLD); Z = axpy(Z, -beta, UOLD)
        betaold = beta
        dp = float(orc.vec_dot(R, Z))
        if dp < 1e-18:
            reason = -8
            break
        beta = math.sqrt(abs(dp))
        coold, cold, soold, sold = cold, c, sold, s
        rho0 = cold * alpha - coold * sold * betaold
        rho1 = math.sqrt(rho0 * rho0 + beta * beta)
        rho2 = sold * alpha + coold * cold * betaold
        rho3 = soold * betaold
        c = rho0 / rho1
        s = beta / rho1
        WOOLD = WOLD.copy(); WOLD = W.copy(); W = U.copy()
        W = axpy(W, -rho2, WOLD); W = axpy(W, -rho3, WOOLD); W = W * (1.0 / rho1)
        X = axpy(X, c * eta, W)
        eta = -s * eta
        VOLD = V.copy(); UOLD = U.copy(); V = R * (1.0 / beta); U = Z * (1.0 / beta)
        rnorm = rnorm * abs(s)
        hist.append(rnorm)
        if rnorm <= ttol:
            reason = 3 if rnorm < 1e-50 else 2
            break
        if rnorm >= 1e4 * nrm:
            reason = -4
            break
        i += 1
    if i >= max_it:
        reason = -3
    return X, np.array(hist), its, reason


PROBLEMS = {"shifted": lambda: shifted_p7(5, 4, 3, 3.1), "spd": lambda: orc.gen_p7(6, 5, 4)}


@pytest.fixture(scope="module")
def shifted(built):
    ai, aj, aa = shifted_p7(5, 4, 3, 3.1)
    b = np.sin(0.3 * np.arange(ai.size - 1)) + 0.5
    return ai, aj, aa, b


@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("max_it", [1, 2, 200])
@pytest.mark.parametrize("prob", list(PROBLEMS))
def test_model_iterated_is_the_sequence_transcribed(built, prob, pc, max_it):
    ai, aj, aa = PROBLEMS[prob]()
    b = np.sin(0.3 * np.arange(ai.size - 1)) + 0.5
    d = cr.jacobi(ai, aj, aa) if pc == "jacobi" else None
    x, hist, its, reason = mr.minres(ai, aj, aa, b, pc=d, max_it=max_it, rtol=1e-8)
    xt, histt, itst, reasont = transcription(ai, aj, aa, b, d, max_it, 1e-8)
    print(prob, pc, max_it, "its", its, itst, "reason", reason, reasont)
    assert (its, reason) == (itst, reasont)
    assert np.array_equal(bits(hist), bits(histt))
    assert np.array_equal(bits(x), bits(xt))


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_model_solves_the_indefinite_problem(shifted, pc):
    """rtol 1e-8 within 60 iterations, a non-increasing history, a final estimate within 1e-5 of the true preconditioned residual norm,
    x within 1e-6 of numpy.linalg.solve.  (A numpy run of the sequence gave 42 / 43 iterations, 1e-6 and 2e-8.)"""
    ai, aj, aa, b = shifted
    M = dense(ai, aj, aa)
    ev = np.linalg.eigvalsh(M)
    assert np.sum(ev < 0) == 6 and np.sum(ev > 0) == 54, "the problem is not the indefinite one it is meant to be"
    d = cr.jacobi(ai, aj, aa) if pc == "jacobi" else None
    x, hist, its, reason = mr.minres(ai, aj, aa, b, pc=d, max_it=60, rtol=1e-8)
    true = np.linalg.norm((b - M @ x) * (d if d is not None else 1.0))
    err = np.max(np.abs(x - np.linalg.solve(M, b)))
    print(pc, "its", its, "reason", reason, "estimate", hist[-1], "true", true, "rel", abs(hist[-1] - true) / true, "max |x - solve|", err)
    assert reason == cr.CONVERGED_RTOL and its <= 60 and hist.size == its + 1
    assert hist[-1] <= 1e-8 * hist[0]
    assert np.all(np.diff(hist) <= 0.0), "the residual history of MINRES is monotone"
    assert abs(hist[-1] - true) <= 1e-5 * true
    assert err <= 1e-6


def test_exits(shifted):
    ai, aj, aa, b = shifted
    n = b.size
    x, hist, its, reason = mr.minres(ai, aj, aa, np.zeros(n), pc=cr.jacobi(ai, aj, aa))
    assert (its, reason, hist.size) == (0, mr.DIVERGED_INDEFINITE_MAT, 0) and not x.any()    # r'z = 0 < 1e-18 before the first checkpoint
    d = cr.jacobi(ai, aj, aa)
    d[7] = -d[7]
    x, hist, its, reason = mr.minres(ai, aj, aa, b, pc=d, max_it=60, rtol=1e-8)
    print("negative diagonal entry: its", its, "reason", reason)
    assert reason == mr.DIVERGED_INDEFINITE_PC and its >= 1
    for max_it in (1, 2):
        x, hist, its, reason = mr.minres(ai, aj, aa, b, pc=cr.jacobi(ai, aj, aa), max_it=max_it, rtol=1e-8)
        assert (its, reason, hist.size) == (max_it, mr.DIVERGED_ITS, max_it + 1)
