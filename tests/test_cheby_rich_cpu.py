"""KSPCHEBYCHEV / KSPRICHARDSON without a GPU: the new names are declared and exported, the harness registers the types and refuses
bad eigenvalue bounds, and the host model the GPU tests compare against (tests/cheby_ref.py) holds against closed forms -- the
Chebyshev polynomial of the iteration matrix through an eigen-decomposition, the explicit Richardson iteration in numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cheby_ref as cr
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_new_names_are_declared_and_exported(built):
    base = os.path.join(ROOT, "petsc-dev_amd")
    kernels = exported(built.kernels_lib_path())
    for name in ("mi355x_vec_cheby_step", "mi355x_vec_rich_step"):
        assert name in kernels and re.search(r"\bint\s+%s\s*\(" % name, header("mi355x_kernels.h")), name
    harness = exported(os.path.join(base, "harness", "libpetscharness.so"))
    mini = header("petscmini.h")
    for name in ("KSPChebychevSetEigenvalues", "KSPRichardsonSetScale", "PCApplyRichardson", "PCApplyRichardsonExists"):
        assert name in harness and re.search(r"PetscErrorCode\s+%s\s*\(" % name, mini), name
    assert '#define KSPCHEBYCHEV  "chebychev"' in mini and '#define KSPRICHARDSON "richardson"' in mini
    plugin = exported(os.path.join(base, "host", "libpetschipmi355x.so"))
    for name in ("KSPCreate_ChebychevHIPMI355X", "KSPCreate_RichardsonHIPMI355X", "VecChebyStep_HIPMI355X", "VecRichStep_HIPMI355X"):
        assert name in plugin, name
    hip = header("petschipmi355x.h")
    assert '"chebychevhipmi355x"' in hip and '"richardsonhipmi355x"' in hip
    fused = header("petsckrylovfused.h")
    body = fused[fused.index("typedef struct {"):fused.index("} VecKrylovFusedOps;")]
    members = re.findall(r"\(\*(\w+)\)\(", body)
    assert members[-2:] == ["cheby_step", "rich_step"] and members[0] == "cg_update", members   # appended at the end


def test_harness_registers_both_types_and_their_setters(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    for t in ("chebychev", "richardson", "chebychevhipmi355x", "richardsonhipmi355x"):
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_type(t)
        name = C.c_char_p()
        L.KSPGetType(ksp.h, C.byref(name))
        assert name.value.decode() == t
        ksp.set_chebychev_eigenvalues(2.0, 0.1)            # a silent no-op on the Richardson types, as PetscTryMethod is
        ksp.set_richardson_scale(0.5)                      # ... and on the Chebyshev types
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_type("cg")
    ksp.set_chebychev_eigenvalues(0.1, 2.0)                # not even looked at: no type composed the method
    ksp.set_richardson_scale(-3.0)


@pytest.mark.parametrize("t", ["chebychev", "chebychevhipmi355x"])
@pytest.mark.parametrize("emax,emin", [(0.1, 2.0), (1.0, 1.0), (2.0, -0.1), (2.0, 0.0), (0.0, -2.0)])
def test_bad_eigenvalue_pairs_are_refused(built, t, emax, emin):
    from petsc_dev_amd import petsc as P
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_type(t)
    with pytest.raises(P.PetscError) as e:
        ksp.set_chebychev_eigenvalues(emax, emin)
    assert e.value.code == 75                              # PETSC_ERR_ARG_INCOMP
    ksp.set_chebychev_eigenvalues(2.0, 0.1)


def test_eigenvalue_and_scale_options(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    try:
        for t in ("chebychev", "chebychevhipmi355x"):
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(("-ksp_type %s -ksp_chebychev_eigenvalues 2.0,0.1 -ksp_richardson_scale 0.5" % t).encode())
            ksp = P.KSP(comm=L.COMM_SELF)
            with pytest.raises(P.PetscError) as e:         # <emin,emax>: 2.0 is not below 0.1
                ksp.set_from_options()
            assert e.value.code == 75
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(("-ksp_type %s -ksp_chebychev_eigenvalues 0.1,2.0" % t).encode())
            P.KSP(comm=L.COMM_SELF).set_from_options()
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(("-ksp_type %s -ksp_chebychev_eigenvalues 0.1" % t).encode())
            with pytest.raises(P.PetscError):
                P.KSP(comm=L.COMM_SELF).set_from_options()
        for t in ("richardson", "richardsonhipmi355x"):
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(("-ksp_type %s -ksp_richardson_scale 0.5" % t).encode())
            P.KSP(comm=L.COMM_SELF).set_from_options()
    finally:
        L.PetscOptionsClear()


def test_plugin_chebyshev_refuses_vectors_without_the_fused_step(built):
    """chebychevhipmi355x cannot fall back (the update needs VecScale, which the plug-in does not take from PETSc): on a solution vector
    whose fused-kernel table is gone KSPSetUp -- reached through KSPSolve before anything touches the device -- returns PETSC_ERR_SUP and
    names -ksp_type chebychev.  The stub: a HIPMI355X vector with "VecKrylovFusedOps_C" composed away."""
    from petsc_dev_amd import petsc as P
    L = P.lib()
    ai, aj, aa = P.gen_poisson7(3, 3, 3)
    A = P.Mat.from_csr(ai, aj, aa)
    x = P.Vec.create(27, comm=L.COMM_SELF)
    b = x.duplicate()
    compose = L.raw("PetscObjectComposeFunction")
    compose.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
    assert compose(x.h, b"VecKrylovFusedOps_C", b"", None) == 0
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_operators(A)
    ksp.set_type("chebychevhipmi355x")
    ksp.set_pc_type("none")
    with pytest.raises(P.PetscError) as e:
        ksp.solve(b, x)
    assert e.value.code == 56 and "-ksp_type chebychev" in str(e.value)      # PETSC_ERR_SUP


# ------------------------------------------------------------------------------------------------ the host model
def p7_jacobi():
    ai, aj, aa = orc.gen_p7(6, 5, 4)
    n = ai.size - 1
    dinv = cr.jacobi(ai, aj, aa)
    dense = np.zeros((n, n))
    for i in range(n):
        dense[i, aj[ai[i]:ai[i + 1]]] = aa[ai[i]:ai[i + 1]]
    return ai, aj, aa, dinv, dense


def cheb_t(m, x):
    """T_m(x) by the three-term recurrence (x a scalar or an array, any magnitude)"""
    t0, t1 = np.ones_like(x), x
    if m == 0:
        return t0
    for _ in range(m - 1):
        t0, t1 = t1, 2.0 * x * t1 - t0
    return t1


@pytest.mark.parametrize("max_it", [1, 2, 3, 4, 5, 6, 7, 8])
def test_chebyshev_model_is_the_chebyshev_polynomial_of_the_iteration_matrix(built, max_it):
    """P7 6 x 5 x 4 (120 rows) with Jacobi, emin / emax the extreme eigenvalues of D^-1 A.  The error after m preconditioner
    applications must be T_m(mu G) / T_m(mu) e0 with G = I - scale D^-1 A -- evaluated through the eigen-decomposition of the symmetric
    D^-1/2 A D^-1/2 -- to 1e-10 |e0|: the restated recurrence (which c, which omega, which rotation) is the textbook one."""
    ai, aj, aa, dinv, dense = p7_jacobi()
    n = dinv.size
    sq = np.sqrt(dinv)
    lam, V = np.linalg.eigh(sq[:, None] * dense * sq[None, :])
    emin, emax = lam[0], lam[-1]
    assert 0.0 < emin < emax < 2.0
    xs = np.cos(0.7 * np.arange(n)) + 0.3 * np.sin(0.11 * np.arange(n) ** 2)
    b = orc.spmv(ai, aj, aa, xs)
    x, hist, its, reason, m = cr.chebychev(ai, aj, aa, b, emin, emax, pc=dinv, norm=cr.NONE, max_it=max_it)
    assert its == max_it and reason == cr.CONVERGED_ITS and hist.size == 0 and m == max_it + 1
    scale = 2.0 / (emax + emin)
    mu = 1.0 / (1.0 - scale * emin)
    e0 = xs                                                   # zero guess
    coef = cheb_t(m, mu * (1.0 - scale * lam)) / cheb_t(m, np.float64(mu))
    predicted = (V @ (coef * (V.T @ (e0 / sq)))) * sq         # D^-1/2 V p(1 - scale L) V' D^1/2 e0
    err = xs - x
    print("max_it %d: |e| / |e0| = %.3e, |e - predicted| / |e0| = %.3e" % (max_it, np.linalg.norm(err) / np.linalg.norm(e0), np.linalg.norm(err - predicted) / np.linalg.norm(e0)))
    assert np.linalg.norm(err - predicted) <= 1e-10 * np.linalg.norm(e0)
    assert np.linalg.norm(err) < np.linalg.norm(e0)


@pytest.mark.parametrize("norm", [cr.NONE, cr.PRECONDITIONED, cr.UNPRECONDITIONED])
def test_chebyshev_model_norms_and_exits(built, norm):
    """the history holds the residual norm of every iterate the test saw, the last entry that of the returned iterate; a tolerance ends
    the solve mid-way with the iterate the norm belongs to"""
    ai, aj, aa, dinv, dense = p7_jacobi()
    b = orc.spmv(ai, aj, aa, np.ones(dinv.size))
    x, hist, its, reason, m = cr.chebychev(ai, aj, aa, b, 0.1, 2.0, pc=dinv, norm=norm, max_it=6, rtol=1e-30)
    assert its == 6 and reason == (cr.CONVERGED_ITS if norm == cr.NONE else cr.DIVERGED_ITS)
    if norm == cr.NONE:
        assert hist.size == 0
        return
    assert hist.size == 7
    r = b - dense @ x
    last = np.linalg.norm(r if norm == cr.UNPRECONDITIONED else dinv * r)
    assert abs(hist[-1] - last) <= 1e-12 * hist[0]
    x2, hist2, its2, reason2, _ = cr.chebychev(ai, aj, aa, b, 0.1, 2.0, pc=dinv, norm=norm, max_it=50, rtol=1e-3)
    assert reason2 == cr.CONVERGED_RTOL and 1 < its2 < 50 and hist2.size == its2 and hist2[-1] <= 1e-3 * hist2[0]
    r2 = b - dense @ x2
    assert abs(np.linalg.norm(r2 if norm == cr.UNPRECONDITIONED else dinv * r2) - hist2[-1]) <= 1e-12 * hist2[0]


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_richardson_model_is_the_explicit_iteration(built, pc, k):
    """after k steps: x0 + the explicit sum x <- x + scale B (b - A x) in numpy, bit for bit (every product and sum rounded on its own)"""
    ai, aj, aa, dinv, dense = p7_jacobi()
    n = dinv.size
    b = np.sin(0.3 * np.arange(n)) + 0.5
    x0 = np.cos(0.2 * np.arange(n))
    d = dinv if pc == "jacobi" else None
    scale = 0.3 if pc == "none" else 0.8
    x, hist, its, reason, m = cr.richardson(ai, aj, aa, b, scale=scale, pc=d, norm=cr.NONE, x0=x0, max_it=k)
    ref = x0.copy()
    for _ in range(k):
        r = b - orc.spmv(ai, aj, aa, ref)
        z = r * d if d is not None else r
        ref = ref + scale * z
    assert its == k and reason == cr.CONVERGED_ITS and m == k and hist.size == 0
    assert np.array_equal(bits(x), bits(ref))
    xz, _, _, _, _ = cr.richardson(ai, aj, aa, b, scale=scale, pc=d, norm=cr.PRECONDITIONED, x0=None, max_it=k, rtol=1e-30)
    ref = np.zeros(n)
    for _ in range(k):
        r = b - orc.spmv(ai, aj, aa, ref) if ref.any() else b.copy()
        z = r * d if d is not None else r
        ref = ref + scale * z
    assert np.array_equal(bits(xz), bits(ref))


def test_step_references_are_the_scalar_formulas(built):
    """cheby_ref.step_ref / rich_step_ref (the op-by-op oracle sequence the kernel tests compare with) against the formulas of
    include/mi355x_kernels.h in numpy, special cases included"""
    rng = np.random.default_rng(3)
    n = 37
    w, b, d, pm, pk, x = (rng.standard_normal(n) for _ in range(6))
    for s, a, c in ((0.37, 0.6, -1.4), (1.0, 0.0, 0.5), (0.0, 0.25, 0.0)):
        r, z, pn = cr.step_ref(s, a, c, w, b, d, pm, pk)
        rv = b - w
        zv = rv * d
        t = zv if s == 1.0 else (np.zeros(n) if s == 0.0 else s * zv)
        t = t if a == 0.0 else t + a * pm
        t = t if c == 0.0 else t + c * pk
        assert np.array_equal(bits(r), bits(rv)) and np.array_equal(bits(z), bits(zv)) and np.array_equal(bits(pn), bits(t))
    r, z, xn = cr.rich_step_ref(0.8, w, b, None, x)
    assert np.array_equal(bits(z), bits(b - w)) and np.array_equal(bits(xn), bits(x + 0.8 * (b - w)))
    assert np.array_equal(bits(cr.rich_step_ref(0.0, w, b, d, x)[2]), bits(x))
