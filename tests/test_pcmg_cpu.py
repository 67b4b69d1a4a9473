"""PCMG without a GPU: the numpy model (tests/mg_ref.py) against multigrid theory and against dense formulas, and what the harness and
the plug-in answer without touching a device: the names, the refusals, the level solvers' options prefixes.

The figures: one damped-Jacobi step (omega = 2/3) before and after, exact coarse solve, Galerkin operators, linear interpolation, on the
1-D Laplacian.  Two grids: the error propagator I - B A has spectral radius 1/9 (local Fourier analysis gives exactly that for this
smoother).  V cycles down to 7 unknowns: 0.1896 (n = 63, 127), 0.1908 (n = 255); W cycles: 0.1167."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PETSC_ERR_SUP, PETSC_ERR_ORDER, PETSC_ERR_ARG_SIZ, PETSC_ERR_ARG_IDN, PETSC_ERR_ARG_WRONG, PETSC_ERR_ARG_OUTOFRANGE, PETSC_ERR_ARG_WRONGSTATE = 56, 58, 60, 61, 62, 63, 73


def hierarchy(n, nmin, interp=mr.interp1d, lap=mr.laplace1d):
    sizes = [n]
    while sizes[-1] > nmin:
        sizes.append((sizes[-1] - 1) // 2)
    sizes = sizes[::-1]
    Ps = [None] + [interp(s) for s in sizes[:-1]]
    return mr.galerkin(lap(n), Ps), Ps


def radius(B, A):
    return np.max(np.abs(np.linalg.eigvals(np.eye(A.shape[0]) - B @ A)))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("n", [63, 127])
def test_two_grid_contraction_is_one_ninth(n):
    As, Ps = hierarchy(n, (n - 1) // 2)
    B = mr.MG(As, Ps, mr.jacobi_smoother(As)).matrix()
    assert len(As) == 2 and abs(radius(B, As[-1]) - 1.0 / 9.0) < 1e-10
    assert np.abs(B - B.T).max() <= 1e-13 * np.abs(B).max()


@pytest.mark.parametrize("n", [63, 127, 255])
def test_v_and_w_cycles_contract_independently_of_the_mesh(n):
    As, Ps = hierarchy(n, 7)
    assert As[0].shape[0] == 7
    Bv = mr.MG(As, Ps, mr.jacobi_smoother(As), cycle="v").matrix()
    Bw = mr.MG(As, Ps, mr.jacobi_smoother(As), cycle="w").matrix()
    rv, rw = radius(Bv, As[-1]), radius(Bw, As[-1])
    print("n = %d: V %.4f W %.4f" % (n, rv, rw))
    assert 1.0 / 9.0 <= rw < 0.12 and rw < rv < 0.2
    for B in (Bv, Bw):
        assert np.abs(B - B.T).max() <= 1e-13 * np.abs(B).max()


def cg_counts(n):
    As, Ps = hierarchy(n, 3, mr.interp2d, mr.laplace2d)
    A = As[-1]
    b = np.sin(0.3 * np.arange(n * n)) + 0.5
    x, its = mr.pcg(A, b, mr.MG(As, Ps, mr.jacobi_smoother(As)).apply)
    assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
    d = np.diag(A)
    return its, mr.pcg(A, b, lambda r: r / d)[1]


def test_preconditioned_cg_count_does_not_grow_with_the_mesh():
    got = {n: cg_counts(n) for n in (15, 31, 63)}
    print(got)
    mg = [got[n][0] for n in (15, 31, 63)]
    assert max(mg) - min(mg) <= 1 and max(mg) <= 12, got                 # computed: 10, 10, 11
    assert [got[n][1] for n in (15, 31, 63)] == [47, 90, 192], got       # Jacobi: doubles with the mesh
    assert got[31][1] >= 4 * got[31][0]


def test_additive_and_full_cycles_against_their_dense_formulas():
    As, Ps = hierarchy(31, 3)
    n = len(As)
    smooth = mr.jacobi_smoother(As)
    S = [np.linalg.inv(As[0])] + [np.diag((2.0 / 3.0) / np.diag(As[l])) for l in range(1, n)]   # each level's solve from a zero guess
    up = [None] * n                                                                            # level l -> finest
    up[n - 1] = np.eye(As[-1].shape[0])
    for l in range(n - 1, 0, -1):
        up[l - 1] = up[l] @ Ps[l]
    Badd = sum(up[l] @ S[l] @ up[l].T for l in range(n))
    got = mr.MG(As, Ps, smooth, kind="additive").matrix()
    assert np.abs(got - Badd).max() <= 1e-13 * np.abs(Badd).max()
    # full: F_0 = A_0^-1, F_l = (I - B_l A_l) P_l F_{l-1} P_l^T + B_l with B_l the V cycle from level l
    F = S[0]
    for l in range(1, n):
        Bl = mr.MG(As[:l + 1], Ps[:l + 1], smooth).matrix()
        F = (np.eye(As[l].shape[0]) - Bl @ As[l]) @ Ps[l] @ F @ Ps[l].T + Bl
    got = mr.MG(As, Ps, smooth, kind="full").matrix()
    assert np.abs(got - F).max() <= 1e-12 * np.abs(F).max()
    two = mr.MG(As, Ps, smooth, cycles=2).matrix()                                             # two cycles: I - B2 A = (I - B A)^2
    B = mr.MG(As, Ps, smooth).matrix()
    E = np.eye(As[-1].shape[0]) - B @ As[-1]
    assert np.abs((np.eye(As[-1].shape[0]) - two @ As[-1]) - E @ E).max() <= 1e-12


def test_transfers():
    P = mr.interp1d(3)
    assert P.shape == (7, 3) and np.array_equal(P[:, 1], [0, 0, .5, 1, .5, 0, 0]) and np.array_equal(P.sum(axis=1), [.5, 1, 1, 1, 1, 1, .5])
    assert mr.interp2d(3).shape == (49, 9) and mr.interp3d(3).shape == (343, 27)
    Q = mr.aggregation(10, 4)
    assert Q.shape == (10, 3) and np.array_equal(Q.sum(axis=1), np.ones(10)) and np.array_equal(Q.sum(axis=0), [4, 4, 2])


# ------------------------------------------------------------------------------------------------ the harness and the plug-in, no device
def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


PCMG_API = ("PCMGSetLevels", "PCMGGetLevels", "PCMGSetType", "PCMGSetCycleType", "PCMGMultiplicativeSetCycles", "PCMGSetNumberSmoothDown",
            "PCMGSetNumberSmoothUp", "PCMGSetGalerkin", "PCMGSetInterpolation", "PCMGSetRestriction", "PCMGSetResidual", "PCMGDefaultResidual",
            "PCMGGetSmoother", "PCMGGetSmootherDown", "PCMGGetSmootherUp", "PCMGGetCoarseSolve", "MatRestrict", "MatInterpolate",
            "MatInterpolateAdd", "MatResidual")


def test_new_names_are_declared_and_exported(built):
    from petsc_dev_amd import _lib, petsc as P
    name = "mi355x_spmv_csr_residual"
    assert name in exported(built.kernels_lib_path()) and re.search(r"\bint\s+%s\s*\(" % name, header("mi355x_kernels.h"))
    assert len(_lib.KERNEL_API[name]) == 8
    harness = exported(built.harness_lib_path())
    for name in PCMG_API + ("PCCreate_MG",):
        assert name in harness, name
    for name in PCMG_API:
        assert re.search(r"\bPetscErrorCode\s+%s\s*\(" % name, header("petscmini.h")), name
        assert name in P._SIG, name
    assert re.search(r'#define\s+PCMG\s+"mg"', header("petscmini.h"))
    assert "MatHIPMI355XGetResidualCounts" in exported(built.host_lib_path())
    assert re.search(r"\bPetscErrorCode\s+MatHIPMI355XGetResidualCounts\s*\(", header("petschipmi355x.h"))
    assert "HIPMI355XGetLiveFactors" in exported(built.host_lib_path())
    assert re.search(r"\bPetscErrorCode\s+HIPMI355XGetLiveFactors\s*\(", header("petschipmi355x.h"))
    live, watched = C.c_int(-1), C.c_int(-1)
    P.lib().HIPMI355XGetLiveFactors(C.byref(live), C.byref(watched))   # asks no device: no factor was made in a process without one
    assert live.value >= watched.value >= 0
    for meth in ("mg_set_levels", "mg_get_levels", "mg_set_type", "mg_set_cycle_type", "mg_set_cycles", "mg_set_number_smooth", "mg_set_galerkin",
                 "mg_set_interpolation", "mg_set_restriction", "mg_get_smoother", "mg_get_smoother_up", "mg_get_smoother_down", "mg_get_coarse_solve"):
        assert callable(getattr(P.PC, meth)), meth
    for meth in ("residual", "restrict", "interpolate", "interpolate_add", "residual_counts"):
        assert callable(getattr(P.Mat, meth)), meth


def mg_pc(P, prefix=None, levels=None):
    L = P.lib()
    ksp = P.KSP(comm=L.COMM_SELF)
    if prefix:
        L.KSPSetOptionsPrefix(ksp.h, prefix)
    ksp.set_pc_type("mg")
    pc = ksp.get_pc()
    if levels:
        pc.mg_set_levels(levels)
    return ksp, pc


def raises(P, code, call, *a):
    with pytest.raises(P.PetscError) as e:
        call(*a)
    assert e.value.code == code, e.value


def test_refusals_that_need_no_device(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*mr.to_csr(mr.laplace1d(7)))
    Pm = P.Mat.from_csr(*mr.to_csr(mr.interp1d(3)), ncols=3)
    ksp, pc = mg_pc(P)
    assert pc.mg_get_levels() == 0
    raises(P, PETSC_ERR_ORDER, pc.mg_get_smoother, 0)                   # no levels yet
    raises(P, PETSC_ERR_ORDER, pc.mg_set_number_smooth, 2)
    ksp.set_operators(A)
    raises(P, PETSC_ERR_ARG_WRONGSTATE, pc.set_up)                      # set-up without levels
    pc.mg_set_levels(2)
    assert pc.mg_get_levels() == 2
    raises(P, PETSC_ERR_SUP, pc.mg_set_type, "kaskade")
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_set_type, 7)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_set_cycle_type, 3)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_set_cycles, 0)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_get_smoother, 2)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_get_smoother_up, 0)       # the coarse level has one solver
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_set_interpolation, 0, Pm)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.mg_set_restriction, 0, Pm)
    with pytest.raises(P.PetscError) as e:                              # neither transfer on level 1
        pc.set_up()
    assert e.value.code == PETSC_ERR_ARG_WRONGSTATE and "level 1" in str(e.value)
    pc.mg_set_restriction(1, Pm)
    with pytest.raises(P.PetscError) as e:                              # no Galerkin, no operators on level 0
        pc.set_up()
    assert e.value.code == PETSC_ERR_ARG_WRONGSTATE and "level 0" in str(e.value)
    other = P.KSP(comm=L.COMM_SELF)
    other.set_pc_type("jacobi")
    for call in (other.get_pc().mg_get_levels, other.get_pc().mg_get_coarse_solve, lambda: other.get_pc().mg_set_levels(2)):
        raises(P, PETSC_ERR_ARG_WRONG, call)
    try:
        L.PetscOptionsInsertString(b"-pc_type mg -pc_mg_levels 3 -pc_mg_type kaskade")
        k2 = P.KSP(comm=L.COMM_SELF)
        raises(P, PETSC_ERR_SUP, k2.set_from_options)
        assert k2.get_pc().mg_get_levels() == 3
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(b"-pc_type mg -pc_mg_levels 2 -pc_mg_cycle_type x")
        raises(P, 86, P.KSP(comm=L.COMM_SELF).set_from_options)
    finally:
        L.PetscOptionsClear()


def test_level_solver_prefixes_defaults_and_the_second_smoother(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    try:
        L.PetscOptionsInsertString(b"-mg_levels_2_ksp_max_it 5 -mg_coarse_ksp_max_it 7 -o_mg_levels_1_ksp_max_it 4 -mg_levels_1_ksp_type chebychev -ksp_max_it 77")
        for prefix, want in ((None, (7, 1, 5)), (b"o_", (10000, 4, 1))):
            ksp, pc = mg_pc(P, prefix, 3)
            coarse = pc.mg_get_coarse_solve()
            assert coarse.h.value == pc.mg_get_smoother(0).h.value and coarse.get_type() == "preonly"
            for l in (1, 2):
                s = pc.mg_get_smoother(l)
                assert s.get_type() == "richardson" and s.get_tolerances()[3] == 1
                assert s.h.value == pc.mg_get_smoother_down(l).h.value
            got = []
            for l in range(3):
                s = pc.mg_get_smoother(l)
                s.set_from_options()                                    # reads under the level's own prefix
                got.append(s.get_tolerances()[3])
            assert tuple(got) == want, (prefix, got)
            assert pc.mg_get_smoother(1).get_type() == ("chebychev" if not prefix else "richardson")
        # one solver per level until a second one is asked for; unequal step counts ask for it
        ksp, pc = mg_pc(P, None, 3)
        pc.mg_set_number_smooth(down=1, up=1)                           # equal to what is there: nothing happens
        down = pc.mg_get_smoother(2)
        pc.mg_set_number_smooth(down=2, up=3)
        up = pc.mg_get_smoother_up(2)
        assert up.h.value != down.h.value and pc.mg_get_smoother(2).h.value == down.h.value
        assert down.get_tolerances()[3] == 2 and up.get_tolerances()[3] == 3 and up.get_type() == "richardson"
        assert pc.mg_get_smoother_up(2).h.value == up.h.value           # created once
        up.set_from_options()                                           # the same prefix as the down smoother
        assert up.get_tolerances()[3] == 5
    finally:
        L.PetscOptionsClear()


def test_the_pc_holds_a_reference_on_its_transfer_matrices(built):
    """PCMGSetInterpolation / PCMGSetRestriction reference the matrix: the caller's MatDestroy right after the hand-over only drops the
    caller's reference, the PC's own goes with a replacement or with the PC"""
    from petsc_dev_amd import petsc as P
    L = P.lib()
    Pm = P.Mat.from_csr(*mr.to_csr(mr.interp1d(3)), ncols=3)
    Qm = P.Mat.from_csr(*mr.to_csr(mr.interp1d(3)), ncols=3)
    ksp, pc = mg_pc(P, None, 2)
    handle = C.c_void_p(Pm.h.value)
    L.PCMGSetInterpolation(pc.h, 1, Pm.h)                              # (the C call: the Python wrapper would keep Pm alive by itself)
    Pm.destroy()                                                        # the caller's reference
    assert not Pm.h
    m, n = C.c_int(), C.c_int()
    L.MatGetSize(handle, C.byref(m), C.byref(n))                        # still a matrix: the PC's reference keeps it
    assert (m.value, n.value) == (7, 3)
    L.PCMGSetInterpolation(pc.h, 1, Qm.h)                              # replaced: the PC's reference on the first one is dropped
    L.PCMGSetRestriction(pc.h, 1, Qm.h)
    Qm.destroy()
    ksp.destroy(); ksp.own = False                                      # both references on the second one go with the PC
