"""PCGAMG without a GPU: the host twins of the coarsening kernels against the model (tests/gamg_ref.py) as integers and bytes, the
invariants of an aggregation checked independently of the model, the model's own figures (the iteration counts DESIGN.md quotes), and
what the harness and the plug-in answer without touching a device: names, options, refusals.  Everything that applies the
preconditioner needs the device copy of a matrix (the HIPMI355X types have no CPU path) and lives in tests/test_gamg_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gamg_ref as gr
import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PETSC_ERR_SUP, PETSC_ERR_ARG_WRONG, PETSC_ERR_ARG_OUTOFRANGE = 56, 62, 63
INVALID = 1   # hipErrorInvalidValue


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_strength(K, ai, aj, aa, theta, diag=None):
    m = len(ai) - 1
    d = gr.diagonal(ai, aj, aa) if diag is None else diag
    guard = 16
    out = np.full(len(aj) + 2 * guard, 0xA5, dtype=np.uint8)
    ai32, aj32, aa64, d64 = np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(aa, np.float64), np.ascontiguousarray(d, np.float64)
    assert K.mi355x_csr_strength_host(m, ptr(ai32), ptr(aj32), ptr(aa64), ptr(d64), float(theta), C.c_void_p(out.ctypes.data + guard)) == 0
    assert np.all(out[:guard] == 0xA5) and np.all(out[len(out) - guard:] == 0xA5)
    return out[guard:len(out) - guard].copy()


def host_mis2(K, ai, aj, strong):
    m = len(ai) - 1
    guard = 8
    out = np.full(m + 2 * guard, -77, dtype=np.int32)
    n = C.c_int(-1)
    ai32, aj32, s8 = np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(strong, np.uint8)
    assert K.mi355x_coarsen_mis2_host(m, ptr(ai32), ptr(aj32), ptr(s8), C.c_void_p(out.ctypes.data + 4 * guard), C.byref(n)) == 0
    assert np.all(out[:guard] == -77) and np.all(out[len(out) - guard:] == -77)
    return out[guard:len(out) - guard].copy(), n.value


SHAPES = [("path%d" % n, gr.path(n), 0.0) for n in range(1, 71)] + [
    ("p7_5_4_3", gr.poisson7(5, 4, 3), 0.0), ("holes", gr.with_empty_rows_and_isolated_nodes(), 0.5), ("star300", gr.star(300), 0.0),
    ("upwind9", gr.upwind(9), 0.25), ("aniso12", gr.anisotropic(12), 0.1)]


@pytest.fixture(scope="module")
def K(built):
    from petsc_dev_amd import _lib
    return _lib.load_kernels()


@pytest.mark.parametrize("name,csr,theta", SHAPES, ids=[s[0] for s in SHAPES])
def test_host_twins_equal_the_model_and_keep_the_invariants(K, name, csr, theta):
    ai, aj, aa = (np.asarray(v) for v in csr)
    want = gr.strength(ai, aj, aa, theta)
    got = host_strength(K, ai, aj, aa, theta)
    assert got.tobytes() == want.tobytes()
    root, agg, nagg = gr.greedy_mis2(ai, aj, want)
    hagg, hn = host_mis2(K, ai, aj, got)
    assert hn == nagg and np.array_equal(hagg, agg)
    gr.check_invariants(ai, aj, got, root, hagg, hn)                   # geometry only: says nothing about how the set was found


def test_special_rows():
    ai, aj, aa = gr.with_empty_rows_and_isolated_nodes()
    s = gr.strength(ai, aj, aa, 0.5)
    root, agg, nagg = gr.greedy_mis2(ai, aj, s)
    for i in (2, 5, 7, 9):                                             # no row, diagonal only, empty, weak entry only: their own roots
        assert root[i] and (agg == agg[i]).sum() == 1
    ai, aj, aa = gr.star(300)
    root, agg, nagg = gr.aggregate(ai, aj, aa, 0.0)
    assert nagg == 1 and root.sum() == 1                               # everything is within 2 of whichever node wins
    ai, aj, aa = gr.upwind(9)
    s = gr.strength(ai, aj, aa, 0.25)
    sym = {(i, int(aj[t])) for i in range(81) for t in range(ai[i], ai[i + 1]) if s[t]}
    assert sym and not any((j, i) in sym for i, j in sym)             # strong in one direction only


def test_anisotropic_aggregates_lie_in_one_grid_line(K):
    n = 12
    ai, aj, aa = gr.anisotropic(n, 1e-3)
    agg, nagg = host_mis2(K, ai, aj, host_strength(K, ai, aj, aa, 0.1))
    for a in range(nagg):
        lines = {int(i) // n for i in np.nonzero(agg == a)[0]}
        assert len(lines) == 1, (a, lines)
    assert nagg >= n                                                   # at least one aggregate per line


def test_strength_specials_by_position(K):
    """NaN / Inf / zero diagonal / signed zeros: a comparison with a NaN is false, a zero diagonal makes nonzero entries strong"""
    nan, inf = float("nan"), float("inf")
    rows = {0: {0: 0.0, 1: 1e-300, 2: -0.0, 3: nan, 4: 1e-300}, 1: {0: 1.0, 1: nan, 2: 1.0}, 2: {0: inf, 2: 4.0, 3: -inf, 4: 0.0}, 3: {2: 1.0, 3: inf, 4: 5.0},
            4: {0: -3.0, 3: 1.0, 4: -0.0}}
    ai, aj, aa = gr.from_rows(5, rows)
    for theta in (0.0, 0.5, inf, nan):
        with np.errstate(all="ignore"):
            want = gr.strength(ai, aj, aa, theta)
        assert host_strength(K, ai, aj, aa, theta).tobytes() == want.tobytes(), theta
    with np.errstate(all="ignore"):
        s = gr.strength(ai, aj, aa, 0.5)
    entry = {(i, int(aj[t])): int(s[t]) for i in range(5) for t in range(ai[i], ai[i + 1])}
    assert entry[(0, 4)] == 1 and entry[(0, 2)] == 0 and entry[(0, 3)] == 0      # zero diagonal: 1e-300 > 0; -0.0 is not; NaN is not
    assert entry[(0, 1)] == 0                                                     # ... unless the column's diagonal is a NaN
    assert entry[(1, 0)] == 0 and entry[(1, 2)] == 0                              # NaN diagonal: the bound is NaN
    assert entry[(2, 0)] == 1 and entry[(2, 3)] == 0 and entry[(2, 4)] == 0      # Inf > finite bound; |-Inf| > Inf is false; 0 > 0 is false
    assert entry[(4, 0)] == 1 and entry[(4, 3)] == 0                              # a -0.0 diagonal is a zero diagonal; 0 * Inf under the root is a NaN


def test_bad_arguments_of_the_host_twins(K):
    ai = np.array([0, 1], dtype=np.int32); aj = np.array([0], dtype=np.int32); aa = np.ones(1); s = np.zeros(1, dtype=np.uint8)
    agg = np.zeros(1, dtype=np.int32); n = C.c_int(5)
    assert K.mi355x_csr_strength_host(-1, ptr(ai), ptr(aj), ptr(aa), ptr(aa), 0.0, ptr(s)) == INVALID
    assert K.mi355x_csr_strength_host(1, None, ptr(aj), ptr(aa), ptr(aa), 0.0, ptr(s)) == INVALID
    assert K.mi355x_csr_strength_host(1, ptr(ai), ptr(aj), ptr(aa), ptr(aa), 0.0, None) == INVALID
    assert K.mi355x_csr_strength_host(0, None, None, None, None, 0.0, None) == 0
    assert K.mi355x_coarsen_mis2_host(-1, ptr(ai), ptr(aj), ptr(s), ptr(agg), C.byref(n)) == INVALID and n.value == 0
    assert K.mi355x_coarsen_mis2_host(1, ptr(ai), ptr(aj), ptr(s), None, C.byref(n)) == INVALID
    assert K.mi355x_coarsen_mis2_host(1, ptr(ai), ptr(aj), ptr(s), ptr(agg), None) == INVALID
    n.value = 5
    assert K.mi355x_coarsen_mis2_host(0, None, None, None, None, C.byref(n)) == 0 and n.value == 0
    assert K.mi355x_coarsen_mis2(None, 1, ptr(ai), ptr(aj), ptr(s), ptr(agg), C.byref(n), None) == INVALID    # (no handle: nothing is launched)
    assert K.mi355x_csr_strength(None, 1, ptr(ai), ptr(aj), ptr(aa), ptr(aa), 0.0, ptr(s)) == INVALID
    assert 1 <= K.mi355x_coarsen_round_cap() <= 1 << 20


# ------------------------------------------------------------------------------------------------ the model's own figures
MODEL = {}


def model(n):
    """cg + the model's gamg and cg + Jacobi on the n x n Poisson problem: (gamg iterations, Jacobi iterations, hierarchy)"""
    if n not in MODEL:
        ai, aj, aa = gr.poisson2d(n)
        H = gr.Hierarchy(ai, aj, aa)
        A = H.As_dense[-1]
        b = np.sin(0.3 * np.arange(n * n)) + 0.5
        x, its = mr.pcg(A, b, H.cycle().apply)
        assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
        d = np.diag(A)
        MODEL[n] = (its, mr.pcg(A, b, lambda r: r / d)[1], H)
    return MODEL[n]


def test_model_counts_do_not_grow_and_beat_jacobi():
    got = {n: model(n)[:2] for n in (16, 32, 64)}
    print(got, {n: model(n)[2].sizes for n in (16, 32, 64)})
    assert [got[n] for n in (16, 32, 64)] == [(7, 48), (10, 92), (13, 182)], got   # the figures DESIGN.md quotes
    assert got[64][0] < got[64][1]


def test_model_hierarchy_shapes():
    H = model(32)[2]
    assert H.sizes[0] == 1024 and H.sizes[-1] <= 50 and all(a > b for a, b in zip(H.sizes, H.sizes[1:]))
    for l in range(1, H.n):
        P = H.Ps_dense[l]
        T = np.zeros_like(P)
        agg, nagg = H.aggs[H.n - 1 - l]
        T[np.arange(len(agg)), agg] = 1.0 / np.sqrt(np.bincount(agg)[agg])
        assert np.allclose(T.T @ T, np.eye(nagg), atol=1e-14)                                  # orthonormal columns
        A = H.As_dense[l]
        S = A / np.diag(A)[:, None]
        rho = np.abs(S).sum(axis=1).max()
        assert abs(rho - H.rho_mg[l]) <= 1e-14 * rho
        assert np.abs(P - (T - (4.0 / (3.0 * rho)) * S @ T)).max() <= 1e-14
        assert np.abs(H.As_dense[l - 1] - P.T @ A @ P).max() <= 1e-12 * np.abs(A).max()
    H1 = gr.Hierarchy(*gr.poisson2d(16), nlevels=2)                                            # the level cap
    assert H1.n == 2 and H1.sizes[0] == 256
    H2 = gr.Hierarchy(*gr.poisson2d(16), coarse_eq_limit=300)                                  # the coarse limit
    assert H2.n == 1
    H3 = gr.Hierarchy(*gr.from_rows(60, {i: {i: 1.0} for i in range(60)}))                     # stall: every node its own aggregate
    assert H3.n == 1 and H3.sizes == [60]


# ------------------------------------------------------------------------------------------------ the harness and the plug-in, no device
def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()}


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


GAMG_API = ("PCGAMGSetThreshold", "PCGAMGSetCoarseEqLimit", "PCGAMGSetNlevels", "PCGAMGSetNSmooths", "PCGAMGSetReuseInterpolation",
            "PCGAMGGetLevelSizes", "MatCoarsenAggregate")
KERNELS = {"mi355x_csr_strength": 8, "mi355x_csr_strength_host": 7, "mi355x_coarsen_mis2": 8, "mi355x_coarsen_mis2_host": 6, "mi355x_coarsen_round_cap": 0}


def test_new_names_are_declared_and_exported(built):
    from petsc_dev_amd import _lib, petsc as P
    kernels = exported(built.kernels_lib_path())
    for name, nargs in KERNELS.items():
        assert name in kernels and re.search(r"\bint\s+%s\s*\(" % name, header("mi355x_kernels.h")), name
        assert len(_lib.KERNEL_API[name]) == nargs, name
    harness = exported(built.harness_lib_path())
    for name in GAMG_API + ("PCCreate_GAMG",):
        assert name in harness, name
    for name in GAMG_API:
        assert re.search(r"\bPetscErrorCode\s+%s\s*\(" % name, header("petscmini.h")), name
        assert name in P._SIG, name
    assert re.search(r'#define\s+PCGAMG\s+"gamg"', header("petscmini.h"))
    assert "MatHIPMI355XGetCoarsenCounts" in exported(built.host_lib_path()) and "MatHIPMI355XGetCoarsenCounts" in P._SIG
    assert re.search(r"\bPetscErrorCode\s+MatHIPMI355XGetCoarsenCounts\s*\(", header("petschipmi355x.h"))
    for meth in ("gamg_set_threshold", "gamg_set_coarse_eq_limit", "gamg_set_nlevels", "gamg_set_nsmooths", "gamg_set_reuse_interpolation", "gamg_level_sizes"):
        assert callable(getattr(P.PC, meth)), meth
    for meth in ("aggregate", "coarsen_counts"):
        assert callable(getattr(P.Mat, meth)), meth
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for opt in ("-pc_gamg_threshold", "-pc_gamg_coarse_eq_limit", "-pc_gamg_agg_nsmooths", "-pc_gamg_reuse_interpolation", "-mat_hipmi355x_coarsen"):
        assert opt in design, opt


def raises(P, code, call, *a):
    with pytest.raises(P.PetscError) as e:
        call(*a)
    assert e.value.code == code, e.value


def test_host_route_through_the_matrix_and_its_counters(built):
    """MatCoarsenAggregate with -mat_hipmi355x_coarsen host works on the host copy alone"""
    from petsc_dev_amd import petsc as P
    L = P.lib()
    try:
        L.PetscOptionsInsertString(b"-mat_hipmi355x_coarsen host")
        for csr, theta in ((gr.poisson7(5, 4, 3), 0.0), (gr.upwind(9), 0.25), (gr.anisotropic(12), 0.1)):
            A = P.Mat.from_csr(*csr)
            before = P.Mat.coarsen_counts_total()
            agg, nagg = A.aggregate(theta)
            _, want, wn = gr.aggregate(*csr, theta)
            assert nagg == wn and np.array_equal(agg, want)
            assert A.coarsen_counts() == (0, 1, 0)
            after = P.Mat.coarsen_counts_total()
            assert (after[0] - before[0], after[1] - before[1]) == (0, 1)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(b"-mat_hipmi355x_coarsen sideways")
        raises(P, PETSC_ERR_ARG_WRONG, P.Mat.from_csr(*gr.path(5)).aggregate, 0.0)
    finally:
        L.PetscOptionsClear()


def test_refusals_that_need_no_device(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_pc_type("gamg")
    pc = ksp.get_pc()
    assert pc.gamg_level_sizes() == [] and pc.mg_get_levels() == 0
    for bad in (2, -1):
        raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.gamg_set_nsmooths, bad)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.gamg_set_threshold, -0.5)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.gamg_set_coarse_eq_limit, 0)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, pc.gamg_set_nlevels, 0)
    pc.mg_set_cycle_type("w"); pc.mg_set_cycles(2)                       # it is a PCMG
    other = P.KSP(comm=L.COMM_SELF)
    other.set_pc_type("mg")
    raises(P, PETSC_ERR_ARG_WRONG, other.get_pc().gamg_set_threshold, 0.1)
    raises(P, PETSC_ERR_ARG_WRONG, other.get_pc().gamg_level_sizes)
    ai, aj, aa = gr.path(6)
    raises(P, PETSC_ERR_ARG_OUTOFRANGE, P.Mat.from_csr(ai, aj, aa).aggregate, -1.0)
    B = P.Mat.from_bsr(2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.arange(8, dtype=np.float64) + 1.0)
    raises(P, PETSC_ERR_SUP, B.aggregate, 0.0)                          # the block type
    try:
        L.PetscOptionsInsertString(b"-pc_type gamg -pc_gamg_agg_nsmooths 3")
        raises(P, PETSC_ERR_ARG_OUTOFRANGE, P.KSP(comm=L.COMM_SELF).set_from_options)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(b"-pc_type gamg -pc_gamg_threshold 0.05 -pc_gamg_coarse_eq_limit 20 -pc_mg_levels 4 -pc_gamg_agg_nsmooths 0 -pc_gamg_reuse_interpolation 1 -pc_mg_cycle_type w")
        k2 = P.KSP(comm=L.COMM_SELF)
        k2.set_from_options()
        assert k2.get_pc().mg_get_levels() == 0                         # -pc_mg_levels is the cap here, not a PCMGSetLevels
    finally:
        L.PetscOptionsClear()
