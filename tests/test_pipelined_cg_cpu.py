"""The fused pipelined CG type without a GPU: the new names are declared, exported and registered, the second fused-kernel table
follows the first in the header, and the host model the GPU tests compare against (tests/pipecg_ref.py: the sweep op by op through the
oracle, iterated with a host product) reproduces the oracle's KSPSolve_PIPECG bit for bit under every norm type."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import pipecg_ref as pr

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
    assert "mi355x_vec_pipecg_step" in kernels and re.search(r"\bint\s+mi355x_vec_pipecg_step\s*\(", header("mi355x_kernels.h"))
    from petsc_dev_amd import _lib
    assert "mi355x_vec_pipecg_step" in open(_lib.__file__).read()
    plugin = exported(os.path.join(base, "host", "libpetschipmi355x.so"))
    for name in ("KSPCreate_PIPECGHIPMI355X", "VecPipeCGStep_HIPMI355X", "KSPHIPMI355XGetFusedStepCounts"):
        assert name in plugin, name
    hip = header("petschipmi355x.h")
    assert '#define KSPPIPECGHIPMI355X  "pipecghipmi355x"' in hip
    assert re.search(r"PetscErrorCode\s+KSPHIPMI355XGetFusedStepCounts\s*\(", hip)


def test_the_second_table_follows_the_first(built):
    fused = header("petsckrylovfused.h")
    assert 0 < fused.index("} VecKrylovFusedOps;") < fused.index("} VecPipelinedCGFusedOps;")
    body = fused[fused.index("typedef struct {", fused.index("} VecKrylovFusedOps;")):fused.index("} VecPipelinedCGFusedOps;")]
    assert re.findall(r"\(\*(\w+)\)\(", body) == ["pipecg_step"]
    assert '"VecPipelinedCGFusedOps_C"' in fused


def test_the_type_is_registered_and_counts_nothing_before_a_solve(built):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_type("pipecghipmi355x")
    name = C.c_char_p()
    L.KSPGetType(ksp.h, C.byref(name))
    assert name.value.decode() == "pipecghipmi355x"
    assert ksp.fused_step_counts() == (0, 0)
    ksp.set_type("cg")                                    # a type that does not answer: zeros, no error
    assert ksp.fused_step_counts() == (0, 0)
    try:
        L.PetscOptionsInsertString(b"-ksp_type pipecghipmi355x -ksp_pipecg_fused false")
        k2 = P.KSP(comm=L.COMM_SELF)
        k2.set_from_options()
        L.KSPGetType(k2.h, C.byref(name))
        assert name.value.decode() == "pipecghipmi355x"
    finally:
        L.PetscOptionsClear()


# ------------------------------------------------------------------------------------------------ the host model
@pytest.fixture(scope="module")
def p7(built):
    ai, aj, aa = orc.gen_p7(5, 4, 3)
    n = ai.size - 1
    b = np.sin(0.3 * np.arange(n)) + 0.5
    return ai, aj, aa, b


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("norm", [pr.PRECONDITIONED, pr.UNPRECONDITIONED, pr.NATURAL, pr.NONE])
@pytest.mark.parametrize("max_it", [1, 2, 25])
def test_model_iterated_is_the_oracles_pipecg(p7, norm, pc, max_it):
    """x, history, iteration count and reason of orc.ksp_solve(ksp="pipecg"), bit for bit; max_it 1 and 2 end on the sweep that queues
    no sums, 25 runs into a tolerance (natural, none) or through the non-converging branch of the other two norms"""
    import cheby_ref as cr
    ai, aj, aa, b = p7
    d = cr.jacobi(ai, aj, aa) if pc == "jacobi" else None
    x, hist, its, reason = pr.pipecg(ai, aj, aa, b, pc=d, norm=norm, max_it=max_it, rtol=1e-8)
    xo, histo, itso, reasono = orc.ksp_solve(ai, aj, aa, b, ksp="pipecg", pc=pc, norm_type=pr.NORM_NUMBER[norm], max_it=max_it, rtol=1e-8)
    print(norm, pc, max_it, "its", its, itso, "reason", reason, reasono, "history", hist.size, histo.size)
    assert its == itso and reason == reasono
    assert np.array_equal(bits(hist), bits(histo))
    assert np.array_equal(bits(x), bits(xo))


def test_step_reference_is_the_scalar_formulas(built):
    """pipecg_ref.step_ref against the formulas of include/mi355x_kernels.h in numpy, special cases included"""
    rng = np.random.default_rng(5)
    n = 37
    nv, mv, d, zrec, qrec, p, s, x, u, w, r = (rng.standard_normal(n) for _ in range(11))
    for first, ratio, step in ((False, 0.37, 0.8), (False, 1.0, 0.8), (False, -1.0, -0.3), (False, 0.0, 0.8), (True, 0.37, 0.8), (False, 0.37, 0.0)):
        z2, q2, p2, s2, x2, u2, w2, r2, m2 = pr.step_ref(first, ratio, step, nv, mv, d, zrec, qrec, p, s, x, u, w, r)
        def rec(a, old):
            if first or ratio == 0.0:
                return a
            return a - old if ratio == -1.0 else a + ratio * old
        ez, eq, ep, es = rec(nv, zrec), rec(mv, qrec), rec(u, p), rec(w, s)
        ex, eu, ew, er = (x, u, w, r) if step == 0.0 else (x + step * ep, u + (-step) * eq, w + (-step) * ez, r + (-step) * es)
        for got, want in ((z2, ez), (q2, eq), (p2, ep), (s2, es), (x2, ex), (u2, eu), (w2, ew), (r2, er), (m2, ew * d)):
            assert np.array_equal(bits(got), bits(want)), (first, ratio, step)
    assert pr.step_ref(True, 0.0, 0.5, nv, mv, None, zrec, qrec, p, s, x, u, w, r, with_m=False)[8] is None
