"""What the null-space projection costs per Krylov iteration: CG + Jacobi on the n^3 pure-Neumann 7-point Laplacian (default n = 256)
for 50 iterations, (a) without a null space, (a') the same with -ksp_cg_fused 0, (b) with the constant null space (one rank: the sync-free "VecShiftByMean_C" route),
(c) with the constant projected out by VecSum + VecShift (a null space without has_cnst whose function makes the two public calls),
alternated three times in one process.  Prints ms per iteration for each round; the spread between rounds is the noise to compare
the differences with.

    python tests/tools/nullspace_rate.py [n] [iterations]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def neumann7(n):
    """the n^3 pure-Neumann 7-point Laplacian as CSR, built with numpy (nullspace_ref.neumann7 is a Python loop)"""
    idx = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)          # [k, j, i], i fastest
    cols, rows = [], []
    for axis in range(3):
        for shift in (-1, 1):
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(1, None) if shift < 0 else slice(None, -1)
            dst[axis] = slice(None, -1) if shift < 0 else slice(1, None)
            rows.append(idx[tuple(src)].ravel()); cols.append(idx[tuple(dst)].ravel())
    r = np.concatenate(rows); c = np.concatenate(cols)
    deg = np.bincount(r, minlength=n ** 3).astype(np.float64)
    r = np.concatenate([r, np.arange(n ** 3)]); c = np.concatenate([c, np.arange(n ** 3)])
    v = np.concatenate([np.full(r.size - n ** 3, -1.0), deg])
    order = np.lexsort((c, r))
    ai = np.zeros(n ** 3 + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n ** 3), out=ai[1:])
    return ai.astype(np.int32), c[order].astype(np.int32), v[order]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*neumann7(n))
    b = np.random.default_rng(1).standard_normal(n ** 3)
    b -= b.mean()
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(n ** 3), comm=L.COMM_SELF)

    @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
    def two_calls(sp, v, ctx):
        s = C.c_double()
        L.VecSum(C.c_void_p(v), C.byref(s))
        L.VecShift(C.c_void_p(v), s.value / (-1.0 * n ** 3))
        return 0

    sync_free = P.NullSpace(True, comm=L.COMM_SELF)
    public = P.NullSpace(False, comm=L.COMM_SELF)
    L.MatNullSpaceSetFunction(public.h, C.cast(two_calls, C.c_void_p), None)
    # "without, unfused": the registered solver's own fusion switched off, as a null space switches it off (every z from KSP_PCApply).
    # The Vec type still runs the noted update sequence as one sweep there, which a VecSum between z and its dots breaks up too, so
    # the rest of the difference is the projection AND that sweep, not separated.  The two-call route goes through a Python
    # callback once per iteration (a few microseconds of its own): it is biased against that route by about that much.
    routes = [("without", None, ""), ("without, unfused", None, "-ksp_cg_fused 0"), ("with (sync-free)", sync_free, ""),
              ("with (VecSum + VecShift)", public, "")]

    def run(sp, opts):
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type cghipmi355x -pc_type jacobi " + opts).encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_tolerances(rtol=1e-30, max_it=its)
        k.set_null_space(sp)
        k.solve(vb, vx)                       # set-up and warm-up
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        dt = time.perf_counter() - t0
        return 1e3 * dt / max(k.its, 1)

    for rnd in range(3):
        print("round %d: " % rnd + "   ".join("%s %.4f ms/it" % (name, run(sp, opts)) for name, sp, opts in routes), flush=True)


if __name__ == "__main__":
    main()
