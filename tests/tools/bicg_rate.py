"""What two sweeps per iteration buy the BiCG type, and what a transposed application of an ILU(0) factor costs: on P7(n) (default n = 256)
with first-order upwinded convection added (tests/tools/tfqmr_rate.py's operator) and Jacobi, ms per iteration of bicghipmi355x fused
against -ksp_bicg_fused 0, a fixed number of iterations per timed solve after a warm-up solve, the legs alternated three times in one
process; then, with ILU(0) under -pc_factor_hipmi355x_trisolve level, ms per MatSolveTranspose against ms per MatSolve on the same
factor, alternated three times.  A timed window ends in a host wait (a norm).  Prints every round and the median of the three; the spread
between the rounds is the noise to read the differences against.

    python tests/tools/bicg_rate.py [n] [iterations] [applications]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]
LEGS = [("fused", ""), ("option off", "-ksp_bicg_fused 0")]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    napp = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    from tfqmr_rate import with_convection
    L = P.lib()
    A = P.Mat.from_csr(*with_convection(*P.gen_poisson7(n, n, n), n))
    b = np.random.default_rng(1).standard_normal(n ** 3)
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(n ** 3), comm=L.COMM_SELF)

    def run(opts):
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type bicghipmi355x -pc_type jacobi %s" % opts).encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_tolerances(rtol=1e-300, abstol=1e-300, dtol=1e300, max_it=its)
        k.solve(vb, vx)                       # set-up and warm-up
        vx.norm()
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        dt = time.perf_counter() - t0
        assert k.its == its, (opts, k.its, its)
        assert k.fused_step_counts() == ((0, 2 * its) if opts else (4 * its, 0)), k.fused_step_counts()
        return 1e3 * dt / its

    print("P7(%d) + upwinded convection, Jacobi, preconditioned norm, %d iterations per solve" % (n, its), flush=True)
    seen = {name: [] for name, _ in LEGS}
    for rnd in range(3):
        for name, opts in LEGS:
            seen[name].append(run(opts))
        print("round %d: " % rnd + "   ".join("bicghipmi355x %s %.4f ms/it" % (name, seen[name][-1]) for name, _ in LEGS), flush=True)
    print("median:  " + "   ".join("bicghipmi355x %s %.4f ms/it" % (name, float(np.median(seen[name]))) for name, _ in LEGS), flush=True)

    # one transposed application against one forward application of the same ILU(0) factor, level mode
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    pc = C.c_void_p()
    L.KSPGetPC(k.h, C.byref(pc))
    L.PCSetType(pc, b"ilu")
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(b"-pc_factor_hipmi355x_trisolve level")
    t0 = time.perf_counter()
    assert L.raw("PCSetUp")(pc) == 0
    L.PetscOptionsClear()
    nl, nu = C.c_int(), C.c_int()
    L.PCILUGetLevels_HIPMI355X(pc, C.byref(nl), C.byref(nu))
    print("ILU(0), level mode: set-up %.2f s, %d + %d levels forward" % (time.perf_counter() - t0, nl.value, nu.value), flush=True)
    F = C.c_void_p()
    L.PCFactorGetMatrix(pc, C.byref(F))

    def apply(fn):
        fn(F, vb.h, vx.h)                     # warm-up (the first transposed application builds the form and captures the graph)
        vx.norm()
        t0 = time.perf_counter()
        for _ in range(napp):
            fn(F, vb.h, vx.h)
        vx.norm()
        return 1e3 * (time.perf_counter() - t0) / napp

    t0 = time.perf_counter()
    L.MatSolveTranspose(F, vb.h, vx.h)
    vx.norm()
    print("first MatSolveTranspose (pattern build, value gather, graph capture): %.2f s" % (time.perf_counter() - t0), flush=True)
    res = {"MatSolve": [], "MatSolveTranspose": []}
    for rnd in range(3):
        res["MatSolve"].append(apply(L.MatSolve))
        res["MatSolveTranspose"].append(apply(L.MatSolveTranspose))
        print("round %d: MatSolve %.3f ms   MatSolveTranspose %.3f ms" % (rnd, res["MatSolve"][-1], res["MatSolveTranspose"][-1]), flush=True)
    print("median:  MatSolve %.3f ms   MatSolveTranspose %.3f ms" % (float(np.median(res["MatSolve"])), float(np.median(res["MatSolveTranspose"]))), flush=True)


if __name__ == "__main__":
    main()
