"""What three sweeps per iteration buy the TFQMR and CGS types: ms per iteration of tfqmr, tfqmrhipmi355x, cgs and cgshipmi355x with Jacobi
on P7(n) (default n = 256) with first-order upwinded convection added (each row's west / south / down neighbour gets -c, its diagonal
+3c, c = 0.5: nonsymmetric, diagonally dominant), a fixed number of iterations per timed solve after a warm-up solve, the types
alternated three times in one process.  A timed window ends in a host wait (a norm).  Prints ms per iteration for every round and the
median of the three; the spread between the rounds is the noise to read the differences against.  The plain types are the harness's
sequences over the kernel library as it was, one kernel per call.

    python tests/tools/tfqmr_rate.py [n] [iterations]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TYPES = ["tfqmr", "tfqmrhipmi355x", "cgs", "cgshipmi355x"]
SWEEPS = {"tfqmrhipmi355x": 3, "cgshipmi355x": 3}


def with_convection(ai, aj, aa, n, c=0.5):
    """P7(n) + c x (upwind differences along x, y and z): the lower neighbours get -c, the diagonal +3c"""
    aa = aa.copy()
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    off = rows - aj
    aa[(off == 1) | (off == n) | (off == n * n)] -= c
    aa[off == 0] += 3.0 * c
    return ai, aj, aa


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*with_convection(*P.gen_poisson7(n, n, n), n))
    b = np.random.default_rng(1).standard_normal(n ** 3)
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(n ** 3), comm=L.COMM_SELF)

    def run(name):
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type %s -pc_type jacobi" % name).encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_tolerances(rtol=1e-300, abstol=1e-300, dtol=1e300, max_it=its)
        k.solve(vb, vx)                       # set-up and warm-up
        vx.norm()
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        dt = time.perf_counter() - t0
        assert k.its == its, (name, k.its, its)
        if name in SWEEPS:
            assert k.fused_step_counts() == (2 * SWEEPS[name] * its, 0), k.fused_step_counts()
        return 1e3 * dt / its

    print("P7(%d) + upwinded convection, Jacobi, preconditioned norm, %d iterations per solve" % (n, its), flush=True)
    seen = {name: [] for name in TYPES}
    for rnd in range(3):
        for name in TYPES:
            seen[name].append(run(name))
        print("round %d: " % rnd + "   ".join("%s %.4f ms/it" % (name, seen[name][-1]) for name in TYPES), flush=True)
    print("median:  " + "   ".join("%s %.4f ms/it" % (name, float(np.median(seen[name]))) for name in TYPES), flush=True)


if __name__ == "__main__":
    main()
