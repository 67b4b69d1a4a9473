"""What five launches and one wait per iteration buy the LSQR type: ms per iteration of lsqr and lsqrhipmi355x with PCNONE on a tall operator,
P7(n) stacked on a diagonal block (2 n^3 rows, n^3 columns; default n = 256), 200 iterations per timed solve after a warm-up solve, the
types alternated three times in one process.  A timed window ends in a host wait (a norm).  Prints ms per iteration for every round, the
median of the three and the ratio of the medians; the spread between the rounds is the noise to read the ratio against.  Both types run
the same two products per iteration (one over the cached transpose), which may dominate: the ratio is reported whatever it is.

    python tests/tools/lsqr_rate.py [n] [iterations]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
TYPES = ["lsqr", "lsqrhipmi355x"]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    L = P.lib()
    ai, aj, aa = P.gen_poisson7(n, n, n)
    N = n ** 3
    ai2 = np.concatenate([ai, ai[-1] + np.arange(1, N + 1, dtype=np.int64)]).astype(np.int32)     # rows N .. 2N - 1: one diagonal entry each
    aj2 = np.concatenate([aj, np.arange(N, dtype=np.int32)])
    aa2 = np.concatenate([aa, 0.5 + 0.25 * np.cos(np.arange(N))])
    A = P.Mat.from_csr(ai2, aj2, aa2, ncols=N)
    b = np.random.default_rng(1).standard_normal(2 * N)
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(N), comm=L.COMM_SELF)

    def run(name):
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type %s -pc_type none" % name).encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_tolerances(rtol=1e-30, max_it=its)
        k.solve(vb, vx)                       # set-up (the transpose is built here) and warm-up
        vx.norm()
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        dt = time.perf_counter() - t0
        assert k.its == its, (name, k.its, its)
        if name == "lsqrhipmi355x":
            assert k.fused_step_counts() == (4 * its, 2 * its), k.fused_step_counts()      # two solves
        return 1e3 * dt / its

    print("P7(%d) stacked on a diagonal block: %d x %d, PCNONE, %d iterations per solve" % (n, 2 * N, N, its), flush=True)
    seen = {name: [] for name in TYPES}
    for rnd in range(3):
        for name in TYPES:
            seen[name].append(run(name))
        print("round %d: " % rnd + "   ".join("%s %.4f ms/it" % (name, seen[name][-1]) for name in TYPES), flush=True)
    med = {name: float(np.median(seen[name])) for name in TYPES}
    print("median:  " + "   ".join("%s %.4f ms/it" % (name, med[name]) for name in TYPES), flush=True)
    print("ratio lsqr / lsqrhipmi355x: %.3f" % (med["lsqr"] / med["lsqrhipmi355x"]), flush=True)


if __name__ == "__main__":
    main()
