"""What the fused step buys per iteration of the two smoother-type solvers: Chebyshev + Jacobi and Richardson + Jacobi on P7(n)
(default n = 256) under KSP_NORM_NONE, 200 iterations per timed solve after a warm-up solve, for
  (a) the harness type (chebychev / richardson) with the Vec type's deferral at its default,
  (b) the harness type with the deferral off (VecHIPMI355XSetDeferral(0): one kernel per Vec call),
  (c) the plug-in's type (chebychevhipmi355x / richardsonhipmi355x: the product and ONE sweep per iteration),
alternated three times in one process.  A timed window ends in a host wait (a norm).  Prints ms per iteration for every round; the
spread between the rounds is the noise to read the differences against.

    python tests/tools/cheby_rate.py [n] [iterations]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*P.gen_poisson7(n, n, n))
    b = np.random.default_rng(1).standard_normal(n ** 3)
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(n ** 3), comm=L.COMM_SELF)
    routes = {"chebychev": ("-ksp_chebychev_eigenvalues 0.1,2.0", [("chebychev", -1), ("chebychev, deferral off", 0), ("chebychevhipmi355x", -1)]),
              "richardson": ("-ksp_richardson_scale 0.8", [("richardson", -1), ("richardson, deferral off", 0), ("richardsonhipmi355x", -1)])}

    def run(name, defer, extra):
        L.VecHIPMI355XSetDeferral(defer)
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type %s -pc_type jacobi -ksp_norm_type none %s" % (name.split(",")[0], extra)).encode())
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_tolerances(max_it=its)
        k.solve(vb, vx)                       # set-up and warm-up
        vx.norm()
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        dt = time.perf_counter() - t0
        assert k.its == its, (k.its, its)
        L.VecHIPMI355XSetDeferral(-1)
        return 1e3 * dt / its

    print("P7(%d), Jacobi, KSP_NORM_NONE, %d iterations per solve" % (n, its), flush=True)
    for kind, (extra, types) in routes.items():
        for rnd in range(3):
            print("%s round %d: " % (kind, rnd) + "   ".join("%s %.4f ms/it" % (name, run(name, defer, extra)) for name, defer in types), flush=True)


if __name__ == "__main__":
    main()
