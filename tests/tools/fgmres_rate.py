"""Step rate of flexible GMRES on one MI355X: P7(n) (default n = 256), Jacobi, restart 30, 300 iterations, three legs interleaved in one
process and repeated five times --
    fused     -ksp_type fgmreshipmi355x -ksp_fgmres_fused 1   the normalising sweep writes the next preconditioned direction
    unfused   -ksp_type fgmreshipmi355x -ksp_fgmres_fused 0   KSP_PCApply + the plain one-wait Gram-Schmidt step
    gmres     -ksp_type gmreshipmi355x -ksp_pc_side right     right-preconditioned GMRES, which unwinds the PC once per cycle
-- ms per iteration per round and the median, and the host waits per iteration.  The waits are not timed but counted from the call
sequence: every step ends in one wait for the published Gram-Schmidt sums, and every restart cycle adds the wait of the VecNormalize of
its start residual: (its + cycles) / its.  Then one line for the README's PCKSP example: outer fgmreshipmi355x with 4 Chebyshev + Jacobi
steps inside against gmreshipmi355x + Jacobi, iterations and seconds to rtol 1e-8 on the same matrix.

    python tests/tools/fgmres_rate.py [n] [iterations]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LEGS = [("fused", "-ksp_type fgmreshipmi355x -ksp_fgmres_fused 1"), ("unfused", "-ksp_type fgmreshipmi355x -ksp_fgmres_fused 0"),
        ("gmres", "-ksp_type gmreshipmi355x -ksp_pc_side right")]
CHEBY = ("-ksp_type fgmreshipmi355x -pc_type ksp -ksp_ksp_type chebychevhipmi355x -ksp_ksp_max_it 4 -ksp_ksp_norm_type none -ksp_pc_type jacobi "
         "-ksp_ksp_chebychev_eigenvalues 0.2,2.0")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    its = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    import petsc_dev_amd as pda  # noqa: F401
    from petsc_dev_amd import petsc as P
    L = P.lib()
    A = P.Mat.from_csr(*P.gen_poisson7(n, n, n))
    b = np.random.default_rng(1).standard_normal(n ** 3)
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(n ** 3), comm=L.COMM_SELF)

    def make(opts):
        k = P.KSP(comm=L.COMM_SELF)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(opts.encode())
        k.set_from_options()                  # the options stay in the database: the inner solver of a PCKSP reads its own at set-up
        return k

    def timed(k):
        t0 = time.perf_counter()
        k.solve(vb, vx)
        vx.norm()                             # a host wait: the queue is empty
        return time.perf_counter() - t0

    print("P7(%d) = %d rows, Jacobi, restart 30, %d iterations per solve" % (n, n ** 3, its), flush=True)
    ms = {name: [] for name, _ in LEGS}
    for rnd in range(5):
        for name, opts in LEGS:
            k = make(opts + " -pc_type jacobi -ksp_gmres_restart 30")
            k.set_tolerances(rtol=1e-30, max_it=its)
            timed(k)                          # set-up and warm-up
            dt = timed(k)
            ms[name].append(1e3 * dt / max(k.its, 1))
            counts = k.fused_step_counts()
            k.destroy()
        print("round %d: " % rnd + "   ".join("%s %.4f ms/it" % (name, ms[name][-1]) for name, _ in LEGS), flush=True)
    cycles = (its + 29) // 30
    for name, _ in LEGS:
        print("%-8s median %.4f ms/it   host waits per iteration %.3f (%d steps + %d cycle starts, counted from the call sequence)"
              % (name, float(np.median(ms[name])), (its + cycles) / its, its, cycles), flush=True)
    print("fused / unfused = %.4f   (last gmres leg counted %r fused steps: it has no such counter)"
          % (float(np.median(ms["fused"])) / float(np.median(ms["unfused"])), counts), flush=True)
    for name, opts in (("fgmreshipmi355x + PCKSP(4 Chebyshev + Jacobi steps)", CHEBY), ("gmreshipmi355x + Jacobi", "-ksp_type gmreshipmi355x -pc_type jacobi")):
        k = make(opts + " -ksp_gmres_restart 30")
        k.set_tolerances(rtol=1e-8, max_it=20000)
        k.record_history()
        dt = timed(k)
        inner = k.get_pc().ksp_total_iterations() if "pc_type ksp" in opts else 0
        print("to rtol 1e-8: %s: %d outer iterations (%d inner), reason %d, %.3f s including set-up" % (name, k.its, inner, k.reason, dt), flush=True)
        k.destroy()


if __name__ == "__main__":
    main()
