"""What MatSOR costs on the device (a tool, not a test):  python tests/tools/sor_rate.py [n]   (default: the P7(256) operator and a 20^3 grid)

  levels and launches per sweep of the level plan, with the fused small-level runs and without;
  the time of one PCApply of PCSOR (one symmetric sweep from a zero guess) through the C ABI, fused and level by level;
  CG + SOR against CG + Jacobi through the Mat / KSP types: iterations to the same tolerance and time per iteration."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pcapply_ms(dev, ai, aj, aa, no_fuse, reps):
    k, n = dev.k, ai.size - 1
    d_ai, d_aj, d_aa = dev.put(ai), dev.put(aj), dev.put(aa)
    vecs = [dev.put(np.cos(0.1 * np.arange(n))) for _ in range(5)]
    b, t, x, idiag, mdiag = vecs
    plan, bad = C.c_void_p(), C.c_int()
    t0 = time.perf_counter()
    dev.chk(k.mi355x_sor_plan_create(dev.h, n, ai.ctypes.data, aj.ctypes.data, 1 if no_fuse else 0, C.byref(plan), C.byref(bad)))
    t_plan = time.perf_counter() - t0
    info = [C.c_int() for _ in range(3)]
    dev.chk(k.mi355x_sor_plan_info(plan, *[C.byref(q) for q in info]))
    dev.chk(k.mi355x_sor_idiag(dev.h, plan, d_aa, 1.0, 0.0, idiag, mdiag))

    def once():
        dev.chk(k.mi355x_sor_apply(dev.h, plan, d_ai, d_aj, d_aa, idiag, mdiag, 1.0, 12 | 16, 1, b, t, x))

    once(); dev.sync()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        dev.chk(k.mi355x_event_create(C.byref(e)))
    dev.chk(k.mi355x_event_record(ev[0], dev.h))
    for _ in range(reps):
        once()
    dev.chk(k.mi355x_event_record(ev[1], dev.h))
    dev.chk(k.mi355x_event_synchronize(ev[1]))
    ms = C.c_float()
    dev.chk(k.mi355x_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
    for e in ev:
        k.mi355x_event_destroy(e)
    k.mi355x_sor_plan_destroy(plan)
    for p in [d_ai, d_aj, d_aa] + vecs:
        dev.free(p)
    return tuple(q.value for q in info), ms.value / reps, t_plan


def solve(P, A, b, pc, rtol):
    L = P.lib()
    vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(b.size), comm=L.COMM_SELF)
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type cg -pc_type %s" % pc).encode())
    k.set_tolerances(rtol=rtol, max_it=2000)
    k.set_from_options()
    L.PetscOptionsClear()
    k.solve(vb, vx)                                         # set-up and the first solve
    vx.set_array(np.zeros(b.size))
    t0 = time.perf_counter()
    k.solve(vb, vx)
    vx.array()
    dt = time.perf_counter() - t0
    return k.its, k.reason, dt


def main():
    import petsc_dev_amd as pda
    pda.load_kernels()
    from petsc_dev_amd import petsc as P
    from gpu import Dev
    import orc
    dev = Dev()
    sizes = [int(sys.argv[1])] if len(sys.argv) > 1 else [256, 20]
    for n in sizes:
        ai, aj, aa = P.gen_poisson7(n, n, n)
        reps = 5 if n > 100 else 50
        for no_fuse in (False, True):
            (nlev, launches, in_runs), ms, t_plan = pcapply_ms(dev, ai, aj, aa, no_fuse, reps)
            print("P7(%d) %-14s levels %d launches/sweep %d levels in fused runs %d  PCApply (symmetric, zero guess) %.3f ms  plan %.2f s"
                  % (n, "level by level" if no_fuse else "fused runs", nlev, launches, in_runs, ms, t_plan), flush=True)
        A = P.Mat.from_csr(ai, aj, aa)
        b = orc.spmv(ai, aj, aa, np.ones(n ** 3))
        for pc in ("jacobi", "sor"):
            its, reason, dt = solve(P, A, b, pc, 1e-8)
            print("P7(%d) CG + %-6s its %d reason %d  %.3f s  %.3f ms/iteration" % (n, pc, its, reason, dt, 1e3 * dt / max(its, 1)), flush=True)
        A.destroy()


if __name__ == "__main__":
    main()
