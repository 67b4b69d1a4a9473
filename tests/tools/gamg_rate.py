"""The measurement behind the README's "Algebraic multigrid" section (one MI355X; the output goes to profiles/gamg_rate.log), medians of
five interleaved rounds, on P7(127):

  (a) MatCoarsenAggregate on the device route against the host route, per level operator of the hierarchy: rows, aggregates, device
      rounds, ms per coarsening (host clock around the call: uploads, launches, the waits of the rounds, the m numbers coming back);
  (b) set-up of -pc_type gamg split into its coarsenings and the rest (the products, their symbolic passes, the level solvers);
  (c) cghipmi355x to rtol 1e-8 with gamg, with the README's geometric five-level mg example, and with Jacobi, in the same process:
      iterations, solve time, set-up time.

    python tests/tools/gamg_rate.py [--n 127] [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from petsc_dev_amd import petsc as P  # noqa: E402
from pcmg_rate import interp3d_csr  # noqa: E402


def med(v):
    return statistics.median(v)


def level_operators(A):
    """the level operators PCGAMG builds, through the same public calls (default options)"""
    ksp = P.KSP(comm=P.lib().COMM_SELF)
    ksp.set_type("preonly"); ksp.set_pc_type("gamg"); ksp.set_operators(A)
    pc = ksp.get_pc()
    pc.set_up()
    ops = [A]
    for l in range(pc.mg_get_levels() - 2, -1, -1):
        Al, Pl, flag = P.vp(), P.vp(), P.i32()
        P.lib().PCGetOperators(pc.mg_get_smoother(l).get_pc().h, P.C.byref(Al), P.C.byref(Pl), P.C.byref(flag))
        ops.append(P.Mat(Al, own=False))
    return ksp, pc, ops


def coarsen_rate(A, rounds):
    L = P.lib()
    ksp, pc, ops = level_operators(A)
    print("(a) MatCoarsenAggregate per level of the hierarchy %s, threshold 0, ms per call" % pc.gamg_level_sizes())
    worst = 0.0
    for l, M in enumerate(ops):
        times = {"device": [], "host": []}
        info = None
        for rnd in range(rounds + 1):
            for route in (("device", "host") if rnd % 2 else ("host", "device")):
                L.PetscOptionsClear()
                L.PetscOptionsInsertString(("-mat_hipmi355x_coarsen " + route).encode())
                t = time.perf_counter()
                agg, nagg = M.aggregate(0.0)
                dt = (time.perf_counter() - t) * 1e3
                if rnd:
                    times[route].append(dt)
                if route == "device":
                    info = (nagg, P.Mat.coarsen_counts_total()[2])
        L.PetscOptionsClear()
        for route in ("device", "host"):
            worst = max(worst, max(times[route]) - min(times[route]))
        print("    level %d: %8d rows -> %7d aggregates, %2d rounds; device %8.3f (rounds %s)  host %8.3f (rounds %s)" % (
            l, M.local_size()[0], info[0], info[1], med(times["device"]), " ".join("%.3f" % v for v in times["device"]),
            med(times["host"]), " ".join("%.3f" % v for v in times["host"])))
    print("    largest spread between rounds of one route on one level: %.3f ms" % worst)
    ksp.destroy(); ksp.own = False


def solve_rate(A, n, rounds):
    L = P.lib()
    sizes = [n]
    while len(sizes) < 5 and sizes[-1] > 3 and sizes[-1] % 2:
        sizes.append((sizes[-1] - 1) // 2)
    T = [None] + [P.Mat.from_csr(*interp3d_csr(nc)[:3], ncols=nc ** 3) for nc in sizes[:0:-1]]
    b = P.Vec.from_array(np.sin(np.arange(n ** 3) * 0.01) + 0.5, comm=L.COMM_SELF)
    kinds = ("gamg", "gamg_host", "mg", "jacobi")
    out = {k: [] for k in kinds}
    levels = None
    for rnd in range(rounds + 1):
        for kind in (kinds if rnd % 2 else kinds[::-1]):
            L.PetscOptionsClear()
            if kind == "mg":
                L.PetscOptionsInsertString(b"-mg_levels_ksp_type chebychevhipmi355x -mg_levels_ksp_max_it 2 -mg_levels_pc_type jacobi "
                                           b"-mg_levels_ksp_chebychev_eigenvalues 0.2,2.0")
            if kind == "gamg_host":
                L.PetscOptionsInsertString(b"-mat_hipmi355x_coarsen host")
            ksp = P.KSP(comm=L.COMM_SELF)
            ksp.set_type("cghipmi355x"); ksp.set_norm_type("unpreconditioned"); ksp.set_pc_type(kind.split("_")[0])
            ksp.set_operators(A); ksp.set_tolerances(rtol=1e-8)
            pc = ksp.get_pc()
            if kind == "mg":
                pc.mg_set_levels(len(sizes)); pc.mg_set_galerkin(True)
                for l in range(1, len(sizes)):
                    pc.mg_set_interpolation(l, T[l])
            x = b.duplicate()
            t0 = time.perf_counter()
            L.KSPSetUp(ksp.h); b.norm()
            t1 = time.perf_counter()
            ksp.solve(b, x); x.norm()
            t2 = time.perf_counter()
            r = b.duplicate()
            A.residual(b, x, r)
            if kind == "gamg":
                levels = pc.gamg_level_sizes()
            if rnd:
                out[kind].append((t1 - t0, t2 - t1, ksp.its, r.norm() / b.norm()))
            ksp.destroy(); ksp.own = False
    L.PetscOptionsClear()
    print("(b), (c) cghipmi355x on P7(%d), rtol 1e-8, unpreconditioned norm; gamg levels %s; mg levels %s" % (n, levels, [s ** 3 for s in sizes]))
    for kind in kinds:
        rows = out[kind]
        print("    %-9s iterations %3d  solve %7.1f ms (rounds %s)  set-up %7.1f ms (rounds %s)  true residual %.2e" % (
            kind, rows[0][2], med(v[1] for v in rows) * 1e3, " ".join("%.1f" % (v[1] * 1e3) for v in rows),
            med(v[0] for v in rows) * 1e3, " ".join("%.1f" % (v[0] * 1e3) for v in rows), rows[0][3]))
    print("    set-up of gamg minus the sum of (a)'s medians on its route = the products, their symbolic passes and the level solvers")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=127)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    A = P.Mat.from_csr(*P.gen_poisson7(a.n, a.n, a.n))
    coarsen_rate(A, a.rounds)
    solve_rate(A, a.n, a.rounds)
