"""Two measurements for the README's "Multigrid" section (run on one MI355X; the output goes to profiles/pcmg_rate.log):

  (a) MatResidual on P7(256): the fused kernel against MatMult + VecAYPX, interleaved rounds, medians (ms per residual);
  (b) cghipmi355x on P7(127) to rtol 1e-8: -pc_type mg (five levels, Galerkin operators, trilinear interpolation, two Chebyshev + Jacobi
      steps down and up) against -pc_type jacobi in the same process: iterations, solve time, set-up time listed separately.

    python tests/tools/pcmg_rate.py [--n 256] [--mg-n 127] [--rounds 5] [--reps 2000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from petsc_dev_amd import petsc as P  # noqa: E402


def interp3d_csr(nc):
    """trilinear interpolation from nc^3 to (2 nc + 1)^3 unknowns: the Kronecker cube of the 1-D stencil (1/2, 1, 1/2)"""
    nf = 2 * nc + 1
    j = np.arange(nc)
    r1 = np.concatenate((2 * j, 2 * j + 1, 2 * j + 2)); c1 = np.concatenate((j, j, j))
    v1 = np.concatenate((np.full(nc, .5), np.ones(nc), np.full(nc, .5)))
    rz, ry, rx = np.meshgrid(r1, r1, r1, indexing="ij"); cz, cy, cx = np.meshgrid(c1, c1, c1, indexing="ij")
    vz, vy, vx = np.meshgrid(v1, v1, v1, indexing="ij")
    rows = ((rz * nf + ry) * nf + rx).ravel(); cols = ((cz * nc + cy) * nc + cx).ravel(); vals = (vz * vy * vx).ravel()
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    ai = np.zeros(nf ** 3 + 1, dtype=np.int32)
    ai[1:] = np.cumsum(np.bincount(rows, minlength=nf ** 3))
    return ai, cols.astype(np.int32), vals, nc ** 3


def residual_rate(n, rounds, reps):
    L = P.lib()
    A = P.Mat.from_csr(*P.gen_poisson7(n, n, n))
    x = P.Vec.from_array(np.sin(np.arange(n ** 3) * 0.01), comm=L.COMM_SELF)
    b, r = x.duplicate(), x.duplicate()
    A.mult(x, b)
    times = {"fused": [], "calls": []}
    L.MatSetOptionsPrefix(A.h, b"rate_")                                # the route of one matrix changes under its own prefix
    for rnd in range(rounds + 1):                                       # round 0 warms up
        for route in (("fused", "calls") if rnd % 2 else ("calls", "fused")):
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(("-rate_mat_hipmi355x_residual " + route).encode())
            L.MatSetFromOptions(A.h)
            A.residual(b, x, r); r.norm()
            t = time.perf_counter()
            for _ in range(reps):
                A.residual(b, x, r)
            r.norm()                                                    # one host wait ends the timed window
            if rnd:
                times[route].append((time.perf_counter() - t) / reps * 1e3)
    L.PetscOptionsClear()
    print("(a) MatResidual on P7(%d), %d residuals per round, ms per residual (one VecNorm wait per round included)" % (n, reps))
    for route in ("fused", "calls"):
        print("    %-5s rounds %s  median %.4f" % (route, " ".join("%.4f" % v for v in times[route]), statistics.median(times[route])))
    f, c = statistics.median(times["fused"]), statistics.median(times["calls"])
    spread = max(max(v) - min(v) for v in times.values())
    print("    fused / calls = %.3f; largest spread between rounds %.4f ms; counts %s" % (f / c, spread, A.residual_counts()))


def solve_rate(n, rounds):
    L = P.lib()
    A = P.Mat.from_csr(*P.gen_poisson7(n, n, n))
    sizes = [n]
    while len(sizes) < 5 and sizes[-1] > 3 and sizes[-1] % 2:
        sizes.append((sizes[-1] - 1) // 2)
    T = [None]
    for nc in sizes[:0:-1]:
        ai, aj, aa, ncols = interp3d_csr(nc)
        T.append(P.Mat.from_csr(ai, aj, aa, ncols=ncols))
    b = P.Vec.from_array(np.sin(np.arange(n ** 3) * 0.01) + 0.5, comm=L.COMM_SELF)
    print("(b) cghipmi355x on P7(%d), rtol 1e-8, unpreconditioned norm; mg: %d levels %s, Galerkin, 2 Chebyshev + Jacobi steps" % (n, len(sizes), sizes))
    out = {"mg": [], "jacobi": []}
    for rnd in range(rounds + 1):
        for pctype in (("mg", "jacobi") if rnd % 2 else ("jacobi", "mg")):
            L.PetscOptionsClear()
            L.PetscOptionsInsertString(b"-mg_levels_ksp_type chebychevhipmi355x -mg_levels_ksp_max_it 2 -mg_levels_pc_type jacobi "
                                       b"-mg_levels_ksp_chebychev_eigenvalues 0.2,2.0")
            ksp = P.KSP(comm=L.COMM_SELF)
            ksp.set_type("cghipmi355x"); ksp.set_norm_type("unpreconditioned"); ksp.set_pc_type(pctype)
            ksp.set_operators(A); ksp.set_tolerances(rtol=1e-8)
            if pctype == "mg":
                pc = ksp.get_pc()
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
            if rnd:
                out[pctype].append((t1 - t0, t2 - t1, ksp.its, r.norm() / b.norm()))
            ksp.destroy(); ksp.own = False
    L.PetscOptionsClear()
    for pctype in ("mg", "jacobi"):
        rows = out[pctype]
        print("    %-6s iterations %d  solve %.1f ms (median of %s)  set-up %.1f ms (median)  true residual %.2e" % (
            pctype, rows[0][2], statistics.median(v[1] for v in rows) * 1e3, " ".join("%.1f" % (v[1] * 1e3) for v in rows),
            statistics.median(v[0] for v in rows) * 1e3, rows[0][3]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--mg-n", type=int, default=127)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)                  # about a quarter of a second per timed window
    a = ap.parse_args()
    residual_rate(a.n, a.rounds, a.reps)
    solve_rate(a.mg_n, a.rounds)
