"""Rank script of tests/test_minres_ranks_gpu.py (started by torch.distributed.run, the ranks sharing one GPU over the host-staged
transport): MINRES with Jacobi on an MPIAIJ P7(6,5,4) slab matrix, zero and nonzero guess.  The plug-in's minreshipmi355x against the
harness's minres on every rank: the local part of x bit for bit, the same history, iteration count and reason (there tdot_begin
refuses, alpha comes from VecDot, and r'z of the Lanczos sweep is all-reduced on the host)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from petsc_dev_amd import petsc as P
    from petsc_dev_amd import dist as PD
    import orc
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    nx, ny, nzl = 6, 5, 4 // world
    mloc, N = nx * ny * nzl, nx * ny * nzl * world
    ai, aj, aa = orc.gen_p7(nx, ny, nzl * world)
    rs, re_ = rank * mloc, (rank + 1) * mloc
    A = P.Mat.from_csr_mpi((ai[rs:re_ + 1] - ai[rs]).astype(np.int32), aj[ai[rs]:ai[re_]].copy(), aa[ai[rs]:ai[re_]].copy(), mloc, N, N, comm=comm)
    bg, xg = np.cos(0.37 * np.arange(N)) + 0.25, 0.1 * np.sin(0.61 * np.arange(N)) - 0.05

    def solve(ksp_type, nonzero, max_it, rtol):
        vb = P.Vec.from_array(bg[rs:re_], comm=comm, N=N)
        vx = P.Vec.from_array(xg[rs:re_] if nonzero else np.zeros(mloc), comm=comm, N=N)
        k = P.KSP(comm=comm)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type %s -pc_type jacobi" % ksp_type).encode())
        k.set_tolerances(rtol=rtol, max_it=max_it)
        k.set_from_options()
        L.PetscOptionsClear()
        if nonzero:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
        return vx.array().copy(), k.history(), k.its, k.reason, k.fused_step_counts()

    failed, cases, its_seen = [], 0, []
    for nonzero in (False, True):
        for max_it, rtol in ((1, 1e-30), (3, 1e-30), (200, 1e-8)):
            xh, hh, ih, rh, _ = solve("minres", nonzero, max_it, rtol)
            xp, hp, ip, rp, counts = solve("minreshipmi355x", nonzero, max_it, rtol)
            cases += 1
            its_seen.append(ip)
            ok = (ih, rh) == (ip, rp) and hh.size == hp.size and np.array_equal(hh.view(np.uint64), hp.view(np.uint64)) \
                and np.array_equal(xh.view(np.uint64), xp.view(np.uint64)) and np.all(np.isfinite(xp)) and counts == (ip, 0)
            if max_it == 200:
                ok = ok and rp == 2 and 2 < ip < 200          # the tolerance ended it mid-way
            if not ok:
                failed.append((nonzero, max_it, ih, ip, rh, rp, counts))
    print("rank %d/%d: MINRES plug-in type equals the harness type=%s cases %d its %s %s"
          % (rank, world, not failed, cases, ",".join(str(i) for i in its_seen), failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
