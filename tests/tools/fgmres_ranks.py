"""Rank script of tests/test_fgmres_ranks_gpu.py (started by torch.distributed.run): fgmreshipmi355x + Jacobi on the 41 x 25
convection-diffusion operator (1025 rows) as an MPIAIJ matrix with the rows split over the ranks, -ksp_fgmres_fused 1 against the default (off), restarts
5 and 20, zero and nonzero guess, a budget of 3 steps and a tolerance.  On every rank: the same iteration count, reason and history, the
local part of x bit for bit (the rule tests/tools/lsqr_ranks.py holds its two types to), and x of all ranks within 1e-8 of
numpy.linalg.solve (that script's bound against numpy).  With MI355X_STAGED=1 the ranks share one GPU over the host-staged transport:
the Vec type refuses both fused Gram-Schmidt entries there and every step runs through the public calls, (0, its) steps counted either
way.  Without it (one GPU per rank, RCCL) the sums of "fgmres_orthog_normalize_pc" are all-reduced on the device and the steps that
have a next direction to write are counted as fused."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fused_steps(its, restart):
    """steps of `its` iterations in full cycles of `restart` that have a next direction to write and at most 32 basis vectors"""
    return sum(1 for j in range(its) if (j % restart) + 1 < restart and (j % restart) + 1 <= 32)


def main():
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from petsc_dev_amd import petsc as P
    from petsc_dev_amd import dist as PD
    import bicg_ref as br
    L = P.lib()
    staged = os.environ.get("MI355X_STAGED", "0") == "1"
    comm = PD.torch_comm(device_comm=not staged)
    gi, gj, ga = br.convdiff(41, 25)
    N = gi.size - 1
    rows = [N * k // world for k in range(world + 1)]
    rs, re_ = rows[rank], rows[rank + 1]
    ai = (gi[rs:re_ + 1] - gi[rs]).astype(np.int32)
    A = P.Mat.from_csr_mpi(ai, gj[gi[rs]:gi[re_]].copy(), ga[gi[rs]:gi[re_]].copy(), re_ - rs, N, N, comm=comm)
    bg = np.cos(0.37 * np.arange(N)) + 0.25
    xg = 0.1 * np.sin(0.61 * np.arange(N)) - 0.05

    def solve(opts, restart, nonzero, max_it, rtol):
        vb = P.Vec.from_array(bg[rs:re_], comm=comm, N=N)
        vx = P.Vec.from_array(xg[rs:re_] if nonzero else np.zeros(re_ - rs), comm=comm, N=N)
        k = P.KSP(comm=comm)
        k.set_operators(A)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type fgmreshipmi355x -pc_type jacobi -ksp_gmres_restart %d %s" % (restart, opts)).encode())
        k.set_tolerances(rtol=rtol, max_it=max_it)
        k.set_from_options()
        L.PetscOptionsClear()
        if nonzero:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
        return vx.array().copy(), k.history(), k.its, k.reason, k.fused_step_counts()

    def u64(a):
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

    failed, cases, its_seen = [], 0, []
    for restart in (5, 20):
        for nonzero in (False, True):
            for max_it, rtol in ((3, 1e-30), (400, 1e-10)):
                xo, ho, io, ro, co = solve("", restart, nonzero, max_it, rtol)
                xf, hf, if_, rf, cf = solve("-ksp_fgmres_fused 1", restart, nonzero, max_it, rtol)
                cases += 1
                its_seen.append(if_)
                nf = 0 if staged else fused_steps(if_, restart)
                ok = (io, ro) == (if_, rf) and ho.size == hf.size and np.array_equal(u64(ho), u64(hf)) and np.array_equal(u64(xo), u64(xf)) \
                    and np.all(np.isfinite(xf)) and co == (0, io) and cf == (nf, if_ - nf)
                if max_it == 400:
                    ok = ok and rf == 2 and restart < if_ < 400           # KSP_CONVERGED_RTOL after more than one cycle
                else:
                    ok = ok and (if_, rf) == (3, -3)
                if not ok:
                    failed.append((restart, nonzero, max_it, io, if_, ro, rf, co, cf))
    xf = solve("-ksp_fgmres_fused 1", 20, False, 400, 1e-10)[0]
    parts = [None] * world
    dist.all_gather_object(parts, xf)
    xs = np.linalg.solve(br.dense(gi, gj, ga), bg)
    err = float(np.linalg.norm(np.concatenate(parts) - xs) / np.linalg.norm(xs))
    if err > 1e-8:
        failed.append(("solve", err))
    print("rank %d/%d: FGMRES fused equals unfused=%s transport=%s cases %d its %s err %.2e %s"
          % (rank, world, not failed, "staged" if staged else "rccl", cases, ",".join(str(i) for i in its_seen), err, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
