"""Rank script of tests/test_lsqr_ranks_gpu.py (started by torch.distributed.run, the ranks sharing one GPU over the host-staged
transport): LSQR on the 60 x 37 operator of tests/test_lsqr_cpu.py as an MPIAIJ matrix with rows AND columns split over the ranks, PCNONE
and Jacobi on a block-diagonal stand-in for A^T A, zero and nonzero guess, with standard errors.  The plug-in's lsqrhipmi355x against the
harness's lsqr on every rank: the local part of x and of the standard-error sum bit for bit, the same history, iteration count, reason,
arnorm and anorm.  There the Vec type refuses the slot routes, both sums of the bidiagonalisation are all-reduced on the host and beta
comes home before step 6: two waits per iteration, two bidiagonalisation sweeps and one update sweep."""
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
    from test_lsqr_cpu import csr, operator
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    Ad = operator()
    M, N = Ad.shape
    rows = [M * k // world for k in range(world + 1)]
    cols = [N * k // world for k in range(world + 1)]
    rs, re_, cs, ce = rows[rank], rows[rank + 1], cols[rank], cols[rank + 1]
    ai, aj, aa = csr(Ad[rs:re_])
    A = P.Mat.from_csr_mpi(ai, aj, aa, ce - cs, M, N, comm=comm)
    # the preconditioner's matrix: n x n with the column split on both sides; the diagonal of A^T A is all PCJACOBI takes from it
    dn = np.einsum("ij,ij->j", Ad, Ad)
    pi_ = np.arange(ce - cs + 1, dtype=np.int32)
    Pm = P.Mat.from_csr_mpi(pi_, np.arange(cs, ce, dtype=np.int32), dn[cs:ce].copy(), ce - cs, N, N, comm=comm)
    bg = np.random.default_rng(5).standard_normal(M)
    xg = 0.1 * np.sin(0.61 * np.arange(N)) - 0.05

    def solve(ksp_type, pc, nonzero, max_it, rtol):
        vb = P.Vec.from_array(bg[rs:re_], comm=comm, N=M)
        vx = P.Vec.from_array(xg[cs:ce] if nonzero else np.zeros(ce - cs), comm=comm, N=N)
        k = P.KSP(comm=comm)
        k.set_operators(A, Pm if pc != "none" else None)
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(("-ksp_type %s -pc_type %s -ksp_lsqr_set_standard_error" % (ksp_type, pc)).encode())
        k.set_tolerances(rtol=rtol, max_it=max_it)
        k.set_from_options()
        L.PetscOptionsClear()
        k.set_convergence_test("KSPLSQRDefaultConverged")
        if nonzero:
            k.set_initial_guess_nonzero(True)
        k.record_history()
        k.solve(vb, vx)
        return vx.array().copy(), k.history(), k.its, k.reason, k.fused_step_counts(), k.lsqr_get_arnorm(), k.lsqr_get_standard_error_vec().array().copy()

    def u64(a):
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

    failed, cases, its_seen = [], 0, []
    for pc in ("none", "jacobi"):
        for nonzero in (False, True):
            for max_it, rtol in ((1, 1e-30), (3, 1e-30), (200, 1e-10)):
                xh, hh, ih, rh, _, nh, sh = solve("lsqr", pc, nonzero, max_it, rtol)
                xp, hp, ip, rp, counts, np_, sp = solve("lsqrhipmi355x", pc, nonzero, max_it, rtol)
                cases += 1
                its_seen.append(ip)
                ok = (ih, rh) == (ip, rp) and hh.size == hp.size and np.array_equal(u64(hh), u64(hp)) and np.array_equal(u64(xh), u64(xp)) \
                    and np.array_equal(u64(sh), u64(sp)) and np.array_equal(u64(nh), u64(np_)) and np.all(np.isfinite(xp)) \
                    and counts == ((2 * ip, ip) if pc == "none" else (ip, ip))
                if max_it == 200:
                    ok = ok and rp == 1 and 3 < ip < 200          # KSP_CONVERGED_RTOL_NORMAL ended it mid-way
                if not ok:
                    failed.append((pc, nonzero, max_it, ih, ip, rh, rp, counts))
    # the solution on all ranks against numpy's
    xp = solve("lsqrhipmi355x", "none", False, 200, 1e-10)[0]
    parts = [None] * world
    dist.all_gather_object(parts, xp)
    xs = np.linalg.lstsq(Ad, bg, rcond=None)[0]
    err = float(np.linalg.norm(np.concatenate(parts) - xs) / np.linalg.norm(xs))
    if err > 1e-8:
        failed.append(("lstsq", err))
    print("rank %d/%d: LSQR plug-in type equals the harness type=%s cases %d its %s err %.2e %s"
          % (rank, world, not failed, cases, ",".join(str(i) for i in its_seen), err, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
