"""Rank script of tests/test_sor_ranks_gpu.py (started by torch.distributed.run, the ranks sharing one GPU over the host-staged transport):
MatSOR of an MPIAIJ matrix -- a P7 slab matrix with perturbed values -- with the local sweeps, from a zero guess and not, its and lits in
{1, 2}: x on every rank against the Python restatement of MatSOR_MPIAIJ (tests/sor_ref.py) over the orc.mpiaij_split blocks, bit for bit.
A non-local sweep answers PETSC_ERR_SUP on every rank; CG + sor converges with one iteration count."""
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
    import sor_ref as sr
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    nx, ny, nzl = 7, 6, 8
    mloc, N = nx * ny * nzl, nx * ny * nzl * world
    ai, aj, aa = orc.gen_p7(nx, ny, nzl * world)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    bg, xg = np.cos(0.37 * np.arange(N)) + 0.25, np.sin(0.61 * np.arange(N)) - 0.1
    parts = [orc.mpiaij_split(r * mloc, (r + 1) * mloc, r * mloc, (r + 1) * mloc, ai, aj, aa) for r in range(world)]
    split = lambda v: [v[r * mloc:(r + 1) * mloc].copy() for r in range(world)]
    rs, re_ = rank * mloc, (rank + 1) * mloc
    A = P.Mat.from_csr_mpi((ai[rs:re_ + 1] - ai[rs]).astype(np.int32), aj[ai[rs]:ai[re_]].copy(), aa[ai[rs]:ai[re_]].copy(), mloc, N, N, comm=comm)
    vb = P.Vec.from_array(bg[rs:re_], comm=comm, N=N)
    failed, cases = [], 0
    for name in ("local_symmetric", "local_forward", "local_backward"):
        for zero in (True, False):
            for its in (1, 2):
                for lits in (1, 2):
                    for omega, fshift in ((1.0, 0.0), (1.3, 0.25)):
                        flag = sr.SWEEPS[name] | (sr.ZERO_INITIAL_GUESS if zero else 0)
                        vx = P.Vec.from_array(xg[rs:re_], comm=comm, N=N)
                        A.sor(vb, vx, omega=omega, flag=flag, shift=fshift, its=its, lits=lits)
                        ref = sr.sor_mpi_ref(parts, split(bg), split(xg), omega, flag, fshift, its, lits)[rank]
                        cases += 1
                        if not np.array_equal(vx.array().view(np.uint64), ref.view(np.uint64)):
                            failed.append((name, zero, its, lits, omega, fshift))
    sup = []
    vx = P.Vec.from_array(xg[rs:re_], comm=comm, N=N)
    for flag in (sr.SYMMETRIC, sr.FORWARD | sr.ZERO_INITIAL_GUESS, sr.LOCAL_SYMMETRIC | sr.BACKWARD, sr.ZERO_INITIAL_GUESS, sr.LOCAL_SYMMETRIC | sr.EISENSTAT, sr.APPLY_UPPER):
        try:
            A.sor(vb, vx, flag=flag)
            sup.append(0)
        except P.PetscError as e:
            sup.append(e.code)
    if sup != [56] * 6 or not np.array_equal(vx.array(), xg[rs:re_]):
        failed.append(("refused flags", sup))
    # CG + SSOR on the symmetric operator
    S = orc.gen_p7(nx, ny, nzl * world)
    B = P.Mat.from_csr_mpi((S[0][rs:re_ + 1] - S[0][rs]).astype(np.int32), S[1][S[0][rs]:S[0][re_]].copy(), S[2][S[0][rs]:S[0][re_]].copy(), mloc, N, N, comm=comm)
    u = np.cos(0.1 * np.arange(N))
    rhs = orc.spmv(S[0], S[1], S[2], u)
    k = P.KSP(comm=comm)
    k.set_operators(B)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(b"-ksp_type cg -pc_type sor")
    k.set_tolerances(rtol=1e-10)
    k.set_from_options()
    L.PetscOptionsClear()
    vr, vs = P.Vec.from_array(rhs[rs:re_], comm=comm, N=N), P.Vec.from_array(np.zeros(mloc), comm=comm, N=N)
    k.solve(vr, vs)
    err = float(np.max(np.abs(vs.array() - u[rs:re_])))
    if k.reason <= 0 or err > 1e-7:
        failed.append(("cg + sor", k.reason, err))
    print("rank %d/%d: MatSOR of MPIAIJ bitexact=%s cases %d refused %s cg+sor its %d reason %d %s"
          % (rank, world, not failed, cases, sup, k.its, k.reason, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
