"""Rank script of tests/test_mat_zero_rows_ranks_gpu.py (started by torch.distributed.run, the ranks sharing one GPU over the host-staged
transport): MatZeroRows of an MPIAIJ matrix with MAT_KEEP_NONZERO_PATTERN -- a P7 slab matrix, every rank passing rows the OTHER ranks
own as well as its own --, used on the device before the update and not; afterwards MatMult and b are compared bit for bit with the
split of the sequential numpy result.  MatZeroRowsColumns of a parallel matrix answers PETSC_ERR_SUP."""
import ctypes as C
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
    from test_mat_zero_rows_cpu import ref_zero_rows
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    nx, ny, nzl = 7, 6, 8
    mloc, N = nx * ny * nzl, nx * ny * nzl * world
    rs, re_ = rank * mloc, (rank + 1) * mloc
    ai, aj, aa = orc.gen_p7(nx, ny, nzl * world)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    xg = np.sin(0.37 * np.arange(N)) + 1.0
    xb = 1.0 + np.sin(0.7 * np.arange(N))
    b0 = np.cos(1.1 * np.arange(N)) - 0.2
    # the boundary rows of the whole grid, dealt to the ranks round-robin: each rank lists rows of every owner, some rows twice
    bnd = np.flatnonzero(np.diff(ai) < 7)
    mine = np.concatenate([bnd[rank::world], bnd[:5]]).astype(np.int32)
    foreign = int(np.sum((mine < rs) | (mine >= re_)))

    def local(a_):
        return P.Mat.from_csr_mpi((ai[rs:re_ + 1] - ai[rs]).astype(np.int32), aj[ai[rs]:ai[re_]].copy(), a_[ai[rs]:ai[re_]].copy(), mloc, N, N, comm=comm)

    def reference(vals):
        pc = orc.mpiaij_split(rs, re_, rs, re_, ai, aj, vals)
        ref = orc.matmult(pc["ad_i"], pc["ad_j"], pc["ad_a"], xg[rs:re_].copy())[0]
        return orc.matmult(pc["bo_i"], pc["bo_j"], pc["bo_a"], xg[pc["garray"]].copy(), ref)[0]

    def diag_uploads(A):
        Ad, n = C.c_void_p(), C.c_int(-1)
        L.MatMPIAIJGetSeqAIJ(A.h, C.byref(Ad), None, None)
        L.MatHIPMI355XGetUploadCount(Ad, C.byref(n))
        return n.value

    x = P.Vec.from_array(xg[rs:re_], comm=comm, N=N)
    y = x.duplicate()
    ok, failed, sup = True, [], 0
    for used_first in (True, False):
        for diag in (2.5, 0.0):
            A = local(aa)
            A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
            if used_first:
                A.mult(x, y)
            xv = P.Vec.from_array(xb[rs:re_], comm=comm, N=N)
            bv = P.Vec.from_array(b0[rs:re_], comm=comm, N=N)
            A.zero_rows(mine, diag, x=xv, b=bv)
            ra, rb = ref_zero_rows(ai, aj, aa, bnd, diag, xb, b0)
            A.mult(x, y)
            if not np.array_equal(y.array().view(np.uint64), reference(ra).view(np.uint64)):
                ok = False; failed.append(("MatMult", used_first, diag))
            if not np.array_equal(bv.array().view(np.uint64), rb[rs:re_].view(np.uint64)):
                ok = False; failed.append(("b", used_first, diag))
            if diag_uploads(A) != 1:
                ok = False; failed.append(("diagonal block uploaded %d times" % diag_uploads(A), used_first, diag))
            A.zero_rows(np.zeros(0, np.int32) if rank else mine, diag)      # a rank that only takes part
            A.mult(x, y)
            if not np.array_equal(y.array().view(np.uint64), reference(ra).view(np.uint64)):
                ok = False; failed.append(("n == 0 on one rank", used_first, diag))
            try:
                A.zero_rows_columns(mine, diag)
            except P.PetscError as e:
                sup = e.code
            if sup != 56:
                ok = False; failed.append(("MatZeroRowsColumns answered %d" % sup, used_first, diag))
    print("rank %d/%d: MatZeroRows of MPIAIJ then MatMult and b bitexact=%s rows listed %d owned by others %d MatZeroRowsColumns %d %s"
          % (rank, world, ok, mine.size, foreign, sup, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
