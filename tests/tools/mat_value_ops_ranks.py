"""Rank script of tests/test_mat_value_ops_gpu.py::test_mpiaij_two_staged_ranks (started by torch.distributed.run, the ranks sharing one
GPU over the host-staged transport): MatShift, MatAXPY with SAME_NONZERO_PATTERN and SUBSET_NONZERO_PATTERN -- X's off-diagonal block
keeps fewer columns than Y's, so the two garrays differ --, MatCopy with equal patterns and MatCopy of X into Y, on MPIAIJ matrices used
on the device before the first update and not; after every update MatMult is compared bit for bit with the products of the blocks the
split of the sequentially updated values gives."""
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
    from test_mat_value_ops_cpu import drop_entries
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    nx, ny, nzl = 7, 6, 8
    mloc, N = nx * ny * nzl, nx * ny * nzl * world
    rs, re_ = rank * mloc, (rank + 1) * mloc
    ai, aj, aa = orc.gen_p7(nx, ny, nzl * world)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    za = np.cos(np.arange(aa.size)) - 0.3
    rows = np.repeat(np.arange(N), np.diff(ai))
    diag = np.flatnonzero(rows == aj)
    xi, xj, xa, xtoy = drop_entries(ai, aj, aa, empty_rows=(5, 6, mloc + 3), diag_only=17, frac=0.5)
    xg = np.sin(0.37 * np.arange(N)) + 1.0

    def local(i_, j_, a_):
        return P.Mat.from_csr_mpi((i_[rs:re_ + 1] - i_[rs]).astype(np.int32), j_[i_[rs]:i_[re_]].copy(), a_[i_[rs]:i_[re_]].copy(), mloc, N, N, comm=comm)

    def reference(vals):
        pc = orc.mpiaij_split(rs, re_, rs, re_, ai, aj, vals)
        ref = orc.matmult(pc["ad_i"], pc["ad_j"], pc["ad_a"], xg[rs:re_].copy())[0]
        return orc.matmult(pc["bo_i"], pc["bo_j"], pc["bo_a"], xg[pc["garray"]].copy(), ref)[0]

    def garray_len(A):
        ec = C.c_int()
        L.MatMPIAIJGetScatter(A.h, None, None, C.byref(ec))
        return ec.value

    def diag_uploads(A):
        Ad, n = C.c_void_p(), C.c_int(-1)
        L.MatMPIAIJGetSeqAIJ(A.h, C.byref(Ad), None, None)
        L.MatHIPMI355XGetUploadCount(Ad, C.byref(n))
        return n.value

    x = P.Vec.from_array(xg[rs:re_], comm=comm, N=N)
    y = x.duplicate()
    ok, failed = True, []
    for used_first in (True, False):
        Y, Z, X = local(ai, aj, aa), local(ai, aj, za), local(xi, xj, xa)
        if used_first:
            Y.mult(x, y); X.mult(x, y)
        cur = aa.copy()
        for op in ("shift", "same", "subset", "copy", "copy_basic"):
            if op == "shift":
                Y.shift(0.37); cur[diag] += 0.37
            elif op == "same":
                Y.axpy(-1.3, Z, P.SAME_NONZERO_PATTERN); cur = cur + (-1.3) * za
            elif op == "subset":
                Y.axpy(0.25, X, P.SUBSET_NONZERO_PATTERN); cur[xtoy] += 0.25 * xa
                Y.axpy(-0.5, X, P.SUBSET_NONZERO_PATTERN); cur[xtoy] += -0.5 * xa      # the map kept with Y serves again
            elif op == "copy":
                Z.copy(Y, P.SAME_NONZERO_PATTERN); cur = za.copy()
            else:
                X.copy(Y, P.DIFFERENT_NONZERO_PATTERN); cur = np.zeros(aa.size); cur[xtoy] += 1.0 * xa
            Y.mult(x, y)
            if not np.array_equal(y.array().view(np.uint64), reference(cur).view(np.uint64)):
                ok = False; failed.append((op, used_first))
        nup = diag_uploads(Y)
        if nup != 1:
            ok = False; failed.append(("diagonal block uploaded %d times" % nup, used_first))
        xec, yec = garray_len(X), garray_len(Y)
        # a refused update changes nothing
        code = 0
        try:
            X.axpy(1.0, Y, P.SUBSET_NONZERO_PATTERN)
        except P.PetscError as e:
            code = e.code
        Y.mult(x, y)
        if code != 62 or not np.array_equal(y.array().view(np.uint64), reference(cur).view(np.uint64)):
            ok = False; failed.append(("refused update", used_first))
    print("rank %d/%d: MatShift, MatAXPY SAME / SUBSET, MatCopy of MPIAIJ then MatMult bitexact=%s garray lengths X %d Y %d %s"
          % (rank, world, ok, xec, yec, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
