"""Rank script of tests/test_mat_reductions_ranks_gpu.py (started by torch.distributed.run, the ranks sharing one GPU over the host-staged
transport): MatNorm, MatGetRowMaxAbs / Max / Min with global columns and MatGetColumnNorms of an MPIAIJ P7 slab matrix on both routes,
against the same queries of the whole matrix as one sequential matrix.  Row-wise results and the infinity norm bit for bit; NORM_1,
Frobenius and the column norms within (n - 1) 2^-53 sum of the one-rank sum, n the number of terms of that sum, taken before the root."""
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
    import matred_ref as R
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    nx, ny, nzl = 7, 6, 8
    mloc, N = nx * ny * nzl, nx * ny * nzl * world
    rs, re_ = rank * mloc, (rank + 1) * mloc
    ai, aj, aa, ncross = R.competing_slab_matrix(nx, ny, nzl * world, [k * mloc for k in range(world + 1)])
    assert ncross >= 2 * nx * ny
    ok, failed = True, []

    def check(cond, what):
        nonlocal ok
        if not cond:
            ok = False; failed.append(what)

    def within(got, ref_sum, nterms, root, what):
        """got against the one-rank sum ref_sum: inside the summation bound taken before the root (sqrt is monotone and correctly rounded)"""
        b = R.sum_bound(nterms, ref_sum)
        lo, hi = ref_sum - b, ref_sum + b
        if root:
            lo, hi = np.sqrt(np.maximum(lo, 0.0)), np.sqrt(hi)
        check(bool(np.all((lo <= got) & (got <= hi))), what)

    cnt = np.bincount(aj, minlength=N)                                     # terms of every column sum
    for route in (b"device", b"host"):
        L.PetscOptionsSetValue(b"-mat_hipmi355x_reductions", route)
        A = P.Mat.from_csr_mpi((ai[rs:re_ + 1] - ai[rs]).astype(np.int32), aj[ai[rs]:ai[re_]].copy(), aa[ai[rs]:ai[re_]].copy(), mloc, N, N, comm=comm)
        S = P.Mat.from_csr(ai, aj, aa)                                     # the whole matrix on one rank
        x = P.Vec.from_array(np.ones(mloc), comm=comm, N=N); y = x.duplicate()
        if route == b"device":
            A.mult(x, y)                                                    # the off-diagonal block's compressed-row device copy exists
        tag = route.decode()
        check(R.bits(np.array([A.norm(P.NORM_INFINITY)]))[0] == R.bits(np.array([S.norm(P.NORM_INFINITY)]))[0], tag + " NORM_INFINITY")
        check(R.bits(np.array([A.norm(P.NORM_1)]))[0] == R.bits(np.array([R.vec_max(A.column_norms(P.NORM_1))]))[0], tag + " NORM_1 is the largest column sum")
        ss = R.sum_squares(aa)
        within(A.norm(P.NORM_FROBENIUS), ss, aa.size, True, tag + " NORM_FROBENIUS")
        for name, ops in (("maxabs", ("row_max_abs",)), ("max", ("row_max",)), ("min", ("row_min",))):
            v, idx = getattr(A, ops[0])()
            sv, sidx = getattr(S, ops[0])()
            check(np.array_equal(R.bits(v.array()), R.bits(sv.array()[rs:re_])), tag + " row " + name + " values")
            check(np.array_equal(idx, sidx[rs:re_]), tag + " row " + name + " columns")
        _, v = A.get_vecs()
        L.MatGetRowMax(A.h, v.h, None)                                      # idx may be NULL
        check(np.array_equal(R.bits(v.array()), R.bits(S.row_max()[0].array()[rs:re_])), tag + " row max without idx")
        within(A.column_norms(P.NORM_1), R.col_reduce(R.ABSSUM, ai, aj, aa, N), cnt, False, tag + " column NORM_1")
        within(A.column_norms(P.NORM_2), R.col_reduce(R.SQSUM, ai, aj, aa, N), cnt, True, tag + " column NORM_2")
        check(np.array_equal(R.bits(A.column_norms(P.NORM_INFINITY)), R.bits(S.column_norms(P.NORM_INFINITY))), tag + " column NORM_INFINITY")
        try:
            A.norm(P.NORM_2)
            check(False, tag + " NORM_2 answered")
        except P.PetscError as e:
            check(e.code == 56, tag + " NORM_2 code %d" % e.code)
        L.PetscOptionsClear()
    mx = P.Mat.from_csr(ai, aj, aa).row_max()[1]
    both = int(np.sum(mx[rs:re_] // mloc != rank))                          # rows of this rank whose maximum lies in the off-diagonal block
    print("rank %d/%d: MPIAIJ reductions against one rank ok=%s rows won by the off-diagonal block %d %s" % (rank, world, ok, both, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
