"""Rank script of tests/test_nullspace_gpu.py::test_two_staged_ranks (started by torch.distributed.run, the ranks sharing one GPU over
the host-staged transport).  On vectors of 4913 entries split 2457 + 2456: VecSum against the one-rank reference (device-order sum of
the whole vector) to 1e-13 * sum|x|; VecMax / VecMin with locations whose extremum sits on both ranks (exact: the lowest global index
and that element's value), and without a location; MatNullSpaceRemove with has_cnst (VecSum + VecShift on several ranks) and through
MatNullSpaceRemoveConstantHIPMI355X against tests/nullspace_ref.py to 1e-13 relative; CG + Jacobi with the null space on the 17^3
Neumann operator, consistent right-hand side, 10 iterations: history and iterate against the one-rank reference to 1e-13 relative."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOL = 1e-13


def main():
    import torch  # noqa: F401
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from petsc_dev_amd import petsc as P
    from petsc_dev_amd import dist as PD
    import orc
    import nullspace_ref as nr
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    csr = nr.neumann7(17, 17, 17)
    N = csr[0].size - 1
    starts = [0, 2457, N] if world == 2 else [N * r // world for r in range(world + 1)]
    rs, re_ = starts[rank], starts[rank + 1]
    V = lambda a: P.Vec.from_array(a[rs:re_], comm=comm, N=N)
    failed = []

    x = np.random.default_rng(8).standard_normal(N)
    x[100] = x[4000] = 7.0                 # the maximum on both ranks: the lower global index is rank 0's
    x[2600] = x[4900] = -7.0               # the minimum twice on rank 1
    x[50] = x[3000] = np.nan               # never selected (not position 0)
    v = V(x)
    if v.max() != (100, 7.0) or v.min() != (2600, -7.0):
        failed.append(("max / min with locations", v.max(), v.min()))
    r = C.c_double()
    L.VecMax(v.h, None, C.byref(r)); mx = r.value
    L.VecMin(v.h, None, C.byref(r)); mn = r.value
    if (mx, mn) != (7.0, -7.0):
        failed.append(("max / min without locations", mx, mn))
    y = x.copy(); y[0] = np.nan            # global position 0: the reference's answer is that NaN, location 0
    w = V(y)
    p, val = w.max()
    if p != 0 or not np.isnan(val):
        failed.append(("NaN at global 0", p, val))
    e = np.full(N, 2.5)                    # all equal: location 0
    if V(e).max() != (0, 2.5) or V(e).min() != (0, 2.5):
        failed.append(("all equal",))

    s_in = np.random.default_rng(9).standard_normal(N) + 0.5
    with orc.device_reduction_order():
        s_ref = nr.vec_sum(s_in)
        rem_ref = nr.remove(s_in, True, ())
    s = V(s_in).sum()
    if abs(s - s_ref) > TOL * np.sum(np.abs(s_in)):
        failed.append(("VecSum", s, s_ref))
    a = V(s_in)
    P.NullSpace(True, comm=comm).remove(a)
    b = V(s_in)
    sp = P.NullSpace(False, comm=comm)
    sp.set_device_constant()
    sp.remove(b)
    scale = np.max(np.abs(s_in))
    for name, got in (("has_cnst", a.array()), ("callback", b.array())):
        if np.max(np.abs(got - rem_ref[rs:re_])) > TOL * scale:
            failed.append(("MatNullSpaceRemove " + name, float(np.max(np.abs(got - rem_ref[rs:re_])))))
    if not np.array_equal(a.array().view(np.uint64), b.array().view(np.uint64)):
        failed.append(("the two routes differ",))

    # CG + Jacobi with the null space
    rhs = np.random.default_rng(11).standard_normal(N)
    with orc.device_reduction_order():
        rhs = nr.remove(rhs, True, ())
        xo, ho, ito, ro = nr.pcg(*csr, rhs, 1e-30, nr.jacobi(*csr), (True, ()), max_it=10)
    ai, aj, aa = csr
    A = P.Mat.from_csr_mpi((ai[rs:re_ + 1] - ai[rs]).astype(np.int32), aj[ai[rs]:ai[re_]].copy(), aa[ai[rs]:ai[re_]].copy(), re_ - rs, N, N, comm=comm)
    k = P.KSP(comm=comm)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(b"-ksp_type cg -pc_type jacobi")
    k.set_tolerances(rtol=1e-30, max_it=10)
    k.set_from_options()
    L.PetscOptionsClear()
    nsp = P.NullSpace(True, comm=comm)
    k.set_null_space(nsp)
    k.record_history()
    vr, vs = V(rhs), V(np.zeros(N))
    k.solve(vr, vs)
    h = k.history()
    herr = float(np.max(np.abs(h - ho) / ho)) if h.size == ho.size else np.inf
    xerr = float(np.max(np.abs(vs.array() - xo[rs:re_])) / np.max(np.abs(xo)))
    if (k.its, k.reason) != (ito, ro) or herr > TOL or xerr > TOL:
        failed.append(("cg + jacobi", k.its, k.reason, ito, ro, herr, xerr))
    print("rank %d/%d: null space on staged ranks ok=%s sum err %.2g history err %.2g iterate err %.2g %s"
          % (rank, world, not failed, abs(s - s_ref) / np.sum(np.abs(s_in)), herr, xerr, failed if failed else ""), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
