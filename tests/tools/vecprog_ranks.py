"""Rank script of tests/test_vecprog_gpu.py::test_two_staged_ranks (started by torch.distributed.run, the ranks sharing one GPU over the
host-staged transport): the call programs of tests/vecprog.py restricted to Vec calls and MatMult, on MPI vectors and an MPIAIJ matrix split
by rows.  Per program: the run with the noted operations on against the run with them off, bit for bit in every scalar and every local
vector, and the local vectors against this rank's slice of the sequential model (its MatMult formed as MatMult_MPIAIJ forms it: the
diagonal block's product, then the off-diagonal block's added).  A failing program is cut to its shortest failing prefix, the ranks
deciding together."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from petsc_dev_amd import petsc as P
    from petsc_dev_amd import dist as PD
    import vecprog as vp
    L = P.lib()
    comm = PD.torch_comm(device_comm=os.environ.get("MI355X_STAGED", "0") != "1")
    setdef = L.raw("VecHIPMI355XSetDeferral")

    def check(p, upto=None):
        """(noting on == off, slices == model, first vector that misses the model) on this rank"""
        n = p["n"]
        lo, hi = (n * rank) // world, (n * (rank + 1)) // world
        runs = []
        try:
            for on in (0, 1):
                setdef(on)
                runs.append(vp.execute(P, p, upto, comm=comm, rows=(lo, hi)))
        finally:
            setdef(-1)
        (o0, v0), (o1, v1) = runs
        ref = vp.reference(p, upto, world=world)[1]
        miss = [j for j, (u, w) in enumerate(zip(v1, ref)) if not vp.same(u, w[lo:hi])]
        return vp.same(o0, o1) and all(vp.same(u, w) for u, w in zip(v0, v1)), not miss, miss

    def anywhere(flag):
        t = torch.tensor([1 if flag else 0]); dist.all_reduce(t, op=dist.ReduceOp.MAX); return bool(t.item())

    same_modes, same_model, failed = True, True, []
    before = vp.deferral_counts(P)
    for i in vp.RANK_SEEDS:
        p = vp.generate(i, ranks=True)
        a, b, miss = check(p)
        same_modes, same_model = same_modes and a, same_model and b
        if anywhere(not (a and b)):
            lo_, hi_ = 1, len(p["calls"])
            while lo_ < hi_:
                mid = (lo_ + hi_) // 2
                a2, b2, _ = check(p, mid)
                if anywhere(not (a2 and b2)): hi_ = mid
                else: lo_ = mid + 1
            a2, b2, miss2 = check(p, lo_)
            failed.append("program %d (%s, motif %s cut at %s by %s): on == off %s, slices == model %s; shortest failing prefix %d calls, then on == off %s, vectors %s miss the model:\n%s"
                          % (i, p["shape"], p["motif"], p["cut"], p["cls"], a, b, lo_, a2, miss2, vp.show(p["calls"][:lo_])))
    taken = vp.deferral_counts(P) - before
    print("rank %d/%d: %d programs, noting on == off: %s, slices == model: %s, fused sweeps %d, shortcuts %s"
          % (rank, world, len(vp.RANK_SEEDS), same_modes, same_model, taken[0], dict(zip(vp.COUNTERS, (int(t) for t in taken)))), flush=True)
    for f in failed[:3]:
        print("rank %d/%d: %s" % (rank, world, f), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
