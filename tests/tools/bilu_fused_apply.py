"""One MatSolve of block ILU(0) on a BAIJ matrix by its two routes, in one process: -pc_factor_hipmi355x_trisolve level (one launch per
dependency level) against fused (one launch per run of narrow levels) at -pc_factor_hipmi355x_bilu_chain_rows 32, 64, 128, 256, 512, 1024,
2048, 4096 and unbounded, next to the AIJ inode route's application of the same matrix.  Two matrices: the FEM stand-in (tests/problems.py gen_fem3
on the fem3_blocks mesh, narrow levels throughout) and a 7-point block operator on a 64^3 grid (levels of up to ~3000 block rows: a
mixed plan).

ONE factor per matrix serves every route: a set-up on the same operator and values re-cuts the launch plan and factors nothing
(PCILUGetNumeric_HIPMI355X is printed to show it).  Every route gets 3 warm-up applications; every round then times 10 applications of
each route, the routes alternating, with a device synchronise before the clock is read; the median of the three rounds and their spread
are reported.  The fused applications are compared with the level route's bit for bit.
  python3 tests/tools/bilu_fused_apply.py [fem|grid|both] [ex ey ez]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import problems as pb  # noqa: E402

UNBOUNDED = (1 << 31) - 1
ROWS = [32, 64, 128, 256, 512, 1024, 2048, 4096, UNBOUNDED]


def grid_blocks(n, bs=3, seed=5):
    """7-point stencil of bs x bs blocks on an n^3 grid, natural ordering, dominant diagonal blocks: (bi, bj, ba), blocks column-major"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n ** 3).reshape(n, n, n)
    rows, cols = [idx.ravel()], [idx.ravel()]
    for ax in range(3):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[ax] = slice(0, n - 1); hi[ax] = slice(1, n)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [a, b]; cols += [b, a]
    G = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3))
    G.sort_indices()
    bi, bj = G.indptr.astype(np.int32), G.indices.astype(np.int32)
    blocks = -rng.random((bj.size, bs, bs))
    diag = bj == np.repeat(np.arange(n ** 3, dtype=np.int32), np.diff(bi))
    blocks[diag] = 8.0 * bs * np.eye(bs) + rng.random((int(diag.sum()), bs, bs))
    return bi, bj, np.ascontiguousarray(blocks.transpose(0, 2, 1)).ravel()


def point_csr(bs, bi, bj, ba):
    B = sp.bsr_matrix((ba.reshape(-1, bs, bs).transpose(0, 2, 1), bj, bi), shape=((bi.size - 1) * bs,) * 2)
    A = B.tocsr(); A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def measure(name, bs, bi, bj, ba, csr):
    import petsc_dev_amd as pda
    from petsc_dev_amd import petsc as P
    L = P.lib(); k = pda.load_kernels()
    n = (bi.size - 1) * bs
    print("%s: n = %d, %d block rows, %d blocks, bs %d" % (name, n, bi.size - 1, bj.size, bs), flush=True)
    b = P.Vec.from_array(np.sin(0.1 * np.arange(n)), comm=L.COMM_SELF)

    def new_pc(A, opts):
        ksp = P.KSP(comm=L.COMM_SELF); ksp.set_operators(A)
        pc = C.c_void_p(); L.KSPGetPC(ksp.h, C.byref(pc))
        L.PetscOptionsClear(); L.PetscOptionsInsertString(("-ksp_type preonly -pc_type ilu " + opts).encode())
        ksp.set_from_options()
        t0 = time.time(); L.PCSetUp(pc); tset = time.time() - t0
        L.PetscOptionsClear()
        return ksp, pc, tset

    Ab = P.Mat.from_bsr(bs, bi, bj, ba)
    kspb, pcb, tset = new_pc(Ab, "")
    v = [C.c_int() for _ in range(4)]; L.PCBILUGetInfo_HIPMI355X(pcb, *[C.byref(a) for a in v])
    print("BAIJ (block ILU)   set-up %.2f s; bs %d, %d + %d block levels, %d blocks" % ((tset,) + tuple(a.value for a in v)), flush=True)
    Aa = P.Mat.from_csr(*csr)
    kspa, pca, tset = new_pc(Aa, "")
    nn, nl, nu = C.c_int(), C.c_int(), C.c_int(); L.PCILUGetNodeInfo_HIPMI355X(pca, C.byref(nn), C.byref(nl), C.byref(nu))
    sf, ab = C.c_int(), C.c_int(); L.PCILUGetSolver_HIPMI355X(pca, C.byref(sf), C.byref(ab))
    print("AIJ (inode route)  set-up %.2f s; %d nodes, %d + %d node levels, sync-free %d" % (tset, abs(nn.value), nl.value, nu.value, sf.value), flush=True)

    def route(opts):
        """the BAIJ factor's route for the next applications: a set-up on the same operator and values"""
        kspb.set_operators(Ab)
        L.PetscOptionsClear()
        if opts:
            L.PetscOptionsInsertString(opts.encode())
        L.PCSetUp(pcb)
        L.PetscOptionsClear()
        p = [C.c_int() for _ in range(3)]; L.PCBILUGetSolvePlan_HIPMI355X(pcb, *[C.byref(a) for a in p])
        return tuple(a.value for a in p)

    routes = [("level", "")] + [("fused %s" % ("unbounded" if r == UNBOUNDED else r), "-pc_factor_hipmi355x_trisolve fused -pc_factor_hipmi355x_bilu_chain_rows %d" % r)
                                for r in ROWS]
    xb, xa = b.duplicate(), b.duplicate()
    plans, outs = {}, {}
    for rname, opts in routes:
        plans[rname] = route(opts)
        for _ in range(3):
            L.PCApply(pcb, b.h, xb.h)
        k.mi355x_device_synchronize()
        outs[rname] = xb.array().copy()
        print("%-16s fused %d, launches %d + %d" % ((rname,) + plans[rname]), flush=True)
    for _ in range(3):
        L.PCApply(pca, b.h, xa.h)
    k.mi355x_device_synchronize()
    num = [C.c_int() for _ in range(3)]; L.PCILUGetNumeric_HIPMI355X(pcb, *[C.byref(a) for a in num])
    print("block factor after all route changes: %d pattern pass(es), %d numeric factorisation(s)" % (num[1].value, num[2].value), flush=True)
    times = {rname: [] for rname, _ in routes}; times["AIJ inode"] = []
    for rnd in range(3):
        for rname, opts in routes + [("AIJ inode", None)]:
            if opts is not None:
                route(opts)
            pc, x = (pca, xa) if opts is None else (pcb, xb)
            k.mi355x_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                L.PCApply(pc, b.h, x.h)
            k.mi355x_device_synchronize()
            times[rname].append((time.perf_counter() - t0) / 10 * 1e3)
            print("round %d  %-16s PCApply %.3f ms" % (rnd, rname, times[rname][-1]), flush=True)
    nlev = plans["level"][1] + plans["level"][2]
    for rname, t in times.items():
        med = float(np.median(t))
        extra = ""
        if rname in plans:
            same = np.array_equal(outs[rname].view(np.uint64), outs["level"].view(np.uint64))
            extra = "  launches %d  %.2f us per level  bits %s" % (plans[rname][1] + plans[rname][2], med * 1e3 / nlev, "equal to level" if same else "DIFFER from level")
        print("median  %-16s %.3f ms  spread %.3f ms%s" % (rname, med, max(t) - min(t), extra), flush=True)
    print("largest relative difference between the level route and the AIJ application: %.3e" % float(np.abs(xa.array() - outs["level"]).max() / np.abs(outs["level"]).max()), flush=True)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    dims = [int(a) for a in sys.argv[2:5]] if len(sys.argv) > 4 else [130, 130, 67]
    if which in ("fem", "both"):
        ai, aj, aa = pb.gen_fem3(*dims)
        n = ai.size - 1
        B = sp.bsr_matrix(sp.csr_matrix((aa, aj, ai), shape=(n, n)), blocksize=(3, 3)); B.sort_indices()
        measure("fem %s" % "x".join(map(str, dims)), 3, B.indptr.astype(np.int32), B.indices.astype(np.int32),
                np.ascontiguousarray(B.data.transpose(0, 2, 1)).ravel(), (ai, aj, aa))
    if which in ("grid", "both"):
        ng = dims[0] if which == "grid" and len(sys.argv) > 4 else 64
        bi, bj, ba = grid_blocks(ng)
        measure("grid %d^3, 7-point blocks" % ng, 3, bi, bj, ba, point_csr(3, bi, bj, ba))


if __name__ == "__main__":
    main()
