"""One MatSolve of block ILU(0) on the BAIJ form of the FEM stand-in (tests/problems.py gen_fem3 on the fem3_blocks mesh) next to the
application of the AIJ inode route's ILU(0) on the same matrix, in one process: every round times 10 applications of each, alternating,
after 3 warm-up applications, with a device synchronise before the clock is read.
  python3 tests/tools/bilu_fem_apply.py [ex ey ez]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import problems as pb  # noqa: E402


def main():
    dims = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else [130, 130, 67]
    import petsc_dev_amd as pda
    from petsc_dev_amd import petsc as P
    L = P.lib(); k = pda.load_kernels()
    ai, aj, aa = pb.gen_fem3(*dims)
    n = ai.size - 1
    B = sp.bsr_matrix(sp.csr_matrix((aa, aj, ai), shape=(n, n)), blocksize=(3, 3)); B.sort_indices()
    bi, bj, ba = B.indptr.astype(np.int32), B.indices.astype(np.int32), np.ascontiguousarray(B.data.transpose(0, 2, 1)).ravel()
    print("fem %s: n = %d, %d nonzeros, %d block rows, %d blocks" % ("x".join(map(str, dims)), n, aj.size, bi.size - 1, bj.size), flush=True)
    b = P.Vec.from_array(np.sin(0.1 * np.arange(n)), comm=L.COMM_SELF)
    routes = {}
    for name, A in (("AIJ (inode route)", P.Mat.from_csr(ai, aj, aa)), ("BAIJ (block ILU)", P.Mat.from_bsr(3, bi, bj, ba))):
        ksp = P.KSP(comm=L.COMM_SELF); ksp.set_operators(A)
        pc = C.c_void_p(); L.KSPGetPC(ksp.h, C.byref(pc)); L.PCSetType(pc, b"ilu")
        t0 = time.time(); L.PCSetUp(pc); tset = time.time() - t0
        x = b.duplicate()
        if name.startswith("AIJ"):
            nn, nl, nu = C.c_int(), C.c_int(), C.c_int(); L.PCILUGetNodeInfo_HIPMI355X(pc, C.byref(nn), C.byref(nl), C.byref(nu))
            sf, ab = C.c_int(), C.c_int(); L.PCILUGetSolver_HIPMI355X(pc, C.byref(sf), C.byref(ab))
            what = "%d nodes, %d + %d node levels, sync-free %d" % (abs(nn.value), nl.value, nu.value, sf.value)
        else:
            v = [C.c_int() for _ in range(4)]; L.PCBILUGetInfo_HIPMI355X(pc, *[C.byref(a) for a in v])
            what = "bs %d, %d + %d block levels (one launch each), %d blocks" % tuple(a.value for a in v)
        print("%-18s set-up %.2f s; %s" % (name, tset, what), flush=True)
        for _ in range(3):
            L.PCApply(pc, b.h, x.h)
        k.mi355x_device_synchronize()
        routes[name] = (ksp, pc, A, x)
    for rnd in range(3):
        for name, (ksp, pc, A, x) in routes.items():
            t0 = time.perf_counter()
            for _ in range(10):
                L.PCApply(pc, b.h, x.h)
            k.mi355x_device_synchronize()
            print("round %d  %-18s PCApply %.3f ms" % (rnd, name, (time.perf_counter() - t0) / 10 * 1e3), flush=True)
    xa, xb = routes["AIJ (inode route)"][3].array(), routes["BAIJ (block ILU)"][3].array()
    print("largest relative difference between the two applications: %.3e" % float(np.abs(xa - xb).max() / np.abs(xa).max()))


if __name__ == "__main__":
    main()
