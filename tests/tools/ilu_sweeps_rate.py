"""Rate of one Jacobi-sweep step pair of -pc_factor_hipmi355x_trisolve sweeps:<k> (one lower step, mi355x_spmv_csr_add on the strict
lower triangle, plus one upper step, mi355x_spmv_csr_add_scaled on the strict upper one) against one MatMult of the matrix the factor
came from by the plain row-block kernel, in the same process, as time per byte.
  python3 tests/tools/ilu_sweeps_rate.py [fem|p7] [reps]
ILU(0) keeps the pattern of A and a kernel's time does not depend on the values, so the triangles are A's own (no factorisation).
Bytes from the counts: 12 B per stored entry and 4 B per row-pointer entry, 8 B per vector entry read or written (x counted once).
Times: a host clock around `reps` launches that end in a device synchronise, after a warm-up; the two measurements alternate."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import problems as pb  # noqa: E402


def triangles(ai, aj, aa):
    n = ai.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(ai))
    out = []
    for mask in (aj < rows, aj > rows):
        ip = np.zeros(n + 1, dtype=np.int64); ip[1:] = np.cumsum(np.bincount(rows[mask], minlength=n))
        out.append((ip.astype(np.int32), aj[mask].copy(), -aa[mask]))
    diag = aa[aj == rows]
    assert diag.size == n
    return out[0], out[1], 1.0 / diag


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "fem"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    from gpu import Dev
    from petsc_dev_amd import petsc as P
    if which == "fem":
        from cfg4_spmv import cached
        ai, aj, aa = cached("fem", pb.gen_fem3)
    else:
        P.lib()
        ai, aj, aa = P.gen_poisson7(256, 256, 256)
    n, nnz = ai.size - 1, aj.size
    (iL, jL, aL), (iU, jU, aU), dinv = triangles(ai, aj, aa)
    dev = Dev(); k = dev.k

    def put_csr(ip, j, a):   # 16 bytes of slack past the index and value arrays (the kernels' paired loads)
        plan = C.c_void_p()
        dev.chk(k.mi355x_spmv_plan_create(dev.h, ip.size - 1, ip.ctypes.data, None, C.byref(plan)))
        return plan, dev.put(ip), dev.put(np.concatenate([j, np.zeros(4, np.int32)])), dev.put(np.concatenate([a, np.zeros(2)]))
    A, Lo, Up = put_csr(ai, aj, aa), put_csr(iL, jL, aL), put_csr(iU, jU, aU)
    x = dev.put(np.random.default_rng(1).standard_normal(n))
    b, dd = dev.put(np.ones(n)), dev.put(dinv)
    w = [dev.put(np.zeros(n)) for _ in range(2)]

    def mult():
        dev.chk(k.mi355x_spmv_csr(dev.h, *A, x, w[0]))

    def pair():
        dev.chk(k.mi355x_spmv_csr_add(dev.h, *Lo, x, b, w[0]))
        dev.chk(k.mi355x_spmv_csr_add_scaled(dev.h, *Up, w[0], b, dd, w[1]))

    def timed(fn):
        for _ in range(3):
            fn()
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dev.sync()
        return (time.perf_counter() - t0) / reps
    bytes_mult = 12.0 * nnz + 4.0 * (n + 1) + 8.0 * n * 2
    bytes_pair = 12.0 * (jL.size + jU.size) + 2 * 4.0 * (n + 1) + 8.0 * n * 7
    print("%s: n=%d nnz=%d (%.1f/row); strict triangles %d + %d entries" % (which, n, nnz, nnz / n, jL.size, jU.size), flush=True)
    print("bytes: MatMult %.1f MB, step pair %.1f MB, byte ratio %.3f" % (bytes_mult / 1e6, bytes_pair / 1e6, bytes_pair / bytes_mult), flush=True)
    for rnd in range(3):
        tm, tp = timed(mult), timed(pair)
        print("round %d: MatMult %.3f ms = %.2f TB/s | step pair %.3f ms = %.2f TB/s | time ratio %.3f = %.2f x byte ratio"
              % (rnd, tm * 1e3, bytes_mult / tm / 1e12, tp * 1e3, bytes_pair / tp / 1e12, tp / tm, (tp / tm) / (bytes_pair / bytes_mult)), flush=True)


if __name__ == "__main__":
    main()
