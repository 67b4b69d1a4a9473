"""One MatShift, one same-pattern MatAXPY and one MatCopy on P7(256), each followed by a MatMult, with the update on the device copy
(-mat_hipmi355x_update_on_device 1, the default) and on the host copy alone (0: the values cross at the next use -- the route a program
took before the type had these slots), alternated in one process, three pairs:
  python3 tests/tools/mat_value_ops_rate.py [nx, default 256]
Per step: `host` is the wall time of the Mat call itself (it returns once the host mirror is updated and, on the device route, the
kernel is queued: no host wait); `rest` is the wall time from there until the device has finished the MatMult that follows
(mi355x_device_synchronize) -- the update kernel and the product on the device route, the upload of the values, the analyses that
follow an upload and the product on the other.  Medians over the pairs at the end.  The products of the two routes are compared."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    nx = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    import petsc_dev_amd as pda
    from petsc_dev_amd import petsc as P
    L = P.lib()
    k = pda.load_kernels()
    ai, aj, aa = P.gen_poisson7(nx, nx, nx)
    aa = aa * (1.0 + 0.05 * np.sin(np.arange(aa.size)))
    n = ai.size - 1
    print("P7(%d): n=%d nnz=%d, values %.2f GB" % (nx, n, aj.size, 8e-9 * aj.size), flush=True)
    A = P.Mat.from_csr(ai, aj, aa); M = P.Mat.from_csr(ai, aj, aa); K = P.Mat.from_csr(ai, aj, 0.01 * np.cos(np.arange(aa.size)))
    del aa
    x = P.Vec.from_array(np.cos(0.3 * np.arange(n)), comm=L.COMM_SELF); y = x.duplicate()
    for o in (A, M, K):
        o.mult(x, y)
    k.mi355x_device_synchronize()
    steps = (("MatShift", lambda: A.shift(0.5)), ("MatAXPY same pattern", lambda: A.axpy(0.01, K, P.SAME_NONZERO_PATTERN)),
             ("MatCopy", lambda: M.copy(A, P.SAME_NONZERO_PATTERN)))
    times = {(name, r): [] for name, _ in steps for r in (1, 0)}
    prod = {}
    for pair in range(3):
        for route in (1, 0):
            L.PetscOptionsClear()
            L.PetscOptionsSetValue(b"-mat_hipmi355x_update_on_device", str(route).encode())
            M.copy(A, P.SAME_NONZERO_PATTERN); A.mult(x, y); k.mi355x_device_synchronize()      # the same start for both routes
            for name, call in steps:
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                A.mult(x, y)
                k.mi355x_device_synchronize()
                t2 = time.perf_counter()
                times[(name, route)].append((t1 - t0, t2 - t1))
                print("pair %d update_on_device %d %-22s host %8.2f ms  rest %8.2f ms" % (pair, route, name, 1e3 * (t1 - t0), 1e3 * (t2 - t1)), flush=True)
                got = y.array().copy()
                if (name, pair) in prod:
                    assert np.array_equal(got.view(np.uint64), prod[(name, pair)].view(np.uint64)), "the two routes' products differ after " + name
                prod[(name, pair)] = got
    L.PetscOptionsClear()
    nup = C.c_int()
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(nup))
    print("uploads of A's values in all: %d" % nup.value)
    print("medians over 3 pairs (ms):           host mirror + queueing | until the product is done | step")
    for name, _ in steps:
        for route in (1, 0):
            h = 1e3 * float(np.median([t[0] for t in times[(name, route)]])); r = 1e3 * float(np.median([t[1] for t in times[(name, route)]]))
            print("  %-22s update_on_device %d: %10.2f | %10.2f | %10.2f" % (name, route, h, r, h + r))
    for name, _ in steps:
        on = float(np.median([sum(t) for t in times[(name, 1)]])); off = float(np.median([sum(t) for t in times[(name, 0)]]))
        print("  %-22s device route %s end to end: %.2f ms against %.2f ms" % (name, "FASTER" if on < off else "NOT faster", 1e3 * on, 1e3 * off))


if __name__ == "__main__":
    main()
