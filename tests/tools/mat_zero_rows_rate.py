"""One MatZeroRows (MAT_KEEP_NONZERO_PATTERN) and one MatZeroRowsColumns on P7(256), the rows of the grid's six faces listed, x and b
given, each followed by a MatMult, with the update on the device copy (-mat_hipmi355x_update_on_device 1, the default) and on the host copy
alone (0: the values cross at the next use), alternated in one process, three pairs:
  python3 tests/tools/mat_zero_rows_rate.py [nx, default 256]
Per step: `host` is the wall time of the Mat call itself (it returns once the host copy is updated and, on the device route, the kernels
are queued: no host wait); `device` is the wall time from there until the device is idle (mi355x_device_synchronize: the queued update
kernels on the device route, nothing on the other); `rest` from there until the device has finished the MatMult that follows -- the
product on the device route, the upload of the values, the analyses that follow an upload and the product on the other.  Medians over
the pairs at the end, next to a MatMult alone.  The products and b of the two routes are compared."""
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
    rows = np.flatnonzero(np.diff(ai) < 7).astype(np.int32)
    print("P7(%d): n=%d nnz=%d, values %.2f GB, column indices %.2f GB; %d rows listed (%.2f %%)"
          % (nx, n, aj.size, 8e-9 * aj.size, 4e-9 * aj.size, rows.size, 100.0 * rows.size / n), flush=True)
    A = P.Mat.from_csr(ai, aj, aa); M = P.Mat.from_csr(ai, aj, aa)
    A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
    del aa
    x = P.Vec.from_array(np.cos(0.3 * np.arange(n)), comm=L.COMM_SELF); y = x.duplicate()
    xb = P.Vec.from_array(1.0 + np.sin(0.7 * np.arange(n)), comm=L.COMM_SELF)
    b0 = np.cos(1.1 * np.arange(n)) - 0.2
    b = P.Vec.from_array(b0, comm=L.COMM_SELF)
    for o in (A, M):
        o.mult(x, y)
    k.mi355x_device_synchronize()
    tm = []
    for _ in range(5):
        t0 = time.perf_counter(); A.mult(x, y); L.VecHIPMI355XFlushDeferred(); k.mi355x_device_synchronize(); tm.append(time.perf_counter() - t0)
    print("MatMult alone: %.3f ms (median of 5, wall)" % (1e3 * float(np.median(tm))), flush=True)
    steps = (("MatZeroRows", lambda: A.zero_rows(rows, 1.0, x=xb, b=b)), ("MatZeroRowsColumns", lambda: A.zero_rows_columns(rows, 1.0, x=xb, b=b)))
    times = {(name, r): [] for name, _ in steps for r in (1, 0)}
    prod = {}
    for pair in range(3):
        for route in (1, 0):
            for name, call in steps:
                L.PetscOptionsClear()
                L.PetscOptionsSetValue(b"-mat_hipmi355x_update_on_device", b"1")
                M.copy(A, P.SAME_NONZERO_PATTERN); b.set_array(b0); A.mult(x, y)      # the same start for every step: values on the device
                nrm = C.c_double()
                L.VecNorm(b.h, 1, C.byref(nrm)); L.VecNorm(xb.h, 1, C.byref(nrm))              # ... and b and x as well
                L.VecHIPMI355XFlushDeferred()
                k.mi355x_device_synchronize()
                L.PetscOptionsSetValue(b"-mat_hipmi355x_update_on_device", str(route).encode())
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                k.mi355x_device_synchronize()
                t2 = time.perf_counter()
                A.mult(x, y)
                L.VecHIPMI355XFlushDeferred()               # (a product alone is noted, not launched: host/vechip.c)
                k.mi355x_device_synchronize()
                t3 = time.perf_counter()
                times[(name, route)].append((t1 - t0, t2 - t1, t3 - t2))
                print("pair %d update_on_device %d %-20s host %8.2f ms  device %8.2f ms  rest %8.2f ms"
                      % (pair, route, name, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)), flush=True)
                got = np.concatenate([y.array(), b.array()])
                if (name, pair) in prod:
                    assert np.array_equal(got.view(np.uint64), prod[(name, pair)].view(np.uint64)), "the two routes' products or b differ after " + name
                prod[(name, pair)] = got
    L.PetscOptionsClear()
    nup, nl, nd = C.c_int(), C.c_int(), C.c_int()
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(nup))
    L.MatHIPMI355XGetZeroRowsCounts(A.h, C.byref(nl), C.byref(nd))
    print("uploads of A's values in all: %d; row lists sent: %d; updates on the device copy: %d" % (nup.value, nl.value, nd.value))
    print("medians over 3 pairs (ms):             host copy + queueing | device update | until the product is done | step")
    for name, _ in steps:
        for route in (1, 0):
            h, d, r = (1e3 * float(np.median([t[j] for t in times[(name, route)]])) for j in range(3))
            print("  %-20s update_on_device %d: %10.2f | %10.2f | %10.2f | %10.2f" % (name, route, h, d, r, h + d + r))
    for name, _ in steps:
        on = float(np.median([sum(t) for t in times[(name, 1)]])); off = float(np.median([sum(t) for t in times[(name, 0)]]))
        print("  %-20s device route %s end to end: %.2f ms against %.2f ms" % (name, "FASTER" if on < off else "NOT faster", 1e3 * on, 1e3 * off))
    d = float(np.median([t[1] for t in times[("MatZeroRowsColumns", 1)]]))
    print("  device update of MatZeroRowsColumns: %.3f ms = %.0f GB/s of the column indices (%.2f GB)" % (1e3 * d, 4e-9 * aj.size / d, 4e-9 * aj.size))


if __name__ == "__main__":
    main()
