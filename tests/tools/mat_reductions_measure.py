"""Times the matrix reductions on P7(N) (device route, host route) next to one MatMult of the same matrix: the source of
profiles/mat_reductions.log.  python tests/tools/mat_reductions_measure.py [N] [log file]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import petsc_dev_amd as pda  # noqa: E402
from petsc_dev_amd import petsc as P  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REP = 20
out = open(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mat_reductions.log"), "w")


def say(s):
    print(s, flush=True)
    out.write(s + "\n"); out.flush()


L = P.lib()
k = pda.load_kernels()
t0 = time.time()
ai, aj, aa = P.gen_poisson7(N, N, N)
aa = aa * (1.0 + 0.25 * np.sin(np.arange(aa.size)))
n, nnz = ai.size - 1, aa.size
say("P7(%d): %d rows, %d stored entries (generated in %.1f s)" % (N, n, nnz, time.time() - t0))
A = P.Mat.from_csr(ai, aj, aa)
x = P.Vec.from_array(np.ones(n), comm=L.COMM_SELF)
y = x.duplicate()
_, v = A.get_vecs()
idx = np.zeros(n, np.int32)
norms = np.zeros(n)


def sync():
    k.mi355x_device_synchronize()


def timed(fn, rep=REP, warm=3):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(rep):
        t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
    ts = np.array(ts) * 1e3
    return np.median(ts), ts.min(), ts.max()


A.mult(x, y); sync()
L.PetscOptionsSetValue(b"-mat_hipmi355x_reductions", b"device")
L.MatSetFromOptions(A.h)
np_ = C.c_int(0)
L.MatHIPMI355XGetRowPatterns(A.h, C.byref(np_))
assert np_.value > 0, "the yardstick's byte count below is the row-pattern kernel's"
t = time.perf_counter(); first = A.norm(P.NORM_1); sync()
say("first NORM_1 (builds the transpose on the host, uploads it): %.1f ms  value %.17g" % ((time.perf_counter() - t) * 1e3, first))
cases = [("MatMult (yardstick, row-pattern kernel)", lambda: A.mult(x, y), 8 * nnz + 4 * n + 16 * n),
         ("MatNorm NORM_INFINITY", lambda: A.norm(P.NORM_INFINITY), 8 * nnz + 4 * n + 16 * n),
         ("MatNorm NORM_1 (transpose cached)", lambda: A.norm(P.NORM_1), 8 * nnz + 4 * n + 16 * n),
         ("MatNorm NORM_FROBENIUS", lambda: A.norm(P.NORM_FROBENIUS), 8 * nnz),
         ("MatGetRowMaxAbs (idx NULL)", lambda: L.MatGetRowMaxAbs(A.h, v.h, None), 8 * nnz + 4 * n + 8 * n),
         ("MatGetRowMaxAbs (idx; + 4 n to the host)", lambda: L.MatGetRowMaxAbs(A.h, v.h, idx.ctypes.data_as(C.c_void_p)), 8 * nnz + 4 * n + 12 * n),
         ("MatGetColumnNorms NORM_2 (+ 8 n to the host)", lambda: L.MatGetColumnNorms(A.h, P.NORM_2, norms.ctypes.data_as(C.c_void_p)), 8 * nnz + 4 * n + 8 * n)]
say("bytes: what the kernels of a call must move on the device (values 8 B per entry, 4 B per row of row pointer or pattern word, vectors read and written); copies to the caller's host arrays are named with the call")
say("device route, %d timed calls after 3 warm-up calls each, host clock around call + device synchronise; bytes = what the kernels must move" % REP)
for rnd in range(2):                      # two passes over the list: the spread between them is the noise
    for name, fn, nbytes in cases:
        med, lo, hi = timed(fn)
        say("  pass %d  %-44s median %8.3f ms  (min %8.3f, max %8.3f)  %7.1f MB  %6.2f TB/s at the median" % (rnd, name, med, lo, hi, nbytes / 1e6, nbytes / med / 1e9))
L.PetscOptionsSetValue(b"-mat_hipmi355x_reductions", b"host")
L.MatSetFromOptions(A.h)
say("host route (one host thread, plain loops), 3 timed calls")
for name, fn, nbytes in cases[1:]:
    if "idx NULL" in name:
        continue
    med, lo, hi = timed(fn, rep=3, warm=1)
    say("  %-44s median %9.1f ms  (min %9.1f, max %9.1f)" % (name, med, lo, hi))
L.PetscOptionsClear()
out.close()
