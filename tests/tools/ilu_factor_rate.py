"""PCSetUp of ILU(0) with the numeric factorisation on the host (the default, the yardstick) and on the device
(-pc_factor_hipmi355x_numeric device), alternated in one process, three pairs:
  python3 tests/tools/ilu_factor_rate.py [p7|fem] [trisolve mode, default level]
Per route and pair: wall time of the first PCSetUp (symbolic work, uploads, numeric), wall time of a second PCSetUp after the values
changed on the same pattern (MatScale on the device copy), and the numeric phase alone: PETSC_HIPMI355X_SETUP_TIMING=1 is set, the
plug-in's phase lines are taken from stderr around each PCSetUp, echoed, and the "factor: numeric passes" (host route) /
"factor (device): numeric passes" (device route) figure is kept.  Times are a host clock around calls that end in a device
synchronise (PCSetUp waits for the pass's outcome); medians over the pairs at the end, the device route's numeric phase also per
level of L.  The first application after each set-up is checked: both routes give the same bits."""
import ctypes as C
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import problems as pb  # noqa: E402

ROUTES = ("host", "device")
NUMERIC = re.compile(r"factor(?: \(device\))?: numeric passes\s+([0-9.eE+-]+) s")


class Stderr:
    """fd 2 into a temporary file for the time of a call (the plug-in prints from C)."""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "p7"
    tri = sys.argv[2] if len(sys.argv) > 2 else "level"
    os.environ["PETSC_HIPMI355X_SETUP_TIMING"] = "1"
    from petsc_dev_amd import petsc as P
    L = P.lib()
    if which == "fem":
        from cfg4_spmv import cached
        ai, aj, aa = cached("fem", pb.gen_fem3)
    else:
        ai, aj, aa = P.gen_poisson7(256, 256, 256)
        aa = aa * (1.0 + 0.05 * np.sin(np.arange(aa.size)))
    n = ai.size - 1
    print("%s: n=%d nnz=%d (%.1f/row), trisolve %s" % (which, n, aj.size, aj.size / n, tri), flush=True)
    b = P.Vec.from_array(np.random.default_rng(1).standard_normal(n), comm=L.COMM_SELF)
    times = {r: [] for r in ROUTES}
    first_bits = {}
    nlevL = 0
    for rnd in range(3):
        for name in ROUTES:
            A = P.Mat.from_csr(ai, aj, aa)
            x = b.duplicate()
            A.mult(b, x)                                    # the operator's device copy exists before the clock starts, as in a solver loop
            pc = C.c_void_p()
            k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc)); L.PCSetType(pc, b"ilu")
            opts = "-pc_factor_hipmi355x_trisolve %s -pc_factor_hipmi355x_numeric %s" % (tri, name)
            out = []
            for again in (False, True):
                if again:
                    L.MatScale(A.h, 1.25)
                    k.set_operators(A)
                L.PetscOptionsClear(); L.PetscOptionsInsertString(opts.encode())
                with Stderr() as err:
                    t0 = time.perf_counter()
                    rc = L.raw("PCSetUp")(pc)
                    wall = time.perf_counter() - t0
                L.PetscOptionsClear()
                print("--- pair %d %s %s" % (rnd, name, "re-factorisation" if again else "first factorisation"), flush=True)
                sys.stdout.write(err.text); sys.stdout.flush()
                assert rc == 0, rc
                m = NUMERIC.findall(err.text)
                assert len(m) == 1, "one numeric-phase line per PCSetUp expected, got %d" % len(m)
                out += [wall, float(m[0])]
                assert L.raw("PCApply")(pc, b.h, x.h) == 0
                got = x.array().view(np.uint64).copy()
                if again in first_bits:
                    assert np.array_equal(first_bits[again], got), "the routes apply different bits"
                else:
                    first_bits[again] = got
            on, sym, num = C.c_int(), C.c_int(), C.c_int()
            L.PCILUGetNumeric_HIPMI355X(pc, C.byref(on), C.byref(sym), C.byref(num))
            nl, nu = C.c_int(), C.c_int(); L.PCILUGetLevels_HIPMI355X(pc, C.byref(nl), C.byref(nu)); nlevL = nl.value
            print("pair %d %-6s: first PCSetUp %.4f s (numeric %.6f s), re-factorisation %.4f s (numeric %.6f s) "
                  "(on_device %d, symbolic builds %d, numeric runs %d, levels of L %d)"
                  % (rnd, name, out[0], out[1], out[2], out[3], on.value, sym.value, num.value, nlevL), flush=True)
            times[name].append(out)
            del k, A
    for name in ROUTES:
        t = np.median(np.array(times[name]), axis=0)
        line = "median %-6s: first PCSetUp %.4f s (numeric %.6f s), re-factorisation %.4f s (numeric %.6f s)" % (name, t[0], t[1], t[2], t[3])
        if name != "host" and nlevL:
            line += "; per level of L (%d): %.2f us" % (nlevL, 1e6 * t[3] / nlevL)
        print(line, flush=True)


if __name__ == "__main__":
    main()
