"""ILU(k) against ILU(0) on P7(n) or the FEM stand-in, one process:
  python3 tests/tools/iluk_rate.py [p7|fem] [levels, default 1] [p7 grid edge, default 256]
For levels 0 and k: factor entries per row, levels of L and U, the numeric phase of PCSetUp on the host route and on the device route
(-pc_factor_hipmi355x_numeric device; first factorisation, and a re-factorisation on the same pattern after MatScale by 2;
PETSC_HIPMI355X_SETUP_TIMING lines taken from stderr), and on the host route's factor the time of one application (default trisolve,
10 after 3) and GMRES(30) to rtol 1e-8 from a zero guess: iterations and wall time.  Times are a host clock around calls that end
in a device synchronise."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import problems as pb  # noqa: E402
from ilu_factor_rate import NUMERIC, Stderr  # noqa: E402


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "p7"
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    edge = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    os.environ["PETSC_HIPMI355X_SETUP_TIMING"] = "1"
    import petsc_dev_amd as pda
    from petsc_dev_amd import petsc as P
    L = P.lib(); k = pda.load_kernels()
    if which == "fem":
        from cfg4_spmv import cached
        ai, aj, aa = cached("fem", pb.gen_fem3)
    else:
        ai, aj, aa = P.gen_poisson7(edge, edge, edge)
    n = ai.size - 1
    print("%s: n=%d nnz=%d (%.1f/row)" % (which, n, aj.size, aj.size / n), flush=True)
    A = P.Mat.from_csr(ai, aj, aa)
    x = P.Vec.create(n, comm=L.COMM_SELF); L.VecSet(x.h, 1.0)
    b = x.duplicate(); u = x.duplicate()
    A.mult(x, b)

    def setup(ksp, pc, route):
        ksp.set_operators(A)
        L.PetscOptionsClear(); L.PetscOptionsInsertString(("-pc_factor_hipmi355x_numeric " + route).encode())
        with Stderr() as err:
            t0 = time.perf_counter()
            rc = L.raw("PCSetUp")(pc)
            wall = time.perf_counter() - t0
        L.PetscOptionsClear()
        assert rc == 0, rc
        m = NUMERIC.findall(err.text)
        return wall, float(m[0]) if len(m) == 1 else float("nan")

    for lv in (0, levels):
        for route in ("host", "device"):
            ksp = P.KSP(comm=L.COMM_SELF); ksp.set_operators(A); ksp.set_type("gmreshipmi355x"); ksp.set_pc_type("ilu")
            pc = C.c_void_p(); L.KSPGetPC(ksp.h, C.byref(pc))
            L.PCFactorSetLevels(pc, lv)
            first = setup(ksp, pc, route)
            fl, nzf, nza = C.c_int(), C.c_int(), C.c_int(); L.PCILUGetFill_HIPMI355X(pc, C.byref(fl), C.byref(nzf), C.byref(nza))
            nl, nu = C.c_int(), C.c_int(); L.PCILUGetLevels_HIPMI355X(pc, C.byref(nl), C.byref(nu))
            if route == "host":
                for _ in range(3):
                    L.raw("PCApply")(pc, b.h, u.h)
                k.mi355x_device_synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    L.raw("PCApply")(pc, b.h, u.h)
                k.mi355x_device_synchronize()
                print("ILU(%d): PCApply %.3f ms" % (lv, (time.perf_counter() - t0) / 10 * 1e3), flush=True)
                ksp.set_tolerances(rtol=1e-8, abstol=1e-50, dtol=1e5, max_it=2000)
                L.VecSet(u.h, 0.0)
                k.mi355x_device_synchronize()
                t0 = time.perf_counter()
                ksp.solve(b, u)
                k.mi355x_device_synchronize()
                dt = time.perf_counter() - t0
                print("ILU(%d): GMRES(30) to rtol 1e-8: its=%d reason=%d in %.3f s, error=%g" % (lv, ksp.its, ksp.reason, dt, np.linalg.norm(u.array() - 1.0) / np.sqrt(n)), flush=True)
            L.MatScale(A.h, 2.0)
            again = setup(ksp, pc, route)
            L.MatScale(A.h, 0.5)
            print("ILU(%d) %-6s: factor %.2f entries per row (A %.2f), levels L=%d U=%d; first PCSetUp %.3f s (numeric %.6f s), "
                  "re-factorisation %.3f s (numeric %.6f s)" % (fl.value, route, nzf.value / n, nza.value / n, nl.value, nu.value, *first, *again), flush=True)
            del ksp


if __name__ == "__main__":
    main()
