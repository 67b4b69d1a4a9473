"""KSPSolve_CGHIP with x += a p moved from the update sweep into the AYPX that reads p anyway (-ksp_cg_x_with_p, default
on): the x-less update (mi355x_vec_cg_update_dev_nox) and the AYPX that carries x (mi355x_vec_aypx_dev_x) against numpy,
and whole solves with the option on and off -- iterates, residual history, iteration count and reason bit for bit."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 25) + 1          # 256 MiB + 8 B per vector: the streaming (non-temporal, contiguous-run) forms


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def rnd(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_bitexact(a, b):
    assert a.shape == b.shape
    assert np.array_equal(bits(a), bits(b)), "max abs diff %g" % (np.max(np.abs(a - b)) if a.size else 0)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", [0, 1, 2, 255, 4097, 1_000_001, BIG])
def test_update_without_x_and_aypx_with_x_against_numpy(dev, n):
    """x-less update: r = r + (-a) w, z = r .* d, the sums and dpi exactly as mi355x_vec_cg_update_dev returns them, x and p
    never touched.  AYPX with x: x = x + a p_old, then p = z + (zr/den) p_old.  Element-wise results against numpy bit for bit
    (numpy rounds each product and sum, as the kernels do); a refused step (dpi = 0, or a sign change) leaves x and r alone."""
    k = dev.k
    beta, dpi, den = 0.83, 1.37, 0.77
    a = beta / dpi
    p, w, d, x, r = rnd(n, 31), rnd(n, 32), 1.0 / (2.0 + rnd(n, 33) ** 2), rnd(n, 34), rnd(n, 35)
    dp, dw, dd = dev.put(p), dev.put(w), dev.put(d)
    x1, r1, z1 = dev.put(x), dev.put(r), dev.alloc(8 * max(n, 2))
    r2, z2 = dev.put(r), dev.alloc(8 * max(n, 2))
    ddpi = dev.put(np.array([dpi, 0.0]))
    hs = dev.host_scratch()
    dev.chk(k.mi355x_vec_cg_update_dev(dev.h, n, beta, ddpi, 0.5, 1, dp, dw, dd, x1, r1, z1, hs, 0)); ref = dev.scalar_out(4)
    dres = dev.alloc(64)
    dev.chk(k.mi355x_vec_cg_update_dev_nox(dev.h, n, beta, ddpi, 0.5, 1, dw, dd, r2, z2, dres, 1))
    dev.chk(k.mi355x_handle_wait_result(dev.h))
    out = np.ctypeslib.as_array((C.c_double * 4).from_address(k.mi355x_handle_host_scratch(dev.h))).copy()
    assert_bitexact(out, ref)
    assert_bitexact(dev.get(dres, 4), out)
    rref = r + (-a) * w
    zref = rref * d
    assert_bitexact(dev.get(r2, n), rref); assert_bitexact(dev.get(z2, n), zref)
    assert_bitexact(dev.get(r1, n), rref); assert_bitexact(dev.get(z1, n), zref)
    assert_bitexact(dev.get(dp, n), p)                                        # p read by neither update
    # the AYPX that carries x: x from the full update's bits, p = z + (zr/den) p
    x2 = dev.put(x)
    dev.chk(k.mi355x_vec_aypx_dev_x(dev.h, n, C.c_void_p(dres.value + 8), den, z2, dp, beta, ddpi, 0.5, 1, x2))
    xref = x + a * p
    pref = zref + (out[1] / den) * p
    assert_bitexact(dev.get(x2, n), xref); assert_bitexact(dev.get(x1, n), xref)
    assert_bitexact(dev.get(dp, n), pref)
    # refused steps: x and r untouched, z = r .* d, p still formed (a work vector the host discards)
    for bad, dpiold, chk in ((0.0, 1.0, 0), (np.nan, 1.0, 0), (-1.0, 2.0, 1)):
        dev.chk(k.mi355x_memcpy_h2d(dev.h, ddpi, np.array([bad]).ctypes.data, 8)); dev.sync()
        rb, xb, pb_ = dev.get(r2, n), dev.get(x2, n), dev.get(dp, n)
        dev.chk(k.mi355x_vec_cg_update_dev_nox(dev.h, n, beta, ddpi, dpiold, chk, dw, dd, r2, z2, dres, 1))
        dev.chk(k.mi355x_handle_wait_result(dev.h))
        o = dev.get(dres, 4)
        assert o[0] == 0.0 and o[1] == 0.0 and o[2] == 0.0 and ((np.isnan(o[3]) and np.isnan(bad)) or o[3] == bad)
        assert_bitexact(dev.get(r2, n), rb)
        dev.chk(k.mi355x_vec_aypx_dev_x(dev.h, n, C.c_void_p(dres.value + 8), den, z2, dp, beta, ddpi, dpiold, chk, x2))
        assert_bitexact(dev.get(x2, n), xb)
        assert_bitexact(dev.get(dp, n), dev.get(z2, n) if o[1] == 0.0 else dev.get(z2, n) + (o[1] / den) * pb_)
    for q in (dp, dw, dd, x1, r1, z1, r2, z2, x2, ddpi, dres):
        dev.free(q)


# ---------------------------------------------------------------------------------------------------------------- solves
def solve(P, ai, aj, aa, b, pc, opts, **tol):
    L = P.lib()
    comm = L.COMM_SELF
    A = P.Mat.from_csr(ai, aj, aa, comm=comm)
    vb = P.Vec.from_array(b, comm=comm)
    vx = P.Vec.from_array(np.zeros(b.size), comm=comm)
    k = P.KSP(comm=comm)
    k.set_operators(A)
    L.PetscOptionsClear()
    L.PetscOptionsInsertString(("-ksp_type cghipmi355x -pc_type %s %s" % (pc, opts)).encode())
    if tol:
        k.set_tolerances(**tol)
    k.set_from_options()
    k.record_history()
    k.solve(vb, vx)
    L.PetscOptionsClear()
    return bits(vx.array()).copy(), bits(k.history()).copy(), k.its, k.reason


def on_off(P, ai, aj, aa, b, pc, opts, **tol):
    on = solve(P, ai, aj, aa, b, pc, opts, **tol)
    off = solve(P, ai, aj, aa, b, pc, opts + " -ksp_cg_x_with_p 0", **tol)
    assert on[2] == off[2] and on[3] == off[3], (on[2:], off[2:])
    assert np.array_equal(on[1], off[1]), "residual history differs"
    assert np.array_equal(on[0], off[0]), "iterate differs"
    return on


@pytest.mark.parametrize("level", ["3", "4"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("norm", ["preconditioned", "natural", "unpreconditioned"])
@pytest.mark.parametrize("shape", [(41, 37), (40, 36)])          # odd and even n
def test_x_with_p_is_bit_identical(P, level, pc, norm, shape):
    ai, aj, aa = pb.lap2d(*shape)
    n = ai.size - 1
    b = np.cos(0.3 * np.arange(n)) + 0.01 * np.arange(n) / n
    x, h, its, reason = on_off(P, ai, aj, aa, b, pc, "-ksp_cg_fused %s -ksp_norm_type %s" % (level, norm), rtol=1e-9)
    assert reason == 2 and its > 20


@pytest.mark.parametrize("level", ["3", "4"])
def test_x_with_p_indefinite_and_max_it_exits(P, level):
    """KSP_DIVERGED_INDEFINITE_MAT / _PC: the device refuses the step in both kernels and x stays the previous iterate;
    KSP_DIVERGED_ITS: x after exactly max_it steps."""
    ai, aj, aa = pb.lap2d(12, 11)
    n = ai.size - 1
    aa = aa.copy()
    for row in (5, 40, 77):
        kk = ai[row] + int(np.where(aj[ai[row]:ai[row + 1]] == row)[0][0])
        aa[kk] = -3.0
    b = np.cos(0.7 * np.arange(n))
    reasons = set()
    for pc in ("none", "jacobi"):
        reasons.add(on_off(P, ai, aj, aa, b, pc, "-ksp_cg_fused " + level, rtol=1e-12, max_it=200)[3])
    assert reasons <= {-8, -10} and -10 in reasons
    ai, aj, aa = pb.lap2d(41, 37)
    b = np.sin(0.1 * np.arange(ai.size - 1))
    for pc in ("none", "jacobi"):
        _, h, its, reason = on_off(P, ai, aj, aa, b, pc, "-ksp_cg_fused " + level, rtol=1e-12, max_it=9)
        assert its == 9 and reason == -3


@pytest.mark.parametrize("level", ["3", "4"])
def test_x_with_p_convergence_right_after_a_queued_front_half(P, level):
    """A diagonal operator with two distinct eigenvalues: CG with PCNONE converges at step 2 from a residual far above 10x
    the target, so the front half of a step that never runs was queued and x came out of the AYPX."""
    n = 1001
    ai = np.arange(n + 1, dtype=np.int32)
    aj = np.arange(n, dtype=np.int32)
    aa = np.where(np.arange(n) % 3 == 0, 1.0, 4.0)
    b = 1.0 + np.cos(0.37 * np.arange(n))
    x, h, its, reason = on_off(P, ai, aj, aa, b, "none", "-ksp_cg_fused " + level, rtol=1e-8)
    assert its == 2 and reason > 0
    assert np.allclose(x.view(np.float64), b / aa, rtol=1e-12)


def test_x_with_p_at_256_mib_per_vector(P):
    """Vectors of 2^25 + 1 doubles: the streaming forms of both kernels (and the odd tail)."""
    n = BIG
    ai = np.arange(n + 1, dtype=np.int32)
    aj = np.arange(n, dtype=np.int32)
    aa = 1.0 + (np.arange(n) % 97).astype(np.float64)
    b = np.cos(0.001 * np.arange(n))
    x, h, its, reason = on_off(P, ai, aj, aa, b, "none", "", rtol=1e-12, max_it=6)
    assert its == 6 and reason == -3


def test_x_with_p_two_ranks_staged(built):
    """bench.py's two-rank rehearsal (host-staged transport): --dump-outputs with the option on and off, byte for byte."""
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, opts in (("on", ""), ("off", "-ksp_cg_x_with_p 0")):
            d = os.path.join(tmp, tag)
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--grid-n", "40",
                   "--dump-outputs", d] + (["--ksp-opts", opts] if opts else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2
            outs.append({f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))})
    assert sorted(outs[0]) == sorted(outs[1]) and any("rank1" in f for f in outs[0])
    for f in outs[0]:
        assert outs[0][f] == outs[1][f], f
