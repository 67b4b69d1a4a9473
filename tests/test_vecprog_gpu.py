"""Random call programs (tests/vecprog.py) on the device against the host model: every program runs with the noted operations off,
on, and on with everything noted run after each call.  The three runs agree bit for bit in every scalar and every final vector (the
matrices' values are read by the programs' last products), and agree bit for bit with the model: the element-wise kernels, the fused
sweeps and the scaled product claim the separate calls' bits, and the oracle sums every reduction kind in the device's order
(orc.device_reduction_order); only a reduction over a borrower that starts at an odd entry of its parent -- a pointer the oracle's
tree does not know -- is held to the worst-case bound of any summation order instead (vecprog.Model.bound).  The shortcuts are
counted: over the whole list each one is taken with the noting on and none with it off.  A failing program is reported with its
shortest failing prefix.  The programs' Vec calls and MatMult also run on two ranks over the host-staged transport."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import vecprog as vp

pytestmark = pytest.mark.gpu
CHUNK = 32
CHUNKS = [vp.SEEDS[k:k + CHUNK] for k in range(0, len(vp.SEEDS), CHUNK)]
_DONE = {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def run_chunk(P, k):
    """every program of a chunk in the three modes, one mode after the other so that the shortcuts can be counted per mode;
    kept, so that the count over the whole list runs nothing twice"""
    if k in _DONE:
        return _DONE[k]
    L = P.lib()
    setdef = L.raw("VecHIPMI355XSetDeferral")
    progs = [vp.generate(i) for i in CHUNKS[k]]
    runs, counts, t0 = [], [], time.perf_counter()
    try:
        for on, fl in ((0, False), (1, False), (1, True)):
            setdef(on)
            L.VecHIPMI355XSetCGUpdateTiming(1)
            before = vp.deferral_counts(P)
            runs.append([vp.execute(P, p, flush_each=fl) for p in progs])
            nl = C.c_int(); L.VecHIPMI355XGetCGUpdateTiming(C.byref(nl), None)
            L.VecHIPMI355XSetCGUpdateTiming(0)
            counts.append((vp.deferral_counts(P) - before, nl.value))
    finally:
        setdef(-1)
    print("chunk %d: %d programs, three runs each, %.2f s; shortcuts with the noting on: %s" % (k, len(progs), time.perf_counter() - t0, dict(zip(vp.COUNTERS, counts[1][0]))))
    _DONE[k] = (progs, runs, counts)
    return _DONE[k]


@pytest.mark.parametrize("k", range(len(CHUNKS)))
def test_programs_agree_in_three_modes_and_with_the_model(P, k):
    progs, runs, counts = run_chunk(P, k)
    for j, p in enumerate(progs):
        ref_out, ref_vecs, model = vp.reference(p)
        ok = all(vp.same(r[j][0], runs[0][j][0]) and vp.same_scalars(r[j][0], model) and len(r[j][1]) == len(ref_vecs) and all(vp.same(u, w) for u, w in zip(r[j][1], ref_vecs)) for r in runs)
        if not ok:
            why = vp.disagreement(P, p) or "the three runs and the model disagree only inside the whole list (state left by an earlier program)"
            pytest.fail(vp.explain(P, p, why), pytrace=False)
    assert not counts[0][0].any() and counts[0][1] == 0, "a shortcut was taken with the noting off: %s" % (counts[0],)
    assert counts[1][0][0] == counts[1][1], "fused CG sweeps counted %d, timed %d" % (counts[1][0][0], counts[1][1])


def test_every_shortcut_is_taken_over_the_whole_list(P):
    on = sum(run_chunk(P, k)[2][1][0] for k in range(len(CHUNKS)))
    off = sum(run_chunk(P, k)[2][0][0] for k in range(len(CHUNKS)))
    print("shortcuts over %d programs: %s" % (len(vp.SEEDS), dict(zip(vp.COUNTERS, on))))
    assert np.all(on > 0), dict(zip(vp.COUNTERS, on))
    assert not off.any(), dict(zip(vp.COUNTERS, off))


def test_two_staged_ranks(built):
    """the programs' Vec calls and MatMult on an MPIAIJ matrix, two ranks sharing the GPU over the host-staged transport (noted
    products are off there: the Vec notes under the host all-reduce): tests/tools/vecprog_ranks.py compares noting on with noting
    off bit for bit on every rank, and each rank's slice of the final vectors with the sequential model, whose MatMult is formed in
    MatMult_MPIAIJ's order (no row loop over all columns gives those bits)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29583",
           os.path.join(root, "tests", "tools", "vecprog_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    for k in range(2):
        m = re.search(r"rank %d/2: %d programs, noting on == off: True, slices == model: True, fused sweeps (\d+)" % (k, len(vp.RANK_SEEDS)), out)
        assert m and int(m.group(1)) > 0, out[-6000:]
