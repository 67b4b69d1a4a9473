"""fgmreshipmi355x + Jacobi on an MPIAIJ matrix of 1025 rows over two ranks, -ksp_fgmres_fused on against off (the launcher of
tests/test_lsqr_ranks_gpu.py, on master ports of its own): tests/tools/fgmres_ranks.py compares the two on every rank -- iteration count,
reason and history equal, the local x bit for bit, x of all ranks within 1e-8 of numpy.linalg.solve -- and both ranks count the same
iterations.  Two ranks sharing the GPU over the host-staged transport, where the Vec type refuses the fused entries and every step runs op
by op; and, on a box with two GPUs, one rank per GPU over RCCL, where the sums of the fused Gram-Schmidt step are all-reduced on the
device (skipped on a one-GPU box, as tests/test_rccl_multigpu.py is)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CASES = 8           # two restarts x two guesses x (a budget + a tolerance)


def run_ranks(staged, port):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if staged:
        env["MI355X_STAGED"] = "1"
    else:
        env.pop("MI355X_STAGED", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "tools", "fgmres_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    its = []
    for k in range(2):
        m = re.search(r"rank %d/2: FGMRES fused equals unfused=True transport=%s cases %d its ([\d,]+)" % (k, "staged" if staged else "rccl", CASES), out)
        assert m, out[-3000:]
        its.append(m.group(1))
    assert its[0] == its[1] and len(its[0].split(",")) == CASES


def test_fgmres_two_staged_ranks(built):
    run_ranks(True, 29603)


def test_fgmres_two_ranks_over_rccl(built):
    import petsc_dev_amd as pda
    n = C.c_int()
    pda.load_kernels().mi355x_device_count(C.byref(n))
    if n.value < 2:
        pytest.skip("needs 2 GPUs, %d visible" % n.value)
    run_ranks(False, 29607)
