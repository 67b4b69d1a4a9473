"""LSQR on a rectangular MPIAIJ matrix over two ranks sharing the GPU over the host-staged transport (the launcher of
tests/test_minres_ranks_gpu.py, on a master port of its own), rows and columns split: tests/tools/lsqr_ranks.py compares the plug-in's type
with the harness's on every rank -- x, the standard-error sum, arnorm and anorm bit for bit, the same history, iteration count and reason,
two bidiagonalisation sweeps and one update sweep per iteration through the all-reduced route -- and x with numpy.linalg.lstsq; both
ranks count the same iterations."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CASES = 12          # two PCs x two guesses x (two budgets + one tolerance)


def test_lsqr_two_staged_ranks(built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29597",
           os.path.join(root, "tests", "tools", "lsqr_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    its = []
    for k in range(2):
        m = re.search(r"rank %d/2: LSQR plug-in type equals the harness type=True cases %d its ([\d,]+)" % (k, CASES), out)
        assert m, out[-3000:]
        its.append(m.group(1))
    assert its[0] == its[1] and len(its[0].split(",")) == CASES
