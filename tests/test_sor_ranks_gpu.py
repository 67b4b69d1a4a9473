"""MatSOR of an MPIAIJ matrix on two ranks sharing the GPU over the host-staged transport (the launcher of
tests/test_mat_zero_rows_ranks_gpu.py, on a master port of its own): tests/tools/sor_ranks.py compares every rank's x with the Python
restatement of MatSOR_MPIAIJ bit for bit, asks the refused flags, and solves with CG + sor."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_mpiaij_sor_two_staged_ranks(built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29577",
           os.path.join(root, "tests", "tools", "sor_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    its = []
    for k in range(2):
        m = re.search(r"rank %d/2: MatSOR of MPIAIJ bitexact=True cases 48 refused \[56, 56, 56, 56, 56, 56\] cg\+sor its (\d+) reason (\d+)" % k, out)
        assert m, out[-3000:]
        its.append(int(m.group(1)))
        assert int(m.group(2)) > 0
    assert its[0] == its[1] and its[0] >= 2
