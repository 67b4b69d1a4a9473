"""MatZeroRows of an MPIAIJ matrix on two ranks sharing the GPU over the host-staged transport (the launcher of
tests/test_mat_value_ops_gpu.py::test_mpiaij_two_staged_ranks): every rank lists rows the other owns as well as its own."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_mpiaij_zero_rows_two_staged_ranks(built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29563",
           os.path.join(root, "tests", "tools", "zero_rows_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    for k in range(2):
        m = re.search(r"rank %d/2: MatZeroRows of MPIAIJ then MatMult and b bitexact=True rows listed (\d+) owned by others (\d+) MatZeroRowsColumns 56" % k, out)
        assert m, out[-3000:]
        assert 0 < int(m.group(2)) < int(m.group(1)), "the run wants every rank to list rows of both owners: %s" % m.group(0)
