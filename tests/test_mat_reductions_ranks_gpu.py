"""MatNorm, MatGetRowMaxAbs / Max / Min and MatGetColumnNorms of an MPIAIJ matrix on two ranks sharing the GPU over the host-staged
transport (the launcher of tests/test_mat_zero_rows_ranks_gpu.py), both routes, against the one-rank results: tests/tools/mat_reductions_ranks.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_mpiaij_reductions_two_staged_ranks(built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29567",
           os.path.join(root, "tests", "tools", "mat_reductions_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    for k in range(2):
        m = re.search(r"rank %d/2: MPIAIJ reductions against one rank ok=True rows won by the off-diagonal block (\d+)" % k, out)
        assert m, out[-3000:]
        assert int(m.group(1)) > 0, "the run wants rows whose maximum lies in the off-diagonal block: %s" % m.group(0)
