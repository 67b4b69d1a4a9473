"""Chebyshev and Richardson on an MPIAIJ matrix over two ranks sharing the GPU over the host-staged transport (the launcher of
tests/test_sor_ranks_gpu.py, on a master port of its own): tests/tools/cheby_ranks.py compares the plug-in's types with the harness's
on every rank -- x bit for bit, the same history, iteration count and reason -- and both ranks count the same iterations."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_cheby_and_richardson_two_staged_ranks(built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355X_STAGED="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29587",
           os.path.join(root, "tests", "tools", "cheby_ranks.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    its = []
    for k in range(2):
        m = re.search(r"rank %d/2: chebychev and richardson plug-in types equal the harness types=True cases 28 its ([\d,]+)" % k, out)
        assert m, out[-3000:]
        its.append(m.group(1))
    assert its[0] == its[1] and len(its[0].split(",")) == 28
