"""A sharded PSK pass executed by REAL processes on the one GPU of the test box (tests/psk_rank_driver.py): 2 and 3 ranks on device 0,
the process group over gloo, each rank with its seeded shard and the raw halo before it; rank 0 checks the stitched pieces against the
oracle over the whole capture."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3])
def test_psk_real_ranks_on_one_gpu(world):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29610 + world), os.path.join(ROOT, "tests", "psk_rank_driver.py")]
    if shutil.which("timeout"):
        cmd = ["timeout", "-k", "10", "420"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=480, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"PSK_SHARD_OK {world}" in r.stdout, (r.stdout + r.stderr)[-3000:]
