"""Two ranks of the sharded search beyond the register path's limits on the box's one GPU: fresh
child processes (torch.distributed.run, gloo) each run tests/_sharded_wide_child.py — ShardedHybrid at k = 300, at 257
probes, under an allow-set, exchanges carried by the hosted transport — and compare their own results bit for bit with
the CPU oracle.

The file name sorts before every module that opens the device: the children must be started before this process has
initialised the GPU (starting another program from a process that holds the device is refused on the GPU pool), and pytest
runs the modules in name order."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu_initialised_here():
    try:
        return any("kfd" in os.readlink(f"/proc/self/fd/{fd}") for fd in os.listdir("/proc/self/fd"))
    except OSError:
        return False


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_every_rank_of_the_sharded_wide_search_matches_the_oracle(tmp_path):
    world = 2
    if _gpu_initialised_here():
        pytest.skip("this process already holds the GPU; run this module first (it sorts first by name)")
    import oracle as orc
    orc.build()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "_sharded_wide_child.py"), str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for r in range(world):
        rep = json.load(open(tmp_path / f"rank{r}.json"))
        assert rep["ok"], rep
        assert [c[0] for c in rep["checks"]] == ["weak_k300", "strong_nprobe257", "weak_allowed", "strong_tiny", "in_flight"]
    owned = [json.load(open(tmp_path / f"rank{r}.json"))["lists_owned"] for r in range(world)]
    assert sum(owned) == 300 and min(owned) > 0
