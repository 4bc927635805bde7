"""EMA codebook updates under data parallelism (tests/vq_ema_dist_worker.py, started in the manner of tests/test_gpu_dist.py): two
ranks over gloo sharing the one GPU, three ae_train-style fused steps on different shards - one of them empty on rank 1.  The update
is a function of the summed stat, the state and the scalars alone, so both ranks must hold bit-identical codebooks and running states
with no broadcast; the counts of the summed stat add up to the global number of frames.  Run with -m gpu."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240      # seconds, each child's own


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_hold_bit_identical_codebooks_and_states(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT, WN_DIST_BACKEND="gloo", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    worker = os.path.join(ROOT, "tests", "vq_ema_dist_worker.py")
    # each rank under a time limit of its own: a rank that hangs in a collective ends there, and takes its peer with it below
    procs = [subprocess.Popen(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, worker, str(tmp_path)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in (0, 1)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=CHILD_TIMEOUT + 30)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d ended with %s\n%s" % (r, p.returncode, out[-4000:])
    a, b = (torch.load(tmp_path / ("vq_ema_rank%d.pt" % r)) for r in (0, 1))
    for k in ("codebook", "state", "flat"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "the ranks differ in %s" % k
        assert bool(torch.isfinite(a[k]).all())
    frames = a["frames_per_rank"]
    assert a["counts"] == b["counts"] == [2.0 * frames, 1.0 * frames, 2.0 * frames]      # (rank 1's shard of step 2 was empty)
    assert a["restarted"] == b["restarted"] > 0
    K = a["codebook"].shape[0]
    assert bool((a["state"][:K] != 1.0).any())               # the state moved
