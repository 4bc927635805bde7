"""The data-parallel path on the real device: `torch.distributed.run` with ONE rank per visible GPU,
backend nccl (= RCCL): process-group init bound to the device, parameter broadcast, the flat-bucket all-reduce on the
engine's gradient buffer between the fused backward and the flat Adam, barrier, teardown.  With one GPU this is the
1-rank RCCL path (the collective must be an identity); the multi-rank arithmetic is covered on CPU by
tests/test_dist_cpu.py (gloo, world_size 2).  Run with -m gpu."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, tmp_path, with_launcher=True, shards=1, backend=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WN_DIST_BACKEND", None)
    if backend:
        env["WN_DIST_BACKEND"] = backend
    worker = os.path.join(ROOT, "tests", "dist_worker_gpu.py")
    if with_launcher:
        # --standalone: torchrun picks and HOLDS the rendezvous port (no bind / close / hand-over race)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", str(nproc), worker, str(tmp_path), str(shards)]
    else:
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, worker, str(tmp_path), str(shards)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.load(open(tmp_path / "dist_gpu.json"))


def test_rccl_path_one_rank_per_gpu(tmp_path):
    n = torch.cuda.device_count()
    assert n >= 1
    plain = _run(1, tmp_path, with_launcher=False)            # no process group at all
    assert plain["backend"] == "none" and len(plain["losses"]) == 3
    if n == 1:
        # one rank under the launcher: the worker forces the process group, so init (device-bound), broadcast,
        # all_reduce on RCCL, barrier and teardown all run; a 1-rank sum is the identity, so the numbers are the plain run's
        one = _run(1, tmp_path)
        assert one["backend"] == "nccl" and one["world"] == 1
        assert one["losses"] == plain["losses"] and one["gsum"] == plain["gsum"]
    else:
        # N ranks with 2 clips each == 1 rank with the same 2N clips (DataParallel's global-batch-mean gradient):
        # losses, the reduced gradient and the parameters after 3 Adam steps agree to fp32 reduction-order noise
        whole = _run(1, tmp_path, with_launcher=False, shards=n)
        many = _run(n, tmp_path, shards=n)
        assert many["backend"] == "nccl" and many["world"] == n
        for a, b in zip(many["losses"], whole["losses"]):
            assert abs(a - b) < 2e-5, (many["losses"], whole["losses"])
        assert abs(many["gsum"] - whole["gsum"]) < 1e-3 * whole["gsum"]
        assert abs(many["psum"] - whole["psum"]) < 1e-5 * whole["psum"]


@pytest.mark.parametrize("world", [2, 3])
def test_n_ranks_equal_one_rank_with_n_times_the_batch(tmp_path, world):
    """The N-rank code path on whatever the box has: N processes, each with its own engine and its contiguous chunk of
    one global batch, one flat all-reduce per step, 1/N inside Adam - against ONE process on the same 2N clips
    (DataParallel's global-batch-mean gradient): losses, the reduced gradient and the parameters after 3 Adam steps
    agree to fp32 reduction-order noise.  With fewer GPUs than ranks the ranks share a device and the collective runs on
    gloo (RCCL refuses duplicate devices); with enough GPUs it is RCCL."""
    n = torch.cuda.device_count()
    backend = None if n >= world else "gloo"
    whole = _run(1, tmp_path, with_launcher=False, shards=world)
    many = _run(world, tmp_path, shards=world, backend=backend)
    assert many["world"] == world and many["backend"] == ("nccl" if backend is None else "gloo")
    for a, b in zip(many["losses"], whole["losses"]):
        assert abs(a - b) < 2e-5, (many["losses"], whole["losses"])
    assert abs(many["gsum"] - whole["gsum"]) < 1e-3 * whole["gsum"]
    assert abs(many["psum"] - whole["psum"]) < 1e-5 * whole["psum"]


def test_bench_two_ranks_on_this_box(tmp_path):
    """`python bench.py --gpus 2` end to end: the parent starts two ranks, they train in lock step (barrier, max-over-ranks
    time, one all-reduce per step) and rank 0 prints ONE line for the whole job.  On a 1-GPU box the two ranks share the
    device over gloo; the line then says so in `backend`."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if torch.cuda.device_count() < 2:
        env["WN_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout          # ONE JSON line on stdout, nothing else
    out = json.loads(lines[0])
    # rccl_ranks counts ranks whose collective really is RCCL: 0 when the two ranks share the device over gloo
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["rccl_ranks"] == (2 if out["backend"] == "nccl" else 0)
    assert out["backend"] == ("gloo" if torch.cuda.device_count() < 2 else "nccl")
    assert out["config"]["global_batch"] == 16 and out["config"]["parallelism"] == "dp2"
    assert "allreduce" in out["phase_ms_per_step"] and out["value"] > 0
    assert abs(out["value"] - 2 * 8 * 16000 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    # what the first real N-GPU line must carry (VERDICT r4 #4c): every rank's own time (min / max / all), the max being the
    # contract's ms_per_step, and the host-thread budget each rank ran with (quota / ranks of this host, music_amd/_lib.py)
    pr = out["ms_per_step_ranks"]
    assert len(pr["all"]) == 2 and pr["min"] <= pr["max"] and abs(pr["max"] - out["ms_per_step"]) < 1e-6 * pr["max"]
    ht = out["host_threads"]
    assert ht["local_world_size"] == 2 and ht["torch_intra_op"] >= 1
    from music_amd import _lib
    q = _lib.cpu_quota()
    if q is not None:
        assert ht["torch_intra_op"] <= _lib.thread_budget(q, 2)


def test_bench_eight_ranks_on_this_box():
    """BASELINE configs[2]'s launch shape - `python bench.py --gpus 8` - end to end on whatever the box has: eight ranks, config 2's batch
    (8 x 16000) EACH, lock step, one all-reduce per step, ONE line for the job.  With fewer than eight GPUs the ranks share devices over gloo
    (the line says so: `backend`, `rccl_ranks` 0); what is checked is everything the first real 8-GPU run depends on besides RCCL itself:
    the self-launch, the per-rank host-thread budget (quota / 8), eight per-rank times, weak-scaling bookkeeping (global batch 64)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OMP_NUM_THREADS")}
    n_gpu = torch.cuda.device_count()
    if n_gpu < 8:
        env["WN_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--settle", "2", "--full"], env=env,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["scaling"] == "weak" and out["config"]["global_batch"] == 64 and out["config"]["parallelism"] == "dp8"
    assert out["backend"] == ("gloo" if n_gpu < 8 else "nccl") and out["rccl_ranks"] == (8 if out["backend"] == "nccl" else 0)
    assert len(out["ms_per_step_ranks"]["all"]) == 8 and "allreduce" in out["phase_ms_per_step"]
    assert abs(out["value"] - 8 * 8 * 16000 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    from music_amd import _lib
    q = _lib.cpu_quota()
    ht = out["host_threads"]
    assert ht["local_world_size"] == 8 and ht["torch_intra_op"] <= _lib.thread_budget(q, 8)
    assert ht["OMP_NUM_THREADS"] == str(min(8, _lib.thread_budget(q, 8)))


def test_bench_under_launcher_prints_one_json_line_with_rccl():
    """The driver's launch form: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` (here N = 1, the
    collective really is RCCL).  RCCL prints a version banner to fd 1 when the process group comes up: stdout must
    still carry exactly ONE line, the JSON."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "WN_DIST_BACKEND")}
    # the DRIVER's launch form, verbatim (explicit master address and port)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1 and out["backend"] == "nccl" and "allreduce" in out["phase_ms_per_step"]


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """`python bench.py --gpus 1` without --full: ONE line with the headline alone (no phase table, roofline, sub-benchmarks or
    CPU baseline), exactly --steps timed steps, and --dump-outputs writes what the last timed step handed its caller - the
    loss, the flat gradient and the parameters after Adam - the same arrays from two runs with the same arguments."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    runs = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle", "2",
                            "--dump-steps", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["full"] is False and len(out["ms_per_step_stats"]["all_in_order"]) == 3
        assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"].startswith("f32")
        assert abs(out["value"] - 8 * 16000 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
        assert not set(out) & {"phase_ms_per_step", "roofline", "mfma_util", "host_enqueue_ms_per_step", "kernels", "extra",
                               "cpu_baseline", "summary"}
        a = {n: np.load(str(d / (n + ".npy"))) for n in ("loss", "grad", "params")}
        assert a["loss"].dtype == np.float64 and a["loss"].shape == (1,)
        assert abs(a["loss"][0] - out["config"]["final_loss"]) <= 1e-6 * abs(out["config"]["final_loss"])
        assert a["grad"].dtype == a["params"].dtype == np.float32 and a["grad"].ndim == 1 and a["grad"].shape == a["params"].shape
        assert np.isfinite(a["grad"]).all() and np.isfinite(a["params"]).all() and np.abs(a["grad"]).max() > 0
        assert sum(v.nbytes for v in a.values()) <= 64 << 20
        runs.append(a)
    for n in ("loss", "grad", "params"):
        x, y = runs[0][n].astype(np.float64), runs[1][n].astype(np.float64)
        assert np.abs(x - y).max() <= 1e-5 * np.abs(x).max(), n


def test_allreduce_flat_through_the_c_abi_one_rank():
    """wn_comm_unique_id / wn_comm_create / wn_allreduce_flat / wn_comm_destroy on this process's RCCL (the copy torch has loaded:
    the library resolves it from the process image): a one-rank communicator on the current device, the in-place sum of a flat
    fp32 buffer on a side stream (an identity for one rank, bit for bit), then the flat Adam step with gscale = 1 / world as
    music_amd/dist.py applies it.  More ranks need more GPUs: the N-rank arithmetic is tests/test_dist_cpu.py's (gloo)."""
    import ctypes
    from music_amd import _lib
    lib = _lib.load()
    assert lib.wn_coll_available() == 1
    torch.cuda.set_device(0)
    ident = ctypes.create_string_buffer(128)
    assert lib.wn_comm_unique_id(ident) == 0, lib.wn_last_error()
    comm = ctypes.c_void_p()
    assert lib.wn_comm_create(1, 0, ident, ctypes.byref(comm)) == 0, lib.wn_last_error()
    try:
        g = torch.randn(1_270_000, device="cuda")
        want = g.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert lib.wn_allreduce_flat(comm, g.data_ptr(), g.numel(), side.cuda_stream) == 0, lib.wn_last_error()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(g, want)
        assert lib.wn_allreduce_flat(comm, g.data_ptr(), 0, None) == 0          # empty buffer: nothing to do
        mapped = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "rccl" in ln})
        assert len(mapped) == 1, mapped                                          # ONE copy of RCCL in the process
    finally:
        assert lib.wn_comm_destroy(comm) == 0

