"""The guarded optimizer step on the Python surface (music_amd/guard.py): train.get_optimizer(..., max_grad_norm, skip_nonfinite)
against torch's optimizer + clip_grad_norm_ on the same gradients, and the fused step of the three engines (adam_init(max_grad_norm,
skip_nonfinite) + loss_and_grad + adam_step) against torch.optim.Adam + clip_grad_norm_ on the engine's own gradients."""
import sys

import numpy as np
import pytest
import torch

from tests.helpers import g1_input, g1_meta, load_npz, params_from, scrambled_input

pytestmark = pytest.mark.gpu
SURFACE_BAR = 4e-6          # tests/test_gpu_parity.py: a few ulp of a step, relative to max(1, |p|max)


def _fixture():
    meta = [m for m in g1_meta() if m["name"] == "tiny_s0_g3_w130"][0]
    d = load_npz("g1_%s.npz" % meta["name"])
    return meta, d, g1_input(d, meta).cuda(), torch.from_numpy(d["target"]).cuda()


def _build(meta, d):
    from music_amd.model import wavenet
    net = wavenet(**meta["cfg"])
    net.load_state_dict(params_from(d))
    return net.cuda()


def _spy(monkeypatch):
    from music_amd import _lib
    calls, real = [], _lib.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", spy)
    for name, mod in list(sys.modules.items()):             # the engines bind the name at import (from ._lib import call)
        if name.startswith("music_amd.") and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", spy)
    return calls


def _moments(opt):
    return [v.detach().clone() for st in opt.state_dict()["state"].values() for k, v in sorted(st.items())
            if torch.is_tensor(v) and k != "step"]


@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_guarded_flat_optimizer_is_torchs_with_clip_grad_norm(kind, monkeypatch):
    from music_amd import train as T
    meta, d, x, target = _fixture()
    ce = torch.nn.CrossEntropyLoss()
    cls = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop}[kind]
    lr = 1e-2 if kind == "sgd" else 1e-3
    kw = {} if kind == "adam" else {"momentum": 0.9}
    nets = [_build(meta, d), _build(meta, d)]
    ce(nets[0](x), target).backward()
    norm0 = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in nets[0].parameters()])).item()
    max_norm = 0.5 * norm0                                  # half the typical norm: the clip is active
    flat = T.get_optimizer(nets[0], kind, lr, 0.9, max_grad_norm=max_norm, skip_nonfinite=True)
    ref = cls(nets[1].parameters(), lr=lr, **kw)
    assert isinstance(flat, cls)
    calls = _spy(monkeypatch)
    for step in range(5):
        flat.zero_grad()
        ce(nets[0](x), target).backward()
        if step == 2:                                       # a poisoned gradient, in place: still the one flat gradient buffer
            next(iter(nets[0].parameters())).grad.view(-1)[0] = float("inf")
            before = [p.detach().clone() for p in nets[0].parameters()], _moments(flat)
            flat.step()
            after = [p.detach().clone() for p in nets[0].parameters()], _moments(flat)
            assert len(before[1]) == len(after[1]) > 0
            assert all(torch.equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1]))
            continue
        for p0, p1 in zip(nets[0].parameters(), nets[1].parameters()):
            p1.grad = p0.grad.clone()                       # the SAME gradients to both (see test_flat_sgd_and_rmsprop_...)
        torch.nn.utils.clip_grad_norm_(nets[1].parameters(), max_norm)
        flat.step()
        ref.step()
    entry = {"adam": "wn_adam_flat", "sgd": "wn_sgd_flat", "rmsprop": "wn_rmsprop_flat"}[kind]
    assert calls.count("wn_grad_guard") == 5 and calls.count(entry + "_guarded") == 5 and calls.count(entry) == 0
    worst = 0.0
    for (n, a), (_, b) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        e = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
        worst = max(worst, e)
        assert e <= SURFACE_BAR, (n, e)
    rep = flat.guard_report()
    print(kind, "worst relative difference %.3g" % worst, rep)
    assert (rep["taken"], rep["skipped"], rep["clipped"]) == (4, 1, 4)
    sd = flat.state_dict()
    if kind != "sgd":
        assert float(sd["state"][0]["step"]) == 4.0         # taken steps only
    plain = cls(nets[1].parameters(), lr=lr, **kw)
    plain.load_state_dict(sd)                               # torch's own class takes it
    flat.load_state_dict(ref.state_dict())                  # ... and the guarded one takes torch's; the device count is re-seeded
    flat.zero_grad()
    ce(nets[0](x), target).backward()
    flat.step()
    if kind != "sgd":
        assert float(flat.state_dict()["state"][0]["step"]) == 5.0
    assert all(torch.isfinite(p).all() for p in nets[0].parameters())


@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_options_unset_launch_what_they_launched(kind, monkeypatch):
    from music_amd import train as T
    meta, d, x, target = _fixture()
    net = _build(meta, d)
    opt = T.get_optimizer(net, kind, 1e-3, 0.9)
    calls = _spy(monkeypatch)
    for _ in range(2):
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(net(x), target).backward()
        opt.step()
    entry = {"adam": "wn_adam_flat", "sgd": "wn_sgd_flat", "rmsprop": "wn_rmsprop_flat"}[kind]
    assert calls.count(entry) == 2 and not [c for c in calls if "guard" in c]
    assert opt.guard_report() is None


def _wavenet_engine():
    meta, d, x, target = _fixture()
    net = _build(meta, d)
    return net, net._engine_for(x.device), lambda eng: eng.loss_and_grad(x, target)


def _general_engine():
    from music_amd.model import wavenet
    torch.manual_seed(3)
    net = wavenet(filter_width=3, dilations=[1, 2, 4], dilation_channels=32, residual_channels=32, skip_channels=32,
                  quantization_channels=256, use_bias=True)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    net = net.cuda()
    rng = np.random.default_rng(4)
    B, W = 2, 100
    x = scrambled_input(rng.integers(0, 256, size=(B, net.receptive_field + W - 1))).cuda()
    target = torch.from_numpy(rng.integers(0, 256, size=(B * W,)).astype(np.int64)).cuda()
    return net, net._engine_for(x.device), lambda eng: eng.loss_and_grad(x, target)


def _autoencoder_engine():
    from music_amd.model1 import wavenet_autoencoder
    from oracle import intops
    cfg = dict(filter_width=2, quantization_channel=256, dilations=[1, 2, 4, 8, 3], en_residual_channel=60,
               en_dilation_channel=52, en_bottleneck_width=10, en_pool_kernel_size=40, de_residual_channel=64,
               de_dilation_channel=60, de_skip_channel=72, use_bias=True)
    torch.manual_seed(72)
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    net = net.cuda()
    rng = np.random.default_rng(71)
    B, W = 2, 333
    idx = rng.integers(0, 256, size=(B, net.receptive_field + W - 1))
    x = torch.from_numpy(np.stack([intops.one_hot_proper(r) for r in idx])).cuda()
    target = torch.from_numpy(rng.integers(0, 256, size=(B * W,)).astype(np.int64)).cuda()

    def step(eng):
        torch.manual_seed(73)
        return eng.loss_and_grad(x, target, net._draw_conditioning())
    return net, net._engine_for(x.device), step


@pytest.mark.parametrize("make", [_wavenet_engine, _general_engine, _autoencoder_engine], ids=["wavenet", "general_fw3", "autoencoder"])
def test_guarded_fused_step(make, monkeypatch):
    """Three guarded fused steps equal torch.optim.Adam + clip_grad_norm_ fed the engine's own gradients; a poisoned flat_grad leaves
    flat, m, v bit for bit and is counted as skipped, and adam_state["t"] follows the steps taken."""
    net, eng, loss_and_grad = make()
    loss_and_grad(eng)
    max_norm = 0.5 * eng.flat_grad.double().norm().item()
    eng.adam_init(lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=True)
    q = eng.flat.detach().clone().requires_grad_(True)
    ref = torch.optim.Adam([q], lr=1e-3)
    calls = _spy(monkeypatch)
    for step in range(4):
        loss_and_grad(eng)
        if step == 1:
            eng.flat_grad[eng.spec.total // 2] = float("inf")
            s = eng.adam_state
            before = [eng.flat.clone(), s["m"].clone(), s["v"].clone()]
            eng.adam_step()
            assert all(torch.equal(a, b) for a, b in zip(before, [eng.flat, s["m"], s["v"]]))
            continue
        q.grad = eng.flat_grad.detach().clone()
        torch.nn.utils.clip_grad_norm_([q], max_norm)
        eng.adam_step()
        ref.step()
    assert calls.count("wn_grad_guard") == 4 and calls.count("wn_adam_flat_guarded") == 4 and calls.count("wn_adam_flat") == 0
    e = (eng.flat - q.detach()).abs().max().item() / max(1.0, q.detach().abs().max().item())
    print("worst relative difference %.3g" % e)
    assert e <= SURFACE_BAR
    assert eng.adam_state["t"] == 4                         # steps issued, until the report ...
    rep = eng.guard_report()
    assert (rep["taken"], rep["skipped"], rep["clipped"]) == (3, 1, 3) and eng.adam_state["t"] == 3
    # the parameters are views of the flat buffer: the module saw the three steps
    assert all(torch.isfinite(p).all() for p in net.parameters())
    # unset: the step is the one plain launch, and there is nothing to report
    eng.adam_init(lr=1e-3)
    del calls[:]
    loss_and_grad(eng)
    eng.adam_step()
    assert calls.count("wn_adam_flat") == 1 and not [c for c in calls if "guard" in c] and eng.guard_report() is None


F16_W = 50           # the smallest length that overflows: the encoding cannot be pooled by 50 below it, and 50 / 100 / 200 / 400 all overflow


def test_f16_range_overflow_is_skipped_and_reported(tmp_path, capsys):
    """The autoencoder of tests/test_gpu_parity.py::test_autoencoder_bf16_forward_survives_activations_beyond_f16 (encoder blocks x 12: the
    residual stream passes f16's 65504, the default f16x3 forward returns NaN gradients).  One train()-style fused step with
    skip_nonfinite: the parameters stay finite and unchanged, guard_log.log counts the skip, and the warning names a tensor and the
    bf16 pair.  That test's shape at the shortest clip the model takes (F16_W output samples: one pooled frame of encoding)."""
    from music_amd import guard
    from music_amd.model1 import wavenet_autoencoder
    from oracle import intops
    cfg = dict(filter_width=2, quantization_channel=256, dilations=[1, 2, 4, 8, 16, 32, 3], en_residual_channel=64, en_dilation_channel=64,
               en_bottleneck_width=16, en_pool_kernel_size=50, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256, use_bias=False)
    torch.manual_seed(11)
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
        for n, p in net.named_parameters():
            if n.startswith("en_dilation_layer_stack"):
                p.mul_(12.0)
        net.bottleneck_layer.weight.mul_(12.0 ** -4)
    net = net.cuda()
    rng = np.random.default_rng(12)
    B, W = 2, F16_W
    idx = rng.integers(0, 256, size=(B, net.receptive_field + W - 1))
    x = torch.from_numpy(np.stack([intops.one_hot_proper(r) for r in idx])).cuda()
    target = torch.from_numpy(rng.integers(0, 256, size=(B * W,)).astype(np.int64)).cuda()
    eng = net._engine_for(x.device)
    eng.adam_init(lr=1e-3, skip_nonfinite=True)
    before = eng.flat.clone()
    log = guard.GuardLog(str(tmp_path / "guard_log.log"), eng.guard_report, lambda: guard.engine_named_grads(eng))
    torch.manual_seed(77)
    eng.loss_and_grad(x, target, net._draw_conditioning())
    eng.adam_step()
    rep = log.tick(1)
    print(rep)
    assert rep["skipped"] == 1 and rep["taken"] == 0 and rep["nonfinite"] > 0
    assert torch.equal(eng.flat, before) and bool(torch.isfinite(eng.flat).all())
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert open(tmp_path / "guard_log.log").read().endswith("clipped 0,skipped 1\n")
    err = capsys.readouterr().err
    assert "was skipped" in err and guard.BF16_HINT in err and any(n in err for n in eng.param_names)


DP_CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16,
              quantization_channels=256, use_bias=False)


def _write_dp_run(tmp, extra):
    import json
    import os
    import pickle
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    data = [rng.integers(0, 256, size=(l,)).astype(np.int32) for l in (900, 700)]            # 24 pieces: six global batches of 4
    pickle.dump(data, open(tmp / "np_audio.pkl", "wb"))
    dp = dict(batch_size=4, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_audio.pkl"), receptive_field=17,
              window_length=100, cuda_available=False, quantization_channels=256)
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=1, print_every=6, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3, **extra)
    for n, p in (("wavenet", DP_CFG), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))


def _run_train(nproc, workdir, poison_step, omit_step):
    """One subprocess call with a timeout, as tests/test_gpu_dist.py::_run starts its ranks."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "WN_DIST_BACKEND"):
        env.pop(k, None)
    worker = [os.path.join(root, "tests", "guard_dist_worker.py"), str(workdir), str(poison_step), str(omit_step)]
    if nproc > 1:
        if torch.cuda.device_count() < nproc:
            env["WN_DIST_BACKEND"] = "gloo"                 # the ranks share the one GPU (RCCL refuses duplicate devices)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", str(nproc)] + worker
    else:
        cmd = [sys.executable] + worker
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "autograd"])
def test_train_two_ranks_skip_the_same_step(tmp_path, fused):
    """train() with both keys on 2 ranks (gloo on one GPU), rank 1's gradient poisoned on global step 2 of 6: the guard runs after the
    all-reduce, so both ranks skip that step and end bit-identical; rank 0 alone reports (one guard_log.log line with one skipped
    step, one warning); and the parameters are those of ONE rank on the same global batches, same keys, that simply leaves the
    optimizer step of global step 2 out - at the bar of tests/test_gpu_dist.py::test_n_ranks_equal_one_rank_with_n_times_the_batch."""
    keys = {"fused_step": fused, "max_grad_norm": 0.01, "skip_nonfinite": True}       # (the gradient norm is 0.02: the clip acts)
    two, one = tmp_path / "two", tmp_path / "one"
    for d in (two, one):
        d.mkdir()
        _write_dp_run(d, keys)
    err = _run_train(2, two, 2, -1)
    _run_train(1, one, -1, 2)
    p0, p1, ref = (torch.load(d / f) for d, f in ((two, "params_rank0.pt"), (two, "params_rank1.pt"), (one, "params_rank0.pt")))
    assert list(p0) == list(p1) == list(ref)
    assert all(torch.equal(p0[k], p1[k]) for k in p0)                       # the same decision on the same bytes
    assert all(bool(torch.isfinite(v).all()) for v in p0.values())
    lines = open(two / "log" / "guard_log.log").read().splitlines()
    print(lines, open(one / "log" / "guard_log.log").read().splitlines())
    assert len(lines) == 1 and lines[0].startswith("Trained over 6 pieces,") and lines[0].endswith(",skipped 1")
    assert open(one / "log" / "guard_log.log").read().splitlines()[0].endswith(",skipped 0")
    assert ",clipped 0," not in lines[0]
    assert err.count("a training step was skipped") == 1                    # rank 0 only, once
    la, lb = (open(d / "log" / "loss_log.log").read().strip().split("\n") for d in (one, two))
    assert len(la) == len(lb) == 1 and abs(float(la[0].split(' ')[-1]) - float(lb[0].split(' ')[-1])) < 2e-5
    psum = lambda p: sum(float(v.double().abs().sum()) for v in p.values())
    worst = max((p0[k] - ref[k]).abs().max().item() for k in p0)
    print("psum %.9g against %.9g, worst element %.3g" % (psum(p0), psum(ref), worst))
    assert abs(psum(p0) - psum(ref)) < 1e-5 * psum(ref)
