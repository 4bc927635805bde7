"""The EMA shadow weights on the device (music_amd/ema.py, wn_ema_flat in music_amd/csrc/wn_guard.hip): the kernel against the float64
recurrence of tests/ema_ref.py (whose docstring derives the bound), plain and behind a real wn_grad_guard; the three flat
optimizers and the three engines' fused step against a twin without EMA; swapped(); train() with its .ema checkpoints and a bit-exact
resume; two ranks."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from music_amd import _lib
from music_amd._lib import call, ptr
from tests.ema_ref import Ref64, kernel_w
from tests.helpers import g1_input, g1_meta, load_npz, params_from, scrambled_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                 # NaN canaries in front of and behind every buffer (a multiple of 4: the base keeps its alignment)
NAN = float("nan")


def _framed(values, misalign):
    """float32 numpy -> (whole device buffer, its host copy, first element): the values between NaN canaries, their base 16-byte
    aligned (misalign 0) or 4 bytes behind such a base (misalign 1)."""
    n = values.size
    host = np.full(PAD + misalign + n + PAD, NAN, dtype=np.float32)
    host[PAD + misalign:PAD + misalign + n] = values
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, host, PAD + misalign


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _launch(ema, e0, p, p0, n, decay, warmup, t, state=None):
    call("wn_ema_flat", ptr(ema, e0), ptr(p, p0), n, decay, 1 if warmup else 0, t, state, _lib.stream())


# decay without warm-up, then the warm-up at t = 1 (d_eff 2/11), 5 (6/15) and 10^6 (the decay itself again)
WEIGHTS = [(0.5, False, 1), (0.999, False, 7), (0.9999, False, 1), (0.9999, True, 1), (0.9999, True, 5), (0.999, True, 10 ** 6)]


@pytest.mark.parametrize("n", [1, 3, 255, 1025, 100003])
def test_kernel_against_float64(n):
    rng = np.random.default_rng(n)
    worst = 0.0
    for ma_e in (0, 1):
        for ma_p in (0, 1):
            e_val = rng.standard_normal(n).astype(np.float32)
            p_val = (e_val + rng.standard_normal(n) * rng.choice([1e-3, 1.0], size=n)).astype(np.float32)
            for decay, warmup, t in WEIGHTS:
                w = kernel_w(decay, warmup, t)
                ref = Ref64(e_val).step(p_val, w)
                outs = []
                for _ in range(2):                          # the same launch into fresh buffers: the same bits
                    ema, e_host, e0 = _framed(e_val, ma_e)
                    p, p_host, p0 = _framed(p_val, ma_p)
                    assert ptr(ema, e0) % 16 == 4 * ma_e and ptr(p, p0) % 16 == 4 * ma_p
                    _launch(ema, e0, p, p0, n, decay, warmup, t)
                    got = ema.cpu().numpy()
                    assert np.array_equal(_bits(p.cpu().numpy()), _bits(p_host))                     # p and its canaries: untouched
                    assert np.array_equal(_bits(got[:e0]), _bits(e_host[:e0])) and np.array_equal(_bits(got[e0 + n:]), _bits(e_host[e0 + n:]))
                    outs.append(got[e0:e0 + n])
                assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
                worst = max(worst, ref.check(outs[0], (n, ma_e, ma_p, decay, warmup, t)))
    if n > 1:
        assert not np.array_equal(outs[0], e_val)
    print("n %d: worst error / bound %.3g" % (n, worst))


def test_kernel_over_many_steps_sums_the_bounds():
    """40 updates with the warm-up running (T = 1 .. 40) towards moving parameters: the bound is the sum of the per-step bounds."""
    n, decay = 1025, 0.99
    rng = np.random.default_rng(2)
    e_val = rng.standard_normal(n).astype(np.float32)
    ema, _, e0 = _framed(e_val, 1)
    ref = Ref64(e_val)
    p_val = e_val.copy()
    for t in range(1, 41):
        p_val = (p_val + 0.05 * rng.standard_normal(n)).astype(np.float32)
        p, _, p0 = _framed(p_val, 0)
        _launch(ema, e0, p, p0, n, decay, True, t)
        ref.step(p_val, kernel_w(decay, True, t))
    print("40 steps: worst error / bound %.3g" % ref.check(ema.cpu().numpy()[e0:e0 + n]))


def test_kernel_follows_a_real_guard():
    """The state block written by wn_grad_guard itself: a gradient with an inf and skip_nonfinite set leaves the shadow bit for bit; a
    finite one with n_taken seeded to 4 is update T = 5 (d_eff = 6 / 15) at offset 0 and T = 105 at offset 100."""
    from music_amd.guard import GradGuard
    n, decay = 1025, 0.9999
    rng = np.random.default_rng(3)
    e_val, p_val = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
    bad = g.clone()
    bad[n // 2] = float("inf")
    gd = GradGuard(torch.device(DEV), None, True)
    p, p_host, p0 = _framed(p_val, 1)
    ema, e_host, e0 = _framed(e_val, 0)
    gd.seed_taken(4)
    gd.run(ptr(bad), n)
    _launch(ema, e0, p, p0, n, decay, True, 0, gd.state_ptr())
    rep = gd.report()
    assert (rep["skipped"], rep["taken"]) == (1, 4)
    assert np.array_equal(_bits(ema.cpu().numpy()), _bits(e_host))
    for offset, T, d_eff in ((0, 5, 6.0 / 15.0), (100, 105, 106.0 / 115.0)):
        ema, e_host, e0 = _framed(e_val, 0)
        gd.seed_taken(4)
        gd.run(ptr(g), n)
        _launch(ema, e0, p, p0, n, decay, True, offset, gd.state_ptr())
        assert gd.report()["taken"] == 5
        w = kernel_w(decay, True, T)
        assert w == np.float32(1.0) - np.float32(d_eff)
        got = ema.cpu().numpy()
        Ref64(e_val).step(p_val, w).check(got[e0:e0 + n], offset)
        assert np.array_equal(_bits(got[:e0]), _bits(e_host[:e0])) and np.array_equal(_bits(got[e0 + n:]), _bits(e_host[e0 + n:]))
        # ... and that is not what the neighbouring update numbers give
        assert not np.array_equal(got[e0:e0 + n], (e_val + kernel_w(decay, True, T + 1) * (p_val - e_val)).astype(np.float32))
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(p_host))


# ---------------------------------------------------------------- the optimizers and the engines
def _spy(monkeypatch):
    calls, real = [], _lib.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", spy)
    for name, mod in list(sys.modules.items()):             # the engines bind the name at import (from ._lib import call)
        if name.startswith("music_amd.") and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", spy)
    return calls


def _fixture():
    meta = [m for m in g1_meta() if m["name"] == "tiny_s0_g3_w130"][0]
    d = load_npz("g1_%s.npz" % meta["name"])
    return meta, d, g1_input(d, meta).cuda(), torch.from_numpy(d["target"]).cuda()


def _build(meta, d):
    from music_amd.model import wavenet
    net = wavenet(**meta["cfg"])
    net.load_state_dict(params_from(d))
    return net.cuda()


def _state_bits(opt):
    return [v.detach().clone().view(torch.int32) for st in opt.state_dict()["state"].values() for k, v in sorted(st.items())
            if torch.is_tensor(v) and k != "step"]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_flat_optimizers_keep_the_shadow(kind, guarded, monkeypatch):
    """Four steps of get_optimizer(..., ema_decay) beside a twin without: parameters and optimizer state bit for bit, the shadow
    within the bound of the float64 recurrence over the parameters after each step, one wn_ema_flat per step."""
    from music_amd import train as T
    meta, d, x, target = _fixture()
    ce = torch.nn.CrossEntropyLoss()
    nets = [_build(meta, d), _build(meta, d)]
    gk = dict(max_grad_norm=0.01, skip_nonfinite=True) if guarded else {}
    decay, lr = 0.9, (1e-2 if kind == "sgd" else 1e-3)
    opt = T.get_optimizer(nets[0], kind, lr, 0.9, ema_decay=decay, ema_warmup=True, **gk)
    twin = T.get_optimizer(nets[1], kind, lr, 0.9, **gk)
    ref = Ref64(torch.cat([p.detach().reshape(-1) for p in nets[0].parameters()]).cpu().numpy())
    calls = _spy(monkeypatch)
    for step in range(1, 5):
        for net, o in zip(nets, (opt, twin)):
            o.zero_grad()
            ce(net(x), target).backward()
            o.step()
        ref.step(nets[0]._engine.flat.cpu().numpy(), kernel_w(decay, True, step))
    entry = {"adam": "wn_adam_flat", "sgd": "wn_sgd_flat", "rmsprop": "wn_rmsprop_flat"}[kind] + ("_guarded" if guarded else "")
    assert calls.count("wn_ema_flat") == 4 and calls.count(entry) == 8
    assert _equal([p.detach().view(torch.int32) for p in nets[0].parameters()], [p.detach().view(torch.int32) for p in nets[1].parameters()])
    assert _equal(_state_bits(opt), _state_bits(twin)) and len(_state_bits(opt)) > 0
    sh = opt.ema
    assert sh.flat is not None and all(t.data_ptr() == sh.flat.data_ptr() + 4 * nets[0]._engine.spec.off[n] for n, t in sh.state_dict().items())
    assert list(sh.state_dict()) == list(nets[0].state_dict())
    print(kind, "worst error / bound %.3g" % ref.check(sh.flat.cpu().numpy()), "updates", sh.updates(opt._guard))
    assert sh.updates(opt._guard) == 4 and not torch.equal(sh.flat, nets[0]._engine.flat)


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
    B, W = 2, 64
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


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("make", [_wavenet_engine, _general_engine, _autoencoder_engine], ids=["wavenet", "general_fw3", "autoencoder"])
def test_fused_step_keeps_the_shadow(make, guarded, monkeypatch):
    """Four fused steps with adam_init(ema_decay=...) beside a twin engine without: flat, m, v bit for bit, the shadow within the
    bound, one wn_ema_flat per step; guarded, a poisoned gradient on the third step leaves the shadow bit for bit and does not
    count."""
    (_, a, step_a), (_, b, step_b) = make(), make()
    gk = dict(max_grad_norm=0.01, skip_nonfinite=True) if guarded else {}
    decay = 0.9
    a.adam_init(lr=1e-3, ema_decay=decay, ema_warmup=True, **gk)
    b.adam_init(lr=1e-3, **gk)
    assert b.ema is None and torch.equal(a.ema.flat, a.flat) and a.ema.flat.data_ptr() != a.flat.data_ptr()
    ref = Ref64(a.flat.cpu().numpy())
    calls = _spy(monkeypatch)
    taken = 0
    for step in range(4):
        for eng, fn in ((a, step_a), (b, step_b)):
            fn(eng)
            if guarded and step == 2:
                eng.flat_grad[eng.spec.total // 2] = float("inf")
        before = a.ema.flat.clone()
        a.adam_step()
        b.adam_step()
        if guarded and step == 2:
            assert torch.equal(before.view(torch.int32), a.ema.flat.view(torch.int32))
            continue
        taken += 1
        ref.step(a.flat.cpu().numpy(), kernel_w(decay, True, taken))
    assert calls.count("wn_ema_flat") == 4 and calls.count("wn_adam_flat_guarded" if guarded else "wn_adam_flat") == 8
    for u, v in ((a.flat, b.flat), (a.adam_state["m"], b.adam_state["m"]), (a.adam_state["v"], b.adam_state["v"])):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    print("worst error / bound %.3g" % ref.check(a.ema.flat.cpu().numpy()))
    assert a.ema.updates(a.adam_state.get("guard")) == taken == (3 if guarded else 4)
    assert list(a.ema.state_dict()) == a.param_names


def test_swapped_on_the_device():
    """Inside swapped() the module computes with the shadow: its forward is, bit for bit, that of a fresh module loaded from
    opt.ema.state_dict(), its greedy generation the same codes; after exit the forward is what it was before."""
    from music_amd import fast_generate as fg
    from music_amd import train as T
    meta, d, x, target = _fixture()
    net = _build(meta, d)
    opt = T.get_optimizer(net, "adam", 1e-2, 0.9, ema_decay=0.5)
    ce = torch.nn.CrossEntropyLoss()
    for _ in range(3):
        opt.zero_grad()
        ce(net(x), target).backward()
        opt.step()
    fresh = _build(meta, d)
    fresh.load_state_dict(opt.ema.state_dict())
    start = x[:1, :, :net.receptive_field].contiguous()
    with torch.no_grad():
        before = net(x).clone()
        want = fresh(x).clone()
        want_codes = fg.generate_codes(fresh, start, 24)
        with opt.ema.swapped(net):
            inside = net(x).clone()
            codes = fg.generate_codes(net, start, 24)
            with pytest.raises(RuntimeError, match="swapped"):
                opt.step()
        after = net(x).clone()
    assert torch.equal(inside.view(torch.int32), want.view(torch.int32)) and torch.equal(codes, want_codes)
    assert torch.equal(after.view(torch.int32), before.view(torch.int32)) and not torch.equal(inside, before)
    assert all(torch.equal(p, q) for p, q in zip(fresh.parameters(), opt.ema.state_dict().values()))


# ---------------------------------------------------------------- train()
CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16,
           quantization_channels=256, use_bias=False)


def _write_run(tmp, extra):
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    data = [rng.integers(0, 256, size=(l,)).astype(np.int32) for l in (417, 417)]                # 8 pieces: two batches of 4
    pickle.dump(data, open(tmp / "np_audio.pkl", "wb"))
    dp = dict(batch_size=4, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_audio.pkl"), receptive_field=17,
              window_length=100, cuda_available=False, quantization_channels=256)
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=1, print_every=2, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3)
    tp.update(extra)
    for n, p in (("wavenet", CFG), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))
    return tp


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "autograd"])
def test_train_writes_the_shadow_and_resumes_bit_for_bit(tmp_path, monkeypatch, fused, guarded):
    """train() for two epochs: wavenet{N}.ema beside every wavenet{N}.model, loadable by load_model and different from the model;
    1 + 1 epochs with "save_optimizer_state" end in the same wavenet2.ema and wavenet2.model, bit for bit, as 2 straight (the warm-up
    is on: the count of updates has to survive too)."""
    from music_amd import train as T
    from music_amd.model import wavenet

    def ctor(**kw):
        net = wavenet(**kw)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
        return net
    extra = {"fused_step": fused, "save_optimizer_state": True, "ema_decay": 0.9, "ema_warmup": True}
    if guarded:
        extra.update(max_grad_norm=0.01, skip_nonfinite=True)
    finals = {}
    for mode in ("straight", "resumed"):
        root = tmp_path / mode
        os.makedirs(root)
        tp = _write_run(root, dict(extra, num_epochs=2 if mode == "straight" else 1))
        monkeypatch.chdir(root)
        monkeypatch.setattr(T, "wavenet", ctor)
        torch.manual_seed(0)
        T.train()
        if mode == "resumed":
            assert sorted(os.listdir(root / "restore")) == ["wavenet1.ema", "wavenet1.model", "wavenet1.opt"]
            assert torch.load(root / "restore" / "wavenet1.opt")["ema_updates"] == 2
            json.dump(dict(tp, restore_model="wavenet1.model"), open(root / "params" / "train_params.json", "w"))
            T.train()
        assert torch.load(root / "restore" / "wavenet2.opt")["ema_updates"] == 4
        finals[mode] = [torch.load(root / "restore" / ("wavenet2" + s)) for s in (".ema", ".model")]
    for a, b in zip(finals["straight"], finals["resumed"]):
        assert list(a) == list(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    shadow, model = finals["straight"]
    assert list(shadow) == list(model) and any(not torch.equal(shadow[k], model[k]) for k in model)
    net = T.load_model(wavenet(**CFG), str(tmp_path / "straight" / "restore") + "/", "wavenet2.ema")
    assert net is not None and all(torch.equal(p, shadow[k]) for k, p in net.state_dict().items())


def test_two_ranks_keep_the_same_shadow(tmp_path):
    """train() on two ranks (gloo on one GPU, as tests/test_gpu_dist.py starts them), guarded fused step with the warm-up on, rank 1's
    gradient poisoned on the second of four global steps: both ranks skip it, and their shadows are bit-equal - and three updates
    old."""
    _write_run(tmp_path, {"fused_step": True, "ema_decay": 0.9, "ema_warmup": True, "max_grad_norm": 0.01, "skip_nonfinite": True,
                          "num_epochs": 2})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "WN_DIST_BACKEND"):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env["WN_DIST_BACKEND"] = "gloo"                     # the ranks share the one GPU (RCCL refuses duplicate devices)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", "2",
           os.path.join(root, "tests", "ema_dist_worker.py"), str(tmp_path), "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    s0, s1 = (torch.load(tmp_path / ("shadow_rank%d.pt" % k)) for k in (0, 1))
    assert s0["updates"] == s1["updates"] == 3
    assert list(s0["shadow"]) == list(s1["shadow"]) and len(s0["shadow"]) > 0
    assert all(torch.equal(s0["shadow"][k].view(torch.int32), s1["shadow"][k].view(torch.int32)) for k in s0["shadow"])
    assert all(bool(torch.isfinite(v).all()) for v in s0["shadow"].values())
    written = torch.load(tmp_path / "restore" / "wavenet2.ema")              # rank 0 wrote what both hold
    assert all(torch.equal(written[k], s0["shadow"][k]) for k in written)
    assert any(not torch.equal(s0["shadow"][k], s0["params"][k]) for k in s0["params"])
