"""The masked, weighted and smoothed NLL objective through the engines and the public surface (weights= / ignore_index= /
label_smoothing= of music_amd/objective.py and the engines' loss_and_grad, "ignore_token" of train_params.json), on a fast-plan
WaveNet (dilations [1, 2, 4], 32 / 32 / 256, Q 256), a general-plan one (filter width 3, Q 64, 16 / 16 / 32) and a small wn_vq
autoencoder, B = 2, T = rf + 70.

(a) a wholly ignored clip leaves the loss and every parameter gradient of the other clip run alone: loss within 1e-5 max(1, |ref|),
    gradients within 3e-4 of each tensor's max-abs (the bar of tests/test_gpu_phase_model.py; the two runs differ in batch, hence in
    the kernels' tiling, not in the rule).
(b) a random mask, float weights and smoothing 0.1: the loss and d loss / d logits against tests/wnll_ref.py applied to the engine's
    OWN logits (the kernel-level bars: loss 1e-5 max(1, |ref|), dx 1e-5 of max|ref| at Q 256 and 1e-4 otherwise), and the fused step
    and the autograd path give the same flat_grad bits.
(c) the default call launches the entry from before and no other; a mask that ignores nothing gives its bits through the new entry.
(d) score: per-clip weighted means, "tokens", NaN for a clip with nothing counted.
(e) train() from JSON with "ignore_token": -1 on tokens that hold -1 entries ends finite; without the key it ends in NaN."""
import functools
import json
import math
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import wnll_ref as ref
from tests.test_gpu_nll_model import GRAD_RTOL, _bits, _engine_grads, _onehot, _scaled

pytestmark = pytest.mark.gpu
B, W, IGN = 2, 71, -1


def _wavenet(kind):
    from music_amd.model import wavenet
    if kind == "fast":
        return wavenet(filter_width=2, dilations=[1, 2, 4], dilation_channels=32, residual_channels=32, skip_channels=256,
                       quantization_channels=256, use_bias=False), 256
    return wavenet(filter_width=3, dilations=[1, 2, 4], dilation_channels=16, residual_channels=16, skip_channels=32,
                   quantization_channels=64, use_bias=True), 64


@functools.lru_cache(maxsize=None)
def _model(kind):
    """(module on the device, Q, one-hot input (B, Q, rf + 70), targets (B, W) without an ignored one, engine class name)"""
    torch.manual_seed(81 + len(kind))
    if kind == "vq":
        from music_amd.model1 import wavenet_autoencoder
        from tests.test_gpu_cond_learned import _cfg
        net, q = wavenet_autoencoder(**dict(_cfg(en=(32, 32), de=(32, 32, 64), bw=16, pool=8, bias=False), bottleneck="vq", vq_codes=16)), 256
    else:
        net, q = _wavenet(kind)
    net = _scaled(net, 2.0)
    rng = np.random.default_rng(82 + len(kind))
    x = _onehot(rng.integers(0, q, size=(B, net.receptive_field + W - 1)), q).cuda()
    assert x.shape[2] == net.receptive_field + 70
    target = torch.from_numpy(rng.integers(0, q, size=(B, W)).astype(np.int64)).cuda()
    name = type(net._engine_for(x.device)).__name__
    assert name == {"fast": "WaveNetEngine", "general": "GenericWaveNetEngine", "vq": "_AutoencoderEngine"}[kind]
    return net, q, x, target


def _param_grads(net):
    return OrderedDict((k, torch.zeros_like(p).cpu().double() if p.grad is None else p.grad.detach().cpu().double())
                       for k, p in net.named_parameters())


def _loss_and_grads(net, x, target, **kw):
    from music_amd import objective
    net.zero_grad()
    loss = objective.nll_loss(net, x, target, **kw)
    loss.backward()
    return float(loss.detach()), _param_grads(net)


def _mask_and_weights(seed):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(B, W, generator=g) < 0.6
    wt = 2.0 * torch.rand(B, W, generator=g)
    wt[torch.rand(B, W, generator=g) < 0.15] = 0.0
    return keep, wt


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("kind", ["fast", "general", "vq"])
def test_a_wholly_ignored_clip_leaves_the_other_clip_run_alone(kind):
    net, q, x, target = _model(kind)
    alone, g_alone = _loss_and_grads(net, x[:1].contiguous(), target[:1].contiguous())
    t = target.clone()
    t[1] = IGN
    masked, g_masked = _loss_and_grads(net, x, t, ignore_index=IGN)
    e_loss = abs(masked - alone) / max(1.0, abs(alone))
    worst = ("", 0.0)
    for k, r in g_alone.items():
        scale = float(r.abs().max())
        e = float((g_masked[k] - r).abs().max()) / scale if scale > 0 else float(g_masked[k].abs().max())
        worst = max(worst, (k, e), key=lambda v: v[1])
    print("  %s: loss %.6f, clip 0 alone %.6f (%.2e, bar 1e-5); worst gradient %.2e of max-abs in %s (bar 3e-4)"
          % (kind, masked, alone, e_loss, worst[1], worst[0]))
    assert math.isfinite(alone) and e_loss <= 1e-5 and worst[1] < GRAD_RTOL
    assert any(float(r.abs().max()) > 0 for r in g_alone.values())
    eng = net._engine_for(x.device)
    assert eng.workspace(B, x.shape[2])["nll_den"].tolist() == [float(W), float(np.float32(1.0 / W))]
    # the same through a weight of 0 per column, the targets left as they are
    wt = torch.ones(B, W)
    wt[1] = 0.0
    by_weight, g_w = _loss_and_grads(net, x, target, weights=wt)
    assert by_weight == masked and all(torch.equal(g_w[k], g_masked[k]) for k in g_w)


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("kind", ["fast", "general", "vq"])
def test_random_mask_weights_and_smoothing_against_the_rule_on_the_engines_own_logits(kind):
    from music_amd import objective
    net, q, x, target = _model(kind)
    keep, wt = _mask_and_weights(90 + len(kind))
    t = torch.where(keep.cuda(), target, torch.full_like(target, IGN))
    kw = dict(weights=wt, ignore_index=IGN, label_smoothing=0.1)
    eng = net._engine_for(x.device)
    with torch.no_grad():
        _, ws = objective._forward_logits(net, x)
        logits = ws["O"][:B * q * W].view(B, q, W).cpu().clone()
        dlog = torch.full((B * q * W,), float("nan"), device=x.device)
        eng.step_nll(ws, t.reshape(-1), dlogits=dlog, **kw)
        loss = float(ws["loss_part"].double().sum())
        den = ws["nll_den"].tolist()
    f = ref.reference(logits, t.cpu(), weight=wt, ignore_index=IGN, smoothing=0.1)
    scale = float(f["dx"].abs().max())
    e_dx = float((dlog.cpu().view(B, q, W).double() - f["dx"]).abs().max()) / scale
    e_loss = abs(loss - f["loss"]) / max(1.0, abs(f["loss"]))
    dx_bar = 1e-5 if q == 256 else 1e-4
    print("  %s: loss %.6f (float64 on the same logits %.6f, %.2e, bar 1e-5); d loss / d logits %.2e of max|ref| (bar %.0e); den %r"
          % (kind, loss, f["loss"], e_loss, e_dx, dx_bar, den))
    assert 0 < int(f["skip"].sum()) < B * W and e_loss <= 1e-5 and e_dx <= dx_bar
    assert abs(den[0] - f["den"][0]) <= 2.0 ** -24 * f["den"][0]
    assert (dlog.cpu().view(B, q, W)[f["skip"].view(B, 1, W).expand(B, q, W)].view(torch.int32) == 0).all()
    # the fused step and the autograd path: the same loss and flat_grad bits
    cond = (net.engine_cond(),) if kind == "vq" else ()
    l_fused = eng.loss_and_grad(x, t.reshape(-1), *cond, objective="nll", **kw).clone()
    g_fused = eng.flat_grad.clone()
    net.zero_grad()
    l_auto = objective.nll_loss(net, x, t, **kw)
    if kind == "vq":
        l_auto = l_auto + net.vq_loss
    l_auto.backward()
    assert torch.equal(_bits(eng.flat_grad), _bits(g_fused)) and bool(g_fused.abs().max() > 0)
    if kind != "vq":
        # (the same partials: `loss` is their float64 sum, the engines' a float32 one - 4 tiles, so 4 non-zero terms)
        assert torch.equal(_bits(l_auto), _bits(l_fused)) and abs(float(l_fused) - loss) <= 4 * 2.0 ** -24 * abs(loss)
    # smoothing and weights change the objective: neither run is the plain one
    plain = float(objective.nll_loss(net, x, target).detach())
    assert abs(plain - loss) > 1e-3


# ---------------------------------------------------------------- (c)
def _launches(monkeypatch):
    from music_amd import engine_base
    names = []
    real = engine_base.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(engine_base, "call", spy)
    return names


@pytest.mark.parametrize("kind", ["fast", "general", "vq"])
def test_the_default_launches_the_entry_from_before_and_a_mask_of_nothing_gives_its_bits(kind, monkeypatch):
    names = _launches(monkeypatch)
    net, q, x, target = _model(kind)
    eng = net._engine_for(x.device)
    cond = (net.engine_cond(),) if kind == "vq" else ()
    l0 = eng.loss_and_grad(x, target.reshape(-1), *cond, objective="nll").clone()
    g0 = eng.flat_grad.clone()
    assert names.count("wn_step_nll") == 1 and "wn_wstep_nll" not in names and "wn_win_step_nll" not in names
    del names[:]
    l1 = eng.loss_and_grad(x, target.reshape(-1), *cond, objective="nll", ignore_index=IGN, weights=torch.ones(B * W)).clone()
    assert names.count("wn_wstep_nll") == 1 and "wn_step_nll" not in names
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(g0), _bits(eng.flat_grad))
    del names[:]
    l2 = eng.loss_and_grad(x, target.reshape(-1), *cond, objective="nll", weights=None, ignore_index=None, label_smoothing=0.0)
    assert names.count("wn_step_nll") == 1 and "wn_wstep_nll" not in names and torch.equal(_bits(l0), _bits(l2))


# ---------------------------------------------------------------- (d)
def test_score_gives_per_clip_weighted_means_tokens_and_nan_for_an_empty_clip():
    from music_amd import ae_generate, objective
    net, q, x, target = _model("fast")
    keep, wt = _mask_and_weights(95)
    t = torch.where(keep.cuda(), target, torch.full_like(target, IGN))
    with torch.no_grad():
        _, ws = objective._forward_logits(net, x)
        logits = ws["O"][:B * q * W].view(B, q, W).cpu().clone()
    f = ref.reference(logits, t.cpu(), weight=wt, ignore_index=IGN)
    wv = f["w"].view(B, W)
    want_nll = (wv * f["row_nll"].view(B, W)).sum(1) / wv.sum(1)
    want_acc = (wv * f["row_hit"].view(B, W).double()).sum(1) / wv.sum(1)
    r = objective.score(net, x, t, weights=wt.cuda(), ignore_index=IGN)
    assert all(tuple(r[k].shape) == (B,) and r[k].dtype == torch.float64 and r[k].is_cuda for k in ("nll", "bits", "accuracy", "tokens"))
    e = float(((r["nll"].cpu() - want_nll).abs() / want_nll).max())
    print("  score: nll %s (relative error %.2e, bar 1e-5), accuracy %s, tokens %s" % (r["nll"].tolist(), e, r["accuracy"].tolist(), r["tokens"].tolist()))
    assert e < 1e-5 and float((r["accuracy"].cpu() - want_acc).abs().max()) < 1e-12 and torch.equal(r["bits"], r["nll"] / math.log(2.0))
    assert float((r["tokens"].cpu() - wv.sum(1)).abs().max()) < 1e-9
    # the default keeps its three keys; an unweighted mask counts the kept targets
    assert sorted(objective.score(net, x, target)) == ["accuracy", "bits", "nll"]
    r = objective.score(net, x, t, ignore_index=IGN)
    assert r["tokens"].tolist() == keep.sum(1).double().tolist()
    # a clip with nothing counted: NaN in all three, the other clip's figures untouched
    t_empty = t.clone()
    t_empty[1] = IGN
    r2 = objective.score(net, x, t_empty, ignore_index=IGN)
    assert r2["tokens"].tolist() == [float(keep[0].sum()), 0.0]
    assert all(math.isnan(float(r2[k][1])) and float(r2[k][0]) == float(r[k][0]) for k in ("nll", "bits", "accuracy"))
    # ae_generate.prior_score hands the keywords through
    stream = torch.cat([x.argmax(1)[:, :net.receptive_field], target], dim=1)       # (B, rf + W) tokens, all present
    assert "tokens" not in ae_generate.prior_score(net, stream, 1, 256)
    rp = ae_generate.prior_score(net, stream, 1, 256, weights=(t != IGN).float())
    assert rp["tokens"].tolist() == keep.sum(1).double().tolist() and bool(torch.isfinite(rp["nll"]).all())


def test_stage_weights_are_built_per_batch_without_a_copy_from_the_host_or_a_synchronisation():
    """ "nll_stage_weights": the table is uploaded once; a batch's weights are index arithmetic on the device from the loader's
    device positions.  torch.cuda.set_sync_debug_mode("error") raises on every synchronising call, a host-to-device copy from
    pageable memory among them (the control below)."""
    from music_amd import objective
    opt = objective.wnll_option({"objective": "nll", "nll_stage_weights": [4.0, 1.0, 0.0], "ignore_token": -1}, {"token_positions": True})
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = [torch.tensor(p, dtype=torch.int64).to(dev) for p in ([0, 5], [7, 2])]
    first = objective.wnll_kwargs(opt, {"audio_pos": pos[0]}, 4, dev)["weights"]         # (the one upload)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.tensor([4.0, 1.0, 0.0], dtype=torch.float32, device=dev)              # the control: what a table per batch would do
        again = objective.wnll_kwargs(opt, {"audio_pos": pos[0]}, 4, dev)["weights"]
        other = objective.wnll_kwargs(opt, {"audio_pos": pos[1]}, 4, dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert other["weights"].is_cuda and other["weights"].dtype == torch.float32 and other["ignore_index"] == -1
    assert first.tolist() == again.tolist() == [[4.0, 1.0, 0.0, 4.0], [0.0, 4.0, 1.0, 0.0]]
    assert other["weights"].tolist() == [[1.0, 0.0, 4.0, 1.0], [0.0, 4.0, 1.0, 0.0]]
    assert len(opt["_device"]) == 1                                                       # one table and one row of offsets per device and width


# ---------------------------------------------------------------- (e) train()
CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16, quantization_channels=64,
           use_bias=False)
RF, WIN, BATCH = 17, 25, 4


def _write_run(tmp, extra):
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    items = []
    for n in (120, 95, 70):                              # 4 + 3 + 2 windows, each with a tail of 20 > rf: 12 pieces, 3 steps
        item = rng.integers(0, 64, size=(n,)).astype(np.int32)
        item[rng.random(n) < 0.15] = -1                  # absent tokens, as inputs (a zero column) and as targets
        items.append(item)
    assert all((item == -1).any() for item in items)
    pickle.dump(items, open(tmp / "np_tokens.pkl", "wb"))
    dp = dict(batch_size=BATCH, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_tokens.pkl"), receptive_field=RF,
              window_length=WIN, cuda_available=False, quantization_channels=64, one_hot="canonical")
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=10, print_every=1, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3,
              objective="nll")
    tp.update(extra)
    for n, p in (("wavenet", CFG), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))


def _train(tmp, monkeypatch, extra):
    from music_amd import train as T
    from music_amd.model import wavenet
    made = []

    def ctor(**kw):
        made.append(wavenet(**kw))
        return made[-1]
    _write_run(tmp, extra)
    monkeypatch.chdir(tmp)
    monkeypatch.setattr(T, "wavenet", ctor)
    torch.manual_seed(0)
    T.train()
    lines = open(tmp / "log" / "loss_log.log").read().splitlines()
    return made[0], [float(l.split(" ")[-1]) for l in lines]


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "autograd"])
def test_train_with_ignore_token_on_tokens_that_hold_absent_entries(tmp_path, monkeypatch, fused):
    """3 steps from JSON: with "ignore_token": -1 every loss line and every parameter is finite and the first loss is near ln 64; the
    same run without the key is NaN from the first step on (a -1 target poisons the loss)"""
    step = dict(fused_step=True) if fused else {}
    net, losses = _train(tmp_path / "with", monkeypatch, dict(step, ignore_token=-1, label_smoothing=0.05))
    print("  loss lines with ignore_token: %s" % losses)
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses) and abs(losses[0] - math.log(64)) < 0.5
    assert all(bool(torch.isfinite(v).all()) for v in net.state_dict().values())
    net0, losses0 = _train(tmp_path / "without", monkeypatch, step)
    print("  loss lines without it: %s" % losses0)
    assert len(losses0) == 3 and all(math.isnan(v) for v in losses0)
    assert not all(bool(torch.isfinite(v).all()) for v in net0.state_dict().values())
