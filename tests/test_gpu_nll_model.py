"""The true-NLL objective through the engines and the public surface (music_amd/objective.py): the fused step under
objective="nll" against float64 autograd through the oracle's pre-softmax logits (fast engine, general plan with filter width 3 and
Q = 100, the autoencoder's fast engine with a fixed conditioning draw), the codes entry, nll_loss, step_probs against the decoder's
own distribution, score, the untouched default, and train() with validation.

Bars: loss 1e-4 absolute, gradients 3e-4 of each tensor's max-abs (the project's small-shape bars, tests/test_gpu_parity.py)."""
from collections import OrderedDict
import functools
import json
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as wo
from tests.helpers import nonvacuous

pytestmark = pytest.mark.gpu
GRAD_RTOL = 3e-4


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _onehot(codes, q):
    """the canonical one-hot (B, q, T) float32 of int codes (B, T)"""
    return F.one_hot(torch.as_tensor(codes).long(), q).permute(0, 2, 1).float().contiguous()


def _nll64(logits, target, leaves=()):
    """float64: mean cross entropy over the channel axis of logits (B, Q, W), its gradients w.r.t. `leaves`, per-timestep probabilities"""
    B, Q, W = logits.shape
    z = logits.permute(0, 2, 1).reshape(-1, Q)
    loss = F.cross_entropy(z, target.reshape(-1))
    grads = torch.autograd.grad(loss, list(leaves), allow_unused=True) if leaves else ()
    return loss.detach(), grads, F.softmax(z.detach(), dim=1), F.cross_entropy(z.detach(), target.reshape(-1), reduction="none").view(B, W)


def _leaves(net):
    return OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())


def _wavenet_ref(net, x, target, input_grad=False):
    leaf = _leaves(net)
    x64 = x.double().cpu().clone().requires_grad_(input_grad)
    inter = {}
    wo.wavenet_forward(leaf, net.dilations, x64, filter_width=net.filter_width, quantization_channels=net.quantization_channels,
                       intermediates=inter)
    loss, grads, probs, rows = _nll64(inter["pre_softmax"], target.cpu(), leaves=list(leaf.values()) + ([x64] if input_grad else []))
    g = OrderedDict((k, torch.zeros_like(v) if gr is None else gr) for (k, v), gr in zip(leaf.items(), grads))
    return dict(loss=float(loss), grads=g, probs=probs, rows=rows, din=grads[-1] if input_grad else None,
                hit=(inter["pre_softmax"].detach().argmax(1) == target.cpu().view(rows.shape)))


def _scaled(net, gain):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gain)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _fast():
    """the fast-engine model of this file, its batch and its float64 reference (computed once, never modified)"""
    from music_amd.model import wavenet
    torch.manual_seed(11)
    net = _scaled(wavenet(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=32, residual_channels=64, skip_channels=256,
                          quantization_channels=256, use_bias=False), 3.0)
    rng = np.random.default_rng(12)
    B, W = 2, 69
    codes = torch.from_numpy(rng.integers(0, 256, size=(B, net.receptive_field + W - 1)).astype(np.int32))
    target = torch.from_numpy(rng.integers(0, 256, size=(B, W)).astype(np.int64)).cuda()
    x = _onehot(codes, 256).cuda()
    ref = _wavenet_ref(net, x, target, input_grad=True)
    nonvacuous(ref["probs"], "fast engine, gain 3")
    from music_amd.engine import WaveNetEngine
    assert type(net._engine_for(x.device)) is WaveNetEngine
    return net, codes.cuda(), x, target, ref


@functools.lru_cache(maxsize=None)
def _general():
    from music_amd.model import wavenet
    torch.manual_seed(21)
    net = _scaled(wavenet(filter_width=3, dilations=[1, 2, 4], dilation_channels=32, residual_channels=32, skip_channels=32,
                          quantization_channels=100, use_bias=True), 3.0)
    rng = np.random.default_rng(22)
    B, W = 2, 69
    x = _onehot(rng.integers(0, 100, size=(B, net.receptive_field + W - 1)), 100).cuda()
    target = torch.from_numpy(rng.integers(0, 100, size=(B, W)).astype(np.int64)).cuda()
    ref = _wavenet_ref(net, x, target)
    nonvacuous(ref["probs"], "general plan fw 3, Q 100, gain 3")
    from music_amd.engine_generic import GenericWaveNetEngine
    assert type(net._engine_for(x.device)) is GenericWaveNetEngine
    return net, x, target, ref


AE_SEED = 33


@functools.lru_cache(maxsize=None)
def _autoencoder():
    from music_amd.model1 import _AutoencoderEngine, wavenet_autoencoder
    cfg = dict(filter_width=2, quantization_channel=256, dilations=[1, 2, 4, 8, 3], en_residual_channel=60, en_dilation_channel=52,
               en_bottleneck_width=10, en_pool_kernel_size=40, de_residual_channel=64, de_dilation_channel=60, de_skip_channel=72,
               use_bias=True)
    torch.manual_seed(31)
    net = _scaled(wavenet_autoencoder(**cfg), 2.5)
    rng = np.random.default_rng(32)
    B, W = 2, 120
    x = _onehot(rng.integers(0, 256, size=(B, net.receptive_field + W - 1)), 256).cuda()
    target = torch.from_numpy(rng.integers(0, 256, size=(B, W)).astype(np.int64)).cuda()
    torch.manual_seed(AE_SEED)
    cond = [(w.double(), b.double()) for w, b in net._draw_conditioning()]
    leaf = _leaves(net)
    # the oracle's decoder ends in the chunk softmax; with that one function as the identity it returns the pre-softmax logits
    keep, wo.chunk_softmax = wo.chunk_softmax, lambda total, q: total
    try:
        logits, _ = wo.autoencoder_forward(leaf, cfg["dilations"], x.double().cpu(), cfg["en_pool_kernel_size"], cond)
    finally:
        wo.chunk_softmax = keep
    assert tuple(logits.shape) == (B, 256, W)
    loss, grads, probs, rows = _nll64(logits, target.cpu(), leaves=leaf.values())
    g = OrderedDict((k, torch.zeros_like(v) if gr is None else gr) for (k, v), gr in zip(leaf.items(), grads))
    nonvacuous(probs, "autoencoder, gain 2.5")
    assert type(net._engine_for(x.device)) is _AutoencoderEngine
    return net, x, target, dict(loss=float(loss), grads=g, probs=probs, rows=rows)


def _engine_grads(eng):
    out = OrderedDict()
    for name in eng.param_names:
        o, shp = eng.spec.off[name], eng.spec.shape[name]
        out[name] = eng.flat_grad[o:o + int(np.prod(shp))].view(shp).detach().cpu().double()
    return out


def _compare(label, loss, grads, ref):
    e_loss = abs(float(loss.detach()) - ref["loss"])
    worst = ("", 0.0)
    assert sorted(grads) == sorted(ref["grads"])
    for k, g in grads.items():
        r = ref["grads"][k]
        scale = float(r.abs().max())
        e = float((g - r).abs().max()) / scale if scale > 0 else float(g.abs().max())
        worst = max(worst, (k, e), key=lambda t: t[1])
    print("  %s: loss %.6f (float64 %.6f, |d| %.2e, bar 1e-4); worst gradient %.2e of max-abs in %s (bar 3e-4)"
          % (label, float(loss.detach()), ref["loss"], e_loss, worst[1], worst[0]))
    assert e_loss < 1e-4 and worst[1] < GRAD_RTOL, (label, e_loss, worst)


def test_fast_engine_nll_step_against_float64():
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    loss = eng.loss_and_grad(x, target, want_probs=True, objective="nll")
    _compare("fast engine", loss, _engine_grads(eng), ref)
    # want_probs under "nll": the per-timestep probabilities
    probs = eng.workspace(*x.shape[::2])["probs"]
    assert tuple(probs.shape) == (2 * 69, 256) and float((probs.cpu().double() - ref["probs"]).abs().max()) < 1e-4


def test_general_plan_nll_step_against_float64():
    net, x, target, ref = _general()
    eng = net._engine_for(x.device)
    _compare("general plan fw 3 Q 100", eng.loss_and_grad(x, target, objective="nll"), _engine_grads(eng), ref)


def test_autoencoder_nll_step_against_float64():
    net, x, target, ref = _autoencoder()
    eng = net._engine_for(x.device)
    torch.manual_seed(AE_SEED)
    loss = eng.loss_and_grad(x, target, net._draw_conditioning(), objective="nll")
    _compare("autoencoder", loss, _engine_grads(eng), ref)


def test_codes_entry_gives_the_bits_of_the_dense_canonical_one_hot():
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    l_codes = eng.loss_and_grad_codes(codes, target, scrambled=False, objective="nll").clone()
    g_codes = eng.flat_grad.clone()
    dense = eng.onehot(codes, scrambled=False)
    assert torch.equal(dense, x)
    l_dense = eng.loss_and_grad(dense, target, objective="nll")
    assert torch.equal(_bits(l_codes), _bits(l_dense)) and torch.equal(_bits(g_codes), _bits(eng.flat_grad))
    assert abs(float(l_codes) - ref["loss"]) < 1e-4


def test_the_attribute_is_the_default_and_reference_stays_bit_equal():
    """objective=None means eng.objective; "reference" - passed or not - is the step the parent computed: same loss and flat_grad
    bits as a call that does not know the argument."""
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    assert eng.objective == "reference"
    l0 = eng.loss_and_grad(x, target).clone()
    g0 = eng.flat_grad.clone()
    l1 = eng.loss_and_grad(x, target, objective="reference").clone()
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(g0), _bits(eng.flat_grad))
    assert abs(float(l0) - ref["loss"]) > 1e-2                      # (the reference's loss is another number altogether)
    try:
        eng.objective = "nll"
        l2 = eng.loss_and_grad(x, target).clone()
        g2 = eng.flat_grad.clone()
    finally:
        del eng.objective                                           # back to the class attribute
    l3 = eng.loss_and_grad(x, target, objective="nll")
    assert torch.equal(_bits(l2), _bits(l3)) and torch.equal(_bits(g2), _bits(eng.flat_grad)) and abs(float(l2) - ref["loss"]) < 1e-4
    with pytest.raises(ValueError, match="objective"):
        eng.loss_and_grad(x, target, objective="mse")


def test_nll_loss_backward_gives_the_fused_step_gradients():
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    l_fused = eng.loss_and_grad(x, target, objective="nll").clone()
    g_fused = eng.flat_grad.clone()
    net.zero_grad()
    xin = x.clone().requires_grad_(True)
    loss = objective.nll_loss(net, xin, target)
    assert loss.dim() == 0 and loss.requires_grad and torch.equal(_bits(loss), _bits(l_fused))
    (2.0 * loss).backward()                                           # the upstream scalar multiplies every gradient (exactly: a power of 2)
    got = torch.cat([p.grad.reshape(-1) for _, p in net._named_ref_params()])
    assert torch.equal(_bits(got), _bits(2.0 * g_fused))
    scale = float(ref["din"].abs().max())
    e = float((xin.grad.cpu().double() / 2.0 - ref["din"]).abs().max()) / scale
    print("  input gradient: %.2e of max-abs (bar 3e-4)" % e)
    assert e < GRAD_RTOL
    with torch.no_grad():                                             # no graph, no held workspace
        assert not objective.nll_loss(net, x, target).requires_grad


def test_nll_loss_on_the_autoencoder():
    from music_amd import objective
    net, x, target, ref = _autoencoder()
    net.zero_grad()
    torch.manual_seed(AE_SEED)
    loss = objective.nll_loss(net, x, target)
    loss.backward()
    grads = OrderedDict((k, p.grad.detach().cpu().double()) for k, p in net.named_parameters())
    _compare("autoencoder nll_loss", loss, grads, ref)
    assert net.last_encoding is not None


def test_step_probs_is_the_decoders_distribution():
    """row b W + w of step_probs is what the module itself gives for the receptive field that ends at output column w (at W = 1 the
    chunk softmax is the per-timestep one) - within 1e-3 - and the float64 reference's softmax"""
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    rf, W = net.receptive_field, 69
    probs = objective.step_probs(net, x)
    assert tuple(probs.shape) == (2 * W, 256) and not probs.requires_grad
    assert float((probs.cpu().double() - ref["probs"]).abs().max()) < 1e-4
    assert float((probs.sum(1) - 1).abs().max()) < 1e-5
    with torch.no_grad():
        for b, w in ((0, 0), (0, 37), (0, 68), (1, 0), (1, 64), (1, 68)):
            one = net(x[b:b + 1, :, w:w + rf].contiguous())
            assert tuple(one.shape) == (1, 256)
            e = float((one[0] - probs[b * W + w]).abs().max())
            assert e < 1e-3, (b, w, e)


def test_score_against_float64():
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    want_nll, want_acc = ref["rows"].mean(1), ref["hit"].double().mean(1)
    for what, inp in (("dense", x), ("codes", codes)):
        r = objective.score(net, inp, target)
        assert all(tuple(r[k].shape) == (2,) and r[k].dtype == torch.float64 and r[k].is_cuda for k in ("nll", "bits", "accuracy"))
        e = float(((r["nll"].cpu() - want_nll).abs() / want_nll).max())
        print("  score (%s): nll %s, relative error %.2e (bar 1e-5), accuracy %s" % (what, r["nll"].tolist(), e, r["accuracy"].tolist()))
        assert e < 1e-5 and torch.equal(r["accuracy"].cpu(), want_acc)
        assert torch.equal(r["bits"], r["nll"] / math.log(2.0))
    # the loader's scrambled layout is another input altogether
    assert float((objective.score(net, codes, target, scrambled=True)["nll"].cpu() - want_nll).abs().max()) > 1e-2


# ---------------------------------------------------------------- train()
CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16,
           quantization_channels=256, use_bias=False)
RF, WIN, BATCH = 17, 100, 4


def _write_run(tmp, extra):
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    pickle.dump([rng.integers(0, 256, size=(417,)).astype(np.int32) for _ in range(3)], open(tmp / "np_audio.pkl", "wb"))     # 12 pieces
    pickle.dump([rng.integers(0, 256, size=(417,)).astype(np.int32)], open(tmp / "np_valid.pkl", "wb"))                       # 4 pieces
    dp = dict(batch_size=BATCH, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_audio.pkl"), receptive_field=RF,
              window_length=WIN, cuda_available=False, quantization_channels=256, one_hot="canonical")
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=1, print_every=1, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3,
              objective="nll", valid_audio_path=str(tmp / "np_valid.pkl"), validate_every=2)
    tp.update(extra)
    for n, p in (("wavenet", CFG), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))
    return dp


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step_ema", "autograd"])
def test_train_with_the_nll_objective_and_validation(tmp_path, monkeypatch, fused):
    """train() for 3 steps with "objective": "nll" on the canonical one-hot: the first loss line is the float64 NLL of the initial
    model on batch 0; validation (every 2 steps) writes its line; with an EMA shadow the validated weights are the shadow's."""
    from music_amd import faster_audio_data as fad
    from music_amd import objective
    from music_amd import train as T
    from music_amd.model import wavenet
    made = []

    def ctor(**kw):
        net = wavenet(**kw)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
        made.append((net, OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items())))
        return net
    seen = []
    real_score = objective.score

    def spy(net, x, target, scrambled=False):
        eng = net._engine
        shadow = eng.ema if eng is not None and eng.adam_state is not None else None
        seen.append((torch.cat([p.detach().reshape(-1) for _, p in net._named_ref_params()]).clone(),
                     None if shadow is None else (shadow.flat.clone(), shadow._swapped)))
        return real_score(net, x, target, scrambled)
    monkeypatch.setattr(objective, "score", spy)
    dp = _write_run(tmp_path, dict(fused_step=True, ema_decay=0.5) if fused else {})
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(T, "wavenet", ctor)
    torch.manual_seed(0)
    T.train()
    net, initial = made[0]
    # batch 0 as the loader built it, and the float64 NLL of the initial model on it
    ds = fad.audio_dataset(dp["audio_path"], RF, WIN)
    assert len(ds) == 12
    codes = torch.stack([ds[i]["audio_piece"] for i in range(BATCH)])
    target = torch.stack([ds[i]["audio_target"] for i in range(BATCH)])
    first = wavenet(**CFG)
    first.load_state_dict(initial)
    ref = _wavenet_ref(first, _onehot(codes, 256), target)
    lines = open(tmp_path / "log" / "loss_log.log").read().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Trained over 1 pieces,Average loss is ")
    got = float(lines[0].split(" ")[-1])
    print("  first loss line %.6f, float64 NLL of the initial model on batch 0 %.6f" % (got, ref["loss"]))
    assert abs(got - ref["loss"]) < 1e-4
    vlines = open(tmp_path / "log" / "valid_log.log").read().splitlines()
    assert len(vlines) == 1 and len(seen) == 1                       # steps 1..3, every 2: once, one batch of 4 clips
    m = re.fullmatch(r"Trained over 2 pieces,Validation nll is (\S+), bits per sample (\S+), accuracy (\S+)", vlines[0])
    assert m, vlines[0]
    nll, bits, acc = (float(v) for v in m.groups())
    assert 0.0 < nll < 50.0 and abs(bits - nll / math.log(2.0)) < 1e-9 * bits and 0.0 <= acc <= 1.0
    params_then, shadow_then = seen[0]
    final = torch.cat([p.detach().reshape(-1) for _, p in net._named_ref_params()])
    if fused:
        flat, swapped = shadow_then
        assert swapped and torch.equal(_bits(params_then), _bits(flat))      # validated under the shadow's weights ...
        assert not torch.equal(params_then, final)
        assert sorted(os.listdir(tmp_path / "restore")) == ["wavenet1.ema", "wavenet1.model"]
    else:
        assert shadow_then is None
    # it trained: every tensor moved, except the last block's dense 1x1, which never reaches the output (its gradient is zero)
    dead = "dilation_layer_stack.%d.weight" % (4 * (len(CFG["dilations"]) - 1) + 2)
    trained = net.state_dict()
    assert torch.equal(initial[dead], trained[dead].cpu())
    assert not any(torch.equal(v, trained[k].cpu()) for k, v in initial.items() if k != dead)
