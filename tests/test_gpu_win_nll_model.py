"""The windowed NLL objective through the engines and the public surface (music_amd/objective.py, windows= / window_pos=), by the
float64 route of tests/test_gpu_nll_model.py: the oracle's pre-softmax logits, then float64 autograd with the window applied in
float64 (tests/win_nll_ref.py).  The fused step and the codes entry on the fast engine (Q = 256 as 4 x 64) and on the general plan
(filter width 3, Q = 96 as 3 x 32), nll_loss with the input gradient, step_probs against the DECODER's own teacher-forced windowed
distribution - what the feature is for -, score, the untouched default, and train() with "nll_windows" + "token_positions".

Bars (tests/test_gpu_nll_model.py): loss 1e-4 absolute, gradients 3e-4 of each tensor's max-abs, step_probs against the decoder 1e-3."""
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

from music_amd.fast_generate import stage_windows
from oracle import wavenet_oracle as wo
from tests import win_nll_ref as ref64
from tests.helpers import nonvacuous
from tests.test_gpu_nll_model import AE_SEED, GRAD_RTOL, _autoencoder, _bits, _compare, _engine_grads, _leaves, _onehot, _scaled

pytestmark = pytest.mark.gpu


def _targets_inside(rng, windows, pos, B, W, q):
    lo, hi, _ = ref64.column_windows(windows, B, W, q, pos)
    return (lo + torch.from_numpy(rng.integers(0, 1 << 30, size=(B, W))) % (hi - lo)).to(torch.int64)


def _windowed_ref(net, x, target, windows, pos, input_grad=False):
    """float64: the oracle's logits, then loss, gradients, probabilities, per-column nll and hits under the windows"""
    leaf = _leaves(net)
    x64 = x.double().cpu().clone().requires_grad_(input_grad)
    inter = {}
    wo.wavenet_forward(leaf, net.dilations, x64, filter_width=net.filter_width, quantization_channels=net.quantization_channels,
                       intermediates=inter)
    logits = inter["pre_softmax"]
    loss = ref64.windowed_nll(logits, target.cpu(), windows, pos)
    grads = torch.autograd.grad(loss, list(leaf.values()) + ([x64] if input_grad else []), allow_unused=True)
    g = OrderedDict((k, torch.zeros_like(v) if gr is None else gr) for (k, v), gr in zip(leaf.items(), grads))
    B, q, W = logits.shape
    f = ref64.reference(logits.detach(), target.cpu(), 1.0 / (B * W), windows, pos)
    assert abs(f["loss"] - float(loss.detach())) < 1e-12
    plain = ref64.reference(logits.detach(), target.cpu(), 1.0 / (B * W), None)
    return dict(loss=float(loss.detach()), grads=g, probs=f["probs"], rows=f["row_nll"].view(B, W), hit=f["row_hit"].view(B, W),
                din=grads[-1] if input_grad else None, plain_rows=plain["row_nll"].view(B, W))


WIN4, POS = stage_windows(4, 64), [3, 8]


@functools.lru_cache(maxsize=None)
def _fast():
    """the fast-engine prior of this file (Q = 256 as 4 x 64), its batch with per-clip positions and its float64 reference (computed
    once, never modified)"""
    from music_amd.model import wavenet
    torch.manual_seed(51)
    net = _scaled(wavenet(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=32, residual_channels=64, skip_channels=256,
                          quantization_channels=256, use_bias=False), 3.0)
    rng = np.random.default_rng(52)
    B, W = 2, 69
    codes = torch.from_numpy(rng.integers(0, 256, size=(B, net.receptive_field + W - 1)).astype(np.int32))
    target = _targets_inside(rng, WIN4, POS, B, W, 256).cuda()
    x = _onehot(codes, 256).cuda()
    ref = _windowed_ref(net, x, target, WIN4, POS, input_grad=True)
    nonvacuous(ref["probs"], "fast engine under windows, gain 3")
    from music_amd.engine import WaveNetEngine
    assert type(net._engine_for(x.device)) is WaveNetEngine
    return net, codes.cuda(), x, target, ref


def test_fast_engine_windowed_step_and_codes_entry_against_float64():
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    pos = torch.tensor(POS, dtype=torch.int64, device=x.device)
    loss = eng.loss_and_grad(x, target, want_probs=True, objective="nll", windows=WIN4, window_pos=pos).clone()
    _compare("fast engine, 4 x 64", loss, _engine_grads(eng), ref)
    g_dense = eng.flat_grad.clone()
    probs = eng.workspace(*x.shape[::2])["probs"]
    assert tuple(probs.shape) == (2 * 69, 256) and float((probs.cpu().double() - ref["probs"]).abs().max()) < 1e-4
    assert (probs.cpu()[ref["probs"] == 0] == 0).all()
    # the codes entry, positions as a host sequence: within the bars, and the bits of the dense one-hot built from those codes
    l_codes = eng.loss_and_grad_codes(codes, target, scrambled=False, objective="nll", windows=WIN4, window_pos=POS).clone()
    _compare("codes entry, 4 x 64", l_codes, _engine_grads(eng), ref)
    g_codes = eng.flat_grad.clone()
    dense = eng.onehot(codes, scrambled=False)
    assert torch.equal(dense, x)
    l_dense = eng.loss_and_grad(dense, target, objective="nll", windows=WIN4, window_pos=POS)
    assert torch.equal(_bits(l_codes), _bits(l_dense)) and torch.equal(_bits(g_codes), _bits(eng.flat_grad))
    assert torch.equal(_bits(l_codes), _bits(loss))
    # the attribute in place of the arguments
    try:
        eng.objective, eng.nll_windows = "nll", WIN4
        l_attr = eng.loss_and_grad(x, target, window_pos=pos)
        assert torch.equal(_bits(l_attr), _bits(loss)) and torch.equal(_bits(eng.flat_grad), _bits(g_dense))
    finally:
        del eng.objective, eng.nll_windows
    # positions count mod the period; a misaligned one is loud
    assert abs(float(eng.loss_and_grad(x, target, objective="nll", windows=WIN4, window_pos=[7, 12])) - ref["loss"]) < 1e-4
    assert math.isnan(float(eng.loss_and_grad(x, target, objective="nll", windows=WIN4, window_pos=[4, 8])))
    with pytest.raises(ValueError, match="objective"):
        eng.loss_and_grad(x, target, objective="reference", windows=WIN4)


def test_nll_loss_backward_under_windows_with_the_input_gradient():
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    net.zero_grad()
    xin = x.clone().requires_grad_(True)
    loss = objective.nll_loss(net, xin, target, windows=WIN4, window_pos=POS)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    grads = OrderedDict((k, p.grad.detach().cpu().double()) for k, p in net.named_parameters())
    _compare("nll_loss under windows", loss, grads, ref)
    scale = float(ref["din"].abs().max())
    e = float((xin.grad.cpu().double() - ref["din"]).abs().max()) / scale
    print("  input gradient: %.2e of max-abs (bar 3e-4)" % e)
    assert e < GRAD_RTOL


def test_general_plan_windowed_step_against_float64():
    from music_amd.engine_generic import GenericWaveNetEngine
    from music_amd.model import wavenet
    torch.manual_seed(61)
    net = _scaled(wavenet(filter_width=3, dilations=[1, 2, 4], dilation_channels=32, residual_channels=32, skip_channels=32,
                          quantization_channels=96, use_bias=True), 3.0)
    rng = np.random.default_rng(62)
    B, W, win, pos = 2, 69, stage_windows(3, 32), [2, 4]
    x = _onehot(rng.integers(0, 96, size=(B, net.receptive_field + W - 1)), 96).cuda()
    target = _targets_inside(rng, win, pos, B, W, 96).cuda()
    ref = _windowed_ref(net, x, target, win, pos)
    nonvacuous(ref["probs"], "general plan fw 3, Q 96, gain 3")
    eng = net._engine_for(x.device)
    assert type(eng) is GenericWaveNetEngine
    _compare("general plan fw 3, 3 x 32", eng.loss_and_grad(x, target, objective="nll", windows=win, window_pos=pos), _engine_grads(eng), ref)


def test_step_probs_under_windows_is_the_windowed_decoders_distribution():
    """Row b W + w of step_probs(net, x, windows=, window_pos=) against what the decoder itself reports, teacher-forced through the
    same codes under the same table and positions (decode_batch_cond(forced=, want_probs=True, windows=, window_pos=) from the state
    the init forward leaves): the distribution sample_code_stream draws from is the one the objective trains and scores."""
    from music_amd import fast_generate as fg
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    rf, W, Q = net.receptive_field, 69, 256
    probs = objective.step_probs(net, x, windows=WIN4, window_pos=POS).clone()
    assert tuple(probs.shape) == (2 * W, Q) and not probs.requires_grad
    assert float((probs.cpu().double() - ref["probs"]).abs().max()) < 1e-4
    assert float((probs.sum(1) - 1).abs().max()) < 1e-5 and (probs.cpu()[ref["probs"] == 0] == 0).all()
    worst = 0.0
    for b in range(2):
        start = x[b:b + 1, :, :rf].contiguous()
        with torch.no_grad():
            first = net(start)                                       # (1, Q): the init forward, which leaves the queues
        eng = net._engine
        K1 = fg._taps(eng)
        rings = fg._rings_from_workspace(eng, 1, rf)
        # column 0 comes from the init forward (its plain distribution, renormalised inside the window of position POS[b])
        lo, hi = WIN4[POS[b] % 4]
        p0 = first[0].double()
        p0 = p0[lo:hi] / p0[lo:hi].sum()
        worst = max(worst, float((p0 - probs[b * W, lo:hi].double()).abs().max()))
        # columns 1 .. W-1: step s pushes input column rf + s and reports the distribution of sample rf + s + 1 = column s + 1
        note0 = x[b:b + 1, :, rf].contiguous()
        prev0 = x[b:b + 1, :, rf - K1:rf].transpose(1, 2).contiguous()
        forced = torch.cat([codes[b, rf + 1:], codes[b, :1]]).view(1, W - 1).to(torch.int32)
        _, dec, _, _ = fg.decode_batch_cond(net, rings, prev0, note0, W - 1, forced=forced, want_probs=True, temperature=1.0, seed=3,
                                            windows=WIN4, window_pos=POS[b] + 1)
        got = probs[b * W + 1:(b + 1) * W]
        assert tuple(dec.shape) == (1, W - 1, Q)
        assert torch.equal(dec[0] == 0, got == 0), "the decoder's support and the objective's differ"
        worst = max(worst, float((dec[0] - got).abs().max()))
    print("  step_probs under windows against the teacher-forced windowed decoder: %.2e (bar 1e-3)" % worst)
    assert worst < 1e-3


def test_score_under_windows_against_float64():
    from music_amd import objective
    net, codes, x, target, ref = _fast()
    want_nll, want_acc = ref["rows"].mean(1), ref["hit"].double().mean(1)
    for what, inp in (("dense", x), ("codes", codes)):
        r = objective.score(net, inp, target, windows=WIN4, window_pos=torch.tensor(POS, device=x.device))
        assert all(tuple(r[k].shape) == (2,) and r[k].dtype == torch.float64 and r[k].is_cuda for k in ("nll", "bits", "accuracy"))
        e = float(((r["nll"].cpu() - want_nll).abs() / want_nll).max())
        print("  score (%s): nll %s, relative error %.2e (bar 1e-5), accuracy %s" % (what, r["nll"].tolist(), e, r["accuracy"].tolist()))
        assert e < 1e-5 and torch.equal(r["accuracy"].cpu(), want_acc)
        assert torch.equal(r["bits"], r["nll"] / math.log(2.0))


def test_a_random_prior_scores_strictly_better_under_windows():
    """an untrained prior (no gain) on a stream whose tokens respect the stages: float64 says every clip's nll under the windows lies
    below the plain one - by about ln 4 - and score() says the same"""
    from music_amd import objective
    from music_amd.model import wavenet
    torch.manual_seed(71)
    net = wavenet(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=32, residual_channels=64, skip_channels=256,
                  quantization_channels=256, use_bias=False).cuda()
    rng = np.random.default_rng(72)
    B, W = 2, 40
    T = net.receptive_field + W - 1
    pos = [net.receptive_field, net.receptive_field + 1]             # clip b is the stream from position b on
    stream = torch.stack([torch.tensor([((b + t) % 4) * 64 for t in range(T + 1)]) for b in range(B)]) + torch.from_numpy(rng.integers(0, 64, size=(B, T + 1)))
    codes, target = stream[:, :T].to(torch.int32), stream[:, net.receptive_field:].to(torch.int64)
    ref = _windowed_ref(net, _onehot(codes, 256), target, WIN4, pos)
    w64, p64 = ref["rows"].mean(1), ref["plain_rows"].mean(1)
    assert (w64 < p64 - 1.0).all(), (w64, p64)
    r_win = objective.score(net, codes.cuda(), target.cuda(), windows=WIN4, window_pos=pos)
    r_plain = objective.score(net, codes.cuda(), target.cuda())
    print("  untrained prior: nll %s under windows, %s without (float64 %s, %s)" % (r_win["nll"].tolist(), r_plain["nll"].tolist(), w64.tolist(), p64.tolist()))
    assert (r_win["nll"] < r_plain["nll"]).all()
    assert float((r_win["nll"].cpu() - w64).abs().max()) < 1e-4 and float((r_plain["nll"].cpu() - p64).abs().max()) < 1e-4
    # ae_generate.prior_score: the same call on a whole stream and its first position (clip 1 is the stream from position 1 on)
    from music_amd import ae_generate
    for b in range(B):
        r = ae_generate.prior_score(net, stream[b:b + 1], 4, 64, start_pos=b)
        assert all(float((r[k] - r_win[k][b:b + 1]).abs().max()) < 1e-6 for k in ("nll", "bits", "accuracy"))


def _launches(monkeypatch):
    from music_amd import engine_base
    names = []
    real = engine_base.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(engine_base, "call", spy)
    return names


def test_the_default_is_untouched_and_whole_alphabet_tables_give_its_bits(monkeypatch):
    """nothing set: loss_and_grad(objective="nll") launches wn_step_nll and no windowed entry, on the fast engine and on the autoencoder's;
    a table of (0, Q) pairs launches wn_win_step_nll and gives the same loss and flat_grad bits"""
    names = _launches(monkeypatch)
    net, codes, x, target, ref = _fast()
    eng = net._engine_for(x.device)
    assert eng.nll_windows is None

    def both(step):
        del names[:]
        l0 = step({}).clone()
        g0 = eng_.flat_grad.clone()
        assert names.count("wn_step_nll") == 1 and not [n for n in names if n.startswith("wn_win_")]
        del names[:]
        l1 = step(dict(windows=[(0, 256)] * 3, window_pos=[5, 1 << 35])).clone()
        assert names.count("wn_win_step_nll") == 1 and "wn_step_nll" not in names
        assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(g0), _bits(eng_.flat_grad))
        return l0
    eng_ = eng
    both(lambda kw: eng.loss_and_grad(x, target, objective="nll", **kw))
    net_ae, x_ae, t_ae, ref_ae = _autoencoder()
    eng_ = net_ae._engine_for(x_ae.device)

    def ae_step(kw):
        torch.manual_seed(AE_SEED)
        return eng_.loss_and_grad(x_ae, t_ae, net_ae._draw_conditioning(), objective="nll", **kw)
    l_ae = both(ae_step)
    assert abs(float(l_ae) - ref_ae["loss"]) < 1e-4                  # (the figure tests/test_gpu_nll_model.py holds the default to)


# ---------------------------------------------------------------- train()
STAGES, CODES = 2, 32
CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16,
           quantization_channels=STAGES * CODES, use_bias=False)
RF, WIN, BATCH = 17, 25, 4            # an odd window length: the clips of an item start at odd and at even stream positions


def _token_items(rng, lengths):
    """frame-major token streams (tools/vq_codes_dataset.py): token = s K + code at position p, s = p mod S; every item starts at a frame"""
    return [((np.arange(n) % STAGES) * CODES + rng.integers(0, CODES, size=(n,))).astype(np.int32) for n in lengths]


def _write_run(tmp, extra):
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    pickle.dump(_token_items(rng, (120, 95, 70)), open(tmp / "np_tokens.pkl", "wb"))      # 4 + 3 + 2 windows, each with a tail of 20 > rf: 12 pieces
    pickle.dump(_token_items(rng, (117,)), open(tmp / "np_valid.pkl", "wb"))              # 4 windows, 17 = rf left: 4 pieces
    dp = dict(batch_size=BATCH, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_tokens.pkl"), receptive_field=RF,
              window_length=WIN, cuda_available=False, quantization_channels=STAGES * CODES, one_hot="canonical", token_positions=True)
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=1, print_every=1, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3,
              objective="nll", nll_windows={"stages": STAGES, "codes": CODES}, valid_audio_path=str(tmp / "np_valid.pkl"), validate_every=2)
    tp.update(extra)
    for n, p in (("wavenet", CFG), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))
    return dp


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "autograd"])
def test_train_with_windows_and_token_positions(tmp_path, monkeypatch, fused):
    """train() for 3 steps on a synthetic token pickle (S = 2, K = 32, items of unequal length) with "nll_windows", "token_positions"
    and validation: the first loss line is the float64 windowed NLL of the initial model on batch 0 - near ln 32, not ln 64 - and the
    validation line is written, scored under the same windows."""
    from music_amd import faster_audio_data as fad
    from music_amd import objective
    from music_amd import train as T
    from music_amd.model import wavenet
    made = []

    def ctor(**kw):
        net = wavenet(**kw)
        made.append((net, OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items())))
        return net
    scored = []
    real_score = objective.score

    def spy(net, x, target, **kw):
        scored.append(kw)
        return real_score(net, x, target, **kw)
    monkeypatch.setattr(objective, "score", spy)
    dp = _write_run(tmp_path, dict(fused_step=True) if fused else {})
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(T, "wavenet", ctor)
    torch.manual_seed(0)
    T.train()
    net, initial = made[0]
    ds = fad.audio_dataset(dp["audio_path"], RF, WIN, token_positions=True)
    assert len(ds) == 12
    pos = [ds[i]["audio_pos"] for i in range(BATCH)]
    assert pos == [17, 42, 67, 92] and {p % 2 for p in pos} == {0, 1}
    codes = torch.stack([ds[i]["audio_piece"] for i in range(BATCH)])
    target = torch.stack([ds[i]["audio_target"] for i in range(BATCH)])
    first = wavenet(**CFG)
    first.load_state_dict(initial)
    win = stage_windows(STAGES, CODES)
    ref = _windowed_ref(first, _onehot(codes, STAGES * CODES), target, win, pos)
    lines = open(tmp_path / "log" / "loss_log.log").read().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Trained over 1 pieces,Average loss is ")
    losses = [float(l.split(" ")[-1]) for l in lines]
    print("  loss lines %s; float64 windowed NLL of the initial model on batch 0 %.6f (ln 32 = %.4f, ln 64 = %.4f)"
          % (losses, ref["loss"], math.log(32), math.log(64)))
    assert all(math.isfinite(v) for v in losses)
    assert abs(losses[0] - ref["loss"]) < 1e-4
    assert abs(losses[0] - math.log(CODES)) < 0.2 < abs(losses[0] - math.log(STAGES * CODES))
    vlines = open(tmp_path / "log" / "valid_log.log").read().splitlines()
    assert len(vlines) == 1 and len(scored) == 1
    m = re.fullmatch(r"Trained over 2 pieces,Validation nll is (\S+), bits per sample (\S+), accuracy (\S+)", vlines[0])
    assert m, vlines[0]
    nll, bits, acc = (float(v) for v in m.groups())
    assert abs(nll - math.log(CODES)) < 0.3 and abs(bits - nll / math.log(2.0)) < 1e-9 * bits and 0.0 <= acc <= 1.0
    assert scored[0]["windows"] == win and scored[0]["window_pos"].tolist() == [17, 42, 67, 92] and scored[0]["window_pos"].is_cuda
    trained = net.state_dict()
    assert any(not torch.equal(v, trained[k].cpu()) for k, v in initial.items())
