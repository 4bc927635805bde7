"""Classifier-free guidance through the generators (music_amd/fast_generate.py, ae_generate.sample_code_stream, objective.guided_probs)
on the models of tests/class_cond_ref.DECODE_CASES with their last class as null_class (tests/cfg_ref.model_case) - the matrix-core
decoder at 64 / 64 / 256 channels with Q = 256 and the fp32 kernel at Q = 100:

  - teacher-forced probabilities of the guided launch against objective.guided_probs, within PROB_TOL (|s| + |s - 1|) per utterance:
    the 1e-3 of tests/test_gpu_class_cond_decode.py times the rule's own amplification of an error of its two logit rows; exact
    zeros outside every step's window; both rows of a pair carry the same values;
  - free-running greedy guided codes equal the float64 roll-out (margins: tests/test_cfg_ref.py), plain and windowed; the
    one-utterance call and a sampled batch's rows equal their single launches with streams=[u];
  - guidance=None issues exactly the entries of the call without the argument; a scale issues wn_cfg_decode_batch;
  - sample_code_stream(guidance=) stays inside every stage's range; the refusals.
Run with -m gpu."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cfg_ref as cr
from tests import class_cond_ref as ref

PROB_TOL = 1e-3
NAMES = sorted(ref.DECODE_CASES)


@functools.lru_cache(maxsize=None)
def _net(name):
    case = cr.model_case(name)
    return ref.build(case["cfg"], case["seed"]).cuda(), case


def _onehot(codes, Q):
    return torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()


def _spy_calls(monkeypatch):
    from music_amd import fast_generate as fg
    seen, real = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: seen.append(fn) or real(fn, *a))
    return seen


@pytest.mark.parametrize("windows", [None, "halves"], ids=["plain", "windowed"])
@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_guided_probabilities_are_the_objectives(name, windows, monkeypatch):
    from music_amd import fast_generate as fg, objective
    net, case = _net(name)
    cfg, classes, guide = case["cfg"], case["classes"], case["guidance"]
    Q, rf, U, n = cfg["quantization_channels"], net.receptive_field, len(classes), 9
    win = None if windows is None else [(0, Q // 2), (Q // 2, Q)]
    p0 = 3
    codes = ref.seed_codes(U, rf + n, Q, 78)
    x = _onehot(codes, Q)
    want = objective.guided_probs(net, x, classes, guide, windows=win, window_pos=p0 if win else None).view(U, n + 1, Q)
    assert want.dtype == torch.float64 and float((want.sum(2) - 1).abs().max()) < 1e-12
    # the float64 restatement agrees with the forward this is compared against
    p64 = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    lc = ref.logits(p64, cfg["dilations"], x.cpu().double(), torch.tensor(classes), cfg["filter_width"])
    lu = ref.logits(p64, cfg["dilations"], x.cpu().double(), torch.full((U,), cfg["null_class"]), cfg["filter_width"])
    g64 = torch.from_numpy(cr.combine(lc.numpy(), lu.numpy(), guide))
    r64 = ref.step_probs(g64, win, p0 if win else None).view(U, n + 1, Q)
    bars = torch.tensor([PROB_TOL * cr.amp([s]) for s in guide], dtype=torch.float64).view(U, 1, 1)
    assert bool(((want.cpu() - r64).abs() <= bars).all())
    # init forward over the first rf samples, rows doubled as [c, null], then n teacher-forced steps of the guided launch
    eng, _, rings, prev0, cls2 = fg._prime(net, x[:, :, :rf], classes, 2)
    assert fg._mfma_decode(eng) == (name == "mfma")
    cond, keep = fg._class_cond(net, eng, cls2, 2 * U, True)
    note0 = x[:, :, rf].repeat_interleave(2, 0).contiguous()
    forced = torch.cat([codes[:, rf + 1:], torch.zeros(U, 1, dtype=torch.int64)], 1).to(torch.int32).repeat_interleave(2, 0)
    smp = fg._Sampling(2 * U, None, None, None, 0, None, eng.device)
    wtail = fg._windows_of(win, p0, Q).tail(1) if win else None
    gtab = torch.tensor(guide, dtype=torch.float32, device=eng.device)
    seen = _spy_calls(monkeypatch)
    _, probs, note_out, _ = fg._launch_decode(net, eng, smp, rings, note0, prev0, 2 * U, n, 0, 1, "decode hand-off timed out", forced=forced,
                                              want_probs=True, cond=cond, win=wtail, guide=gtab)
    assert seen.count("wn_cfg_decode_batch") == 1 and not [s for s in seen if s.startswith("wn_decode") or s.startswith("wn_win")]
    assert torch.equal(probs[0::2].view(torch.int32), probs[1::2].view(torch.int32)) and torch.equal(note_out[0::2], note_out[1::2])
    err = (probs[0::2].double() - want[:, 1:]).abs().amax((1, 2)).cpu()
    for u, s in enumerate(guide):
        print("  %s %s: s = %g teacher-forced guided probabilities err %.2e (bar %.1e)" % (name, windows, s, float(err[u]), float(bars[u])))
    assert bool((err <= bars.view(-1)).all())
    if win:                                              # exact zeros outside every step's window, from both
        outside = torch.ones(n, Q, dtype=torch.bool)
        for j in range(n):
            lo, hi = win[(p0 + 1 + j) % len(win)]
            outside[j, lo:hi] = False
        assert bool((probs[0::2].cpu()[:, outside] == 0).all()) and bool((want[:, 1:].cpu()[:, outside] == 0).all())
    # the scales reach the launch: every utterance with s != 1 is far from the conditional model's distribution
    plain = objective.step_probs(net, x, classes=classes, windows=win, window_pos=p0 if win else None).view(U, n + 1, Q)[:, 1:]
    moved = (probs[0::2] - plain).abs().amax((1, 2)).cpu()
    for u, s in enumerate(guide):
        assert (float(moved[u]) > 10 * float(bars[u])) if s != 1.0 else (float(moved[u]) <= PROB_TOL), (u, s, float(moved[u]))


@pytest.mark.parametrize("name", NAMES)
def test_greedy_guided_codes_are_the_float64_roll_outs(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, classes, steps, guide = case["cfg"], case["classes"], case["steps"], case["guidance"]
    Q, rf, U = cfg["quantization_channels"], net.receptive_field, len(classes)
    seeds = ref.seed_codes(U, rf, Q, case["seed"])
    params = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    x0 = _onehot(seeds, Q)
    for win in (None, [(0, Q // 2), (Q // 2, Q)]):
        want, margin = cr.guided_rollout(params, cfg["dilations"], seeds, classes, cfg["null_class"], guide, steps, Q, cfg["filter_width"],
                                         windows=win, pos0=0)
        assert all(m > 1e-4 * cr.amp([s]) for m, s in zip(margin, guide))
        seen = _spy_calls(monkeypatch)
        got = fg.generate_codes_batch(net, x0, steps, correct_queue=True, classes=classes, guidance=guide, windows=win)
        assert seen.count("wn_cfg_decode_batch") == 1
        assert torch.equal(got.cpu(), want), (got.cpu(), want)
        for u in range(U):
            one = fg.generate_codes(net, x0[u:u + 1], steps, correct_queue=True, classes=[classes[u]], guidance=guide[u], windows=win)
            assert torch.equal(one.cpu(), want[u])
    # sampled: row u of the batch is the one-utterance launch with streams=[u] (one pair, one group of eight rows: the same form)
    kw = dict(correct_queue=True, temperature=1.0, seed=5, top_k=20)
    batch = fg.generate_codes_batch(net, x0, steps, classes=classes, guidance=guide, **kw)
    for u in range(U):
        one = fg.generate_codes_batch(net, x0[u:u + 1], steps, classes=[classes[u]], guidance=[guide[u]], streams=[u], **kw)
        assert torch.equal(one[0], batch[u]), (name, u)
    # s = 1 for everybody: the conditional model's launch, code for code
    cond_only = fg.generate_codes_batch(net, x0, steps, classes=classes, **kw)
    assert torch.equal(fg.generate_codes_batch(net, x0, steps, classes=classes, guidance=1.0, **kw), cond_only)


@pytest.mark.parametrize("name", NAMES)
def test_guidance_none_is_todays_call(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, U = cfg["quantization_channels"], len(classes)
    x0 = _onehot(ref.seed_codes(U, net.receptive_field, Q, 5), Q)
    seen = _spy_calls(monkeypatch)
    for kw in (dict(), dict(temperature=0.9, top_k=7, seed=3), dict(windows=[(0, Q // 2), (Q // 2, Q)], window_pos=1)):
        del seen[:]
        a = fg.generate_codes_batch(net, x0, 6, correct_queue=True, classes=classes, **kw)
        today = list(seen)
        del seen[:]
        b = fg.generate_codes_batch(net, x0, 6, correct_queue=True, classes=classes, guidance=None, **kw)
        assert seen == today and torch.equal(a, b) and not [s for s in seen if s.startswith("wn_cfg")]
        del seen[:]
        c = fg.generate_codes(net, x0[:1], 6, correct_queue=True, classes=classes[:1], guidance=None, **kw)
        assert not [s for s in seen if s.startswith("wn_cfg")] and torch.equal(c, a[0])
    logits = torch.randn(5, Q, device="cuda")
    del seen[:]
    fg.sample_logits(logits, guidance=None)
    assert seen == ["wn_sample_logits"]


@pytest.mark.parametrize("name", NAMES)
def test_guided_code_streams_stay_in_range(name):
    from music_amd import ae_generate
    net, case = _net(name)
    cfg, classes, guide = case["cfg"], case["classes"], case["guidance"]
    Q, rf, U = cfg["quantization_channels"], net.receptive_field, len(classes)
    stages, K, frames = 2, Q // 2, 5
    n0 = rf + (rf % 2)                                       # generation starts on a frame boundary
    start = torch.stack([torch.tensor([(p % stages) * K + int(v) % K for p, v in enumerate(row)]) for row in ref.seed_codes(U, n0, Q, 3)])
    for kw in (dict(), dict(temperature=1.0, seed=4), dict(temperature=1.3, top_p=0.8, seed=9)):
        codes = ae_generate.sample_code_stream(net, stages, K, frames, start, classes=classes, guidance=guide, **kw)
        assert codes.shape == (U, stages, frames) and int(codes.min()) >= 0 and int(codes.max()) < K
    strong = ae_generate.sample_code_stream(net, stages, K, frames, start, classes=classes, guidance=8.0)
    plain = ae_generate.sample_code_stream(net, stages, K, frames, start, classes=classes)
    assert strong.shape == plain.shape and int(strong.max()) < K and not torch.equal(strong, plain)


def test_refusals():
    from music_amd import ae_generate, fast_generate as fg
    from music_amd.model import wavenet
    net, case = _net("fp32")
    cfg, classes = case["cfg"], case["classes"]
    Q, U = cfg["quantization_channels"], len(classes)
    x0 = _onehot(ref.seed_codes(U, net.receptive_field, Q, 1), Q)
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg.generate_codes_batch(net, x0, 4, classes=classes, guidance=2.0)
    with pytest.raises(ValueError, match="classes"):
        fg.generate_codes_batch(net, x0, 4, correct_queue=True, guidance=2.0)
    with pytest.raises(ValueError, match="guidance"):
        fg.generate_codes_batch(net, x0, 4, correct_queue=True, classes=classes, guidance=[1.0, 2.0])
    with pytest.raises(ValueError, match="guidance"):
        fg.generate_codes(net, x0[:1], 4, correct_queue=True, classes=classes[:1], guidance=float("nan"))
    # a class-conditional model without null_class; a model without classes
    no_null = ref.build({k: v for k, v in cfg.items() if k != "null_class"}, 3).cuda()
    with pytest.raises(ValueError, match="null_class"):
        fg.generate_codes_batch(no_null, x0, 4, correct_queue=True, classes=classes, guidance=2.0)
    with pytest.raises(ValueError, match="null_class"):
        ae_generate.sample_code_stream(no_null, 2, Q // 2, 2, ref.seed_codes(U, net.receptive_field + net.receptive_field % 2, Q // 2, 1), classes=classes,
                                       guidance=2.0)
    torch.manual_seed(2)
    plain = wavenet(**{k: v for k, v in cfg.items() if not k.startswith("global") and k != "null_class"}).cuda()
    with pytest.raises(ValueError, match="global_classes"):
        fg.generate_codes_batch(plain, x0, 4, correct_queue=True, guidance=2.0)
    assert fg.generate_codes_batch(plain, x0, 4, correct_queue=True, guidance=None).shape == (U, 4)
    from music_amd import objective
    with pytest.raises(ValueError, match="null_class"):
        objective.guided_probs(no_null, _onehot(ref.seed_codes(U, net.receptive_field + 2, Q, 1), Q), classes, 2.0)
