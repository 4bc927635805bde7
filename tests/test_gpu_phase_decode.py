"""The cached-queue decoder of a phase-conditioned WaveNet (music_amd/fast_generate.py: the phase tables' columns as the per-utterance
tables of wn_decode_batch_cond under a tile schedule of P frames), on both decode kernel families - the matrix-core decoder at 64 / 64 /
256 channels with Q = 256, P = 4, and the fp32 kernel (decode_k) at the general plan's shape, filter width 3, Q = 40, 24 / 20 / 36, P = 3:

  - teacher-forced probabilities of the launch against objective.step_probs(net, x, phase_pos=), within 1e-3 - also where the launch's
    first steps lie in front of stream position 0 (priming steps: the launcher hands the entry pos0 mod P);
  - free-running greedy codes equal the float64 roll-out, also from a start piece longer than phase_pos leaves room for;
  - phase_pos + P gives the same codes, phase_pos + 1 others;
  - one guided pair with classes against objective.guided_probs;
  - sample_code_stream / prior_score detect the prior and run it without windows.
The bars are tests/test_gpu_class_cond_decode.py's.  Run with -m gpu."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_cond_ref as cref
from tests import phase_ref as ref

PROB_TOL = 1e-3
DIL = [1, 2, 4]
CASES = {
    "mfma": dict(cfg=dict(filter_width=2, dilations=DIL, dilation_channels=64, residual_channels=64, skip_channels=256,
                          quantization_channels=256, use_bias=False, phase_period=4), seed=21, steps=12),
    "fp32": dict(cfg=dict(filter_width=3, dilations=DIL, dilation_channels=24, residual_channels=20, skip_channels=36,
                          quantization_channels=40, use_bias=False, phase_period=3), seed=22, steps=12),
}
GUIDED = dict(cfg=dict(CASES["mfma"]["cfg"], global_classes=4, global_channels=7, null_class=3), seed=23)


@functools.lru_cache(maxsize=None)
def _net(name):
    case = GUIDED if name == "guided" else CASES[name]
    return cref.build(case["cfg"], case["seed"]).cuda(), case


def _onehot(codes, Q):
    return torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()


def _params(net):
    return {k: v.detach().cpu() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("where", ["inside", "priming_in_front_of_0"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_teacher_forced_probabilities_are_the_forwards(name, where, monkeypatch):
    """x holds rf + n codes.  The init forward covers the first rf samples; the launch then runs n teacher-forced steps.
    inside: the first target sits at stream position 6, the launch is told phase_pos = 6 and pos0 = 1.
    priming: the launch is told phase_pos = 1 and pos0 = -5 - its steps are priming steps that start at stream position -4, in front of
    the stream, where the entry alone would read column 0.  The phase is periodic, so the forward it is held to is the one whose first
    target sits at a position congruent to -5 mod P; the launcher hands the entry -4 mod P, never a negative position."""
    from music_amd import fast_generate as fg, objective
    net, case = _net(name)
    cfg = case["cfg"]
    Q, rf, P, U, n = cfg["quantization_channels"], net.receptive_field, cfg["phase_period"], 3, 9
    dec_phase, dec_pos0 = (6, 1) if where == "inside" else (1, -5)
    pf = dec_phase + dec_pos0 - 1                                # the stream position of the forward's first target ...
    pf = pf if pf >= 0 else pf % P + 2 * P                       # ... or one congruent to it
    codes = cref.seed_codes(U, rf + n, Q, 77)
    x = _onehot(codes, Q)
    want = objective.step_probs(net, x, phase_pos=pf).view(U, n + 1, Q)
    p64 = cref.step_probs(ref.logits({k: v.double() for k, v in _params(net).items()}, DIL, x.cpu().double(), [pf] * U, None,
                                     cfg["filter_width"])).view(U, n + 1, Q)
    assert float((want.cpu().double() - p64).abs().max()) <= PROB_TOL
    eng, _, rings, prev0, _ = fg._prime(net, x[:, :, :rf], phase_pos=pf)
    assert fg._mfma_decode(eng) == (name == "mfma")
    note0 = x[:, :, rf].contiguous()
    forced = torch.cat([codes[:, rf + 1:], torch.zeros(U, 1, dtype=torch.int64)], 1).to(torch.int32)
    seen, real = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: seen.append((fn, a)) or real(fn, *a))
    _, probs, _, _ = fg.decode_batch_cond(net, rings.clone(), prev0, note0, n, pos0=dec_pos0, phase_pos=dec_phase, forced=forced,
                                          want_probs=True)
    launch = [a for fn, a in seen if fn == "wn_decode_batch_cond"]
    assert len(launch) == 1 and launch[0][-2] == (dec_phase + dec_pos0) % P and launch[0][-3] == P     # pos0 mod P >= 0; le = P
    err = float((probs - want[:, 1:]).abs().max())
    print("  %s %s: teacher-forced probabilities err %.2e (bar %.0e)" % (name, where, err, PROB_TOL))
    assert err <= PROB_TOL
    # one position further: another distribution (the table reaches the launch)
    _, probs2, _, _ = fg.decode_batch_cond(net, rings.clone(), prev0, note0, n, pos0=dec_pos0 + 1, phase_pos=dec_phase, forced=forced,
                                           want_probs=True)
    assert float((probs2 - probs).abs().max()) > 10 * PROB_TOL
    with pytest.raises(ValueError, match="phase_pos"):
        fg.decode_batch_cond(net, rings.clone(), prev0, note0, n, forced=forced)
    with pytest.raises(ValueError, match="negative"):
        fg.decode_batch_cond(net, rings.clone(), prev0, note0, n, phase_pos=-1, forced=forced)


@pytest.mark.parametrize("name", sorted(CASES))
def test_greedy_codes_are_the_float64_roll_outs(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, steps = case["cfg"], case["steps"]
    Q, rf, P, U = cfg["quantization_channels"], net.receptive_field, cfg["phase_period"], 3
    seeds = cref.seed_codes(U, rf, Q, case["seed"])
    x0 = _onehot(seeds, Q)
    # phase_pos = 2: the start piece (rf > 2 samples) reaches in front of stream position 0; 1000003: far inside a stream
    for p0 in (2, 1000003):
        want, margin = ref.greedy_rollout(_params(net), DIL, seeds, p0, steps, Q, None, cfg["filter_width"])
        assert margin > 1e-4, margin
        got = fg.generate_codes_batch(net, x0, steps, correct_queue=True, phase_pos=p0)
        assert torch.equal(got.cpu(), want), (p0, got.cpu(), want)
        one = fg.generate_codes(net, x0[1:2], steps, correct_queue=True, phase_pos=p0)
        assert torch.equal(one.cpu(), want[1])
    # sampled: a shift by the period is the same launch bit for bit, a shift by one is not
    kw = dict(correct_queue=True, temperature=1.0, seed=5)
    a = fg.generate_codes_batch(net, x0, 40, phase_pos=7, **kw)
    b = fg.generate_codes_batch(net, x0, 40, phase_pos=7 + P, **kw)
    c = fg.generate_codes_batch(net, x0, 40, phase_pos=8, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError, match="phase_pos must be given"):
        fg.generate_codes_batch(net, x0, steps, correct_queue=True)
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg.generate_codes_batch(net, x0, steps, phase_pos=3)
    with pytest.raises(ValueError, match="negative"):
        fg.generate_codes(net, x0[:1], steps, correct_queue=True, phase_pos=-2)
    with pytest.raises(ValueError, match="one integer"):
        fg.generate_codes_batch(net, x0, steps, correct_queue=True, phase_pos=[1, 2, 3])


def test_phase_pos_is_refused_by_a_model_without_the_mode():
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    cfg = {k: v for k, v in CASES["fp32"]["cfg"].items() if k != "phase_period"}
    torch.manual_seed(2)
    net = wavenet(**cfg).cuda()
    x0 = _onehot(cref.seed_codes(2, net.receptive_field, 40, 1), 40)
    assert fg.generate_codes_batch(net, x0, 4, correct_queue=True).shape == (2, 4)
    with pytest.raises(ValueError, match="phase_pos must be None"):
        fg.generate_codes_batch(net, x0, 4, correct_queue=True, phase_pos=0)
    with pytest.raises(ValueError, match="phase_pos must be None"):
        fg.generate_codes(net, x0[:1], 4, correct_queue=True, phase_pos=0)


def test_one_guided_pair_with_classes_against_the_guided_forward():
    """classes + phase + guidance: rows [class, null_class] of one utterance, teacher-forced, against objective.guided_probs"""
    from music_amd import fast_generate as fg, objective
    net, case = _net("guided")
    cfg = case["cfg"]
    Q, rf, P, n, p0, s = cfg["quantization_channels"], net.receptive_field, cfg["phase_period"], 9, 5, 2.0
    codes = cref.seed_codes(1, rf + n, Q, 31)
    x = _onehot(codes, Q)
    want = objective.guided_probs(net, x, [1], s, phase_pos=p0).view(1, n + 1, Q)
    rows = [1, cfg["null_class"]]
    x2 = x.repeat_interleave(2, 0)
    eng, _, rings, prev0, _ = fg._prime(net, x2[:, :, :rf].contiguous(), rows, phase_pos=p0)
    forced = torch.cat([codes[:, rf + 1:], torch.zeros(1, 1, dtype=torch.int64)], 1).to(torch.int32).repeat_interleave(2, 0)
    _, probs, _, _ = fg.decode_batch_cond(net, rings, prev0, x2[:, :, rf].contiguous(), n, pos0=1, phase_pos=p0, classes=rows,
                                          forced=forced, want_probs=True, guidance=[s])
    err = float((probs[0].double().cpu() - want[0, 1:].cpu()).abs().max())
    print("  guided pair: teacher-forced probabilities err %.2e (bar %.0e)" % (err, PROB_TOL))
    assert err <= PROB_TOL
    plain = objective.step_probs(net, x, classes=[1], phase_pos=p0).view(1, n + 1, Q)
    assert float((plain[0, 1:].double().cpu() - want[0, 1:].cpu()).abs().max()) > 10 * PROB_TOL
    # the generator's way in: a guided greedy run is deterministic and moves with the scale
    g2 = fg.generate_codes_batch(net, x[:, :, :rf].contiguous(), 16, correct_queue=True, classes=[1], guidance=s, phase_pos=p0)
    g2b = fg.generate_codes(net, x[:, :, :rf].contiguous(), 16, correct_queue=True, classes=[1], guidance=s, phase_pos=p0 + P)
    assert torch.equal(g2[0], g2b)


def test_code_streams_come_from_a_detected_phase_prior_without_windows(monkeypatch):
    from music_amd import ae_generate, fast_generate as fg, objective
    net, case = _net("fp32")
    cfg = case["cfg"]
    K, rf, stages, U, frames = cfg["quantization_channels"], net.receptive_field, cfg["phase_period"], 2, 5
    n0 = rf + (-rf) % stages                                     # generation starts on a frame boundary
    start = cref.seed_codes(U, n0, K, 3)
    seen, real = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: seen.append(fn) or real(fn, *a))
    codes = ae_generate.sample_code_stream(net, stages, K, frames, start, start_pos=stages * 4, temperature=1.0, seed=4)
    assert codes.shape == (U, stages, frames) and int(codes.min()) >= 0 and int(codes.max()) < K
    assert "wn_decode_batch_cond" in seen and "wn_win_decode_batch" not in seen
    tokens = fg.generate_codes_batch(net, _onehot(start[:, -rf:], K), frames * stages, correct_queue=True, temperature=1.0, seed=4,
                                     phase_pos=stages * 4 + n0)
    assert torch.equal(codes, ae_generate.split_code_stream(tokens, stages, K, "phase").to(codes.device))
    keep = codes.clone()
    keep[:, 1:] = -1
    kept = ae_generate.sample_code_stream(net, stages, K, frames, start, start_pos=stages * 4, keep_codes=keep)
    assert torch.equal(kept[:, 0], codes[:, 0])
    stream = torch.cat([start, ae_generate.join_code_stream(codes, K, "phase").cpu()], 1)
    a = ae_generate.prior_score(net, stream, stages, K, start_pos=stages * 4)
    b = objective.score(net, stream[:, :-1].to(torch.int32).cuda(), stream[:, rf:].to(torch.int64).cuda(), phase_pos=stages * 4 + rf)
    assert all(torch.equal(a[k], b[k]) for k in ("nll", "bits", "accuracy")) and bool(torch.isfinite(a["nll"]).all())
    with pytest.raises(ValueError, match="phase_period = %d and quantization_channels = %d" % (stages, K)):
        ae_generate.sample_code_stream(net, stages + 1, K, frames, torch.zeros(U, rf + (-rf) % (stages + 1), dtype=torch.int64))
