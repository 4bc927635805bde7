"""The cached-queue decoder of a class-conditional WaveNet (music_amd/fast_generate.py: the tables of wn_gclass_fwd as the
per-utterance tables of wn_decode_batch_cond / wn_win_decode_batch), on both decode kernel families - the matrix-core decoder at
64 / 64 / 256 channels with Q = 256 and the fp32 kernel at Q = 100 (the cases of tests/class_cond_ref.py, whose float64 top-2 margins
tests/test_class_cond_cpu.py holds above 1e-4):

  - teacher-forced probabilities of the conditioned launch against objective.step_probs(net, x, classes=), within 1e-3, with the same
    support under position windows;
  - free-running greedy codes equal the float64 roll-out;
  - row u of a batch with per-utterance classes equals the single-utterance launch with streams=[u];
  - sample_code_stream(classes=) stays inside every stage's range, prior_score(classes=) is objective.score on the same tokens.
Run with -m gpu."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_cond_ref as ref

PROB_TOL = 1e-3


@functools.lru_cache(maxsize=None)
def _net(name):
    case = ref.DECODE_CASES[name]
    return ref.build(case["cfg"], case["seed"]).cuda(), case


def _onehot(codes, Q):
    return torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()


def _spy_calls(monkeypatch):
    from music_amd import fast_generate as fg
    seen, real = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: seen.append(fn) or real(fn, *a))
    return seen


@pytest.mark.parametrize("windows", [None, "halves"], ids=["plain", "windowed"])
@pytest.mark.parametrize("name", sorted(ref.DECODE_CASES))
def test_teacher_forced_probabilities_are_the_forwards(name, windows, monkeypatch):
    from music_amd import fast_generate as fg, objective
    net, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, rf, U, n = cfg["quantization_channels"], net.receptive_field, len(classes), 9
    win = None if windows is None else [(0, Q // 2), (Q // 2, Q)]
    p0 = 3
    codes = ref.seed_codes(U, rf + n, Q, 77)
    x = _onehot(codes, Q)
    want = objective.step_probs(net, x, classes=classes, windows=win, window_pos=p0 if win else None).view(U, n + 1, Q)
    # the float64 restatement agrees with the forward this is compared against
    p64 = ref.step_probs(ref.logits({k: v.detach().cpu().double() for k, v in net.state_dict().items()}, cfg["dilations"],
                                    x.cpu().double(), torch.tensor(classes), cfg["filter_width"]), win, p0 if win else None).view(U, n + 1, Q)
    assert float((want.cpu().double() - p64).abs().max()) <= PROB_TOL
    # init forward over the first rf samples with the classes, then n teacher-forced steps of the conditioned launch
    eng, _, rings, prev0, _ = fg._prime(net, x[:, :, :rf], classes)
    assert fg._mfma_decode(eng) == (name == "mfma")
    cond, keep = fg._class_cond(net, eng, classes, U, True)
    note0 = x[:, :, rf].contiguous()
    forced = torch.cat([codes[:, rf + 1:], torch.zeros(U, 1, dtype=torch.int64)], 1).to(torch.int32)
    smp = fg._Sampling(U, None, None, None, 0, None, eng.device)
    wtail = fg._windows_of(win, p0, Q).tail(1) if win else None
    seen = _spy_calls(monkeypatch)
    _, probs, _, _ = fg._launch_decode(net, eng, smp, rings, note0, prev0, U, n, 0, 1, "decode hand-off timed out", forced=forced,
                                               want_probs=True, cond=cond, win=wtail)
    assert ("wn_win_decode_batch" if win else "wn_decode_batch_cond") in seen
    err = float((probs - want[:, 1:]).abs().max())
    print("  %s %s: teacher-forced probabilities err %.2e (bar %.0e)" % (name, windows, err, PROB_TOL))
    assert err <= PROB_TOL
    if win:
        assert torch.equal(probs == 0, want[:, 1:] == 0)
    # another class: another distribution (the table reaches the launch)
    other = [(c + 1) % cfg["global_classes"] for c in classes]
    cond2, keep2 = fg._class_cond(net, eng, other, U, True)
    rings2 = fg._prime(net, x[:, :, :rf], other)[2]
    _, probs2, _, _ = fg._launch_decode(net, eng, smp, rings2, note0, prev0, U, n, 0, 1, "decode hand-off timed out", forced=forced,
                                        want_probs=True, cond=cond2, win=wtail)
    assert float((probs2 - probs).abs().max()) > 10 * PROB_TOL


@pytest.mark.parametrize("name", sorted(ref.DECODE_CASES))
def test_greedy_codes_are_the_float64_roll_outs_and_rows_are_single_launches(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, classes, steps = case["cfg"], case["classes"], case["steps"]
    Q, rf, U = cfg["quantization_channels"], net.receptive_field, len(classes)
    seeds = ref.seed_codes(U, rf, Q, case["seed"])
    want, margin = ref.greedy_rollout({k: v.detach().cpu() for k, v in net.state_dict().items()}, cfg["dilations"], seeds,
                                      torch.tensor(classes), steps, Q, cfg["filter_width"])
    assert margin > 1e-4
    x0 = _onehot(seeds, Q)
    seen = _spy_calls(monkeypatch)
    got = fg.generate_codes_batch(net, x0, steps, correct_queue=True, classes=classes)
    assert "wn_decode_batch_cond" in seen
    assert torch.equal(got.cpu(), want), (got.cpu(), want)
    for u in range(U):
        one = fg.generate_codes(net, x0[u:u + 1], steps, correct_queue=True, classes=[classes[u]])
        assert torch.equal(one.cpu(), want[u])
    # sampled: row u of the batch is the single-utterance launch with streams=[u] (the fp32 kernel has one form; on the matrix cores
    # both launches are one workgroup pair)
    kw = dict(correct_queue=True, temperature=1.0, seed=5)
    batch = fg.generate_codes_batch(net, x0, steps, classes=classes, **kw)
    for u in range(U):
        one = fg.generate_codes_batch(net, x0[u:u + 1], steps, classes=[classes[u]], streams=[u], **kw)
        assert torch.equal(one[0], batch[u]), (name, u)
    # the refusals: the mode without classes, the as-written recurrence
    with pytest.raises(ValueError, match="classes must be given"):
        fg.generate_codes_batch(net, x0, steps, correct_queue=True)
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg.generate_codes_batch(net, x0, steps, classes=classes)
    with pytest.raises(ValueError, match="class"):
        fg.generate_codes_batch(net, x0, steps, correct_queue=True, classes=[cfg["global_classes"]] * U)


def test_classes_are_refused_by_a_model_without_the_mode():
    from music_amd import ae_generate, fast_generate as fg
    from music_amd.model import wavenet
    cfg = {k: v for k, v in ref.DECODE_CASES["fp32"]["cfg"].items() if not k.startswith("global")}
    torch.manual_seed(2)
    net = wavenet(**cfg).cuda()
    x0 = _onehot(ref.seed_codes(2, net.receptive_field, 100, 1), 100)
    plain = fg.generate_codes_batch(net, x0, 4, correct_queue=True)
    assert plain.shape == (2, 4)
    with pytest.raises(ValueError, match="classes must be None"):
        fg.generate_codes_batch(net, x0, 4, correct_queue=True, classes=[0, 1])
    with pytest.raises(ValueError, match="classes must be None"):
        fg.generate_codes(net, x0[:1], 4, correct_queue=True, classes=[0])
    with pytest.raises(ValueError, match="classes must be None"):
        ae_generate.sample_code_stream(net, 2, 50, 2, ref.seed_codes(2, net.receptive_field + 1, 100, 1), classes=[0, 1])


@pytest.mark.parametrize("name", sorted(ref.DECODE_CASES))
def test_code_streams_stay_in_range_and_prior_score_is_the_objectives(name):
    from music_amd import ae_generate, fast_generate as fg, objective
    net, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, rf, U = cfg["quantization_channels"], net.receptive_field, len(classes)
    stages, K, frames = 2, Q // 2, 5
    n0 = rf + (rf % 2)                                       # generation starts on a frame boundary
    start = torch.stack([torch.tensor([(p % stages) * K + int(v) % K for p, v in enumerate(row)]) for row in ref.seed_codes(U, n0, Q, 3)])
    codes = ae_generate.sample_code_stream(net, stages, K, frames, start, temperature=1.0, seed=4, classes=classes)
    assert codes.shape == (U, stages, frames) and int(codes.min()) >= 0 and int(codes.max()) < K
    greedy = ae_generate.sample_code_stream(net, stages, K, frames, start, classes=classes)
    other = ae_generate.sample_code_stream(net, stages, K, frames, start, classes=[(c + 1) % cfg["global_classes"] for c in classes])
    assert greedy.shape == other.shape
    with pytest.raises(ValueError, match="classes must be given"):
        ae_generate.sample_code_stream(net, stages, K, frames, start)
    tokens = torch.cat([start, torch.stack([torch.tensor([(p % stages) * K + int(v) for p, v in enumerate(codes[u].t().reshape(-1).tolist())])
                                            for u in range(U)])], 1)
    a = ae_generate.prior_score(net, tokens, stages, K, classes=classes)
    b = objective.score(net, tokens[:, :-1].to(torch.int32).cuda(), tokens[:, rf:].to(torch.int64).cuda(), classes=classes,
                        windows=fg.stage_windows(stages, K), window_pos=rf)
    assert all(torch.equal(a[k], b[k]) for k in ("nll", "bits", "accuracy")) and bool(torch.isfinite(a["nll"]).all())
    with pytest.raises(ValueError, match="classes must be given"):
        ae_generate.prior_score(net, tokens, stages, K)
