"""Partially forced decode through the generators (music_amd/fast_generate.py: keep= of generate_codes / generate_codes_batch;
music_amd/ae_generate.py: sample_code_stream(keep_codes=), resynthesize(regions=)) on tiny models of both decode kernel families: the
class-conditional models of tests/class_cond_ref.DECODE_CASES with a null_class (tests/cfg_ref.model_case; the matrix-core decoder at
64 / 64 / 256 with Q = 256, the fp32 kernel at Q = 100) and the autoencoders of tests/test_gpu_cond_learned.py.  Run with -m gpu.

  - generate_codes_batch(keep=): the returned stream holds the kept codes; the launch's probabilities equal decode_batch_cond with the
    resolved stream forced, bit for bit; keep all -1 is the call without it; keep=None issues today's entries (the arguments:
    tests/test_infill_ref.py on the recorded traces); one case under windows=stage_windows(4, 16) and guidance=;
  - sample_code_stream(keep_codes= the first 2 of 4 stages): the kept stages come back unchanged, the sampled ones are what
    generate_codes_batch draws under the same seed, the result goes through decode_codes;
  - resynthesize(regions=): outside the regions the stream is the clip, the probabilities at every position are those of the
    teacher-forced launch on the composed stream, bit for bit; [(0, W)] is today's free run, [] feeds what teacher_forced=True feeds."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cfg_ref as cr
from tests import class_cond_ref as ref

NAMES = sorted(ref.DECODE_CASES)
STAGES, K = 4, 16


@functools.lru_cache(maxsize=None)
def _net(name):
    case = cr.model_case(name)
    return ref.build(case["cfg"], case["seed"]).cuda(), case


def _onehot(codes, Q):
    return torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()


def _keep(U, n, Q, seed, windows=None, pos=0):
    """(U, n) int64: rows with their own patterns - a stage prefix, alternating positions, a prompt of 3 -, random tokens (inside the
    window of position pos + j where there is a table), -1 elsewhere"""
    g = torch.Generator().manual_seed(seed)
    keep = torch.full((U, n), -1, dtype=torch.int64)
    for u in range(U):
        for j in range(n):
            kept = (j % 4 < 2, j % 2 == 1, j < 3)[u % 3]
            if kept:
                lo, hi = windows[(pos + j) % len(windows)] if windows else (0, Q)
                keep[u, j] = int(torch.randint(lo, hi, (1,), generator=g))
    return keep


def _spy_launch(monkeypatch, fg):
    """every _launch_decode with want_probs on (the kernel's other outputs do not depend on it) -> the list of (entry, codes, probs)"""
    seen, real_launch, real_call = [], fg._launch_decode, fg.call
    entries = []
    monkeypatch.setattr(fg, "call", lambda fn, *a: entries.append(fn) or real_call(fn, *a))

    def spy(*a, **kw):
        kw["want_probs"] = True
        out = real_launch(*a, **kw)
        seen.append((entries[-1], out[0].clone(), out[1].clone(), out[2].clone()))
        return out
    monkeypatch.setattr(fg, "_launch_decode", spy)
    return seen, entries


@pytest.mark.parametrize("name", NAMES)
def test_keep_is_held_and_is_the_forced_launch_on_the_resolved_stream(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, rf, U, n = cfg["quantization_channels"], net.receptive_field, len(classes), 11
    x0 = _onehot(ref.seed_codes(U, rf, Q, 21), Q)
    keep = _keep(U, n, Q, 5)
    assert (keep[:, 0] >= 0).any() and (keep[:, 0] < 0).any()
    kw = dict(correct_queue=True, classes=classes, temperature=0.9, seed=7)
    seen, entries = _spy_launch(monkeypatch, fg)
    out = fg.generate_codes_batch(net, x0, n, keep=keep, **kw)
    assert out.dtype == torch.int64 and tuple(out.shape) == (U, n) and out.is_cuda
    k = keep.cuda()
    assert torch.equal(out[k >= 0], k[k >= 0]) and int(out.min()) >= 0 and int(out.max()) < Q
    assert len(seen) == 1 and seen[0][0] == "wn_decode_batch_cond"
    _, codes, probs, note_out = seen[0]
    assert torch.equal(torch.where(k[:, 1:] >= 0, k[:, 1:], codes.to(torch.int64)), out[:, 1:])        # the fed stream is what comes back
    assert bool((k[:, 1:] >= 0).logical_and(codes.to(torch.int64) != k[:, 1:]).any()), "the model's own pick is still reported"
    # decode_batch_cond from the same prompt state with the resolved stream forced: the same bits
    eng, _, rings, prev0, cls = fg._prime(net, x0, classes, 1)
    cond, (cond_fg, cond_p1, _, _) = fg._class_cond(net, eng, cls, U, True)
    monkeypatch.undo()
    f_codes, f_probs, f_note, _ = fg.decode_batch_cond(net, rings, prev0, fg._note0(out[:, 0], 1, Q, eng.device), n - 1, forced=out[:, 1:].to(torch.int32),
                                                       want_probs=True, temperature=0.9, seed=7, cond_fg=cond_fg, cond_p1=cond_p1,
                                                       schedule=[(0, 0, 1)] * (eng.N + 1))
    assert torch.equal(f_probs.view(torch.int32), probs.view(torch.int32)) and torch.equal(f_codes, codes) and torch.equal(f_note, note_out)
    # the one-utterance call: row u with streams=[u] (one group of eight either way: the same kernel form)
    for u in range(U):
        one = fg.generate_codes_batch(net, x0[u:u + 1], n, keep=keep[u:u + 1], streams=[u], **dict(kw, classes=[classes[u]]))
        assert torch.equal(one[0], out[u]), (name, u)
    single = fg.generate_codes(net, x0[:1], n, keep=keep[0], **dict(kw, classes=classes[:1]))
    assert tuple(single.shape) == (n,) and torch.equal(single, out[0])


@pytest.mark.parametrize("name", NAMES)
def test_keep_all_free_and_keep_none_are_the_call_without_it(name, monkeypatch):
    from music_amd import fast_generate as fg
    net, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, U, n = cfg["quantization_channels"], len(classes), 9
    x0 = _onehot(ref.seed_codes(U, net.receptive_field, Q, 22), Q)
    seen, entries = _spy_launch(monkeypatch, fg)
    free = torch.full((U, n), -1, dtype=torch.int64)
    for kw in (dict(), dict(temperature=0.9, top_k=7, seed=3), dict(windows=[(0, Q // 2), (Q // 2, Q)], window_pos=1, temperature=1.1, seed=2)):
        del seen[:], entries[:]
        a = fg.generate_codes_batch(net, x0, n, correct_queue=True, classes=classes, **kw)
        today, pa = list(entries), seen[-1][2]
        del seen[:], entries[:]
        b = fg.generate_codes_batch(net, x0, n, correct_queue=True, classes=classes, keep=None, **kw)
        assert entries == today and torch.equal(a, b)
        del seen[:], entries[:]
        c = fg.generate_codes_batch(net, x0, n, correct_queue=True, classes=classes, keep=free, **kw)
        assert entries == today and torch.equal(a, c) and torch.equal(seen[-1][2].view(torch.int32), pa.view(torch.int32))
        d = fg.generate_codes(net, x0[:1], n, correct_queue=True, classes=classes[:1], keep=free[0], **kw)
        assert torch.equal(d, a[0])
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg.generate_codes_batch(net, x0, n, classes=classes, keep=free)
    assert tuple(fg.generate_codes_batch(net, x0, 1, correct_queue=True, classes=classes, keep=torch.tensor([[5], [-1], [6]])).shape) == (U, 1)
    assert fg.generate_codes_batch(net, x0, 1, correct_queue=True, classes=classes, keep=torch.tensor([[5], [6], [7]])).flatten().tolist() == [5, 6, 7]


@pytest.mark.parametrize("name", NAMES)
def test_keep_under_stage_windows_and_guidance(name, monkeypatch):
    from music_amd import ae_generate, fast_generate as fg
    net, case = _net(name)
    cfg, classes, guide = case["cfg"], case["classes"], case["guidance"]
    Q, U, frames = cfg["quantization_channels"], len(classes), 3
    n, pos = frames * STAGES, 8
    win = fg.stage_windows(STAGES, K)
    x0 = _onehot(ref.seed_codes(U, net.receptive_field, Q, 23), Q)
    keep = _keep(U, n, Q, 6, win, pos)
    kw = dict(correct_queue=True, classes=classes, guidance=guide, windows=win, window_pos=pos, temperature=1.0, seed=4)
    seen, entries = _spy_launch(monkeypatch, fg)
    out = fg.generate_codes_batch(net, x0, n, keep=keep, **kw)
    k = keep.cuda()
    assert torch.equal(out[k >= 0], k[k >= 0])
    assert entries.count("wn_cfg_decode_batch") == 1 and len(seen) == 1
    _, codes, probs, _ = seen[0]
    assert torch.equal(codes[0::2], codes[1::2]) and torch.equal(probs[0::2].view(torch.int32), probs[1::2].view(torch.int32))
    split = ae_generate.split_code_stream(out, STAGES, K)              # every token inside its position's stage
    assert tuple(split.shape) == (U, STAGES, frames)
    # the resolved stream kept entirely: the fully forced guided launch, the same bits; all free: the call without keep
    del seen[:]
    again = fg.generate_codes_batch(net, x0, n, keep=out, **kw)
    assert torch.equal(again, out) and torch.equal(seen[0][2].view(torch.int32), probs.view(torch.int32)) and torch.equal(seen[0][1], codes)
    assert torch.equal(fg.generate_codes_batch(net, x0, n, keep=torch.full((U, n), -1), **kw), fg.generate_codes_batch(net, x0, n, **kw))
    # a kept token of another stage is refused before any launch, the position named
    wrong = keep.clone()
    wrong[1, 5] = 3                                                     # position 5 is stream position 13: stage 1, [16, 32)
    del entries[:]
    with pytest.raises(ValueError, match=r"token 3 of utterance 1 at position 5 \(stream position 13\) lies outside that position's range \[16, 32\)"):
        fg.generate_codes_batch(net, x0, n, keep=wrong, **kw)
    assert entries == []


@functools.lru_cache(maxsize=None)
def _rvq4():
    """an autoencoder with a residual-VQ bottleneck of 4 stages x 16 codes (the long_encoding shapes of tests/test_gpu_cond_learned.py)"""
    from music_amd.model1 import wavenet_autoencoder
    from tests.test_gpu_cond_learned import CASES, _cfg
    torch.manual_seed(91)
    return wavenet_autoencoder(**dict(_cfg(**CASES["long_encoding"][0]), bottleneck="vq", vq_codes=K, vq_stages=STAGES)).cuda()


@pytest.mark.parametrize("name", NAMES)
def test_sample_code_stream_fills_the_absent_stages(name, monkeypatch):
    from music_amd import ae_generate, fast_generate as fg
    prior, case = _net(name)
    cfg, classes = case["cfg"], case["classes"]
    Q, rf, U, frames = cfg["quantization_channels"], prior.receptive_field, len(classes), 5
    n0 = rf + (-rf) % STAGES                                            # generation starts on a frame boundary
    start = torch.stack([torch.tensor([(p % STAGES) * K + int(v) % K for p, v in enumerate(row)]) for row in ref.seed_codes(U, n0, Q, 3)])
    coarse = torch.randint(0, K, (U, STAGES, frames), generator=torch.Generator().manual_seed(8))
    coarse[:, 2:] = -1                                                  # encode_codes(..., stages=2)'s format
    kw = dict(temperature=1.0, seed=4, classes=classes)
    seen, _ = _spy_launch(monkeypatch, fg)
    codes = ae_generate.sample_code_stream(prior, STAGES, K, frames, start, keep_codes=coarse, **kw)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (U, STAGES, frames) and int(codes.min()) >= 0 and int(codes.max()) < K
    assert torch.equal(codes[:, :2].cpu(), coarse[:, :2])
    # the sampled stages: generate_codes_batch's draw under the same seed, given the kept ones
    x = _onehot(start[:, -rf:], Q)
    tokens = fg.generate_codes_batch(prior, x, frames * STAGES, correct_queue=True, windows=fg.stage_windows(STAGES, K), window_pos=n0,
                                     keep=ae_generate.join_code_stream(coarse, K), **kw)
    assert torch.equal(ae_generate.split_code_stream(tokens, STAGES, K), codes)
    # the fine stages are drawn GIVEN the kept ones: the prior was fed the caller's coarse codes, not its own draws, and the
    # distributions behind them are other ones than the call without keep_codes meets
    plain = ae_generate.sample_code_stream(prior, STAGES, K, frames, start, **kw)
    assert not torch.equal(plain[:, :2].cpu(), coarse[:, :2])
    assert len(seen) == 3 and seen[0][0] == seen[1][0] == seen[2][0] == "wn_win_decode_batch"
    assert torch.equal(seen[0][2].view(torch.int32), seen[1][2].view(torch.int32)), "sample_code_stream's launch is generate_codes_batch's"
    assert not torch.equal(seen[0][2][:, 2:], seen[2][2][:, 2:])
    monkeypatch.undo()
    # every kept pattern: everything (nothing is drawn), nothing (today's call), single frames
    full = ae_generate.sample_code_stream(prior, STAGES, K, frames, start, keep_codes=codes, **kw)
    assert torch.equal(full, codes)
    none = ae_generate.sample_code_stream(prior, STAGES, K, frames, start, keep_codes=torch.full((U, STAGES, frames), -1), **kw)
    assert torch.equal(none, plain)
    some = torch.full((U, STAGES, frames), -1)
    some[:, :, 2] = codes[:, :, 2].cpu()
    assert torch.equal(ae_generate.sample_code_stream(prior, STAGES, K, frames, start, keep_codes=some, **kw)[:, :, 2], codes[:, :, 2])
    # ... and the result goes through decode_codes
    ae = _rvq4()
    W = frames * 8
    audio, probs = ae_generate.decode_codes(ae, codes, W, want_probs=True)
    assert tuple(audio.shape) == (U, W) and bool(torch.isfinite(probs).all())


@pytest.mark.parametrize("name", ["long_encoding", "fast64_bias"])
def test_resynthesize_regions(name, monkeypatch):
    """long_encoding: the matrix-core decoder (64 / 64 / 256); fast64_bias: the fp32 kernel (72 skip channels)"""
    from music_amd import ae_generate, fast_generate as fg
    from tests.test_gpu_cond_learned import W, _batch, _build
    net, cfg, B = _build(name)
    x, _ = _batch(net, cfg, B)
    rf = net.receptive_field
    wnet, _ = ae_generate.conditioned_decoder(net, net.conditioning_projections())
    assert fg._mfma_decode(wnet._engine_for(x.device)) == (name == "long_encoding")
    clip = x.argmax(1)[:, rf:]                                          # (B, W - 1): the sample behind output position j
    regions = [(40, 90), (200, 201), (W - 3, W)]
    inside = ae_generate._region_mask(regions, B, W).cuda()
    kw = dict(want_probs=True, temperature=0.9, seed=3)
    calls, real = [], ae_generate._decode_from_encoding
    monkeypatch.setattr(ae_generate, "_decode_from_encoding", lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    launches, real_call = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: launches.append(fn) or real_call(fn, *a))
    codes, probs, enc = ae_generate.resynthesize(net, x, regions=regions, **kw)
    assert len([e for e in launches if "decode" in e]) == 2, "the priming launch and ONE launch for the W positions"
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (B, W) and tuple(probs.shape) == (B, W, 256)
    out = ~inside[:, :W - 1]
    assert torch.equal(codes[:, :W - 1][out], clip[out]), "outside the regions the stream is the clip"
    assert not torch.equal(codes[:, :W - 1][~out], clip[~out]), "inside them it is the model's"
    # the teacher-forced launch on the composed stream: the same probabilities at every position
    (a, k), = calls
    composed = torch.cat([codes[:, :W - 1], torch.zeros(B, 1, dtype=torch.int64, device=codes.device)], 1).to(torch.int32)
    f_codes, f_probs = real(*a[:6], composed, **k)
    assert torch.equal(f_probs.view(torch.int32), probs.view(torch.int32))
    assert torch.equal(f_codes.to(torch.int64)[inside], codes[inside])
    # [(0, W)]: today's free run; []: what teacher_forced=True feeds; per-clip lists
    free = ae_generate.resynthesize(net, x, **kw)
    whole = ae_generate.resynthesize(net, x, regions=[(0, W)], **kw)
    assert torch.equal(whole[0], free[0]) and torch.equal(whole[1].view(torch.int32), free[1].view(torch.int32))
    tf = ae_generate.resynthesize(net, x, teacher_forced=True, **kw)
    none = ae_generate.resynthesize(net, x, regions=[], **kw)
    assert torch.equal(none[1].view(torch.int32), tf[1].view(torch.int32))
    assert torch.equal(none[0][:, :W - 1], clip) and torch.equal(none[0][:, W - 1], tf[0][:, W - 1])
    per = ae_generate.resynthesize(net, x, regions=[regions] + [[]] * (B - 1), **kw)
    assert torch.equal(per[1][0].view(torch.int32), probs[0].view(torch.int32)) and torch.equal(per[1][1:].view(torch.int32), tf[1][1:].view(torch.int32))
    assert torch.equal(per[0][0], codes[0]) and torch.equal(per[0][1:, :W - 1], clip[1:])
    with pytest.raises(ValueError, match="teacher_forced"):
        ae_generate.resynthesize(net, x, regions=regions, teacher_forced=True)
    with pytest.raises(ValueError, match="region"):
        ae_generate.resynthesize(net, x, regions=[(0, W + 1)])
