"""CPU conditions of partially forced decode (include/wavenet_hip.h, wn_decode): tests/infill_ref.py's masked recurrence against
tests/decode_ref.py and tests/cfg_ref.py, the pure host pieces of the feature - ae_generate.join_code_stream, fast_generate.check_keep,
the refusals of sample_code_stream(keep_codes=) and resynthesize(regions=) - and, on the recorded launch traces, that keep=None is
today's call.  No device is touched."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cfg_ref as cr
from tests import decode_ref as dr
from tests import infill_ref as ir

WIN = [(0, 20), (20, 50), (7, 8)]


def _case(k, U, seed, cond=True):
    rng = np.random.default_rng(seed)
    net = dr.Net(k, [1, 2, 3], 12, 10, 24, 50, bias=True, seed=seed + 1)
    eye = np.eye(net.Q, dtype=np.float32)
    note0 = eye[rng.integers(0, net.Q, U)]
    prev0 = eye[rng.integers(0, net.Q, (U, k - 1))] if k > 1 else None
    c = None
    if cond:
        c = dict(shift=[2, 1, 0, 3], q=[0, 2, 0, 1], le=3, pos0=-1,
                 fg=(rng.standard_normal((U, net.N, 3, 2 * net.D)) * 0.5).astype(np.float32),
                 p1=(rng.standard_normal((U, 3, net.S)) * 0.5).astype(np.float32))
    return net, net.rings(U, seed + 2), note0, prev0, c, rng


def _same(a, b, keys):
    for key in keys:
        x, y = a[key], b[key]
        if key == "rings":
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), key
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y)), key


KEYS = ("probs", "logits", "codes", "rings", "note_out", "prev_out")


@pytest.mark.parametrize("k,mode", [(2, "64"), (3, "64"), (1, "64"), (2, "32"), (3, "x3")])
def test_masked_ref_is_decode_ref_at_both_ends(k, mode):
    """no negative entry: decode_ref(forced=); all -1 (or no mask): the free run - every output, bit for bit"""
    U, n = 3, 9
    net, rings, note0, prev0, cond, rng = _case(k, U, 40 + k)
    kw = dict(step0=2 ** 33 + 5, cond=cond, windows=WIN, win_pos0=2, mode=mode)
    forced = ir.in_window_stream(rng, U, n, net.Q, WIN, 2)
    a = ir.masked_ref(net, rings, note0, prev0, n, forced, **kw)
    _same(a, dr.decode_ref(net, rings, note0, prev0, n, forced=forced, **kw), KEYS)
    assert np.array_equal(a["fed"], forced)
    free = dr.decode_ref(net, rings, note0, prev0, n, **kw)
    for m in (None, np.full((U, n), -1), np.full((U, n), -7)):
        b = ir.masked_ref(net, rings, note0, prev0, n, m, **kw)
        _same(b, free, KEYS)
        assert np.array_equal(b["fed"], free["codes"])
    # the as-written recurrence (filter width 2) and a temperature travel through the stepping too
    if k == 2:
        kw2 = dict(step0=3, push_input=0, temperature=0.7, mode=mode)
        _same(ir.masked_ref(net, rings, note0, prev0, n, forced, **kw2), dr.decode_ref(net, rings, note0, prev0, n, forced=forced, **kw2), KEYS)


@pytest.mark.parametrize("kind", ir.MASKS)
def test_masked_ref_feeds_the_resolved_stream(kind):
    """a real mask: the run equals the fully forced run on ITS resolved stream (the identity the GPU tests hold the kernels to), the
    kept entries are fed, the free ones are the run's own codes, and the mask matters (it is neither of the two ends)"""
    U, n = 3, 9
    net, rings, note0, prev0, cond, rng = _case(2, U, 50)
    kw = dict(step0=4, cond=cond, windows=WIN, win_pos0=1)
    mask = ir.make_mask(kind, ir.in_window_stream(rng, U, n, net.Q, WIN, 1))
    assert (mask >= 0).any() and (mask < 0).any()
    a = ir.masked_ref(net, rings, note0, prev0, n, mask, **kw)
    assert np.array_equal(a["fed"][mask >= 0], mask[mask >= 0]) and np.array_equal(a["fed"][mask < 0], a["codes"][mask < 0])
    _same(a, dr.decode_ref(net, rings, note0, prev0, n, forced=a["fed"], **kw), KEYS)
    free = dr.decode_ref(net, rings, note0, prev0, n, **kw)
    # (the last step's entry reaches note_out alone)
    assert np.array_equal(a["probs"], free["probs"]) == (kind == "last_only")


def test_per_row_masks_differ_inside_a_step():
    stream = np.arange(9 * 8).reshape(9, 8)
    m = ir.make_mask("per_row", stream)
    for s in range(8):
        assert (m[:, s] >= 0).any() and (m[:, s] < 0).any(), "a row forced at step s next to a row free at step s"
    assert np.array_equal(ir.make_mask("stage_prefix", stream) >= 0, np.tile(np.arange(8) % 4 < 2, (9, 1)))
    pm = ir.pair_mask("per_row", np.repeat(stream[:3], 2, 0))
    assert np.array_equal(pm[0::2], pm[1::2]) and np.array_equal(pm[0::2], ir.make_mask("per_row", stream[:3]))


@pytest.mark.parametrize("k", [2, 3])
def test_masked_guided_ref_is_guided_ref_at_both_ends(k):
    P, n = 2, 7
    net, rings, note0, prev0, cond, rng = _case(k, 2 * P, 60 + k)
    note0 = np.repeat(note0[0::2], 2, 0)
    prev0 = np.repeat(prev0[0::2], 2, 0)
    g = np.array([1.5, -0.5])
    kw = dict(step0=6, cond=cond, windows=WIN, win_pos0=1)
    forced = np.repeat(ir.in_window_stream(rng, P, n, net.Q, WIN, 1), 2, 0)
    keys = KEYS + ("g",)
    a = ir.masked_guided_ref(net, rings, note0, prev0, n, g, forced, **kw)
    _same(a, cr.guided_ref(net, rings, note0, prev0, n, g, forced=forced, **kw), keys)
    free = cr.guided_ref(net, rings, note0, prev0, n, g, **kw)
    b = ir.masked_guided_ref(net, rings, note0, prev0, n, g, np.full((2 * P, n), -1), **kw)
    _same(b, free, keys)
    assert b["margin"] == free["margin"]
    # a real mask: the fully forced guided run on its resolved stream
    mask = ir.pair_mask("alternate", forced)
    c = ir.masked_guided_ref(net, rings, note0, prev0, n, g, mask, **kw)
    _same(c, cr.guided_ref(net, rings, note0, prev0, n, g, forced=np.repeat(c["fed"], 2, 0), **kw), keys)
    assert np.array_equal(c["fed"][mask[0::2] >= 0], mask[0::2][mask[0::2] >= 0])


# ---------------------------------------------------------------------------------------------- join / split
def test_join_is_the_inverse_of_split():
    from music_amd.ae_generate import join_code_stream, split_code_stream
    g = torch.Generator().manual_seed(3)
    B, S, Le, K = 3, 4, 5, 16
    codes = torch.randint(0, K, (B, S, Le), generator=g)
    tok = join_code_stream(codes, K)
    assert tok.shape == (B, Le * S) and tok.dtype == torch.int64
    assert torch.equal(split_code_stream(tok, S, K), codes)
    # frame-major, token = s K + code: the expression of tools/vq_codes_dataset.py
    want = (codes + torch.arange(S)[None, :, None] * K).permute(0, 2, 1).reshape(B, -1)
    assert torch.equal(tok, want)
    assert torch.equal(join_code_stream(split_code_stream(tok, S, K), K), tok)
    # -1 stays -1 (the absent stages of encode_codes(..., stages=2)); everything else keeps its token
    part = codes.clone()
    part[:, 2:] = -1
    part[1, 1, 3] = -1
    t2 = join_code_stream(part, K)
    assert torch.equal(t2 < 0, (part < 0).permute(0, 2, 1).reshape(B, -1)) and torch.equal(t2[t2 >= 0], tok[t2 >= 0]) and int(t2.min()) == -1
    assert torch.equal(join_code_stream(part.numpy(), K), t2) and torch.equal(join_code_stream(part.to(torch.int32), K), t2)
    for bad in (codes.float(), codes[0], codes.bool()):
        with pytest.raises(ValueError, match="integers"):
            join_code_stream(bad, K)
    for v in (K, -2):
        wrong = codes.clone()
        wrong[2, 1, 4] = v
        with pytest.raises(ValueError, match=r"clip 2 at frame 4, stage 1 lies outside \[0, 16\)"):
            join_code_stream(wrong, K)


# ---------------------------------------------------------------------------------------------- check_keep
def test_check_keep():
    from music_amd import fast_generate as fg
    U, n, Q = 3, 8, 64
    win = fg._Windows(fg.stage_windows(4, 16), 6, Q)               # position j sits at stream position 6 + j: stage (6 + j) % 4
    keep = torch.full((U, n), -1, dtype=torch.int64)
    for j in range(n):
        keep[j % U, j] = ((6 + j) % 4) * 16 + j
    out = fg.check_keep(keep, U, n, Q, win)
    assert out.dtype == torch.int64 and out.device.type == "cpu" and torch.equal(out, keep)
    assert torch.equal(fg.check_keep(keep.numpy().astype(np.int32), U, n, Q, win), keep)
    assert torch.equal(fg.check_keep(keep.tolist(), U, n, Q), keep)
    assert torch.equal(fg.check_keep(keep[0], 1, n, Q, win), keep[:1])          # (note_num,) for one utterance
    assert torch.equal(fg.check_keep(torch.full((U, n), -1), U, n, Q, win), torch.full((U, n), -1))
    for bad in (keep[:, :-1], keep[:2], keep[0], keep[None]):
        with pytest.raises(ValueError, match=r"keep must be \(3, 8\)"):
            fg.check_keep(bad, U, n, Q, win)
    for bad in (keep.float(), keep.double().numpy(), keep >= 0):
        with pytest.raises(ValueError, match="keep must hold integers"):
            fg.check_keep(bad, U, n, Q, win)
    for v in (Q, Q + 100, -2):
        wrong = keep.clone()
        wrong[1, 5] = v
        with pytest.raises(ValueError, match=r"token %d of utterance 1 at position 5 is neither -1 nor a token in \[0, 64\)" % v):
            fg.check_keep(wrong, U, n, Q)
    # a token of another stage: position 5 is stream position 11, stage 3, range [48, 64)
    wrong = keep.clone()
    wrong[2, 5] = 47
    with pytest.raises(ValueError, match=r"token 47 of utterance 2 at position 5 \(stream position 11\) lies outside that position's "
                                         r"range \[48, 64\)"):
        fg.check_keep(wrong, U, n, Q, win)
    assert torch.equal(fg.check_keep(wrong, U, n, Q), wrong)        # without a table every token of the alphabet is welcome
    # the generators refuse it on the as-written recurrence, before anything else
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg._keep_of(keep, U, n, Q, None, False)
    assert fg._keep_of(None, U, n, Q, None, False) is None
    # forced= of the launchers: a host tensor with an entry >= Q is refused, negative entries are welcome
    fg._check_forced(torch.tensor([[0, -1, Q - 1]]), Q, "x")
    fg._check_forced(None, Q, "x")
    with pytest.raises(ValueError, match="forced holds a code >= Q"):
        fg._check_forced(torch.tensor([[0, -1, Q]]), Q, "decode_batch_cond")


def test_sample_code_stream_refuses_a_kept_code_outside_the_codebook():
    from music_amd import ae_generate
    from music_amd.model import wavenet
    torch.manual_seed(0)
    stages, K, frames = 4, 16, 3
    prior = wavenet(2, [1, 2], 8, 8, 16, stages * K, False)
    rf = prior.receptive_field
    n0 = rf + (-rf) % stages
    start = torch.stack([torch.tensor([(p % stages) * K + (3 * p + u) % K for p in range(n0)]) for u in range(2)])
    keep = torch.full((2, stages, frames), -1, dtype=torch.int64)
    keep[:, :2] = 5
    for v in (K, -2, 3 * K):
        wrong = keep.clone()
        wrong[1, 0, 2] = v
        with pytest.raises(ValueError, match=r"keep_codes: .*code %d of clip 1 at frame 2, stage 0 lies outside \[0, 16\)" % v):
            ae_generate.sample_code_stream(prior, stages, K, frames, start, keep_codes=wrong)
    for bad in (keep[:, :2], keep[:1], keep.float(), keep[:, :, :2]):
        with pytest.raises(ValueError, match=r"keep_codes must be \(2, 4, 3\) integers"):
            ae_generate.sample_code_stream(prior, stages, K, frames, start, keep_codes=bad)


def test_region_masks():
    from music_amd.ae_generate import _region_mask
    assert _region_mask(None, 2, 10) is None
    m = _region_mask([(2, 5), (7, 7), (9, 10)], 2, 10)
    assert m.shape == (2, 10) and m.dtype == torch.bool and m[0].tolist() == [j in (2, 3, 4, 9) for j in range(10)] and torch.equal(m[0], m[1])
    assert not _region_mask([], 2, 10).any() and _region_mask([(0, 10)], 2, 10).all()
    m = _region_mask([[(0, 3)], []], 2, 10)
    assert m[0].tolist() == [j < 3 for j in range(10)] and not m[1].any()
    for bad in ([(3, 2)], [(-1, 2)], [(0, 11)], [[(0, 3)]], [(0, 3), 4], "ab", [(0.0, 3)]):
        with pytest.raises(ValueError, match="region"):
            _region_mask(bad, 2, 10)
    with pytest.raises(ValueError, match="teacher_forced"):
        _region_mask([(0, 3)], 2, 10, teacher_forced=True)


# ---------------------------------------------------------------------------------------------- keep=None is today's call
GOLDEN_DECODE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces_decode.json")
NONE_CASES = ["one", "one_sampled", "batch", "batch_tables", "batch_windows", "classes_batch", "guided_batch", "general_batch", "short_batch"]


@pytest.mark.parametrize("name", NONE_CASES)
def test_keep_none_is_the_recorded_call(name, monkeypatch):
    """keep=None through generate_codes / generate_codes_batch: the launches recorded in tests/golden/launch_traces_decode.json for
    the call without the argument - entry for entry, argument for argument"""
    from tests import launch_trace as lt
    from tests.test_launch_trace import _same as same_trace
    with open(GOLDEN_DECODE) as f:
        want = json.load(f)["cases"][name]
    build, run = lt.DECODE_CASES[name]

    def with_keep_none(fg, net):
        a, b = fg.generate_codes, fg.generate_codes_batch
        monkeypatch.setattr(fg, "generate_codes", lambda *x, **kw: a(*x, keep=None, **kw))
        monkeypatch.setattr(fg, "generate_codes_batch", lambda *x, **kw: b(*x, keep=None, **kw))
        run(fg, net)
    monkeypatch.setitem(lt.DECODE_CASES, name + "_keep_none", (build, with_keep_none))
    same_trace(want, *lt.record_decode(name + "_keep_none", monkeypatch))


def test_keep_reaches_the_launch_as_forced(monkeypatch):
    """keep= on the recorder: the same entries as the call without it, the launch's `forced` pointer no longer NULL and the rows of a
    guided pair doubled"""
    from tests import launch_trace as lt
    seen = {}

    def run(fg, net):
        real = fg._launch_decode

        def spy(*a, **kw):
            seen["forced"] = kw.get("forced")
            seen["U"] = a[6]
            return real(*a, **kw)
        monkeypatch.setattr(fg, "_launch_decode", spy)
        keep = torch.full((lt.DEC_U, lt.DEC_N), -1, dtype=torch.int64)
        keep[:, 0], keep[1, 5], keep[2, 6] = 200, 3, 130
        out = fg.generate_codes_batch(net, lt._prompt(net, lt.DEC_U), lt.DEC_N, keep=keep, guidance=2.0, classes=lt.DEC_CLASSES,
                                      correct_queue=True, windows=lt._halves(256), window_pos=5)
        assert out.shape == (lt.DEC_U, lt.DEC_N) and int(out[1, 5]) == 3 and int(out[2, 6]) == 130 and out[:, 0].tolist() == [200] * 3
        seen["keep"] = keep
    monkeypatch.setitem(lt.DECODE_CASES, "guided_keep", ("classes", run))
    trace, _, _ = lt.record_decode("guided_keep", monkeypatch)
    calls = [i for i in trace if i[0] == "call"]
    assert [c[1] for c in calls].count("wn_cfg_decode_batch") == 1
    f = seen["forced"]
    assert seen["U"] == 2 * lt.DEC_U and f.dtype == torch.int32 and tuple(f.shape) == (2 * lt.DEC_U, lt.DEC_N - 1)
    assert torch.equal(f[0::2], f[1::2]) and torch.equal(f[0::2].to(torch.int64), seen["keep"][:, 1:])
