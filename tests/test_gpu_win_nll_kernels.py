"""wn_win_step_nll / wn_win_step_softmax (music_amd/csrc/wn_nll.hip, the WIN instantiations) one entry at a time against the float64
restatement of the rule in tests/win_nll_ref.py, from the same float32 inputs.  As in tests/test_gpu_nll_kernels.py every output buffer
is pre-filled with NaN (the int32 one with a sentinel) and everything outside the declared ranges must still be that afterwards, and
every launch runs twice into fresh buffers and must return the same bits.

Bars: those of tests/test_gpu_nll_kernels.py unchanged (the arithmetic is the same kernel's on fewer rows) - probabilities 1e-6 (5e-7
for general q), dx 1e-5 of max|ref| for q = 256 and 1e-4 otherwise, loss 1e-5 max(1, |ref|), row_nll 2e-6 max(1, |ref|).
Run with -s for the worst values."""
import ctypes
import math

import numpy as np
import pytest
import torch

from music_amd import _lib
from music_amd._lib import call, ptr
from music_amd.fast_generate import stage_windows
from tests import win_nll_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PAD = 67                 # NaN canaries in front of and behind every buffer (odd: bases are 4-byte aligned only)
SENTINEL = -7            # what row_hit holds where nothing was written
OUTPUTS = ("dx", "probs", "row_nll", "row_hit")
TABLE100 = [(0, 10), (10, 11), (5, 100)]          # unequal, overlapping, one of width 1


def _framed(n, fill=NAN, dtype=torch.float32):
    return torch.full((PAD + n + PAD,), fill, dtype=dtype)


def _win_tail(windows, pos, pos0):
    """(keep-alive objects, [win_host, win_period, win_pos, win_pos0]); windows None: period 0 with NULL table"""
    host = (ctypes.c_int32 * (2 * len(windows)))(*[v for pr in windows for v in pr]) if windows else None
    pd = torch.tensor(list(pos), dtype=torch.int64).to(DEV) if pos is not None else None
    return (host, pd), [ctypes.cast(host, ctypes.c_void_p) if host is not None else None, len(windows) if windows else 0, ptr(pd), pos0]


def launch(x, target, inv_n, windows=None, pos=None, pos0=0, plain=False, x_pitch=None, dx_pitch=None, x_extra=0, dx_extra=0, want=OUTPUTS):
    """One wn_win_step_nll launch (plain: wn_step_nll, the yardstick of the equivalence tests) on x (B, q, W) float32 / target (B W,)
    int64 CPU tensors.  Returns a dict of CPU results; checks that nothing outside the declared ranges was written."""
    B, q, W = x.shape
    n = B * W
    xp, dp = x_pitch or W, dx_pitch or W
    xbs, dbs = q * xp + x_extra, q * dp + dx_extra
    xh = _framed(B * xbs)
    for b in range(B):
        xh[PAD + b * xbs:PAD + b * xbs + q * xp].view(q, xp)[:, :W] = x[b]
    xd, td = xh.to(DEV), target.reshape(-1).to(DEV)
    bufs = dict(dx=_framed(B * dbs), probs=_framed(n * q), row_nll=_framed(n), row_hit=_framed(n, SENTINEL, torch.int32))
    dev = {k: (v.to(DEV) if k in want else None) for k, v in bufs.items()}
    part = torch.full((_lib.CE_NUM_PARTIALS + 2 * PAD,), NAN, dtype=torch.float32, device=DEV)
    o = lambda k: ptr(dev[k], PAD) if dev[k] is not None else None
    head = [ptr(xd, PAD), xbs, xp, ptr(td), o("dx"), dbs, dp, o("probs"), o("row_nll"), o("row_hit"), ptr(part, PAD), W, q, B, inv_n]
    if plain:
        call("wn_step_nll", *head, _lib.stream())
    else:
        keep, tail = _win_tail(windows, pos, pos0)
        call("wn_win_step_nll", *head, *tail, _lib.stream())
    torch.cuda.synchronize()
    out = {}
    assert torch.equal(xd.cpu().view(torch.int32), xh.view(torch.int32)), "x was written"
    ph = part.cpu()
    assert ph[:PAD].isnan().all() and ph[PAD + _lib.CE_NUM_PARTIALS:].isnan().all()
    out["part"] = ph[PAD:PAD + _lib.CE_NUM_PARTIALS]
    out["loss"] = float(out["part"].double().sum())
    for k in want:
        h = dev[k].cpu()
        blank = (lambda t: t.isnan().all()) if k != "row_hit" else (lambda t: bool((t == SENTINEL).all()))
        assert blank(h[:PAD]) and blank(h[-PAD:]), k + ": written outside its buffer"
        body = h[PAD:-PAD]
        if k == "dx":
            got = torch.empty(B, q, W)
            for b in range(B):
                clip = body[b * dbs:(b + 1) * dbs]
                assert blank(clip[q * dp:]), "dx: written between two clips"
                rows = clip[:q * dp].view(q, dp)
                assert blank(rows[:, W:]), "dx: a column >= w was written"
                got[b] = rows[:, :W]
            body = got
        out[k] = body.view(n, q) if k == "probs" else body
    return out


def same_bits(r1, r2, what, keys=None):
    for key in (keys or [k for k in r1 if k != "loss"]):
        assert torch.equal(r1[key].view(torch.int32), r2[key].view(torch.int32)), "%s: %s differs in its bits" % (what, key)


def launch_twice(*a, **k):
    """... and again into fresh buffers: the same bits (no float atomics, a fixed summation order)"""
    r1, r2 = launch(*a, **k), launch(*a, **k)
    same_bits(r1, r2, "a second launch")
    return r1


def softmax_alone(x, windows=None, pos=None, pos0=0, plain=False):
    B, q, W = x.shape
    n = B * W
    xd = x.to(DEV).contiguous()
    probs = torch.full((n * q + PAD,), NAN, dtype=torch.float32, device=DEV)
    if plain:
        call("wn_step_softmax", ptr(xd), q * W, W, ptr(probs), W, q, B, _lib.stream())
    else:
        keep, tail = _win_tail(windows, pos, pos0)
        call("wn_win_step_softmax", ptr(xd), q * W, W, ptr(probs), W, q, B, *tail, _lib.stream())
    ph = probs.cpu()
    assert ph[n * q:].isnan().all()
    return ph[:n * q].view(n, q)


def check(x, target, windows, label, pos=None, pos0=0, **kw):
    """The full comparison with tests/win_nll_ref.py; the columns it calls poisoned must be NaN (and the loss), every other one within
    the bars.  Also: the softmax entry alone gives the same probabilities bit for bit."""
    B, q, W = x.shape
    n = B * W
    inv_n = 1.0 / n
    r = launch_twice(x, target, inv_n, windows, pos, pos0, **kw)
    t_ref = target.reshape(-1)
    f = ref.reference(x, t_ref, inv_n, windows, pos, pos0)
    good = ~f["bad"]
    p_bar, dx_bar = (1e-6, 1e-5) if q == 256 else (5e-7, 1e-4)
    e_p = float((r["probs"].double() - f["probs"]).abs().max())
    gmask = good.view(B, 1, W).expand(B, q, W)
    scale = float(f["dx"][gmask].abs().max()) if good.any() else 0.0
    a_dx = float((r["dx"].double() - f["dx"])[gmask].abs().max()) if good.any() else 0.0
    e_dx = a_dx / scale if scale > 0 else a_dx
    e_nll = float(((r["row_nll"].double() - f["row_nll"]).abs() / f["row_nll"].abs().clamp(min=1.0))[good].max()) if good.any() else 0.0
    if not good.all():
        assert np.isnan(r["loss"]) and r["row_nll"][~good].isnan().all() and r["dx"][~gmask].isnan().all()
        assert not r["row_hit"][~good].any()
        e_loss = 0.0
    else:
        assert not r["part"].isnan().any(), "a loss partial was not rewritten"
        e_loss = abs(r["loss"] - f["loss"]) / max(1.0, abs(f["loss"]))
    assert not r["dx"][gmask].isnan().any() and not r["row_nll"][good].isnan().any() and not r["probs"].isnan().any()
    assert torch.equal(r["row_hit"][good], f["row_hit"][good]), "row_hit"
    # outside the windows: the bits of +0.0, in probs everywhere and in dx on every column that is not poisoned
    k = torch.arange(q).view(1, q, 1)
    outside = ~((k >= f["lo"].view(B, 1, W)) & (k < f["hi"].view(B, 1, W)))
    assert (r["dx"][outside & gmask].view(torch.int32) == 0).all(), "dx outside a window is not +0.0"
    assert (r["probs"].view(B, W, q).permute(0, 2, 1)[outside].contiguous().view(torch.int32) == 0).all(), "probs outside a window is not 0"
    print("  %s: probs %.2e (bar %.0e)  dx %.2e of max|ref| (bar %.0e)  loss %.2e (bar 1e-5)  row_nll %.2e (bar 2e-6)  loss %.4f"
          % (label, e_p, p_bar, e_dx, dx_bar, e_loss, e_nll, f["loss"]))
    assert e_p <= p_bar and a_dx <= dx_bar * scale and e_loss <= 1e-5 and e_nll <= 2e-6, (label, e_p, e_dx, e_loss, e_nll)
    sm = softmax_alone(x, windows, pos, pos0)
    assert torch.equal(sm.view(torch.int32), r["probs"].view(torch.int32)), "wn_win_step_softmax gives other bits than wn_win_step_nll"
    return r, f


def _inputs(B, q, W, windows, pos, seed, pos0=0, gain=1.0):
    """float32 logits, and targets drawn inside each column's window"""
    g = torch.Generator().manual_seed(seed)
    x = gain * torch.randn(B, q, W, generator=g)
    lo, hi, _ = ref.column_windows(windows, B, W, q, None if pos is None else [max(0, p) for p in pos], pos0)
    t = lo + (torch.rand(B, W, generator=g, dtype=torch.float64) * (hi - lo)).long()
    return x, torch.minimum(t, hi - 1).reshape(-1)


def _outside(f, B, q, W):
    k = torch.arange(q).view(1, q, 1)
    return ~((k >= f["lo"].view(B, 1, W)) & (k < f["hi"].view(B, 1, W)))


@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_q256_stage_windows_with_per_clip_positions(W):
    """the q = 256 instantiation under stage_windows(4, 64); positions 0, 1, 7: the lanes of one tile differ in window"""
    win, pos = stage_windows(4, 64), [0, 1, 7]
    x, t = _inputs(3, 256, W, win, pos, 100 + W)
    check(x, t, win, "Q=256 4x64 W=%d" % W, pos=pos)


@pytest.mark.parametrize("q,win", [(96, stage_windows(3, 32)), (100, TABLE100), (640, stage_windows(5, 128)), (1024, stage_windows(16, 64))],
                         ids=["q96_3x32", "q100_unequal", "q640_5x128", "q1024_16x64"])
def test_general_q(q, win):
    pos = [0, 5]
    x, t = _inputs(2, q, 65, win, pos, 7 * q)
    check(x, t, win, "q=%d period %d" % (q, len(win)), pos=pos)


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100), (640, stage_windows(5, 128))], ids=["q256", "q100", "q640"])
def test_hostile_values_outside_the_windows_influence_nothing(q, win):
    """NaN, +inf and 1e30 in every entry outside the windows: every output has the bits of the same call with zeros there"""
    B, W, pos = 2, 70, [3, 0]
    x, t = _inputs(B, q, W, win, pos, 200 + q)
    f = ref.reference(x, t, 1.0, win, pos)
    out = _outside(f, B, q, W)
    x0 = torch.where(out, torch.zeros(()), x)
    base, _ = check(x0, t, win, "zeros outside q=%d" % q, pos=pos)
    for v in (NAN, float("inf"), 1e30):
        r = launch(torch.where(out, torch.tensor(v), x), t, 1.0 / (B * W), win, pos)
        same_bits(r, base, "outside = %r" % v)
        assert (r["dx"][out].view(torch.int32) == 0).all() and (r["probs"].view(B, W, q).permute(0, 2, 1)[out].contiguous().view(torch.int32) == 0).all()
        assert torch.equal(softmax_alone(torch.where(out, torch.tensor(v), x), win, pos).view(torch.int32), base["probs"].view(torch.int32))


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100)], ids=["q256", "q100"])
def test_zero_logits_cost_the_log_of_the_window_width(q, win):
    B, W, pos = 2, 66, [1, 2]
    _, t = _inputs(B, q, W, win, pos, 300 + q)
    r, f = check(torch.zeros(B, q, W), t, win, "zero logits q=%d" % q, pos=pos)
    want = (f["hi"] - f["lo"]).double().log()
    assert ((r["row_nll"].double() - want).abs() <= 2e-6).all()


def test_a_width_1_window_has_nll_0_and_gradient_0():
    B, q, W, pos = 2, 100, 67, [0, 2]
    x, t = _inputs(B, q, W, TABLE100, pos, 400)
    r, f = check(x, t, TABLE100, "width 1", pos=pos)
    one = (f["hi"] - f["lo"]) == 1
    assert int(one.sum()) >= W // 3 * B
    assert (r["row_nll"][one].view(torch.int32) == 0).all() and (r["row_hit"][one] == 1).all()
    assert (r["dx"].permute(0, 2, 1).reshape(B * W, q)[one] == 0).all()
    assert (r["probs"][one][:, 10] == 1.0).all()


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (640, stage_windows(5, 128))], ids=["q256", "q640"])
def test_row_hit_is_the_first_index_argmax_inside_the_window(q, win):
    """a larger logit outside the window does not count; ties inside take the first index, within one wave's rows and across two"""
    B, W = 1, 70
    x, t = _inputs(B, q, W, win, None, 500 + q)
    f = ref.reference(x, t, 1.0, win)
    lo, hi = f["lo"], f["hi"]
    top = float(x.abs().max()) + 1.0
    inside_arg = f["arg"].clone()
    t = inside_arg.clone()                                                # every column a hit ...
    t[1::2] = lo[1::2] + (t[1::2] - lo[1::2] + 1) % (hi[1::2] - lo[1::2])  # ... every second one a miss
    for c in range(W):                                                    # a far larger logit outside every column's window
        x[0, int(hi[c]) if int(hi[c]) < q else int(lo[c]) - 1, c] = top + 5.0
    f2 = ref.reference(x, t, 1.0, win)
    assert torch.equal(f2["arg"], inside_arg), "the edit above touched a window"
    # ties: two equal maxima inside the window, the target on the first (hit) or on the second (miss)
    span = int(hi[0] - lo[0])
    ties = ((4, 3, 5, True), (5, 3, 5, False), (12, 0, span - 1, True), (13, 0, span - 1, False))
    for c, k1, k2, first in ties:
        assert (int(hi[c]) - int(lo[c])) == span
        x[0, int(lo[c]) + k1, c] = x[0, int(lo[c]) + k2, c] = top
        t[c] = int(lo[c]) + (k1 if first else k2)
    r, f3 = check(x, t, win, "hits and ties q=%d" % q)
    assert [int(r["row_hit"][c]) for c, _, _, _ in ties] == [1, 0, 1, 0]
    assert int(r["row_hit"].sum()) == W // 2                              # even columns hit, odd ones miss; the edits change no count
    assert torch.equal(f3["arg"] >= lo, torch.ones(W, dtype=torch.bool)) and torch.equal(f3["arg"] < hi, torch.ones(W, dtype=torch.bool))


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100)], ids=["q256", "q100"])
def test_a_target_outside_its_window_poisons_its_column_only(q, win):
    B, W, pos = 2, 67, [0, 6]
    x, t = _inputs(B, q, W, win, pos, 600 + q)
    f = ref.reference(x, t, 1.0, win, pos)
    cols = (5, W + 66)
    for c in cols:                                                        # inside [0, q), outside [lo, hi)
        t[c] = int(f["hi"][c]) % q if int(f["hi"][c]) < q else int(f["lo"][c]) - 1
        assert 0 <= int(t[c]) < q and not int(f["lo"][c]) <= int(t[c]) < int(f["hi"][c])
    r, f2 = check(x, t, win, "target outside its window q=%d" % q, pos=pos)
    assert sorted(int(i) for i in f2["bad"].nonzero().view(-1)) == sorted(cols) and math.isnan(r["loss"])


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100)], ids=["q256", "q100"])
@pytest.mark.parametrize("neg", [-1, -(1 << 40)], ids=["minus1", "minus2pow40"])
def test_a_negative_device_position_poisons_its_clip_only(q, win, neg):
    B, W = 3, 67
    pos = [2, neg, 5]
    x, t = _inputs(B, q, W, win, pos, 700 + q)
    r, f = check(x, t, win, "negative position q=%d" % q, pos=pos)
    assert torch.equal(f["bad"].view(B, W), torch.tensor([False, True, False]).view(B, 1).expand(B, W)) and math.isnan(r["loss"])


@pytest.mark.parametrize("q", [256, 100])
def test_period_0_and_whole_alphabet_tables_are_the_plain_entries_bit_for_bit(q):
    B, W = 2, 131
    g = torch.Generator().manual_seed(800 + q)
    x, t = torch.randn(B, q, W, generator=g), torch.randint(0, q, (B * W,), generator=g)
    t[7] = q                                                              # (a poisoned column too)
    plain = launch(x, t, 1.0 / (B * W), plain=True)
    sm = softmax_alone(x, plain=True)
    for label, win, pos in (("period 0", None, None), ("period 0 with positions", None, [3, 9]), ("(0, q) x 1", [(0, q)], None),
                            ("(0, q) x 16", [(0, q)] * 16, [5, 1 << 33])):
        same_bits(launch(x, t, 1.0 / (B * W), win, pos), plain, label)
        assert torch.equal(softmax_alone(x, win, pos).view(torch.int32), sm.view(torch.int32)), label


def test_positions_add_and_large_ones_wrap():
    """win_pos0 = 2^40 + 3 with NULL win_pos is the same shift given per clip; win_pos0 and win_pos add"""
    B, q, W, win = 2, 100, 65, TABLE100
    big = (1 << 40) + 3
    x, t = _inputs(B, q, W, win, None, 900, pos0=big)
    a, _ = check(x, t, win, "pos0 = 2^40 + 3", pos0=big)
    same_bits(launch(x, t, 1.0 / (B * W), win, [big, big]), a, "the shift per clip")
    same_bits(launch(x, t, 1.0 / (B * W), win, [big - 2, big - 2], 2), a, "pos0 + pos")
    same_bits(launch(x, t, 1.0 / (B * W), win, [1, 1], big - 1), a, "pos0 + pos")
    win, pos = stage_windows(4, 64), [(1 << 40) + 1, 6]
    x, t = _inputs(B, 256, W, win, pos, 901, pos0=(1 << 33) + 2)
    check(x, t, win, "Q=256 large positions", pos=pos, pos0=(1 << 33) + 2)


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100), (640, stage_windows(5, 128))], ids=["q256", "q100", "q640"])
def test_pitched_rows_with_nan_in_every_slack_column(q, win):
    """x_pitch = W + 37, dx_pitch = W + 5, a gap between the clips too: NaN in every slack float of x must not reach a result, no slack
    float of dx may be written"""
    W, pos = 131, [1, 0, 2]
    x, t = _inputs(3, q, W, win, pos, 1000 + q)
    check(x, t, win, "pitched q=%d" % q, pos=pos, x_pitch=W + 37, dx_pitch=W + 5, x_extra=3, dx_extra=9)


def test_more_tiles_than_loss_partials():
    """q = 64 as 2 x 32, B = 33, W = 1985: 1056 tiles of 64 columns, so the grid-stride loop runs twice in some blocks and the grid is
    smaller than the partial count; the loss against float64, every partial rewritten"""
    B, q, W, win = 33, 64, 1985, stage_windows(2, 32)
    assert B * ((W + 63) // 64) == 1056 > _lib.CE_NUM_PARTIALS
    pos = list(range(B))
    x, t = _inputs(B, q, W, win, pos, 1100)
    r, _ = check(x, t, win, "tiles > partials", pos=pos)
    assert not r["part"].isnan().any() and (r["part"] == 0).any() and (r["part"] != 0).sum() == 528


@pytest.mark.parametrize("q,win", [(256, stage_windows(4, 64)), (100, TABLE100)], ids=["q256", "q100"])
@pytest.mark.parametrize("skip", OUTPUTS)
def test_each_output_may_be_null(q, win, skip):
    W, B, pos = 65, 2, [0, 3]
    x, t = _inputs(B, q, W, win, pos, 1200 + q)
    full = launch(x, t, 1.0 / (B * W), win, pos)
    want = tuple(k for k in OUTPUTS if k != skip)
    part = launch_twice(x, t, 1.0 / (B * W), win, pos, want=want)
    assert skip not in part
    same_bits(part, full, "without " + skip, want + ("part",))


def test_the_softmax_entry_alone():
    B, q, W, win, pos = 2, 96, 65, stage_windows(3, 32), [2, 4]
    x, _ = _inputs(B, q, W, win, pos, 1300)
    f = ref.reference(x, torch.zeros(B * W, dtype=torch.int64), 1.0, win, pos)
    p1, p2 = softmax_alone(x, win, pos), softmax_alone(x, win, pos)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert float((p1.double() - f["probs"]).abs().max()) <= 5e-7
    assert (p1.view(B, W, q).permute(0, 2, 1)[_outside(f, B, q, W)] == 0).all()
    assert float((p1.double().sum(1) - 1).abs().max()) < 1e-6


def test_empty_calls_zero_the_partials_and_nothing_else():
    keep, tail = _win_tail(stage_windows(4, 64), None, 0)
    part = torch.full((_lib.CE_NUM_PARTIALS + PAD,), NAN, dtype=torch.float32, device=DEV)
    call("wn_win_step_nll", None, 0, 0, None, None, 0, 0, None, None, None, ptr(part), 0, 256, 3, 1.0, *tail, _lib.stream())
    h = part.cpu()
    assert (h[:_lib.CE_NUM_PARTIALS] == 0).all() and h[_lib.CE_NUM_PARTIALS:].isnan().all()
    part.fill_(NAN)
    call("wn_win_step_nll", None, 256 * 9, 9, None, None, 0, 0, None, None, None, ptr(part), 9, 256, 0, 1.0, *tail, _lib.stream())
    h = part.cpu()
    assert (h[:_lib.CE_NUM_PARTIALS] == 0).all() and h[_lib.CE_NUM_PARTIALS:].isnan().all()
    call("wn_win_step_softmax", None, 256 * 9, 9, None, 9, 256, 0, *tail, _lib.stream())
    call("wn_win_step_softmax", None, 0, 0, None, 0, 256, 3, *tail, _lib.stream())
    torch.cuda.synchronize()
