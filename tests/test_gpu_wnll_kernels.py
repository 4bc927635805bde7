"""wn_wstep_nll (music_amd/csrc/wn_nll.hip: nll_den_k and the WT instantiations of step_nll_k) through ctypes against the float64
restatement of the rule in tests/wnll_ref.py, from the same float32 inputs.  As in tests/test_gpu_win_nll_kernels.py every output
buffer is pre-filled with NaN (the int32 one with a sentinel) and everything outside the declared ranges must still be that
afterwards, and every checked launch runs twice into fresh buffers and must return the same bits.

Bars: those of tests/test_gpu_win_nll_kernels.py for the same quantities - probabilities 1e-6 at q = 256 and 5e-7 for general q, dx 1e-5
of max|ref| at q = 256 and 1e-4 otherwise, loss 1e-5 max(1, |ref|), row_nll 2e-6 max(1, |ref|).  The extra arithmetic is one multiply by
the weight and, with smoothing, one more fp32 sum of n terms that enters the loss as (e / n) sum x: its error is at most
e n 2^-24 max|x| (here 0.1 * 256 * 6e-8 * 5 < 1e-5 in absolute terms, against losses near log n), so NO bar is widened for
smoothing.  den[0] is exact for 0/1 masks and within 2^-24 relative for float weights (a double sum rounded once); den[1] is the
float of the reciprocal of that double sum.  Skipped columns: the exact bits of +0.0 / 0.  Run with -s for the worst values."""
import math

import numpy as np
import pytest
import torch

from music_amd import _lib
from music_amd._lib import call, ptr
from tests import test_gpu_win_nll_kernels as wk
from tests import wnll_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PAD, SENTINEL, OUTPUTS = wk.PAD, wk.SENTINEL, wk.OUTPUTS
IGN = -1


def table(q):
    """three unequal, overlapping windows, one of width 1"""
    return [(0, q // 3), (q // 3, q // 3 + 1), (q // 5, q)]


def launch(x, target, windows=None, pos=None, pos0=0, weight=None, ignore=IGN, eps=0.0, x_pitch=None, dx_pitch=None, x_extra=0, dx_extra=0,
           want=OUTPUTS, slack=NAN):
    """One wn_wstep_nll launch on x (B, q, W) float32 / target (B W,) int64 / weight None or (B W,) float32 CPU tensors.  Returns a
    dict of CPU results; checks that nothing outside the declared ranges was written.  `slack`: what every float of x outside the
    declared columns holds."""
    B, q, W = x.shape
    n = B * W
    xp, dp = x_pitch or W, dx_pitch or W
    xbs, dbs = q * xp + x_extra, q * dp + dx_extra
    xh = wk._framed(B * xbs, slack)
    for b in range(B):
        xh[PAD + b * xbs:PAD + b * xbs + q * xp].view(q, xp)[:, :W] = x[b]
    xd, td = xh.to(DEV), target.reshape(-1).to(DEV)
    wd = None if weight is None else torch.as_tensor(weight, dtype=torch.float32).reshape(-1).to(DEV)
    bufs = dict(dx=wk._framed(B * dbs), probs=wk._framed(n * q), row_nll=wk._framed(n), row_hit=wk._framed(n, SENTINEL, torch.int32))
    dev = {k: (v.to(DEV) if k in want else None) for k, v in bufs.items()}
    part = torch.full((_lib.CE_NUM_PARTIALS + 2 * PAD,), NAN, dtype=torch.float32, device=DEV)
    den = torch.full((2 + 2 * PAD,), NAN, dtype=torch.float32, device=DEV)
    o = lambda k: ptr(dev[k], PAD) if dev[k] is not None else None
    keep, tail = wk._win_tail(windows, pos, pos0)
    call("wn_wstep_nll", ptr(xd, PAD), xbs, xp, ptr(td), o("dx"), dbs, dp, o("probs"), o("row_nll"), o("row_hit"), ptr(part, PAD), W, q, B,
         *tail, ptr(wd), ignore, eps, ptr(den, PAD), _lib.stream())
    torch.cuda.synchronize()
    out = {}
    assert torch.equal(xd.cpu().view(torch.int32), xh.view(torch.int32)), "x was written"
    ph, dh = part.cpu(), den.cpu()
    assert ph[:PAD].isnan().all() and ph[PAD + _lib.CE_NUM_PARTIALS:].isnan().all()
    assert dh[:PAD].isnan().all() and dh[PAD + 2:].isnan().all(), "den: written outside its two floats"
    out["part"], out["den"] = ph[PAD:PAD + _lib.CE_NUM_PARTIALS], dh[PAD:PAD + 2]
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


def launch_twice(*a, **k):
    """... and again into fresh buffers: the same bits (no float atomics, fixed summation orders in both kernels)"""
    r1, r2 = launch(*a, **k), launch(*a, **k)
    wk.same_bits(r1, r2, "a second launch")
    return r1


def check(x, target, label, windows=None, pos=None, pos0=0, weight=None, ignore=IGN, eps=0.0, hostile=None, **kw):
    """The full comparison with tests/wnll_ref.py.  hostile: a (B W,) mask of columns whose logits are not finite (they must be skipped
    ones): their probabilities are not compared."""
    B, q, W = x.shape
    r = launch_twice(x, target, windows, pos, pos0, weight, ignore, eps, **kw)
    f = ref.reference(x, target, windows, pos, pos0, weight, ignore, eps)
    skip, bad = f["skip"], f["bad"]
    good = ~skip & ~bad
    clean = torch.ones(B * W, dtype=torch.bool) if hostile is None else ~hostile
    assert hostile is None or bool(skip[hostile].all())
    p_bar, dx_bar = (1e-6, 1e-5) if q == 256 else (5e-7, 1e-4)
    col = lambda m: m.view(B, 1, W).expand(B, q, W)
    # the denominator
    if math.isnan(f["den"][0]):
        assert r["den"].isnan().all()
    else:
        unit = weight is None or bool(((torch.as_tensor(weight) == 0) | (torch.as_tensor(weight) == 1)).all())
        e_den = abs(float(r["den"][0]) - f["den"][0]) / max(f["den"][0], 1e-30) if f["den"][0] else abs(float(r["den"][0]))
        assert e_den <= (0.0 if unit else 2.0 ** -24), ("den[0]", float(r["den"][0]), f["den"][0])
        want1 = np.float32(1.0 / np.float64(np.float32(f["den"][0]))) if unit and f["den"][0] else np.float32(f["den"][1])
        assert abs(float(r["den"][1]) - float(want1)) <= (0.0 if unit else 2.0 ** -23 * float(want1)), ("den[1]", float(r["den"][1]), want1)
    # skipped columns: exact zeros, whatever they hold
    assert (r["dx"][col(skip)].view(torch.int32) == 0).all(), "dx of a skipped column is not +0.0"
    assert (r["row_nll"][skip].view(torch.int32) == 0).all() and (r["row_hit"][skip] == 0).all(), "row_nll / row_hit of a skipped column"
    # poisoned columns, and nothing else
    den_nan = math.isnan(f["den"][0])
    if bad.any() or den_nan:
        assert np.isnan(r["loss"]) and r["row_nll"][bad].isnan().all() and not r["row_hit"][bad].any()
        assert r["dx"][col(bad if not den_nan else ~skip)].isnan().all()
    assert not r["row_nll"][good].isnan().any() and not r["probs"][clean].isnan().any()
    assert torch.equal(r["row_hit"][good], f["row_hit"][good]), "row_hit"
    e_p = float((r["probs"].double() - f["probs"])[clean].abs().max())
    e_nll = float(((r["row_nll"].double() - f["row_nll"]).abs() / f["row_nll"].abs().clamp(min=1.0))[good].max()) if good.any() else 0.0
    a_dx = scale = e_loss = 0.0
    if not den_nan:
        assert not r["dx"][col(good)].isnan().any()
        if good.any():
            scale = float(f["dx"][col(good)].abs().max())
            a_dx = float((r["dx"].double() - f["dx"])[col(good)].abs().max())
        if not bad.any():
            assert not r["part"].isnan().any(), "a loss partial was not rewritten"
            e_loss = abs(r["loss"] - f["loss"]) / max(1.0, abs(f["loss"]))
    # outside the windows: the bits of +0.0, in probs on every clean column and in dx on every column that is not poisoned
    k = torch.arange(q).view(1, q, 1)
    outside = ~((k >= f["lo"].view(B, 1, W)) & (k < f["hi"].view(B, 1, W)))
    if not den_nan:
        assert (r["dx"][outside & col(~bad)].view(torch.int32) == 0).all(), "dx outside a window is not +0.0"
    assert (r["probs"].view(B, W, q).permute(0, 2, 1)[outside & col(clean)].contiguous().view(torch.int32) == 0).all()
    e_dx = a_dx / scale if scale > 0 else a_dx
    print("  %s: probs %.2e (bar %.0e)  dx %.2e of max|ref| (bar %.0e)  loss %.2e (bar 1e-5)  row_nll %.2e (bar 2e-6)  loss %.4f  den %r"
          % (label, e_p, p_bar, e_dx, dx_bar, e_loss, e_nll, f["loss"], r["den"].tolist()))
    assert e_p <= p_bar and a_dx <= dx_bar * scale and e_loss <= 1e-5 and e_nll <= 2e-6, (label, e_p, e_dx, e_loss, e_nll)
    return r, f


def _inputs(B, q, W, windows, pos, seed, pos0=0, gain=1.0):
    return wk._inputs(B, q, W, windows, pos, seed, pos0, gain)


def _mask(n, seed, p=0.5):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < p).float()


SHAPES = [(q, W) for q in (256, 100, 600) for W in (1, 63, 64, 65, 130)]


@pytest.mark.parametrize("q,W", SHAPES, ids=["q%d_w%d" % s for s in SHAPES])
def test_random_masks_weights_and_smoothing(q, W):
    """q = 256 (its own kernel), 100 (masked rows of the <= 512 one), 600 (the 1024 one) at the tile edges, batch 1..3, with and
    without windows: a 0/1 mask through ignore_index, a 0/1 weight, float weights in [0, 2] with exact zeros, smoothing 0 and 0.1"""
    B = 1 + (W + q) % 3
    for j, (win, eps) in enumerate(((None, 0.0), (None, 0.1), (table(q), 0.0), (table(q), 0.1))):
        pos = None if win is None else [0, 1, 7][:B]
        x, t = _inputs(B, q, W, win, pos, 10 * W + q + j, gain=1.5)
        g = torch.Generator().manual_seed(77 * W + q + j)
        keep = _mask(B * W, 31 * W + q + j)
        wt = 2.0 * torch.rand(B * W, generator=g) * _mask(B * W, 5 * W + q + j, 0.7)
        # column 0 of clip 0 always counts: its window is the wide first pair, so max|ref dx| is never the rounding residue that a
        # width-1 window leaves under smoothing (p - (1 - e) - e: 0 in exact arithmetic), which no relative bar can be held to
        keep[0], wt[0] = 1.0, 1.5
        t_ign = torch.where(keep > 0, t, torch.full_like(t, IGN))
        label = "q=%d W=%d B=%d %s eps=%.1f " % (q, W, B, "period 3" if win else "no windows", eps)
        if j == 0:
            check(x, t_ign, label + "ignore_index", win, pos, eps=eps)
        elif j == 1:
            check(x, t, label + "float weights", win, pos, weight=wt, eps=eps)
        elif j == 2:
            check(x, t_ign, label + "float weights and ignore_index", win, pos, weight=wt, eps=eps)
        else:
            check(x, t, label + "0/1 weights", win, pos, weight=keep, eps=eps)


@pytest.mark.parametrize("q", [256, 100, 600])
def test_lonely_columns_whole_clips_and_everything_ignored(q):
    B, W, win, pos = 3, 130, table(q), [2, 2, 4]
    x, t = _inputs(B, q, W, win, pos, 2000 + q)
    only = torch.zeros(B * W)
    only[63] = only[W + 127] = 1.0                      # the last lane of clip 0's first tile, of clip 1's second: nothing else counts
    r, f = check(x, t, "lonely columns q=%d" % q, win, pos, weight=only, eps=0.1)
    assert r["den"].tolist() == [2.0, 0.5] and int((r["dx"] != 0).any(1).sum()) == 2
    t1 = t.clone()
    t1[W:2 * W] = IGN                                   # a whole clip ignored
    r, f = check(x, t1, "clip 1 ignored q=%d" % q, win, pos)
    assert r["den"][0] == 2 * W and (r["dx"][1].view(torch.int32) == 0).all()
    for eps in (0.0, 0.1):                              # everything ignored, by either means
        for kw in (dict(weight=torch.zeros(B * W)), dict()):
            tt = t if kw else torch.full_like(t, IGN)
            r, f = check(x, tt, "nothing counted q=%d" % q, win, pos, eps=eps, **kw)
            assert r["den"].tolist() == [0.0, 0.0] and (r["part"].view(torch.int32) == 0).all() and (r["dx"].view(torch.int32) == 0).all()


@pytest.mark.parametrize("q", [256, 100, 600])
def test_hostile_values_in_skipped_columns_and_in_every_slack_column_influence_nothing(q):
    """NaN, +inf and 1e30 in every logit of every skipped column and in every slack float of pitched rows, a garbage target under
    weight 0: every output outside those columns' own probabilities has the bits of the same call with zeros there"""
    B, W, win, pos = 2, 131, table(q), [1, 3]
    x, t = _inputs(B, q, W, win, pos, 3000 + q)
    wt = _mask(B * W, 3100 + q, 0.6)
    wt[5] = wt[W + 70] = 1.0
    t[5] = IGN                                          # skipped by its target under weight 1 ...
    skipped = (wt == 0) | (t == IGN)
    t[(wt == 0).nonzero().view(-1)[::2]] = 1 << 40      # ... and garbage targets under weight 0
    t[(wt == 0).nonzero().view(-1)[1::4]] = -12345
    pitched = dict(x_pitch=W + 37, dx_pitch=W + 5, x_extra=3, dx_extra=9)
    sk = skipped.view(B, 1, W).expand(B, q, W)
    for eps in (0.0, 0.1):
        base, f = check(torch.where(sk, torch.zeros(()), x), t, "zeros in skipped columns q=%d eps=%.1f" % (q, eps), win, pos, weight=wt,
                        eps=eps, slack=0.0, **pitched)
        assert torch.equal(f["skip"], skipped)
        for v in (NAN, float("inf"), 1e30):
            r, _ = check(torch.where(sk, torch.tensor(v), x), t, "%r in skipped columns q=%d" % (v, q), win, pos, weight=wt, eps=eps,
                         hostile=skipped, slack=v, **pitched)
            wk.same_bits(r, base, "skipped = %r" % v, ("dx", "row_nll", "row_hit", "part", "den"))
            assert torch.equal(r["probs"][~skipped].view(torch.int32), base["probs"][~skipped].view(torch.int32))


@pytest.mark.parametrize("q", [256, 100])
def test_a_bad_target_under_a_nonzero_weight_poisons_its_column_only(q):
    B, W, win, pos = 2, 67, table(q), [0, 6]
    x, t = _inputs(B, q, W, win, pos, 4000 + q)
    f0 = ref.reference(x, t, win, pos)
    wt = torch.ones(B * W)
    wt[3], wt[9] = 0.0, 0.25
    cols = (9, W + 66)
    t[9] = q                                            # outside [0, q), under weight 0.25
    c = W + 66                                          # inside [0, q), outside its window, under weight 1
    t[c] = int(f0["hi"][c]) % q if int(f0["hi"][c]) < q else int(f0["lo"][c]) - 1
    t[3] = q + 7                                        # outside [0, q) under weight 0: skipped, not poisoned
    r, f = check(x, t, "bad targets q=%d" % q, win, pos, weight=wt)
    assert sorted(int(i) for i in f["bad"].nonzero().view(-1)) == sorted(cols) and math.isnan(r["loss"])
    assert int(r["dx"].isnan().any(1).sum()) == 2 and r["den"][0] == B * W - 1 + 0.25 - 1
    pos = [0, -1]                                       # a negative position poisons its clip's counted columns
    wt[W + 4] = 0.0
    r, f = check(x, t, "negative position q=%d" % q, win, pos, weight=wt)
    assert bool(f["bad"][W:].sum() == W - 1) and (r["dx"][1, :, 4].view(torch.int32) == 0).all()


@pytest.mark.parametrize("q", [256, 100])
@pytest.mark.parametrize("v", [-1.0, float("inf"), NAN], ids=["negative", "inf", "nan"])
def test_a_negative_or_non_finite_weight_poisons_everything(q, v):
    """den, the loss and the dx of every counted column are NaN; a skipped column stays +0.0 (it is skipped by a predicate); under an
    ignored target the weight is not looked at"""
    B, W = 2, 70
    x, t = _inputs(B, q, W, None, None, 5000 + q)
    wt = torch.ones(B * W)
    wt[W + 69], wt[7] = v, 0.0
    r, f = check(x, t, "weight %r q=%d" % (v, q), weight=wt)
    assert r["den"].isnan().all() and math.isnan(r["loss"]) and int(r["dx"].isnan().all(1).sum()) == B * W - 1
    t[W + 69] = IGN
    r, f = check(x, t, "weight %r under an ignored target q=%d" % (v, q), weight=wt)
    assert r["den"][0] == B * W - 2 and math.isfinite(r["loss"])


def test_a_minus_inf_logit_without_smoothing_makes_no_nan():
    B, q, W, win = 1, 100, 65, table(100)
    x, t = _inputs(B, q, W, win, None, 6000)
    f0 = ref.reference(x, t, win)
    for c in range(W):                                  # one -inf inside every column's window, away from the target
        if int(f0["hi"][c] - f0["lo"][c]) > 1:
            k = int(f0["lo"][c]) + (int(t[c]) - int(f0["lo"][c]) + 1) % int(f0["hi"][c] - f0["lo"][c])
            x[0, k, c] = -float("inf")
    r, f = check(x, torch.where(_mask(W, 1) > 0, t, torch.full_like(t, IGN)), "-inf logits", win)
    assert math.isfinite(r["loss"]) and not r["dx"].isnan().any()


def test_more_tiles_than_loss_partials():
    """q = 64, B = 33, W = 1985: 1056 tiles of 64 columns, so the grid-stride loop runs twice in some blocks, and nll_den_k's threads
    take 64 columns each"""
    B, q, W, win = 33, 64, 1985, [(0, 32), (32, 64)]
    assert B * ((W + 63) // 64) == 1056 > _lib.CE_NUM_PARTIALS
    pos = list(range(B))
    x, t = _inputs(B, q, W, win, pos, 7000)
    g = torch.Generator().manual_seed(7001)
    wt = 2.0 * torch.rand(B * W, generator=g) * _mask(B * W, 7002, 0.5)
    r, _ = check(x, t, "tiles > partials", win, pos, weight=wt, eps=0.1)
    assert not r["part"].isnan().any() and (r["part"] == 0).any() and (r["part"] != 0).sum() == 528


@pytest.mark.parametrize("q", [256, 100])
@pytest.mark.parametrize("skip", OUTPUTS)
def test_each_output_may_be_null(q, skip):
    W, B, win, pos = 65, 2, table(q), [0, 3]
    x, t = _inputs(B, q, W, win, pos, 8000 + q)
    wt = 2.0 * _mask(B * W, 8001, 0.7)
    full = launch(x, t, win, pos, weight=wt, eps=0.1)
    want = tuple(k for k in OUTPUTS if k != skip)
    part = launch_twice(x, t, win, pos, weight=wt, eps=0.1, want=want)
    assert skip not in part
    wk.same_bits(part, full, "without " + skip, want + ("part", "den"))


@pytest.mark.parametrize("q", [256, 100, 600])
def test_the_degenerate_call_is_the_entry_from_before_bit_for_bit(q):
    """weight NULL, no target equal to ignore_index, smoothing 0: every output of wn_step_nll (no windows) / wn_win_step_nll with
    inv_n = (float)(1.0 / (batch * w)), a poisoned column included"""
    B, W = 3, 131
    inv_n = 1.0 / (B * W)
    outs = OUTPUTS + ("part",)
    g = torch.Generator().manual_seed(9000 + q)
    x, t = torch.randn(B, q, W, generator=g), torch.randint(0, q, (B * W,), generator=g)
    t[7] = q
    plain = wk.launch(x, t, inv_n, plain=True)
    r = launch(x, t)
    wk.same_bits(r, plain, "no windows", outs)
    assert r["den"].tolist() == [float(B * W), float(np.float32(inv_n))]
    wk.same_bits(launch(x, t, weight=torch.ones(B * W)), plain, "unit weights", outs)
    win, pos = table(q), [3, 0, (1 << 33) + 1]
    x, t = _inputs(B, q, W, win, pos, 9100 + q)
    t[11] = (int(t[11]) + q // 2) % q
    old = wk.launch(x, t, inv_n, win, pos, 2)
    wk.same_bits(launch(x, t, win, pos, 2), old, "windows", outs)
    wk.same_bits(launch(x, t, win, pos, 2, ignore=1 << 40, x_pitch=W + 3, dx_pitch=W + 1), old, "windows, pitched", outs)


def test_empty_calls_zero_the_partials_and_den_and_nothing_else():
    keep, tail = wk._win_tail(table(256), None, 0)
    part = torch.full((_lib.CE_NUM_PARTIALS + PAD,), NAN, dtype=torch.float32, device=DEV)
    den = torch.full((2 + PAD,), NAN, dtype=torch.float32, device=DEV)
    for shape in ((0, 0, 0, 256, 3), (256 * 9, 9, 9, 256, 0)):
        part.fill_(NAN)
        den.fill_(NAN)
        xbs, xp, w, q, b = shape
        call("wn_wstep_nll", None, xbs, xp, None, None, 0, 0, None, None, None, ptr(part), w, q, b, *tail, None, IGN, 0.1, ptr(den),
             _lib.stream())
        h, d = part.cpu(), den.cpu()
        assert (h[:_lib.CE_NUM_PARTIALS].view(torch.int32) == 0).all() and h[_lib.CE_NUM_PARTIALS:].isnan().all()
        assert (d[:2].view(torch.int32) == 0).all() and d[2:].isnan().all()
    call("wn_wstep_nll", None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 256, 3, None, 0, None, 0, None, IGN, 0.0, None, _lib.stream())
    torch.cuda.synchronize()
