"""wn_step_nll / wn_step_softmax (music_amd/csrc/wn_nll.hip) against float64 on the CPU from the same float32 inputs:
F.cross_entropy over the channel axis, its autograd gradient and softmax(dim=1).  Every output buffer is pre-filled with NaN (the
int32 one with a sentinel) and everything outside the declared ranges must still be that afterwards; x carries NaN in every slack
column and around it; every launch runs twice into fresh buffers and must return the same bits.

Bars (those of the chunk-softmax tests in tests/test_gpu_kernels.py): probabilities 1e-6 (5e-7 for general q), dx 1e-5 of
max|ref| for Q = 256 and 1e-4 for general q, loss 1e-5 max(1, |ref|), row_nll 2e-6 max(1, |ref|).  Run with -s for the worst values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from music_amd import _lib
from music_amd._lib import call, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PAD = 67                 # NaN canaries in front of and behind every buffer (odd: bases are 4-byte aligned only)
SENTINEL = -7            # what row_hit holds where nothing was written


def reference(x, target, inv_n):
    """float64: (probs (B W, q), dx (B, q, W), row_nll (B W,), loss, first-index argmax (B W,)) - bad targets must be masked by the caller"""
    B, q, W = x.shape
    z = x.double().permute(0, 2, 1).reshape(-1, q).clone().requires_grad_(True)
    rows = F.cross_entropy(z, target.reshape(-1), reduction="none")
    loss = rows.sum() * inv_n
    g, = torch.autograd.grad(loss, z)
    zd = z.detach()
    arg = torch.where(zd == zd.max(1, keepdim=True)[0], torch.arange(q).expand_as(zd), q).min(1)[0]      # first index of the maximum
    return (F.softmax(z.detach(), dim=1), g.view(B, W, q).permute(0, 2, 1).contiguous(), rows.detach(), float(loss.detach()), arg)


def _framed(n, fill=NAN, dtype=torch.float32):
    return torch.full((PAD + n + PAD,), fill, dtype=dtype)


def launch(x, target, inv_n, x_pitch=None, dx_pitch=None, x_extra=0, dx_extra=0, want=("dx", "probs", "row_nll", "row_hit")):
    """One wn_step_nll launch on x (B, q, W) float32 / target (B W,) int64 CPU tensors.  Returns a dict of CPU results; checks that
    nothing outside the declared ranges was written."""
    B, q, W = x.shape
    n = B * W
    xp, dp = x_pitch or W, dx_pitch or W
    xbs, dbs = q * xp + x_extra, q * dp + dx_extra
    xh = _framed(B * xbs)
    for b in range(B):
        xh[PAD + b * xbs:PAD + b * xbs + q * xp].view(q, xp)[:, :W] = x[b]
    xd, td = xh.to(DEV), target.to(DEV)
    bufs = dict(dx=_framed(B * dbs), probs=_framed(n * q), row_nll=_framed(n), row_hit=_framed(n, SENTINEL, torch.int32))
    dev = {k: (v.to(DEV) if k in want else None) for k, v in bufs.items()}
    part = torch.full((_lib.CE_NUM_PARTIALS + 2 * PAD,), NAN, dtype=torch.float32, device=DEV)
    call("wn_step_nll", ptr(xd, PAD), xbs, xp, ptr(td), ptr(dev["dx"], PAD) if dev["dx"] is not None else None, dbs, dp,
         ptr(dev["probs"], PAD) if dev["probs"] is not None else None, ptr(dev["row_nll"], PAD) if dev["row_nll"] is not None else None,
         ptr(dev["row_hit"], PAD) if dev["row_hit"] is not None else None, ptr(part, PAD), W, q, B, inv_n, _lib.stream())
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


def launch_twice(*a, **k):
    """... and again into fresh buffers: the same bits"""
    r1, r2 = launch(*a, **k), launch(*a, **k)
    for key in r1:
        if key != "loss":
            assert torch.equal(r1[key].view(torch.int32), r2[key].view(torch.int32)), key + ": a second launch gave other bits"
    return r1


def check(x, target, label, bad_cols=(), **kw):
    """The full comparison; bad_cols: flat column indices whose target is out of range (NaN expected there, and in the loss)."""
    B, q, W = x.shape
    n = B * W
    inv_n = 1.0 / n
    r = launch_twice(x, target, inv_n, **kw)
    good = torch.ones(n, dtype=torch.bool)
    good[list(bad_cols)] = False
    t_ref = target.clone()
    t_ref[~good] = 0
    p_ref, dx_ref, nll_ref, loss_ref, arg = reference(x, t_ref, inv_n)
    p_bar, dx_bar = (1e-6, 1e-5) if q == 256 else (5e-7, 1e-4)
    e_p = float((r["probs"].double() - p_ref).abs().max())
    gmask = good.view(B, 1, W).expand(B, q, W)
    scale = float(dx_ref[gmask].abs().max())
    a_dx = float((r["dx"].double() - dx_ref)[gmask].abs().max())
    e_dx = a_dx / scale if scale > 0 else a_dx                           # (q = 1: the gradient is exactly zero, and must be)
    e_nll = float(((r["row_nll"].double() - nll_ref).abs() / nll_ref.abs().clamp(min=1.0))[good].max())
    assert r["part"].shape[0] == _lib.CE_NUM_PARTIALS
    if len(bad_cols):
        assert np.isnan(r["loss"]) and r["row_nll"][~good].isnan().all() and r["dx"][~gmask].isnan().all()
        assert not r["row_hit"][~good].any()
        e_loss = 0.0
    else:
        assert not r["part"].isnan().any(), "a loss partial was not rewritten"
        e_loss = abs(r["loss"] - loss_ref) / max(1.0, abs(loss_ref))
    assert not r["dx"][gmask].isnan().any() and not r["row_nll"][good].isnan().any()
    hit_ref = (arg == t_ref).to(torch.int32)
    assert torch.equal(r["row_hit"][good], hit_ref[good]), "row_hit"
    print("  %s: probs %.2e (bar %.0e)  dx %.2e of max|ref| (bar %.0e)  loss %.2e (bar 1e-5)  row_nll %.2e (bar 2e-6)  loss %.4f"
          % (label, e_p, p_bar, e_dx, dx_bar, e_loss, e_nll, loss_ref))
    assert e_p <= p_bar and a_dx <= dx_bar * scale and e_loss <= 1e-5 and e_nll <= 2e-6, (label, e_p, e_dx, e_loss, e_nll)
    # the softmax alone: the same probabilities, bit for bit
    xd = x.to(DEV).contiguous()
    probs = torch.full((n * q + PAD,), NAN, dtype=torch.float32, device=DEV)
    call("wn_step_softmax", ptr(xd), q * W, W, ptr(probs), W, q, B, _lib.stream())
    ph = probs.cpu()
    assert ph[n * q:].isnan().all() and torch.equal(ph[:n * q].view(n, q).view(torch.int32), r["probs"].view(torch.int32))
    return r


def _inputs(B, q, W, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    return gain * torch.randn(B, q, W, generator=g), torch.randint(0, q, (B * W,), generator=g)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 255, 257, 1000])
def test_q256_against_float64(W, B):
    x, t = _inputs(B, 256, W, 1000 * B + W)
    check(x, t, "Q=256 W=%d B=%d" % (W, B))


@pytest.mark.parametrize("W", [1, 65, 257])
@pytest.mark.parametrize("q", [1, 64, 100, 512, 1024])
def test_general_q_against_float64(q, W):
    x, t = _inputs(2, q, W, 7 * q + W)
    check(x, t, "q=%d W=%d" % (q, W))


@pytest.mark.parametrize("q", [256, 100, 600])
def test_pitched_rows_with_nan_in_every_slack_column(q):
    """x_pitch = W + 37, dx_pitch = W + 5, a gap between the clips too: NaN in every slack float of x must not reach a result, no
    slack float of dx may be written."""
    W = 131
    x, t = _inputs(3, q, W, 50 + q)
    check(x, t, "pitched q=%d" % q, x_pitch=W + 37, dx_pitch=W + 5, x_extra=3, dx_extra=9)


@pytest.mark.parametrize("q,B,W", [(256, 1030, 1), (2, 1, 64 * 1030 + 5)], ids=["q256", "q2"])
def test_more_tiles_than_loss_partials(q, B, W):
    """more than WN_CE_NUM_PARTIALS tiles of 64 columns: the grid-stride loop runs more than once per block and the grid is smaller
    than the partial count (the slots behind it are zeroed)"""
    assert B * ((W + 63) // 64) > _lib.CE_NUM_PARTIALS
    x, t = _inputs(B, q, W, 99 + q)
    r = check(x, t, "tiles > partials q=%d" % q)
    assert (r["part"] == 0).any()


@pytest.mark.parametrize("q", [256, 100])
def test_peaked_and_extreme_logits(q):
    x, t = _inputs(2, q, 70, 11 + q, gain=3.0)
    check(x, t, "gain 3 q=%d" % q)
    x, t = _inputs(2, q, 70, 12 + q)
    x = x * (80.0 / x.abs().max())                                        # logits in [-80, 80]
    assert 79.99 < float(x.abs().max()) < 80.01
    check(x, t, "+-80 q=%d" % q)


@pytest.mark.parametrize("q", [256, 100])
def test_target_far_below_the_maximum(q):
    """a column whose target logit lies 120 below the maximum: exp(-120) is a float32 denormal's neighbourhood, the nll stays finite
    (120 + log S) and dx at the target is -inv_n"""
    W = 66
    x, t = _inputs(1, q, W, 21 + q)
    c, y, top = 40, 5, q - 3
    t[c] = y
    x[0, top, c] = 60.0
    x[0, y, c] = -60.0
    r = check(x, t, "target 120 below q=%d" % q)
    inv_n = 1.0 / W
    assert np.isfinite(float(r["row_nll"][c])) and abs(float(r["row_nll"][c]) - 120.0) < 1e-3
    assert abs(float(r["dx"][0, y, c]) + inv_n) <= 1e-6 * inv_n


@pytest.mark.parametrize("q", [256, 600])
def test_hits_and_ties_take_the_first_index(q):
    """row_hit is exact; two equal maxima resolve to the first index, in one wave's rows and across two waves'"""
    W = 70
    x, t = _inputs(1, q, W, 31 + q)
    top = float(x.abs().max()) + 1.0
    t[:] = x[0].argmax(0)                                                 # every column a hit ...
    t[1::2] = (t[1::2] + 1) % q                                           # ... every second one a miss
    for c, (k1, k2), y in ((3, (3, 5), 3), (4, (3, 5), 5), (10, (10, q - 56), 10), (11, (10, q - 56), q - 56), (64, (0, q - 1), 0),
                           (69, (0, q - 1), q - 1)):
        x[0, k1, c] = x[0, k2, c] = top
        t[c] = y
    r = check(x, t, "ties q=%d" % q)
    assert [int(r["row_hit"][c]) for c in (3, 4, 10, 11, 64, 69)] == [1, 0, 1, 0, 1, 0]
    assert int(r["row_hit"].sum()) == W // 2               # even columns hit, odd ones miss; the six edited ones change no count


@pytest.mark.parametrize("q", [256, 100])
@pytest.mark.parametrize("bad", [None, -1, 1 << 40], ids=["q", "minus1", "2pow40"])
def test_bad_target_poisons_its_column_only(q, bad):
    W, B = 67, 2
    x, t = _inputs(B, q, W, 41 + q)
    cols = (5, W + 66)
    t[list(cols)] = q if bad is None else bad
    check(x, t, "bad target %s q=%d" % (bad, q), bad_cols=cols)


@pytest.mark.parametrize("q", [256, 100])
@pytest.mark.parametrize("skip", ["dx", "probs", "row_nll", "row_hit"])
def test_each_output_may_be_null(q, skip):
    W, B = 65, 2
    x, t = _inputs(B, q, W, 61 + q)
    full = launch(x, t, 1.0 / (B * W))
    want = tuple(k for k in ("dx", "probs", "row_nll", "row_hit") if k != skip)
    part = launch_twice(x, t, 1.0 / (B * W), want=want)
    assert skip not in part
    for k in want + ("part",):
        assert torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), k


def test_empty_calls_zero_the_partials_and_nothing_else():
    part = torch.full((_lib.CE_NUM_PARTIALS + PAD,), NAN, dtype=torch.float32, device=DEV)
    call("wn_step_nll", None, 0, 0, None, None, 0, 0, None, None, None, ptr(part), 0, 256, 3, 1.0, _lib.stream())
    h = part.cpu()
    assert (h[:_lib.CE_NUM_PARTIALS] == 0).all() and h[_lib.CE_NUM_PARTIALS:].isnan().all()
    part.fill_(NAN)
    call("wn_step_nll", None, 256 * 9, 9, None, None, 0, 0, None, None, None, ptr(part), 9, 256, 0, 1.0, _lib.stream())
    h = part.cpu()
    assert (h[:_lib.CE_NUM_PARTIALS] == 0).all() and h[_lib.CE_NUM_PARTIALS:].isnan().all()
