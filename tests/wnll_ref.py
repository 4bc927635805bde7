"""The masked, weighted and smoothed objective's rule (include/wavenet_hip.h, wn_wstep_nll) restated in float64 on the CPU.
tests/test_wnll_ref.py holds this file to torch.nn.functional.cross_entropy(ignore_index=, label_smoothing=) and to a hand-written
weighted sum; the GPU tests hold the kernel and the models to this file."""
import math

import torch

from tests.win_nll_ref import column_windows

NO_IGNORE = -(1 << 63)          # what the host passes when no target value is ignored


def column_weights(target, weight, ignore_index, B, W):
    """(B, W) float64: 0 under an ignored target, else the column's weight (ones without weights).  Float32 weights enter exactly."""
    y = target.reshape(B, W).to(torch.int64)
    w = torch.ones(B, W, dtype=torch.float64) if weight is None else torch.as_tensor(weight).reshape(B, W).double()
    return torch.where(y == int(ignore_index), torch.zeros((), dtype=torch.float64), w)


def reference(x, target, windows=None, pos=None, pos0=0, weight=None, ignore_index=NO_IGNORE, smoothing=0.0):
    """x (B, q, W) logits, target (B W,) or (B, W) int64, weight None or (B W,) / (B, W) floats.  Float64 / integer CPU tensors:
      w (B W,)         the column's weight, 0 under an ignored target
      skip (B W,)      w == 0 exactly: the column adds nothing and reports zeros, whatever its target and its logits hold
      den              [sum of w, 1 / sum of w (0 for a sum of 0)]; NaN both when a counted weight is negative or not finite
      probs (B W, q)   the column's softmax inside its window, skipped columns included; an exact 0 outside
      dx (B, q, W)     (w den[1]) (p_k - (1 - e) [k == y] - e / n) inside the window, +0.0 outside and on skipped columns; NaN in every
                       row of a poisoned column (and of every counted one under a NaN den)
      row_nll (B W,)   the UNSMOOTHED log S + m - x_y; 0 where skipped, NaN where poisoned
      row_hit (B W,)   int32: the first index of the maximum inside the window equals y; 0 where skipped or poisoned
      bad (B W,)       poisoned: counted, and the target outside its window (or [0, q)), or the clip's position negative
      lo, hi (B W,)    the column's window
      loss             float: den[1] * sum of w l over the counted columns, l = log S + m - (1 - e) x_y - (e / n) sum of the window's x"""
    B, q, W = x.shape
    eps = float(smoothing)
    lo, hi, negative = column_windows(windows, B, W, q, pos, pos0)
    y = target.reshape(B, W).to(torch.int64)
    wv = column_weights(target, weight, ignore_index, B, W)
    skip = wv == 0
    counted = ~skip
    poisoned_den = bool((counted & ~((wv >= 0) & (wv < math.inf))).any())
    total = float(wv[counted].sum()) if counted.any() else 0.0
    den = [math.nan, math.nan] if poisoned_den else [total, 1.0 / total if total != 0 else 0.0]
    k = torch.arange(q).view(1, q, 1)
    inside = (k >= lo.view(B, 1, W)) & (k < hi.view(B, 1, W))
    neg_inf, zero, nan = (torch.tensor(v, dtype=torch.float64) for v in (-math.inf, 0.0, math.nan))
    # a skipped column's logits enter its own probabilities alone
    xm = torch.where(inside, x.double(), neg_inf)
    m = xm.max(1)[0]
    e = torch.where(inside, (xm - m.view(B, 1, W)).exp(), zero)
    S = e.sum(1)
    p = e / S.view(B, 1, W)
    arg = torch.where(xm == m.view(B, 1, W), k.expand(B, q, W), q).min(1)[0]
    bad = counted & ((y < lo) | (y >= hi) | negative.view(B, 1))
    ys = torch.where(bad | skip, lo, y)
    xy = xm.gather(1, ys.view(B, 1, W)).view(B, W)
    n = (hi - lo).double()
    nll = S.log() + m - xy
    ell = nll
    if eps != 0.0:                                   # (the bypass: without smoothing the window's sum is not formed)
        sx = torch.where(inside, x.double(), zero).sum(1)
        ell = S.log() + m - (1.0 - eps) * xy - (eps / n) * sx
    onehot = torch.zeros(B, q, W, dtype=torch.float64).scatter_(1, ys.view(B, 1, W), 1.0)
    g = p - (1.0 - eps) * onehot - (eps / n).view(B, 1, W)
    dx = torch.where(inside, g * (wv * den[1]).view(B, 1, W), zero)
    dx = torch.where(bad.view(B, 1, W), nan, dx)
    dx = torch.where(skip.view(B, 1, W), zero, dx)
    terms = torch.where(bad, nan, wv * ell)[counted]
    loss = float(terms.sum() * den[1]) if counted.any() else 0.0
    row_nll = torch.where(skip, zero, torch.where(bad, nan, nll))
    hit = ((arg == y) & counted & ~bad).to(torch.int32)
    return dict(w=wv.reshape(-1), skip=skip.reshape(-1), den=den, probs=p.permute(0, 2, 1).reshape(B * W, q).contiguous(), dx=dx,
                row_nll=row_nll.reshape(-1), row_hit=hit.reshape(-1), bad=bad.reshape(-1), lo=lo.reshape(-1), hi=hi.reshape(-1), loss=loss)


def weighted_nll(logits, target, windows=None, pos=None, pos0=0, weight=None, ignore_index=NO_IGNORE, smoothing=0.0):
    """Differentiable float64 loss of logits (B, q, W) under the same rule (torch autograd runs through it): what a model's loss and
    d loss / d logits are compared with.  Counted targets must lie inside their windows; skipped columns are cut out by index, so
    that whatever they hold reaches neither the value nor the gradient."""
    B, q, W = logits.shape
    eps = float(smoothing)
    lo, hi, negative = column_windows(windows, B, W, q, pos, pos0)
    assert not negative.any()
    wv = column_weights(target, weight, ignore_index, B, W)
    cols = (wv != 0).reshape(-1).nonzero().view(-1)
    if cols.numel() == 0:
        return logits.double().sum() * 0.0
    k = torch.arange(q).view(1, q, 1)
    inside = ((k >= lo.view(B, 1, W)) & (k < hi.view(B, 1, W))).permute(0, 2, 1).reshape(B * W, q)[cols]
    z = logits.double().permute(0, 2, 1).reshape(B * W, q)[cols]
    y = target.reshape(-1).to(torch.int64)[cols].view(-1, 1)
    assert bool(inside.gather(1, y).all()), "a counted target outside its window"
    zm = z.masked_fill(~inside, -math.inf)
    ell = torch.logsumexp(zm, dim=1) - (1.0 - eps) * z.gather(1, y).view(-1)
    if eps != 0.0:
        ell = ell - eps * z.masked_fill(~inside, 0.0).sum(1) / inside.sum(1).double()
    w = wv.reshape(-1)[cols]
    return (w * ell).sum() / w.sum()
