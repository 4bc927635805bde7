"""The windowed objective's rule (include/wavenet_hip.h, wn_win_step_nll / wn_win_step_softmax) restated in float64 on the CPU: the
per-timestep softmax, its negative log-likelihood, the gradient, the hit flag and the probabilities, each taken inside the window
of the column's stream position.  tests/test_win_nll_ref.py checks this file against torch's cross_entropy / softmax on the sliced
window; the GPU tests check the kernels and the models against this file."""
import torch


def column_windows(windows, B, W, q, pos=None, pos0=0):
    """(lo (B, W), hi (B, W), negative (B,)) int64 / bool: the pair of every column - column c of clip b sits at stream position
    pos0 + pos[b] + c and uses pair p mod len(windows).  No windows (None or empty: period 0): (0, q) everywhere.  A clip with a
    negative position is flagged, and never looked up: its columns report (0, q)."""
    pos = torch.zeros(B, dtype=torch.int64) if pos is None else torch.as_tensor(pos, dtype=torch.int64).reshape(B)
    negative = pos < 0
    lo, hi = torch.zeros(B, W, dtype=torch.int64), torch.full((B, W), q, dtype=torch.int64)
    if not windows:
        return lo, hi, torch.zeros(B, dtype=torch.bool)
    tab = torch.tensor([[int(a), int(b)] for a, b in windows], dtype=torch.int64)
    for b in range(B):
        if not negative[b]:
            j = [(int(pos0) + int(pos[b]) + c) % len(windows) for c in range(W)]          # (Python integers: positions beyond 2^63 never arise)
            lo[b], hi[b] = tab[j, 0], tab[j, 1]
    return lo, hi, negative


def reference(x, target, inv_n, windows, pos=None, pos0=0):
    """x (B, q, W) logits, target (B W,) or (B, W) int64.  Returns a dict of float64 / integer CPU tensors:
      probs (B W, q)   p_k = exp(x_k - m) / S over k in [lo, hi), an exact 0 outside
      dx (B, q, W)     (p_k - [k == y]) inv_n, an exact +0.0 outside the window; NaN in every row of a poisoned column
      row_nll (B W,)   log S + m - x_y; NaN where poisoned
      row_hit (B W,)   int32: the first index of the maximum INSIDE the window equals y; 0 where poisoned
      arg (B W,)       that first index
      bad (B W,)       poisoned: the target outside its column's window (or outside [0, q)), or a negative position of the clip
      lo, hi (B W,)    the column's window
      loss             float: inv_n times the sum of row_nll (NaN with any poisoned column)
    Values of x outside a column's window are never looked at (they may be NaN or inf)."""
    B, q, W = x.shape
    lo, hi, negative = column_windows(windows, B, W, q, pos, pos0)
    y = target.reshape(B, W).to(torch.int64)
    k = torch.arange(q).view(1, q, 1)
    inside = (k >= lo.view(B, 1, W)) & (k < hi.view(B, 1, W))
    xm = torch.where(inside, x.double(), torch.tensor(float("-inf"), dtype=torch.float64))
    m = xm.max(1)[0]                                                     # (B, W)
    e = torch.where(inside, (xm - m.view(B, 1, W)).exp(), torch.zeros((), dtype=torch.float64))
    S = e.sum(1)
    p = e / S.view(B, 1, W)
    arg = torch.where(xm == m.view(B, 1, W), k.expand(B, q, W), q).min(1)[0]
    bad = (y < lo) | (y >= hi) | negative.view(B, 1)
    ys = torch.where(bad, lo, y)                                         # a valid row to gather from; masked below
    xy = xm.gather(1, ys.view(B, 1, W)).view(B, W)
    nll = S.log() + m - xy
    onehot = torch.zeros(B, q, W, dtype=torch.float64).scatter_(1, ys.view(B, 1, W), 1.0)
    dx = (p - onehot) * inv_n
    dx = torch.where(inside, dx, torch.zeros((), dtype=torch.float64))
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    dx = torch.where(bad.view(B, 1, W), nan, dx)
    nll = torch.where(bad, nan, nll)
    hit = ((arg == y) & ~bad).to(torch.int32)
    return dict(probs=p.permute(0, 2, 1).reshape(B * W, q).contiguous(), dx=dx, row_nll=nll.reshape(-1), row_hit=hit.reshape(-1),
                arg=arg.reshape(-1), bad=bad.reshape(-1), lo=lo.reshape(-1), hi=hi.reshape(-1), loss=float(nll.sum() * inv_n))


def windowed_nll(logits, target, windows, pos=None, pos0=0):
    """Differentiable float64 mean NLL of logits (B, q, W) under the windows (torch autograd runs through it): what a model's loss is
    compared with.  The targets must lie inside their windows."""
    B, q, W = logits.shape
    lo, hi, negative = column_windows(windows, B, W, q, pos, pos0)
    assert not negative.any()
    k = torch.arange(q).view(1, q, 1)
    inside = (k >= lo.view(B, 1, W)) & (k < hi.view(B, 1, W))
    z = logits.double().masked_fill(~inside, float("-inf"))
    lse = torch.logsumexp(z, dim=1)
    y = target.reshape(B, 1, W).to(torch.int64)
    assert bool(inside.gather(1, y).all()), "a target outside its window"
    return (lse - z.gather(1, y).view(B, W)).mean()
