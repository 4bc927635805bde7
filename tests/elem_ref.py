"""Float64 restatements of the formulas include/wavenet_hip.h gives for the memory-bound helpers (wn_elem.hip, wn_generic.hip,
wn_optim.h): chunk softmax, its backward and the fused cross-entropy-on-probabilities step, the gate and its derivatives, the
two bucket rules with their sums and expansion, one step of Adam / SGD / RMSprop, the one-hot layouts, the gradient gather and
mu-law.  Plain numpy, no device; tests/test_elem_ref.py holds them to independent authorities (float64 autograd, torch.optim),
tests/test_gpu_elem_kernels.py holds the kernels to them."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- chunk softmax over rows of q consecutive floats
def softmax(x):
    x = _f64(x)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def softmax_bwd(y, dy):
    """dx = y (dy - <dy, y>)"""
    y, dy = _f64(y), _f64(dy)
    return y * (dy - (dy * y).sum(1, keepdims=True))


def softmax_ce(x, target, inv_n):
    """nn.CrossEntropyLoss applied to the PROBABILITIES p = softmax(x): loss_r = logsumexp(p_r) - p_r[y_r]; dp = (softmax(p) - e_y)
    inv_n; dx = p (dp - <dp, p>).  A target outside [0, q) gives a NaN loss for its row and a NaN row of dx.
    Returns (p, per-row loss, inv_n * sum of the per-row losses, dx)."""
    p = softmax(x)
    n, q = p.shape
    t = np.asarray(target, dtype=np.int64)
    bad = (t < 0) | (t >= q)
    tc = np.where(bad, 0, t)
    e2 = np.exp(p)
    s2 = e2.sum(1, keepdims=True)
    rows = np.arange(n)
    loss = np.log(s2[:, 0]) - p[rows, tc]
    dp = e2 / s2
    dp[rows, tc] -= 1.0
    dp *= float(inv_n)
    dx = p * (dp - (dp * p).sum(1, keepdims=True))
    loss[bad] = np.nan
    dx[bad] = np.nan
    return p, loss, float(inv_n) * loss.sum(), dx


# ---- gate
def sigmoid(g):
    g = _f64(g)
    return 1.0 / (1.0 + np.exp(-g))


def gate(f, g):
    return np.tanh(_f64(f)) * sigmoid(g)


def gate_d(f, g):
    """(dz/df, dz/dg) = (sigma(g) (1 - tanh^2 f), tanh f sigma(g) (1 - sigma(g)))"""
    th, s = np.tanh(_f64(f)), sigmoid(g)
    return s * (1.0 - th * th), th * s * (1.0 - s)


# ---- conditioning buckets: idx(t) of column t - t_lo
def bucket_index(length, mode, le, q):
    r = np.arange(max(length, 0))
    if mode == 1:
        return np.minimum(r // q, le - 1)                      # stretch: the last bucket absorbs the tail
    assert mode == 2
    return r % le                                              # tile


def bucket_sums(win, mode, le, q):
    """win [..., L] -> [..., le]: out[j] = sum of the columns with idx == j (an empty bucket is exactly 0)"""
    win = _f64(win)
    ix = bucket_index(win.shape[-1], mode, le, q)
    out = np.zeros(win.shape[:-1] + (le,))
    for j in range(le):
        out[..., j] = win[..., ix == j].sum(-1)
    return out


def bucket_abs_sums(win, mode, le, q):
    """(sum of |terms|, number of terms) per bucket: what the bound of a fixed-order fp32 sum is made of"""
    ix = bucket_index(np.shape(win)[-1], mode, le, q)
    return bucket_sums(np.abs(_f64(win)), mode, le, q), np.bincount(ix, minlength=le)[:le]


def bucket_expand(tab, length, mode, le, q):
    """tab [..., le] -> [..., length]: out[t] = tab[idx(t)]; the dtype is kept (a copy, nothing is computed)"""
    return np.asarray(tab)[..., bucket_index(length, mode, le, q)]


# ---- one optimizer step, as wn_optim.h and the header write it; every scalar is the float32 value the entry point receives
def _s(v):
    return float(np.float32(v))


def adam_step(p, g, m, v, lr, b1, b2, eps, bc1, bc2, gscale):
    """torch.optim.Adam: m' = b1 m + (1 - b1) g s, v' = b2 v + (1 - b2) (g s)^2, p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)"""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, bc1, bc2, gscale = map(_s, (lr, b1, b2, eps, bc1, bc2, gscale))
    gi = g * gscale
    m2 = b1 * m + (1.0 - b1) * gi
    v2 = b2 * v + (1.0 - b2) * gi * gi
    return adam_p(p, m2, v2, lr, eps, bc1, bc2), m2, v2


def adam_p(p, m2, v2, lr, eps, bc1, bc2):
    """the parameter step from given new moments"""
    lr, eps, bc1, bc2 = map(_s, (lr, eps, bc1, bc2))
    return _f64(p) - (lr / bc1) * _f64(m2) / (np.sqrt(_f64(v2)) / np.sqrt(bc2) + eps)


def sgd_step(p, g, buf, lr, momentum, gscale, first_step):
    """torch.optim.SGD(lr, momentum): buf' = first_step ? g s : momentum buf + g s; p' = p - lr buf'.  momentum == 0: p' = p - lr g s
    and there is no buffer (buf may be None, None is returned for it)."""
    p, gi = _f64(p), _f64(g) * _s(gscale)
    lr, momentum = _s(lr), _s(momentum)
    if momentum == 0.0:
        return p - lr * gi, None
    b2 = gi if first_step else momentum * _f64(buf) + gi
    return p - lr * b2, b2


def rmsprop_step(p, g, sq, buf, lr, alpha, eps, momentum, gscale):
    """torch.optim.RMSprop(lr, alpha, eps, momentum), not centered: sq' = alpha sq + (1 - alpha) (g s)^2; avg = sqrt(sq') + eps;
    momentum > 0: buf' = momentum buf + g s / avg, p' = p - lr buf'; else p' = p - lr g s / avg (buf may be None)."""
    p, gi, sq = _f64(p), _f64(g) * _s(gscale), _f64(sq)
    lr, alpha, eps, momentum = map(_s, (lr, alpha, eps, momentum))
    s2 = alpha * sq + (1.0 - alpha) * gi * gi
    avg = np.sqrt(s2) + eps
    if momentum > 0.0:
        b2 = momentum * _f64(buf) + gi / avg
        return p - lr * b2, s2, b2
    return p - lr * (gi / avg), s2, None


# ---- exact movers
def onehot(codes, q, scrambled):
    """int codes [B][T] -> float32 [B][q][T].  scrambled: the one of sample s sits at flat offset s * q + code of the clip's q * T
    floats; proper: out[b][code][s].  A code outside [0, q) sets no one."""
    codes = np.asarray(codes, dtype=np.int64)
    b, t = codes.shape
    out = np.zeros((b, q * t), np.float32)
    for i in range(b):
        s = np.arange(t)
        ok = (codes[i] >= 0) & (codes[i] < q)
        pos = s * q + codes[i] if scrambled else codes[i] * t + s
        out[i, pos[ok]] = 1.0
    return out.reshape(b, q, t)


def gather(packed, idx):
    """flat[i] = packed[idx[i]], a negative index gives 0"""
    packed, idx = np.asarray(packed), np.asarray(idx, dtype=np.int64)
    return np.where(idx >= 0, packed[np.maximum(idx, 0)], packed.dtype.type(0))


def mulaw_encode(audio, thresholds):
    """code = number of thresholds <= the sample (thresholds ascending, float32 compared as float32)"""
    return np.searchsorted(np.asarray(thresholds, np.float32), np.asarray(audio, np.float32), side="right")


def mulaw_decode(codes, table):
    """table[code clamped to [0, q)]"""
    table = np.asarray(table)
    return table[np.clip(np.asarray(codes, dtype=np.int64), 0, len(table) - 1)]
