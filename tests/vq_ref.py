"""Float64 restatement of the vector-quantised bottleneck (include/wavenet_hip.h: wn_vq_fwd, wn_vq_bwd, wn_vq_lookup), shared by
tests/test_vq_ref.py, tests/test_gpu_vq_kernels.py, tests/test_gpu_vq_model.py.

enc (B, Bw, Le): the pooled encoding, frame (b, l) = enc[b, :, l]; cb (K, Bw): the codebook; C = B Le frames.
  dist[b, l, k] = sum_j (e_j - c_kj)^2                 idx = argmin_k, ties to the smallest k          q[b, :, l] = cb[idx[b, l]]
  mse = sum (q - e)^2 / (C Bw)                         vq_loss = (1 + beta) mse
  d_e = d_q + g beta s (e - q),  d_c[k] = g s sum_{idx = k} (c_k - e),  s = 2 / (C Bw)      (straight-through: e + sg(q - e))
  counts[k] = frames of code k,  perplexity = exp(-sum p ln p), p = counts / C
"""
import numpy as np


def distances(enc, cb):
    """(B, Le, K) float64 squared distances in the difference form."""
    e = np.asarray(enc, dtype=np.float64).transpose(0, 2, 1)            # (B, Le, Bw)
    c = np.asarray(cb, dtype=np.float64)
    out = np.empty(e.shape[:2] + (c.shape[0],))
    for k0 in range(0, c.shape[0], 64):                                  # (in slices: 210 x 1024 x 512 doubles at once is 880 MB)
        d = e[:, :, None, :] - c[None, None, k0:k0 + 64, :]
        out[:, :, k0:k0 + 64] = (d * d).sum(-1)
    return out


def forward(enc, cb, beta=0.25):
    """dict(idx (B, Le) int64, q (B, Bw, Le), mse, vq_loss, counts (K,) int64, perplexity, dist (B, Le, K))."""
    enc = np.asarray(enc, dtype=np.float64)
    cb = np.asarray(cb, dtype=np.float64)
    dist = distances(enc, cb)
    idx = dist.argmin(-1)                                                # numpy: the first of equal minima
    q = cb[idx].transpose(0, 2, 1)
    mse = float(((q - enc) ** 2).sum() / enc.size)
    counts = np.bincount(idx.reshape(-1), minlength=cb.shape[0]).astype(np.int64)
    return dict(idx=idx, q=q, mse=mse, vq_loss=(1.0 + float(beta)) * mse, counts=counts, perplexity=perplexity(counts), dist=dist)


def perplexity(counts):
    p = np.asarray(counts, dtype=np.float64)
    p = p[p > 0] / p.sum()
    return float(np.exp(-(p * np.log(p)).sum()))


def backward(enc, cb, idx, d_q, beta=0.25, g=1.0):
    """(d_enc (B, Bw, Le), d_cb (K, Bw)) in float64; d_q None = no gradient reaches q (the loss term alone)."""
    enc = np.asarray(enc, dtype=np.float64)
    cb = np.asarray(cb, dtype=np.float64)
    s = 2.0 / enc.size
    q = cb[idx].transpose(0, 2, 1)
    d_enc = (0.0 if d_q is None else np.asarray(d_q, dtype=np.float64)) + float(g) * float(beta) * s * (enc - q)
    d_cb = np.zeros_like(cb)
    np.add.at(d_cb, idx.reshape(-1), (q - enc).transpose(0, 2, 1).reshape(-1, cb.shape[1]))
    return d_enc, float(g) * s * d_cb


def margins(dist):
    """Relative margin of every frame: (second-best - best) / best over the codes (inf where the best distance is 0 and the second is not)."""
    part = np.partition(dist, 1, axis=-1)
    best, second = part[..., 0], part[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(best > 0, (second - best) / best, np.where(second > 0, np.inf, 0.0))
