"""Float64 restatement of the EMA codebook update and the restart of dead codes (include/wavenet_hip.h: wn_vq_bwd_stats,
wn_vq_ema_update), shared by tests/test_vq_ema_ref.py, tests/test_gpu_vq_ema_kernels.py, tests/test_gpu_vq_ema_model.py and
tests/test_gpu_vq_ema_dist.py.  The quantiser itself is tests/vq_ref.py.

enc (B, Bw, Le): the pooled encoding; idx (B, Le): the chosen codes; K codes, C = B Le frames.  Stats and state share one layout,
a vector of K (Bw + 1): the K counts, then K rows of Bw.
  stat  = [n | s]    n_k = frames with idx = k,  s_k = their sum (ascending frame order)
  state = [N | m]    running usage and running sums; m / N is the codebook, [1 | c] the initial state
  update(g, eps, r):   N' = g N + (1 - g) n     m' = g m + (1 - g) s     tot = sum_k N'_k     Nhat = (N' + eps) / (tot + K eps) tot
                       c' = m' / Nhat
  restart (r > 0):     dead = {k: N'_k < r} ascending; donors = {k not dead, n_k >= 2} by n descending, ties to the smaller index;
                       the d-th dead code j takes the d-th donor k: c'_j = m'_j = s_k / n_k, N'_j = 1 (the donor is unchanged);
                       a dead code without a donor stays as the plain update left it
  loss:                vq_loss = beta mse,  d_e = d_q + g beta s (e - q) as in gradient mode,  d_c = 0
"""
import numpy as np


def split(vec, K):
    """[counts | rows] -> (counts (K,), rows (K, Bw)) as float64 copies."""
    vec = np.asarray(vec, dtype=np.float64).reshape(-1)
    assert vec.size % K == 0 and vec.size > K
    return vec[:K].copy(), vec[K:].reshape(K, vec.size // K - 1).copy()


def join(counts, rows):
    return np.concatenate([np.asarray(counts, dtype=np.float64).reshape(-1), np.asarray(rows, dtype=np.float64).reshape(-1)])


def stats(enc, idx, K):
    """stat = [n | s] of one batch in float64; an idx outside [0, K) belongs to no code."""
    enc = np.asarray(enc, dtype=np.float64)
    idx = np.asarray(idx).reshape(-1)
    frames = enc.transpose(0, 2, 1).reshape(-1, enc.shape[1])
    n, s = np.zeros(K), np.zeros((K, enc.shape[1]))
    ok = (idx >= 0) & (idx < K)
    np.add.at(n, idx[ok], 1.0)
    np.add.at(s, idx[ok], frames[ok])
    return join(n, s)


def initial_state(cb):
    cb = np.asarray(cb, dtype=np.float64)
    return join(np.ones(cb.shape[0]), cb)


def pairing(n, N1, restart):
    """donor[k] = the code whose batch mean dead code k takes, else -1; and the dead codes left without a donor."""
    K = len(n)
    donor = np.full(K, -1, dtype=np.int64)
    if not restart > 0:
        return donor, 0
    dead = [k for k in range(K) if N1[k] < restart]
    donors = sorted((k for k in range(K) if not N1[k] < restart and n[k] >= 2), key=lambda k: (-n[k], k))
    for j, k in zip(dead, donors):
        donor[j] = k
    return donor, max(0, len(dead) - len(donors))


def update(stat, state, K, decay, eps=1e-5, restart=0.0):
    """-> dict(state [N' | m'], cb (K, Bw), donor (K,), restarted, left, plus what the error bounds are made of: N1 = the plain
    N', tot, nhat, and scale = |g m| + |(1 - g) s| per element)."""
    g = float(decay)
    n, s = split(stat, K)
    N, m = split(state, K)
    N1 = g * N + (1.0 - g) * n
    m1 = g * m + (1.0 - g) * s
    tot = 0.0
    for k in range(K):                                                   # ascending k
        tot += N1[k]
    nhat = (N1 + eps) / (tot + K * eps) * tot
    with np.errstate(divide="ignore", invalid="ignore"):
        cb = m1 / nhat[:, None]
    donor, left = pairing(n, N1, restart)
    N2, m2 = N1.copy(), m1.copy()
    for j in np.nonzero(donor >= 0)[0]:
        cb[j] = s[donor[j]] / n[donor[j]]
        N2[j], m2[j] = 1.0, cb[j]
    return dict(state=join(N2, m2), cb=cb, donor=donor, restarted=int((donor >= 0).sum()), left=int(left), N1=N1, tot=tot, nhat=nhat,
                scale=np.abs(g * m) + np.abs((1.0 - g) * s))
