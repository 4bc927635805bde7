"""Float64 restatement of the residual vector quantiser (include/wavenet_hip.h: wn_rvq_fwd, wn_rvq_bwd, wn_rvq_bwd_stats,
wn_rvq_ema_update, wn_rvq_lookup), shared by tests/test_rvq_ref.py, tests/test_gpu_rvq_kernels.py, tests/test_gpu_rvq_model.py.
One stage is tests/vq_ref.py, one stage's EMA update tests/vq_ema_ref.py: both are called, not copied.

enc (B, Bw, Le): the pooled encoding; cb (S K, Bw): stage s owns rows [s K, (s + 1) K); C = B Le frames.  With r_0 = e:
  idx_s = argmin_k |r_s - c_s,k|^2 (ties to the smallest k)     q_s = c_s[idx_s]     r_s+1 = r_s - q_s
  q = ((q_0 + q_1) + ..) + q_S-1                                mse_s = sum (r_s - q_s)^2 / (C Bw)       vq_loss = coef sum_s mse_s
  the residual passes between the stages DETACHED:
  d_e = d_q + g beta s (r_1 + .. + r_S)      d_c_s[k] = g s sum_{idx_s = k} (c_s,k - r_s)      s = 2 / (C Bw)
  EMA mode: stat = S blocks of [n | sums of r_s]; every stage follows vq_ema_ref.update on its own block
"""
import numpy as np

from tests import vq_ema_ref, vq_ref


def stage_rows(cb, S):
    cb = np.asarray(cb, dtype=np.float64)
    assert cb.shape[0] % S == 0
    return cb.reshape(S, cb.shape[0] // S, cb.shape[1])


def forward(enc, cb, S, beta=0.25, ema=False):
    """dict(idx (S, B, Le) int64, q (B, Bw, Le), res (S, B, Bw, Le) with res[s] = r_s+1, r (S, ...) with r[s] = r_s, stage_q, mse (S,),
    vq_loss, counts (S, K), dist (S, B, Le, K))."""
    c = stage_rows(cb, S)
    r = np.asarray(enc, dtype=np.float64)
    out = dict(idx=[], res=[], r=[], stage_q=[], mse=[], counts=[], dist=[])
    q = None
    for s in range(S):
        f = vq_ref.forward(r, c[s], beta)
        out["r"].append(r)
        r = r - f["q"]
        q = f["q"] if q is None else q + f["q"]
        for k, v in (("idx", f["idx"]), ("res", r), ("stage_q", f["q"]), ("mse", f["mse"]), ("counts", f["counts"]), ("dist", f["dist"])):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out["q"] = q
    out["vq_loss"] = (float(beta) if ema else 1.0 + float(beta)) * float(out["mse"].sum())
    return out


def backward(enc, cb, S, idx, d_q, beta=0.25, g=1.0, residuals=None):
    """(d_enc (B, Bw, Le), d_cb (S K, Bw)) in float64 for the codes idx (S, B, Le).  `residuals` (S, ...): the r_s+1 to use in place
    of the float64 chain's (the device's own, where its rounding is not under test)."""
    c = stage_rows(cb, S)
    r = np.asarray(enc, dtype=np.float64)
    size = r.size
    tot = np.zeros_like(r)
    d_cb = []
    for s in range(S):
        _, d_c = vq_ref.backward(r, c[s], idx[s], None, beta, g)
        d_cb.append(d_c)
        r = r - c[s][idx[s]].transpose(0, 2, 1) if residuals is None else np.asarray(residuals[s], dtype=np.float64)
        tot = tot + r
    d_enc = (0.0 if d_q is None else np.asarray(d_q, dtype=np.float64)) + float(g) * float(beta) * (2.0 / size) * tot
    return d_enc, np.concatenate(d_cb)


def lookup(cb, S, codes, n=None):
    """q (B, Bw, Le) from codes (n, B, Le): the first n stages' rows, summed in stage order."""
    c = stage_rows(cb, S)
    codes = np.asarray(codes)
    n = codes.shape[0] if n is None else n
    q = None
    for s in range(n):
        row = c[s][codes[s]].transpose(0, 2, 1)
        q = row if q is None else q + row
    return q


def stats(enc, cb, S, idx):
    """stat (S, K (Bw + 1)): every stage's [n | s] over its own input r_s."""
    c = stage_rows(cb, S)
    r = np.asarray(enc, dtype=np.float64)
    out = []
    for s in range(S):
        out.append(vq_ema_ref.stats(r, idx[s], c.shape[1]))
        r = r - c[s][idx[s]].transpose(0, 2, 1)
    return np.stack(out)


def initial_state(cb, S):
    return np.stack([vq_ema_ref.initial_state(c) for c in stage_rows(cb, S)])


def update(stat, state, S, K, decay, eps=1e-5, restart=0.0):
    """Every stage on its own block: a list of S vq_ema_ref.update results."""
    stat, state = np.asarray(stat, dtype=np.float64).reshape(S, -1), np.asarray(state, dtype=np.float64).reshape(S, -1)
    return [vq_ema_ref.update(stat[s], state[s], K, decay, eps, restart) for s in range(S)]
