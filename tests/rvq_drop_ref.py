"""Float64 restatement of quantiser dropout for the residual quantiser (include/wavenet_hip.h: wn_rvq_fwd_n, wn_rvq_bwd_n,
wn_rvq_bwd_stats_n, wn_rvq_lookup_n), shared by tests/test_rvq_drop_ref.py, tests/test_gpu_rvq_drop_kernels.py and
tests/test_gpu_rvq_drop_model.py.  One stage is tests/vq_ref.py, its statistics tests/vq_ema_ref.py, the chain without dropout
tests/rvq_ref.py: they are called per stage on the ACTIVE clips, not copied.

enc (B, Bw, Le); cb (S K, Bw); nstage (B,): clip b takes part in stage s iff s < n_b (a value outside [1, S] is clamped, as on the
device).  With r_0 = e, for an active frame:   idx_s, q_s, r_s+1 = r_s - q_s   as in rvq_ref;   for an inactive one idx_s = -1 and
r_s+1 = r_s.   q = q_0 + .. + q_n_b-1.   mse_s = sum over ACTIVE frames (r_s - q_s)^2 / (C Bw), the FIXED denominator.
  d_e = d_q + g beta s (r_1 + .. + r_n_b)       d_c_s[k] = g s sum_{active, idx_s = k} (c_s,k - r_s)       s = 2 / (C Bw)
"""
import numpy as np

from tests import rvq_ref, vq_ema_ref, vq_ref


def clamp(nstage, S, B=None):
    n = np.asarray(nstage, dtype=np.int64).reshape(-1)
    assert B is None or n.shape == (B,)
    return np.clip(n, 1, S)


def forward(enc, cb, S, nstage, beta=0.25, ema=False):
    """dict(idx (S, B, Le) int64 with -1 where inactive, q, res (S, ...) with res[s] = r_s+1 (carried where inactive), r (S, ...), mse (S,),
    vq_loss, counts (S, K), stage_frames (S,), dist (S, B, Le, K) with NaN where inactive, n (B,) the clamped counts)."""
    c = rvq_ref.stage_rows(cb, S)
    K = c.shape[1]
    r = np.array(enc, dtype=np.float64)
    B, Bw, Le = r.shape
    n = clamp(nstage, S, B)
    q = np.zeros_like(r)
    out = dict(idx=np.full((S, B, Le), -1, dtype=np.int64), res=np.empty((S,) + r.shape), r=np.empty((S,) + r.shape), mse=np.zeros(S),
               counts=np.zeros((S, K), dtype=np.int64), stage_frames=np.zeros(S, dtype=np.int64), dist=np.full((S, B, Le, K), np.nan))
    for s in range(S):
        act = n > s
        out["r"][s] = r
        if act.any():
            f = vq_ref.forward(r[act], c[s], beta)
            out["idx"][s][act] = f["idx"]
            out["dist"][s][act] = f["dist"]
            out["counts"][s] = f["counts"]
            out["stage_frames"][s] = int(act.sum()) * Le
            out["mse"][s] = f["mse"] * r[act].size / r.size             # vq_ref divides by its own frames: back to C Bw
            r = r.copy()
            r[act] = r[act] - f["q"]
            q[act] = q[act] + f["q"]
        out["res"][s] = r
    out["q"], out["n"] = q, n
    out["vq_loss"] = (float(beta) if ema else 1.0 + float(beta)) * float(out["mse"].sum())
    return out


def backward(enc, cb, S, nstage, idx, d_q, beta=0.25, g=1.0, residuals=None):
    """(d_enc (B, Bw, Le), d_cb (S K, Bw)) in float64 for the codes idx (S, B, Le); `residuals` as in rvq_ref.backward."""
    c = rvq_ref.stage_rows(cb, S)
    r = np.array(enc, dtype=np.float64)
    n = clamp(nstage, S, r.shape[0])
    idx = np.asarray(idx)
    tot = np.zeros_like(r)
    d_cb = []
    for s in range(S):
        act = n > s
        d_c = np.zeros_like(c[s])
        if act.any():
            _, d_c = vq_ref.backward(r[act], c[s], idx[s][act], None, beta, g)
            d_c = d_c * (r[act].size / r.size)                          # vq_ref's s = 2 / its own size: back to 2 / (C Bw)
            r = r.copy()
            r[act] = r[act] - c[s][idx[s][act]].transpose(0, 2, 1)
            if residuals is not None:
                r[act] = np.asarray(residuals[s], dtype=np.float64)[act]
            tot[act] = tot[act] + r[act]
        d_cb.append(d_c)
    d_enc = (0.0 if d_q is None else np.asarray(d_q, dtype=np.float64)) + float(g) * float(beta) * (2.0 / r.size) * tot
    return d_enc, np.concatenate(d_cb)


def lookup(cb, S, codes, nstage):
    """q (B, Bw, Le) from codes (S, B, Le): clip b's first n_b stages' rows, summed in stage order (rvq_ref.lookup per clip)."""
    codes = np.asarray(codes)
    n = clamp(nstage, S, codes.shape[1])
    return np.concatenate([rvq_ref.lookup(cb, S, codes[:n[b], b:b + 1]) for b in range(codes.shape[1])])


def stats(enc, cb, S, nstage, idx):
    """stat (S, K (Bw + 1)): every stage's [n | s] over the active frames' r_s; a stage nobody used: zeros."""
    c = rvq_ref.stage_rows(cb, S)
    r = np.array(enc, dtype=np.float64)
    n = clamp(nstage, S, r.shape[0])
    idx = np.asarray(idx)
    out = np.zeros((S, c.shape[1] * (c.shape[2] + 1)))
    for s in range(S):
        act = n > s
        if act.any():
            out[s] = vq_ema_ref.stats(r[act], idx[s][act], c.shape[1])
            r = r.copy()
            r[act] = r[act] - c[s][idx[s][act]].transpose(0, 2, 1)
    return out
