"""Float64 reference of wn_resblock_bwd (the recompute half of the gated block's backward), include/wavenet_hip.h's formulas
written out in numpy - no autograd, so that it can be checked AGAINST autograd (tests/test_recompute_ref.py):

    f = bias_f + Wf[:, :, 0] x[t-d] + Wf[:, :, 1] x[t] + cond[b][row][idx(t)]        (g alike, rows ch.. of the table)
    idx(t) = min((t - t_lo) // cond_q, cond_le - 1)  (mode 1)   |   (t - t_lo) % cond_le  (mode 2)
    th = tanh f, sg = sigmoid g, z = th sg
    dzt = Wd^T dy[t] (0 if dy is None) + (dz[t] if t >= z_lo else 0)
    df = dzt sg (1 - th^2)      dg = dzt th sg (1 - sg)                               on [t_lo, t_hi)

All arrays are indexed by ABSOLUTE time on their last axis, as the kernel's buffers are; only the columns the formulas name
are read, so the rest may hold NaN."""
import numpy as np


def cond_index(t_lo, t_hi, mode, le, q):
    """table column of every t in [t_lo, t_hi)"""
    tr = np.arange(t_hi - t_lo)
    if mode == 1:
        return np.minimum(tr // q, le - 1)
    if mode == 2:
        return tr % le
    raise ValueError("cond_mode must be 1 or 2")


def recompute_bwd(x, wf, wg, wd, d, t_lo, t_hi, z_lo, dy=None, dz=None, bias_f=None, bias_g=None, tab=None, tab_g_row=None,
                  cond_mode=0, cond_le=0, cond_q=0):
    """x [B][>=R][>=t_hi], wf / wg [D][R][2], wd [R][D][1], dy [B][>=R][>=t_hi] or None, dz [B][>=D][>=t_hi] or None (no crop),
    bias_f / bias_g [>=D] or None, tab [B][rows][>=cond_le] with the g rows starting at row tab_g_row.
    Returns float64 (df, dg, z), each [B][D][t_hi - t_lo]."""
    wf, wg, wd = (np.asarray(a, np.float64) for a in (wf, wg, wd))
    D, R = wf.shape[0], wf.shape[1]
    x = np.asarray(x)
    xa = x[:, :R, t_lo - d:t_hi - d].astype(np.float64)
    xb = x[:, :R, t_lo:t_hi].astype(np.float64)
    f = np.einsum("dr,brt->bdt", wf[:, :, 0], xa) + np.einsum("dr,brt->bdt", wf[:, :, 1], xb)
    g = np.einsum("dr,brt->bdt", wg[:, :, 0], xa) + np.einsum("dr,brt->bdt", wg[:, :, 1], xb)
    if bias_f is not None:
        f = f + np.asarray(bias_f)[:D].astype(np.float64)[None, :, None]
    if bias_g is not None:
        g = g + np.asarray(bias_g)[:D].astype(np.float64)[None, :, None]
    if tab is not None:
        idx = cond_index(t_lo, t_hi, cond_mode, cond_le, cond_q)
        tab = np.asarray(tab)
        f = f + tab[:, :D][:, :, idx].astype(np.float64)
        g = g + tab[:, tab_g_row:tab_g_row + D][:, :, idx].astype(np.float64)
    th = np.tanh(f)
    sg = 1.0 / (1.0 + np.exp(-g))
    z = th * sg
    dzt = np.zeros_like(z)
    if dy is not None:
        dzt += np.einsum("rd,brt->bdt", wd[:, :, 0], np.asarray(dy)[:, :R, t_lo:t_hi].astype(np.float64))
    if dz is not None and z_lo < t_hi:
        lo = max(z_lo, t_lo)
        dzt[:, :, lo - t_lo:] += np.asarray(dz)[:, :D, lo:t_hi].astype(np.float64)
    df = dzt * sg * (1.0 - th * th)
    dg = dzt * th * sg * (1.0 - sg)
    return df, dg, z
