"""float64 restatement of the phase-conditioned WaveNet (include/wavenet_hip.h, wn_phase_tab_fwd / wn_phase_tab_bwd; music_amd.model
wavenet(phase_period=P)).

The rule: clip b's first target sits at stream position pos[b]; output column c predicts the token at position pos[b] + c and every
block's column that feeds it gains the learned column (pos[b] + c) mod P of that block's table T_i (2 Dd x P, gate rows first), the
output stage T_f's (Sd x P) in front of post_process_1's ReLU.  The kernels read a table of P frames per clip in the tile mode,
frame l = (t - t_lo) mod P of each stage's own t_lo, so stage i's frame l is the parameter's column (l + pos[b] + rot[i]) mod P with
rot[i] = t_lo_i - (rf - 1).  The mod is the mathematical one on Python integers.  A negative position makes its clip NaN and is
never an index."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests.class_cond_ref import _b, chunk_probs, global_block, receptive_field, step_probs

U = 2.0 ** -24


def shift(pos, rot, P):
    return (int(pos) + int(rot)) % P


# ---------------------------------------------------------------------- the two table kernels
def tab_fwd(T, Tf, pos, rot, add_en=None, add_enf=None):
    """T (N, 2Dd, P), Tf (Sd, P) float32, pos (B,), rot (N + 1,), the class term add_en (N, B, 2Dd) / add_enf (B, Sd) float32 or None
    -> en (N, B, 2Dd, P), enf (B, Sd, P) float32: copies, or the correctly rounded fp32 sums"""
    T, Tf = np.asarray(T, dtype=np.float32), np.asarray(Tf, dtype=np.float32)
    N, _, P = T.shape
    B = len(pos)
    en = np.full((N, B, T.shape[1], P), np.nan, dtype=np.float32)
    enf = np.full((B, Tf.shape[0], P), np.nan, dtype=np.float32)
    for b in range(B):
        if int(pos[b]) < 0:
            continue
        for l in range(P):
            for i in range(N):
                en[i, b, :, l] = T[i][:, (l + shift(pos[b], rot[i], P)) % P]
            enf[b, :, l] = Tf[:, (l + shift(pos[b], rot[N], P)) % P]
    if add_en is not None:
        en = np.asarray(add_en, dtype=np.float32)[..., None] + en              # (IEEE: one correctly rounded fp32 add)
        enf = np.asarray(add_enf, dtype=np.float32)[..., None] + enf
    return en, enf


def tab_bwd(d_en, d_enf, pos, rot):
    """d_en (N, B, 2Dd, P), d_enf (B, Sd, P) -> float64 (dT, dTf), their bounds n 2^-24 sum |terms| with n = B terms, and the frame
    sums (s_en (N, B, 2Dd), s_enf (B, Sd)) with theirs, n = P terms"""
    d_en, d_enf = np.asarray(d_en, dtype=np.float64), np.asarray(d_enf, dtype=np.float64)
    N, B, _, P = d_en.shape
    dT, dTf = np.zeros((N,) + d_en.shape[2:]), np.zeros(d_enf.shape[1:])
    aT, aTf = np.zeros_like(dT), np.zeros_like(dTf)
    for b in range(B):
        for s in range(P):
            for i in range(N):
                l = (s - shift(pos[b], rot[i], P)) % P
                dT[i, :, s] += d_en[i, b, :, l] if int(pos[b]) >= 0 else np.nan
                aT[i, :, s] += np.abs(d_en[i, b, :, l])
            l = (s - shift(pos[b], rot[N], P)) % P
            dTf[:, s] += d_enf[b, :, l] if int(pos[b]) >= 0 else np.nan
            aTf[:, s] += np.abs(d_enf[b, :, l])
    sums = (d_en.sum(-1), d_enf.sum(-1))
    sum_bounds = (P * U * np.abs(d_en).sum(-1), P * U * np.abs(d_enf).sum(-1))
    return (dT, dTf), (B * U * aT, B * U * aTf), sums, sum_bounds


def table(en, CH, pair, fill):
    """en (N, B, 2Dd, le) in the reference's row order -> the block table [N][tensors][rows][le] of include/wavenet_hip.h: per clip
    (rows 2 CH: filter rows, then gate rows at CH) or as clip pairs (rows 4 CH: f of A, f of B, g of A, g of B); other rows = fill"""
    N, B, Dd, le = en.shape[0], en.shape[1], en.shape[2] // 2, en.shape[3]
    rows, nt = (4 * CH, B // 2) if pair else (2 * CH, B)
    tab = np.full((N, nt, rows, le), fill, dtype=en.dtype)
    for b in range(B):
        t, h = (b >> 1, b & 1) if pair else (b, 0)
        tab[:, t, h * CH:h * CH + Dd] = en[:, b, Dd:]
        g0 = (2 * CH if pair else CH) + h * CH
        tab[:, t, g0:g0 + Dd] = en[:, b, :Dd]
    return tab


# ---------------------------------------------------------------------- the model
def rotations(dilations, filter_width, P):
    """rot[i] of block i (its t_lo = off[i + 1] against the output's rf - 1), rot[N] = 0 of the output stage"""
    k = filter_width - 1
    off = [k]
    for d in dilations:
        off.append(off[-1] + k * d)
    return [(off[i + 1] - off[-1]) % P for i in range(len(dilations))] + [0]


# ---------------------------------------------------------------------- the model in float64 torch (tests/class_cond_ref.py's, + phase)
def phase_tables(params, n_blocks):
    """(T_0 .. T_N-1 as (2D, P), gate rows first; T_f (S, P))"""
    return [params["phase_layer_stack.%d" % i] for i in range(n_blocks)], params["connection_phase"]


def logits(params, dilations, x, pos, classes=None, filter_width=2):
    """x (B, Q, T), pos (B,) stream positions of the clips' first targets, classes (B,) int64 or None -> pre-softmax (B, Q, W).
    A block's column at absolute time t feeds output column c = t - (rf - 1) and gains phase column (pos + c) mod P."""
    rf = receptive_field(filter_width, dilations)
    out_w = x.size(2) - rf + 1
    if out_w <= 0:
        raise ValueError("wave sample not long enough")
    Tn, Tf = phase_tables(params, len(dilations))
    P, D = Tf.shape[1], Tn[0].shape[0] // 2
    v = None
    if classes is not None:
        G, Gf, emb = global_block(params, len(dilations))
        v = emb[classes]

    def cols(tab, t0, n):
        """(B, rows, n): column (pos_b + t - (rf - 1)) mod P of tab for t = t0 .. t0 + n - 1"""
        idx = torch.tensor([[(int(p) + t - (rf - 1)) % P for t in range(t0, t0 + n)] for p in pos])
        return tab[:, idx].permute(1, 0, 2)
    h = F.conv1d(x, params["causal_layer.weight"], _b(params, "causal_layer"))
    skip, t0 = None, filter_width - 1
    for i, d in enumerate(dilations):
        n = "dilation_layer_stack.%d"
        t0 += (filter_width - 1) * d
        f = F.conv1d(h, params[n % (4 * i) + ".weight"], _b(params, n % (4 * i)), dilation=d)
        g = F.conv1d(h, params[n % (4 * i + 1) + ".weight"], _b(params, n % (4 * i + 1)), dilation=d)
        c = cols(Tn[i], t0, f.size(2))
        if v is not None:
            c = c + (v @ G[i].t())[:, :, None]
        f, g = f + c[:, D:], g + c[:, :D]
        z = torch.sigmoid(g) * torch.tanh(f)
        dense = F.conv1d(z, params[n % (4 * i + 2) + ".weight"], _b(params, n % (4 * i + 2)))
        h = dense + h[:, :, -dense.size(2):]
        s = F.conv1d(z[:, :, -out_w:], params[n % (4 * i + 3) + ".weight"], _b(params, n % (4 * i + 3)))
        skip = s if skip is None else skip + s
    h1 = F.conv1d(F.relu(skip), params["post_process_1.weight"], _b(params, "post_process_1")) + cols(Tf, rf - 1, out_w)
    if v is not None:
        h1 = h1 + (v @ Gf.t())[:, :, None]
    return F.conv1d(F.relu(h1), params["post_process_2.weight"], _b(params, "post_process_2"))


def loss(params, dilations, x, target, pos, classes=None, objective="reference", filter_width=2):
    lg = logits(params, dilations, x, pos, classes, filter_width)
    if objective == "reference":                                       # CrossEntropyLoss on the chunk-softmax probabilities
        return F.cross_entropy(chunk_probs(lg), target.reshape(-1)), lg
    return -torch.log(step_probs(lg).gather(1, target.reshape(-1, 1))).mean(), lg


def loss_and_grads(params, dilations, x, target, pos, classes=None, **kw):
    """(loss, logits, OrderedDict name -> gradient) on float64 copies of params"""
    leaf = OrderedDict((k, v.detach().double().clone().requires_grad_(True)) for k, v in params.items())
    val, lg = loss(leaf, dilations, x.double(), target, pos, classes, **kw)
    grads = torch.autograd.grad(val, list(leaf.values()), allow_unused=True)
    return val.detach(), lg.detach(), OrderedDict((k, g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(leaf, grads))


def greedy_rollout(params, dilations, seed_codes, pos0, n_steps, Q, classes=None, filter_width=2):
    """Free-running argmax decode in float64, one full forward per step: seed_codes (U, rf) int64, pos0 the stream position of the
    first generated token -> (codes (U, n_steps), the smallest top-2 logit margin met)"""
    p64 = {k: v.detach().double() for k, v in params.items()}
    rf = receptive_field(filter_width, dilations)
    hist, out, margin = seed_codes.clone(), [], float("inf")
    U = hist.size(0)
    for n in range(n_steps):
        x = F.one_hot(hist[:, -rf:], Q).permute(0, 2, 1).double()
        lg = logits(p64, dilations, x, [pos0 + n] * U, classes, filter_width)[:, :, -1]
        top = lg.topk(2, dim=1).values
        margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
        code = lg.argmax(1)
        out.append(code)
        hist = torch.cat([hist, code[:, None]], 1)
    return torch.stack(out, 1), margin
