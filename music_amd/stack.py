"""The gated residual stack of the two fast engines (engine.WaveNetEngine, the decoder of model1._AutoencoderEngine) on the block
kernels, the autoencoder's encoder block calls, and the weight-pack helpers of both _build_packs.

Every block entry point has ONE writer here: the only place its positional argument list is composed.  "No conditioning" is the
default of one argument (`Cond`); "pair" is one flag: two clips side by side as one 64-row tensor on the 64-channel kernels -
doubled clip strides, the block-diagonal packs (`...2_%d`), the second clip's z / dz rows in a slice of their own, half the batch.

PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK


# ---------------------------------------------------------------------- weight packs
def full(m, k):
    """An [m][k] map of flat-parameter offsets, all -1 (= zero)"""
    return np.full((m, k), -1, dtype=np.int64)


def diag(m32, rb, cb):
    """m32: [rb*32][cb*32] blocks of 32 x 32 -> [rb*64][cb*64] with every block doubled on the diagonal (clip A, clip B): what the
    64-channel block kernels multiply in pair mode"""
    out = full(rb * 64, cb * 64)
    for a_ in range(rb):
        for b_ in range(cb):
            blk = m32[a_ * 32:(a_ + 1) * 32, b_ * 32:(b_ + 1) * 32]
            for c_ in range(2):
                out[a_ * 64 + c_ * 32:a_ * 64 + (c_ + 1) * 32, b_ * 64 + c_ * 32:b_ * 64 + (c_ + 1) * 32] = blk
    return out


def finish(lst, mode, device):
    """[(name, idx array)] -> (offset of every pack in halfs of the packed buffer, all index maps as one tensor, the packed buffer)"""
    halfs_per_frag = 1024 if mode in (_lib.F16X3, _lib.BF16X3) else 512
    offs, o = {}, 0
    for name, idx in lst:
        offs[name] = o * halfs_per_frag // 512
        o += len(idx)
    idx_all = torch.from_numpy(np.concatenate([i for _, i in lst]).astype(np.int32)).to(device)
    return offs, idx_all, torch.zeros(o * halfs_per_frag // 512, dtype=torch.int16, device=device)


# ---------------------------------------------------------------------- the (P, Q) hand-over of the one-launch blocks
def hand_over(i, N, chain, PQ, dX0, dil, off):
    """(p_in, q_in, dn, p_lo, p_out) of one-launch backward block i.  dx travels down the stack as the unshifted pair (P, Q) of the
    block above (dilation dn, P valid from p_lo), in the (P, Q) buffers PQ[(i + 1) % 2]; a block above in chain form handed dx on
    WHOLE: no Q, valid from ITS t_lo - d = this block's t_lo.  The last block has nothing above.  A first block in chain form writes
    dx_0 whole, straight into dX0, the buffer the causal layer's weight gradient reads (same layout and stride as the (P, Q) buffers)."""
    p_out = ptr(dX0 if i == 0 and chain[0] else PQ[i % 2][0], SLACK)
    if i == N - 1:
        return None, None, 0, 0, p_out
    p_in, q_in = (ptr(t, SLACK) for t in PQ[(i + 1) % 2])
    if chain[i + 1]:
        return p_in, None, 0, off[i + 1], p_out
    return p_in, q_in, dil[i + 1], off[i + 2], p_out


# ---------------------------------------------------------------------- the encoder's block calls (model1.py:137-156)
def enc_resblock_fwd(fr, i, x_in, x_out, h, eb, pitch, bias, De, Re, CHe, d, t_lo, T, B, mode, st, pair=False):
    """h = dilated_conv(relu(x)), x' = dense(relu(h)) + x[tail] in one launch; bias = (dilation bias, dense bias)"""
    two = 2 if pair else 1
    packs = ("en_dil2_%d", "en_dense2_%d") if pair else ("en_dil%d", "en_dense_c%d")
    call("wn_enc_resblock_fwd", x_in, x_out, h, two * eb, two * eb, pitch, fr(packs[0] % i), fr(packs[1] % i),
         *((None, None, 64, 64, 64) if pair else (*bias, De, Re, CHe)), d, t_lo, T, B // two, mode, st)


def enc_resblock_bwd_pq(br, plan, slab, i, x, hand, h, q_out, eb, pitch, CHe, d, t_lo, T, chain, B, mode, st, pair=False):
    """The whole backward of encoder block i in one launch; hand = hand_over()'s tuple, chain = the block's own form (0 / 1 / 2)"""
    p_in, q_in, dn, p_lo, p_out = hand
    two, sfx = (2, "2_%d" % i) if pair else (1, "%d" % i)
    call("wn_enc_resblock_bwd_pq", x, p_in, q_in, dn, p_lo, h, p_out, q_out, two * eb, two * eb, pitch, br("en_denseT" + sfx), br("en_pq" + sfx),
         64 if pair else CHe, d, t_lo, T, ptr(slab, plan["en_dil" + sfx].so), ptr(slab, plan["en_dense" + sfx].so), chain, B // two, mode, st)


# ---------------------------------------------------------------------- the gated stack
# Conditioning of one block: the fp32 table (pointer, clip stride; `le` pooled frames = its pitch), stretch / tile mode and quotient,
# and for the matrix-core forms the tables as packed A fragments (pointer, halfs per clip), the bucket bytes of every sample and the
# slab the one-launch backward leaves its bucket sums in
Cond = namedtuple("Cond", "tab stride le mode q packed packed_stride cidx cslab", defaults=(None, 0, None, None))
NO_COND = Cond(None, 0, 0, 0, 0)


class GatedStack:
    """z = tanh(f) * sigmoid(g) of a 2-tap dilated conv (+ conditioning), x' = dense(z) + x[tail], for blocks 0 .. N - 1: the forward
    and the three backward forms.  What differs between its users is handed in: `eng` (an EngineBase: side stream, wgrad), the prefix
    of the pack and slab-op names, the padded / real channel counts, `fr` / `br` (pack name -> pointer, forward / backward arithmetic),
    `bias` (i -> (bias_f, bias_g, bias_d) pointers or Nones), `fmark` (fine timing marks), and two habits of the user's launches:
      side_wgrad   the fallback form's two wn_wgrad (and the hook's launches behind them) go to the side stream, [df;dg] double-buffered
      zero_tail    [df;dg] holds zeros beyond T (never written: every store is masked to t < T, and pitch >= T + 512 >= T + d), so the
                   data-gradient product reads it up to the pitch and the waves at a clip's end skip the guarded loads of the shifted
                   tap; the residual's strides are then named for the top block too, which has none"""

    def __init__(self, eng, prefix, CH, R, D, fr, br, bias, mode_f, mode_b, fmark=lambda name: None, side_wgrad=False, zero_tail=False):
        self.eng, self.prefix, self.CH, self.R, self.D, self.fr, self.br, self.bias = eng, prefix, CH, R, D, fr, br, bias
        self.mode_f, self.mode_b, self.fmark, self.side_wgrad, self.zero_tail = mode_f, mode_b, fmark, side_wgrad, zero_tail
        self.dil, self.off, self.N = eng.dil, eng.off, eng.N

    def _names(self, i, pair):
        """(fg, d): names of block i's forward packs = its gradient matrices = its slab ops; ...T / pq: the backward packs"""
        sfx = ("2_%d" if pair else "%d") % i
        return self.prefix + "fg" + sfx, self.prefix + "d" + sfx, self.prefix + "dT" + sfx, self.prefix + "pq" + sfx

    # ------------------------------------------------------------------ one writer per entry point
    def block_fwd(self, i, x_in, x_out, z, xb, zb, pitch, t_lo, T, z_lo, B, st, cond=NO_COND, pair=False):
        """z is stored on [z_lo, T); x' (not of the last block: nothing reads it) on [t_lo, T)"""
        fg, dd, _, _ = self._names(i, pair)
        two, c = 2 if pair else 1, cond
        call("wn_resblock_fwd", x_in, x_out, z, two * xb, two * zb, pitch, self.fr(fg), self.fr(dd),
             *((None, None, None, 64, 64, 64) if pair else (*self.bias(i), self.D, self.R, self.CH)), self.dil[i], t_lo, T, z_lo,
             1 if i < self.N - 1 else 0, c.tab, c.stride, c.le, c.mode, c.le, c.q, c.packed, c.packed_stride, c.cidx,
             zb if pair else 0, B // two, self.mode_f, st)

    def block_bwd_pq(self, i, x, hand, dz, q_out, xb, zb, pitch, t_lo, T, bw, chain, B, st, cond=NO_COND, pair=False):
        """Everything of block i's backward in one launch: both weight gradients into their slabs, dx as the pair (p_out, q_out)"""
        fg, dd, dT, pq = self._names(i, pair)
        p_in, q_in, dn, p_lo, p_out = hand
        two, c, plan = 2 if pair else 1, cond, bw["plan"]
        call("wn_resblock_bwd_pq", x, p_in, q_in, dn, p_lo, dz, p_out, q_out, two * xb, two * zb, pitch, self.fr(fg), self.br(dT), self.br(pq),
             64 if pair else self.CH, self.dil[i], t_lo, T, self.off[-1], ptr(bw["slab"], plan[fg].so),
             ptr(bw["slab"], plan[dd].so) if i < self.N - 1 else None, c.tab, c.stride, c.le, c.le, c.cidx, c.cslab,
             zb if pair else 0, chain, B // two, self.mode_f, self.mode_b, st)

    def block_bwd_ms(self, i, x, dy, dz, dfg, xb, zb, pitch, t_lo, T, bw, B, st, cond=NO_COND):
        """Channel-split block: [df;dg] to HBM, both weight gradients into their slabs"""
        fg, dd, dT, _ = self._names(i, False)
        c, plan, (bias_f, bias_g, _) = cond, bw["plan"], self.bias(i)
        call("wn_resblock_bwd_ms", x, dy, dz, dfg, xb, zb, 2 * xb, pitch, self.fr(fg), self.br(dT), bias_f, bias_g, self.D, self.CH, self.dil[i],
             t_lo, T, self.off[-1], ptr(bw["slab"], plan[fg].so), ptr(bw["slab"], plan[dd].so) if i < self.N - 1 else None,
             c.tab, c.stride, c.le, c.mode, c.le, c.q, B, self.mode_f, self.mode_b, st)

    def block_bwd(self, i, x, dy, dz, dfg, zs, xb, zb, pitch, t_lo, T, B, st, cond=NO_COND):
        """[df;dg] to HBM (and z to zs, where the forward's is not used); the weight gradients are launches of their own"""
        fg, _, dT, _ = self._names(i, False)
        c, (bias_f, bias_g, _) = cond, self.bias(i)
        call("wn_resblock_bwd", x, dy, dz, dfg, zs, xb, zb, 2 * xb, xb, pitch, self.fr(fg), self.br(dT), bias_f, bias_g, self.D, self.CH, self.dil[i],
             t_lo, T, self.off[-1], c.tab, c.stride, c.le, c.mode, c.le, c.q, B, self.mode_f, self.mode_b, st)

    # ------------------------------------------------------------------ the stack
    def forward(self, B, T, pitch, X, Z, z_whole, st, cond=None, pair=False):
        """X: [N + 1][B][CH][pitch] (x_0 given), Z: [B][N][CH][pitch].  z_whole: z on every block's whole valid range [t_lo, T) (what a
        backward that reads the forward's z needs), else on the crop [rf - 1, T) the skip product reads.  cond: i -> Cond."""
        CH, N = self.CH, self.N
        xb, zb = CH * pitch, N * CH * pitch
        for i in range(N):
            t_lo = self.off[i + 1]
            self.block_fwd(i, ptr(X, SLACK + i * B * xb), ptr(X, SLACK + (i + 1) * B * xb), ptr(Z, SLACK + i * xb), xb, zb, pitch, t_lo, T,
                           t_lo if z_whole else self.off[-1], B, st, cond(i) if cond else NO_COND, pair)

    def backward(self, form, B, T, pitch, X, Z, bw, dX, st, chain=None, dfg=None, zs=None, cond=None, pair=False, hook=lambda *a: None):
        """From dz (bw["dZ"], all blocks) down to dx_0 in dX[0]; the weight gradients go to the slabs of bw["plan"].  form:
          "pq"  one launch per block (clips or clip pairs); dx travels through bw["PQ"] (hand_over); chain: which blocks hand dx on whole
          "ms"  channel-split block + data-gradient product, dx_i alternating between dX[0] and dX[1]
          "rw"  wn_resblock_bwd + two wn_wgrad + data-gradient product
        dfg: the [df;dg] buffers of "ms" / "rw" (one, or two to alternate between), zs: the recomputed z's of "rw" (None: the forward's Z).
        hook(i, dfg, dy, t_lo, stream): the user's launches on [df;dg] and dy - conditioning and bias gradients - behind the block launch;
        with side_wgrad, in form "rw", behind the weight gradients on the side stream."""
        eng, CH, N, mb = self.eng, self.CH, self.N, self.mode_b
        xb, zb = CH * pitch, N * CH * pitch
        main = torch.cuda.current_stream()
        ev_w = [None, None]          # side-stream completion of the wgrads that read scratch buffer k
        ev_prev = None               # ... of the previous layer's wgrads (they read dX[(i+1)%2])
        for i in range(N - 1, -1, -1):
            d, t_lo, k = self.dil[i], self.off[i + 1], i % 2
            x, dz = ptr(X, SLACK + i * B * xb), ptr(bw["dZ"], SLACK + i * xb)
            c = cond(i) if cond else NO_COND
            if ev_w[k] is not None:
                main.wait_event(ev_w[k])
            if form == "pq":
                hand, q_out = hand_over(i, N, chain, bw["PQ"], dX[0], self.dil, self.off), ptr(bw["PQ"][k][1], SLACK)
                self.block_bwd_pq(i, x, hand, dz, q_out, xb, zb, pitch, t_lo, T, bw, 1 if chain[i] else 0, B, st, c, pair)
                self.fmark("b_block")
                if i == 0 and not chain[0]:
                    # dx_0 for the causal layer: the pair made whole once (19 us; the scatter from codes can also take the
                    # pair as it is - wn_causal_wgrad_codes(dx_q) - but its doubled, masked tile loads cost the same 20 us)
                    call("wn_shift_add", hand[4], q_out, ptr(dX[0], SLACK), xb, pitch, CH, d, t_lo, self.off[0], T, B, st)
                continue
            f = ptr(dfg[i % len(dfg)], SLACK)
            dy = ptr(dX[(i + 1) % 2], SLACK) if i < N - 1 else None

            def dx():
                # dx_i[t] = W1^T dfg[t] + W0^T dfg[t+d] + dy[t]        on [off_i, T)
                # (input from t_lo: dx exists on [t_lo - d, T) and the unshifted tap must read zeros below t_lo, not another layer's stale rows)
                resid = (dy, xb, pitch, t_lo) if dy is not None or self.zero_tail else (None, 0, 0)
                eng._gemm(st, B, mb, self.br(self.prefix + "fgT%d" % i), f, f, 2 * xb, pitch, t_lo, pitch if self.zero_tail else T, 0, d,
                          2 * CH // 32, 2 * CH // 32, CH // 16, self.R, ptr(dX[k], SLACK), xb, pitch, 0, None, resid, (None, 0, 0), self.off[i], T, 0)
            if form == "ms":
                self.block_bwd_ms(i, x, dy, dz, f, xb, zb, pitch, t_lo, T, bw, B, st, c)
                self.fmark("b_block")
                hook(i, f, dy, t_lo, st)
                dx()
                self.fmark("b_dx")
                continue
            z_s = ptr(zs[k], SLACK) if zs else None
            self.block_bwd(i, x, dy, dz, f, z_s, xb, zb, pitch, t_lo, T, B, st, c)
            fg, dd, _, _ = self._names(i, False)

            def wgrads(s2):
                eng.wgrad(bw, B, mb, s2, fg, f, 2 * xb, pitch, 0, pitch, x, x, xb, pitch, -d, 0, pitch, CH // 16, 2 * CH // 16, 0, 2 * CH, t_lo, T)
                if i < N - 1:
                    zsrc, zstr = (z_s, xb) if zs else (ptr(Z, SLACK + i * xb), zb)
                    eng.wgrad(bw, B, mb, s2, dd, dy, xb, pitch, 0, pitch, zsrc, None, zstr, pitch, 0, 0, pitch, CH // 16, CH // 16, 0, CH, t_lo, T)

            def on_side(s2):
                wgrads(s2)
                hook(i, f, dy, t_lo, s2)
                if eng.overlap_wgrad:
                    ev_w[k] = torch.cuda.Event()
                    ev_w[k].record()
            if self.side_wgrad:
                eng.on_side(on_side)
                # the product below writes dX[i % 2], which the PREVIOUS layer's weight gradients may still be reading
                if ev_prev is not None:
                    main.wait_event(ev_prev)
                ev_prev = ev_w[k]
            else:
                hook(i, f, dy, t_lo, st)
                wgrads(st)
            dx()
        for e in ev_w:
            if e is not None:
                main.wait_event(e)
