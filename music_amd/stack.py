"""The gated residual stack and the skip epilogue of the two fast engines (engine.WaveNetEngine, the decoder of
model1._AutoencoderEngine) on the block and epilogue kernels, and the autoencoder's encoder block calls.

Every block entry point has ONE writer here: the only place its positional argument list is composed.  "No conditioning" is the
default of one argument (`Cond`); "pair" is one flag: two clips side by side as one 64-row tensor on the 64-channel kernels -
doubled clip strides, the block-diagonal packs (`...2_%d`), the second clip's z / dz rows in a slice of their own, half the batch.

PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
from collections import namedtuple

import torch

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK


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


# ---------------------------------------------------------------------- the skip epilogue
# What the engine's bias=True adds to an epilogue: the names of the N skip biases and of the two products' (the engine's own), src:
# name -> pointer of the bias in the flat buffer, dst: name -> where wn_bias_grad leaves its gradient, and the flat-buffer offsets
# of the skip biases (their sum is the skip product's bias)
EpiBias = namedtuple("EpiBias", "skips b1 b2 src dst skip_offs")
# One backward pass: the shape, the clip strides of the S-row and of the z tensors, and every pointer
_EpiBwd = namedtuple("_EpiBwd", "bw B T W pitch sb zb dO dH dU dZ U H Z")


class SkipEpilogue:
    """u = sum_i Ws_i z_i;  h = W1 relu(u) (+ c);  o = W2 relu(h), written compact (B, Q, W) - on the crop [rf - 1, T), forward and
    backward, in one launch each where the fused kernels apply (256 skip / 256 quantisation channels, x3 modes, whole tile groups of
    the skip product's K / rows), else in three.  What differs between its users is handed in: `eng` (an EngineBase: side stream,
    wgrad), the names of the three packs (= gradient matrices = slab ops; "<name>T", "<name>c", "<name>Tc": packs.PackSet.epilogue),
    `keys` = the workspace keys of u, h and of c (the residual of the second product, None: none) and the backward workspace's key of
    dh, the channel counts, `fr` / `br` (pack name -> pointer), `bias` (an EpiBias, None without biases), `fmark` (fine timing
    marks), and where the bias gradients go in the three-launch backward (bias_early: as soon as dh and du exist, else last)."""

    def __init__(self, eng, names, keys, CH, S, SP, fr, br, mode_f, mode_b, bias=None, fmark=lambda name: None, bias_early=False):
        self.eng, self.names, self.keys, self.CH, self.S, self.SP, self.fr, self.br = eng, names, keys, CH, S, SP, fr, br
        self.mode_f, self.mode_b, self.bias, self.fmark, self.bias_early = mode_f, mode_b, bias, fmark, bias_early
        self.N, self.Q, self.lo, self.K = eng.N, eng.Q, eng.rf - 1, eng.N * CH
        x3 = (_lib.F16X3, _lib.BF16X3)
        self.fused_fwd_ok = SP == 256 and self.Q == 256 and (self.K // 32) % 2 == 0 and mode_f in x3 and keys[2] is None
        self.fused_bwd_ok = SP == 256 and self.Q == 256 and (self.K // 16) % 3 == 0 and mode_b in x3

    # ------------------------------------------------------------------ one writer per entry point
    def fused_fwd(self, ws, bias_s, st):
        """the three products in ONE launch per 128-column tile, U and H handed on chip (wn_skip_epilogue_fwd, ABI v5)"""
        (skip, p1, p2), (kU, kH, _, _), b, pitch, W, Q = self.names, self.keys, self.bias, ws["pitch"], ws["W"], self.Q
        call("wn_skip_epilogue_fwd", ptr(ws["Z"], SLACK), self.K * pitch, pitch, self.K // 32, self.fr(skip), bias_s,
             ptr(ws[kU], SLACK), ptr(ws[kH], SLACK), self.SP * pitch, self.fr(p1 + "c"), b.src(b.b1) if b else None,
             self.fr(p2 + "c"), b.src(b.b2) if b else None, ptr(ws["O"]), Q * W, W, self.S, Q, self.lo, ws["T"], ws["B"], self.mode_f, st)

    def products_fwd(self, ws, bias_s, b0, nb, s_):
        """skip product -> second product (+ c) -> third product for clips b0 .. b0 + nb - 1 on stream s_"""
        (skip, p1, p2), (kU, kH, kC, _), b, fr = self.names, self.keys, self.bias, self.fr
        pitch, T, W, lo, SP, S, Q, K, mf = ws["pitch"], ws["T"], ws["W"], self.lo, self.SP, self.S, self.Q, self.K, self.mode_f
        sb, zb = SP * pitch, K * pitch
        U, H = ptr(ws[kU], SLACK + b0 * sb), ptr(ws[kH], SLACK + b0 * sb)
        call("wn_chan_gemm", ptr(ws["Z"], SLACK + b0 * zb), None, zb, pitch, lo, T, 0, 0, K // 32, 0, fr(skip), SP // 16, S,
             U, sb, pitch, 0, bias_s, None, 0, 0, 0, None, 0, 0, lo, T, 0, nb, mf, s_)
        self.fmark("f_skip")
        call("wn_chan_gemm", U, None, sb, pitch, lo, T, 0, 0, SP // 32, 0, fr(p1), SP // 16, S, H, sb, pitch, 0, b.src(b.b1) if b else None,
             *((ptr(ws[kC], SLACK + b0 * sb), sb, pitch, lo) if kC else (None, 0, 0, 0)), None, 0, 0, lo, T, 1, nb, mf, s_)
        self.fmark("f_p1")
        call("wn_chan_gemm", H, None, sb, pitch, lo, T, 0, 0, SP // 32, 0, fr(p2), Q // 16, Q, ptr(ws["O"], b0 * Q * W), Q * W, W, -lo,
             b.src(b.b2) if b else None, None, 0, 0, 0, None, 0, 0, lo, T, 1, nb, mf, s_)

    def fused_bwd(self, a, st):
        """dH, dU and dZ in ONE launch per 128-column tile (wn_skip_epilogue_bwd, ABI v5)"""
        skip, p1, p2 = self.names
        call("wn_skip_epilogue_bwd", a.dO, self.Q * a.W, a.W, a.H, a.U, a.sb, a.pitch, a.dH, a.dU, a.dZ, a.zb, self.br(p2 + "T"),
             self.br(p1 + "Tc"), self.br(skip + "Tc"), self.K // 16, self.K, self.S, self.lo, a.T, a.B, self.mode_b, st)

    def wgrad(self, k, a, st):
        """Weight gradient of product k (0: the skip convs', from dU and Z; 1: from dH and relu(U); 2: from dO and relu(H)) on stream
        st; None: on the side stream, as soon as its operands exist"""
        SP, Q, K, lo, pitch = self.SP, self.Q, self.K, self.lo, a.pitch
        args = ((a.dU, a.sb, pitch, 0, pitch, a.Z, None, a.zb, pitch, 0, 0, pitch, K // 16, SP // 16, 0, K, lo, a.T) if k == 0 else
                (a.dH, a.sb, pitch, 0, pitch, a.U, None, a.sb, pitch, 0, 0, pitch, SP // 16, SP // 16, 1, SP, lo, a.T) if k == 1 else
                (a.dO, Q * a.W, a.W, -lo, a.W, a.H, None, a.sb, pitch, 0, 0, pitch, SP // 16, Q // 16, 1, SP, lo, a.T))
        if st is None:
            self.eng.wgrad_s(a.bw, a.B, self.mode_b, self.names[k], *args)
        else:
            self.eng.wgrad(a.bw, a.B, self.mode_b, st, self.names[k], *args)

    def data_grad(self, k, a, st):
        """dH = (W2^T dO) * [H > 0] (k = 2);  dU = (W1^T dH) * [U > 0] (1);  dZ = Ws^T dU, all N crops at once (0)"""
        SP, S, Q, K, lo, pitch, T, sb, br = self.SP, self.S, self.Q, self.K, self.lo, a.pitch, a.T, a.sb, self.br(self.names[k] + "T")
        if k == 2:
            call("wn_chan_gemm", a.dO, None, Q * a.W, a.W, 0, a.W, -lo, 0, Q // 32, 0, br, SP // 16, S,
                 a.dH, sb, pitch, 0, None, None, 0, 0, 0, a.H, sb, pitch, lo, T, 0, a.B, self.mode_b, st)
        elif k == 1:
            call("wn_chan_gemm", a.dH, None, sb, pitch, lo, T, 0, 0, SP // 32, 0, br, SP // 16, S,
                 a.dU, sb, pitch, 0, None, None, 0, 0, 0, a.U, sb, pitch, lo, T, 0, a.B, self.mode_b, st)
        else:
            call("wn_chan_gemm", a.dU, None, sb, pitch, lo, T, 0, 0, SP // 32, 0, br, K // 16, K,
                 a.dZ, a.zb, pitch, 0, None, None, 0, 0, 0, None, 0, 0, lo, T, 0, a.B, self.mode_b, st)

    def bias_grads(self, a, st):
        """row sums of dO, dH and (for every block's skip conv alike) dU"""
        b, lo = self.bias, self.lo
        if b:
            call("wn_bias_grad", a.dO, self.Q * a.W, a.W, -lo, self.Q, lo, a.T, a.B, b.dst(b.b2), st)
            call("wn_bias_grad", a.dH, a.sb, a.pitch, 0, self.S, lo, a.T, a.B, b.dst(b.b1), st)
            for name in b.skips:
                call("wn_bias_grad", a.dU, a.sb, a.pitch, 0, self.S, lo, a.T, a.B, b.dst(name), st)

    # ------------------------------------------------------------------ the epilogue
    def skip_bias(self, ws):
        """The skip product's bias, the sum of the N skip convs' (None without biases): a torch sum of its own on the current stream"""
        if not self.bias:
            return None
        flat = self.eng.flat
        ws["bias_skip"] = sum(flat[o:o + self.S] for o in self.bias.skip_offs).contiguous()
        return ptr(ws["bias_skip"])

    def forward(self, ws, bias_s, st, fused, chains):
        """From ws["Z"] to the logits in ws["O"]; bias_s = skip_bias(ws).  fused: the one launch, where it applies; else `chains`
        per-clip-group chains of the three products, every second one on the side stream (1 = one chain on the main stream;
        bit-identical results: tests/test_gpu_switches.py)"""
        B = ws["B"]
        nsplit = min(chains, B)
        if fused and self.fused_fwd_ok:
            self.fused_fwd(ws, bias_s, st)
        elif nsplit >= 2:
            # the three products of each part of the clips as a chain of its own, every second chain on the side stream: a
            # product's half-empty last round of workgroups (408 tiles of 256 columns on 256 CUs) then packs into the other
            # chain's launches (0.435-0.445 vs 0.466-0.469 ms with two chains)
            main, side = torch.cuda.current_stream(), self.eng._side_stream()
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
            bounds = [B * k // nsplit for k in range(nsplit + 1)]
            for k in range(nsplit):
                b0, nb = bounds[k], bounds[k + 1] - bounds[k]
                if k % 2 == 1:
                    with torch.cuda.stream(side):
                        self.products_fwd(ws, bias_s, b0, nb, _lib.stream())
                else:
                    self.products_fwd(ws, bias_s, b0, nb, st)
            ev2 = torch.cuda.Event()
            ev2.record(side)
            main.wait_event(ev2)
        else:
            self.products_fwd(ws, bias_s, 0, B, st)

    def begin_backward(self, ws, bw):
        """The pass's pointers, and the first launch of the backward: the last product's weight gradient, on the side stream.  (On
        its own for a user with launches of its own between this one and the data gradients.)"""
        pitch, (kU, kH, _, kdH) = ws["pitch"], self.keys
        a = _EpiBwd(bw, ws["B"], ws["T"], ws["W"], pitch, self.SP * pitch, self.K * pitch, ptr(bw["dO"]), ptr(bw[kdH], SLACK),
                    ptr(bw["dU"], SLACK), ptr(bw["dZ"], SLACK), ptr(ws[kU], SLACK), ptr(ws[kH], SLACK), ptr(ws["Z"], SLACK))
        self.wgrad(2, a, None)
        self.fmark("b_wgrad_p2")
        return a

    def backward(self, a, st, fused, side_skip=False, after_dh=lambda: None):
        """a = begin_backward(ws, bw).  From bw["dO"] (B, Q, W) to dz of every block in bw["dZ"], the three weight gradients into
        their slabs, the bias gradients.  The weight gradients only feed the slab reduction at the very end: they run on the side
        stream as soon as their operands exist, where their half-empty last rounds of workgroups pack into the data-gradient launches
        beside them.  fused: the one launch for the data gradients, where it applies; side_skip: its skip weight gradient on the
        side stream too, nothing joined; after_dh(): the user's launches on dh (the gradient of c), directly behind the launch that
        produces it."""
        if fused and self.fused_bwd_ok:
            # the two weight gradients that read dH / dU follow the fused launch
            self.fused_bwd(a, st)
            self.fmark("b_fused")
            after_dh()
            self.wgrad(1, a, None)
            # the skip weight gradient on the MAIN stream, beside the second product's on the side stream, and the stack starts when both
            # are done: left to run beside the stack (side_skip, WN_EPI_BWD_ORDER=0) they stretch every backward-block launch - a block
            # launch wants all 256 CUs at once - for the same total (bench A/B on one box: 0.95 + 2.0 against 0.52 + 2.6 ms), and the
            # stack's own time (what `roofline` is computed from) would read 40 % high
            self.wgrad(0, a, None if side_skip else st)
            if not side_skip:
                self.eng.join_side()
            self.bias_grads(a, st)
            return
        self.data_grad(2, a, st)
        self.fmark("b_p2T")
        after_dh()
        self.wgrad(1, a, None)
        self.fmark("b_wgrad_p1")
        self.data_grad(1, a, st)
        self.fmark("b_p1T")
        if self.bias_early:
            self.bias_grads(a, st)
        self.wgrad(0, a, None)
        self.fmark("b_wgrad_skip")
        self.data_grad(0, a, st)
        if not self.bias_early:
            self.bias_grads(a, st)
