"""What the two GENERAL plans (music_amd/engine_generic.py, music_amd/ae_generic.py) are both built from.

The autoencoder's decoder with its conditioning folded away IS a wavenet (wavenet_autoencoder/model1.py:158-225 against
wavenet/model.py:104-144), so both plans are sequences of the same few layers, one product per launch:

    GeneralPlan   the host side every general plan has on top of engine_base.EngineBase: geometry of a k-tap dilated stack (`k`,
                  `rf`, `off`, `pairs`), weight packing, workspaces and their slab plan, the padded input copy, the chunk softmax by Q
    PackBuilder   places the weights' flat-parameter offsets into the matrices of a packs.PackSet (forward packs, transposed
                  backward packs, gradient matrices; the gather map is derived from them)
    Pass          the launches of ONE forward or backward pass: k-tap conv, gated block, epilogue, each forward and backward,
                  with an optional conditioning table (None = the WaveNet plan)

Nothing here knows which plan calls it: what differs between them (row order of the gate's halves, bias layout, pack tags,
conditioning) arrives as data.  PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK, PAD_BACK, EngineBase, SlabPlan, _pad
from .packs import PackSet, transposed

NONE4, NONE3 = (None, 0, 0, 0), (None, 0, 0)


class PackBuilder(PackSet):
    """The weight matrices of a general plan (packs.PackSet: forward packs, transposed backward packs, gradient matrices, gather map),
    placed weight by weight.  Several weights may share one matrix (same tag, different rows)."""

    def __init__(self, spec, k, pairs):
        super().__init__(spec.total)
        self.sp, self.k, self.pairs = spec, k, pairs

    def conv_k(self, pname, tag, rows, rows_p, cols, cols_p, row_map=None, tagT=None):
        """A k-tap conv weight [rows][cols][k] as per-pair forward packs "<tag>_<p>" (rows_p x taps * cols_p) and their transposes
        "<tagT>_<p>" (cols_p x taps * rows_p; tagT defaults to <tag>T).  row_map: pack row of weight row r (a second weight with
        the same tag and other rows lands in the same matrices)."""
        w3 = self.sp.conv(pname)
        rm = np.arange(rows) if row_map is None else row_map
        for p, pair in enumerate(self.pairs):
            tp = [j for j in pair if j is not None]
            w = self.matrix(self.f, "%s_%d" % (tag, p), rows_p, len(tp) * cols_p)
            wt = self.matrix(self.b, "%s_%d" % (tagT or tag + "T", p), cols_p, len(tp) * rows_p)
            for tl, j in enumerate(tp):
                w[rm, tl * cols_p:tl * cols_p + cols] = w3[:, :, j]
                wt[:cols, tl * rows_p + rm] = w3[:, :, j].T

    def stacked_1x1(self, pnames, tag, rows, rows_p, cols, cols_p, tagT=None):
        """1x1 conv weights [rows][cols][1] side by side on the K axis of one forward pack "<tag>" (rows_p x len(pnames) * cols_p)
        and its transpose "<tagT>": the skip convs of all blocks are one product."""
        w = self.matrix(self.f, tag, rows_p, len(pnames) * cols_p)
        for i, pname in enumerate(pnames):
            w[:rows, i * cols_p:i * cols_p + cols] = self.sp.conv(pname)[:, :, 0]
        self.bwd(tagT or tag + "T", transposed(w))

    def conv_1(self, pname, tag, rows, rows_p, cols, cols_p, tagT=None):
        self.stacked_1x1([pname], tag, rows, rows_p, cols, cols_p, tagT)

    def bias_rows(self, names, row_maps):
        """Rows of the gradient pack for every bias in `names`.  row_maps[name] = (gradient row of bias row r, rows reserved): a bias
        whose gradient wn_bias_grad writes in another row order than the parameter's."""
        for name in names:
            self.bias(name, self.sp.off[name], self.sp.shape[name][0], *row_maps.get(name, ()))

    def gather_rows(self, layers, rows_p):
        """Gather map flat buffer -> one padded column of rows_p rows per layer; layers[i] = [(bias name, pack row of its row r)]."""
        bi = np.full((len(layers), rows_p), -1, dtype=np.int64)
        for i, lst in enumerate(layers):
            for name, rm in lst:
                bi[i, rm] = self.sp.off[name] + np.arange(len(rm))
        return bi.reshape(-1).astype(np.int32)


class GeneralPlan(EngineBase):
    """Host side common to the general plans.  A plan sets `dil`, `k`, `Q`, `QP`, `use_bias`, `mode_fwd`, `mode_bwd`, `device`,
    `spec`, `param_names`, `flat`, `flat_grad`, then calls _geometry(), _finish_packs() and _init_state(); it provides
    _make_workspace(), _bwd_buffers(), backward_from_dlogits() and its own forward."""

    def _geometry(self):
        if self.k < 1:
            raise ValueError("filter_width must be >= 1")
        self.N = len(self.dil)
        self.rf = (self.k - 1) * (sum(self.dil) + 1) + 1
        self.off = [self.k - 1]                            # first valid absolute time of x_i
        for d in self.dil:
            self.off.append(self.off[-1] + (self.k - 1) * d)
        assert self.off[-1] == self.rf - 1
        self.pairs = [(j, j + 1 if j + 1 < self.k else None) for j in range(0, self.k, 2)]

    def _bias_ptr(self, name):
        return ptr(self.flat, self.spec.off[name]) if self.use_bias else None

    def _taps(self, pair, d):
        """(shift of tap j0, shift of tap j1 or 0, 1 if there is a second tap): input column = t - (k-1-j) d"""
        j0, j1 = pair
        return -(self.k - 1 - j0) * d, (-(self.k - 1 - j1) * d if j1 is not None else 0), (1 if j1 is not None else 0)

    # ------------------------------------------------------------------ packs
    def _finish_packs(self, pb, gate_bias, gate_rows_p):
        """pb: the plan's PackBuilder, every weight and bias placed.  gate_bias: per block, the biases of the [f | g] product as
        [(name, pack row of bias row r)] - gathered into `bfg` in the product's padded row order by pack_weights()."""
        gidx = pb.gather_maps()[0]
        assert (gidx[:self.n_gather] >= 0).all()             # (learned conditioning projections: wn_cond_proj_bwd writes theirs)
        dev = self.device
        self.gp_off, self.gp_bias_off = pb.gp_off, pb.gp_bias_off
        self.gpack = torch.zeros(pb.go, dtype=torch.float32, device=dev)
        self.gidx = torch.from_numpy(gidx.astype(np.int32)).to(dev)
        self.pk_f_off, self.pk_f_idx, self.pk_f = pb.finish(pb.f, self.mode_fwd, dev)
        self.pk_b_off, self.pk_b_idx, self.pk_b = pb.finish(pb.b, self.mode_bwd, dev)
        if self.use_bias:
            self.bfg_idx = torch.from_numpy(pb.gather_rows(gate_bias, gate_rows_p)).to(dev)
            self.bfg = torch.zeros(self.N * gate_rows_p, dtype=torch.float32, device=dev)

    def pack_weights(self):
        st = _lib.stream()
        call("wn_pack_weights", ptr(self.flat), ptr(self.pk_f_idx), ptr(self.pk_f), self.pk_f_idx.numel(), self.mode_fwd, st)
        call("wn_pack_weights", ptr(self.flat), ptr(self.pk_b_idx), ptr(self.pk_b), self.pk_b_idx.numel(), self.mode_bwd, st)
        if self.use_bias:
            call("wn_gather_grads", ptr(self.flat), ptr(self.bfg_idx), ptr(self.bfg), self.bfg.numel(), st)

    # ------------------------------------------------------------------ workspaces
    def _new_workspace(self, B, T):
        """(workspace with what every plan has, allocator of a [clip][rows][pitch] activation buffer)"""
        dev, Q = self.device, self.Q
        pitch = _pad(T, 256) + 512
        W = T - self.rf + 1
        buf = lambda rows: self.act_buf(B, rows, pitch)
        ws = dict(B=B, T=T, W=W, pitch=pitch, bwd=None)
        # the compact (B, Q, W) logits; rows Q .. QP-1 of the LAST clip are read (against zero weights) by the products that
        # take this tensor as an operand, so QP - Q rows of finite slack follow it
        ws["O"] = torch.zeros(B * Q * W + 32 * W + PAD_BACK, dtype=torch.float32, device=dev)
        if self.QP != Q:
            ws["Xin"] = torch.zeros(B * self.QP * T + PAD_BACK, dtype=torch.float32, device=dev)
        return ws, buf

    # layer i of a per-layer stacked buffer laid out [layer][clip][rows][pitch]
    def _lay(self, ws, key, i, rows):
        return ptr(ws[key], SLACK + i * ws["B"] * rows * ws["pitch"])

    def _stage_input(self, ws, x):
        """A new generation of `ws` on input x (B, Q, T); returns (pointer, clip stride) of what the causal products read."""
        B, Q, T = x.shape
        QP = self.QP
        self._gen += 1
        ws["gen"], ws["x_in"], ws["x_ver"] = self._gen, x, x._version
        if QP != Q:                                          # K runs over whole 32-row steps: a zero-padded copy of the input
            xin = ws["Xin"][:B * QP * T].view(B, QP, T)
            xin[:, :Q].copy_(x)
            ws["xin"] = (ptr(ws["Xin"]), QP * T)
        else:
            ws["xin"] = (ptr(x), Q * T)
        return ws["xin"]

    def _bwd_workspace(self, ws):
        """Backward buffers of the plan plus the slab plan of its weight gradients: the plan's _bwd_buffers() calls add(gradient
        matrix, t_lo, chunk) for every wn_wgrad call, in the order the backward launches them."""
        if ws["bwd"] is not None:
            return ws["bwd"]
        B, T, W, pitch, dev = ws["B"], ws["T"], ws["W"], ws["pitch"], self.device
        plan = SlabPlan(self.gp_off)
        bw = self._bwd_buffers(lambda rows: self.act_buf(B, rows, pitch),
                               lambda name, t_lo, chunk: plan.add(name, _lib.wgrad_slabs(t_lo, T, chunk, B), chunk))
        bw["dO"] = torch.zeros(B * self.Q * W + 32 * W + PAD_BACK, dtype=torch.float32, device=dev)
        bw.update(plan.finish(dev))
        ws["bwd"] = bw
        return bw

    def _add_stack(self, add, fg, dense, causal, n_dense):
        """Slab-plan entries of a stack: per block the k-tap conv's pairs then its 1x1 (the first n_dense blocks), then the
        causal layer's pairs - the order the backward launches them in."""
        np_ = len(self.pairs)
        for i in range(self.N):
            for p in range(np_):
                add(fg % i + "_%d" % p, self.off[i + 1], 512)
            if i < n_dense:
                add(dense % i, self.off[i + 1], 512)
        for p in range(np_):
            add(causal + "_%d" % p, self.k - 1, 512)

    # ------------------------------------------------------------------ chunk softmax: the 256-wide kernels or the any-Q ones
    def _softmax(self, what, ptrs, n, tail=()):
        if self.Q == 256:
            call("wn_chunk_softmax256_" + what, *ptrs, n, *tail, _lib.stream())
        else:
            call("wn_chunk_softmax_" + what, *ptrs, n, self.Q, *tail, _lib.stream())

    def softmax_fwd(self, logits, probs, n):
        self._softmax("fwd", (ptr(logits), ptr(probs)), n)

    def softmax_bwd(self, probs, dprobs, dlogits, n):
        self._softmax("bwd", (ptr(probs), ptr(dprobs), ptr(dlogits)), n)

    def softmax_ce(self, logits, target, probs, dlogits, loss_part, n):
        self._softmax("ce", (ptr(logits), ptr(target), ptr(probs), ptr(dlogits), ptr(loss_part)), n, (1.0 / n,))

    # ------------------------------------------------------------------ backward entry points
    def backward(self, ws, dprobs):
        """Fills self.flat_grad from d loss / d probabilities (B*W, Q), the gradient w.r.t. what forward() returned; dprobs None =
        bw["dO"] already holds d loss / d logits."""
        bw = self._bwd_workspace(ws)
        if dprobs is not None:
            self.softmax_bwd(ws["probs"], dprobs.contiguous(), bw["dO"], ws["B"] * ws["W"])
        self.backward_from_dlogits(ws)

    def _causal_input_grad(self, ws, layers):
        """Gradient of the last backward w.r.t. the module's INPUT, the data gradient of its causal nn.Conv1d's:
        din[q][s] = sum over layers, taps j and rows r of  Wc_j[r][q] dx0[r][s + (k-1-j)],  dx0 living on [k-1, T).
        layers = [(transposed pack tag, padded rows of dx0, backward-workspace key of the dx ping-pong pair)]; one channel
        product per tap pair, summed by torch."""
        if ws["bwd"] is None:
            raise RuntimeError("music_amd: input_grad() needs the backward of this forward to have run")
        B, T, Q = ws["B"], ws["T"], self.Q
        ps = Pass(self, ws, ws["bwd"])
        outs = []
        for tagT, rp, key in layers:
            dx0 = ptr(ws["bwd"][key][0], SLACK)
            outs += [torch.empty(B, Q, T, dtype=torch.float32, device=self.device) for _ in self.pairs]
            ps.conv_k_bwd(None, dx0, rp * ws["pitch"], rp, 1, self.k - 1, tagT=tagT, out=[ptr(o) for o in outs[-len(self.pairs):]],
                          out_bs=Q * T, out_pitch=T, K_p=self.QP, K=Q, t_in=0)
        din = outs[0]
        for o in outs[1:]:
            din.add_(o)
        return din


class Pass:
    """The launches of one forward (bw None: forward packs, forward arithmetic) or backward pass over a workspace.  Activation
    arguments are device pointers of [clip][rows][pitch] buffers on absolute time with their clip stride `*_bs`; `*_p` are
    channel counts padded to 32.  cond = (table (B, rows, Le), rows, Le, mode, q) of _conditon (model1.py:227-247) or None."""

    def __init__(self, eng, ws, bw=None):
        self.eng, self.st, self.bw = eng, _lib.stream(), bw
        self.B, self.T, self.pitch = ws["B"], ws["T"], ws["pitch"]
        self.mode, self.pk, self.pk_off = ((eng.mode_fwd, eng.pk_f, eng.pk_f_off) if bw is None else
                                           (eng.mode_bwd, eng.pk_b, eng.pk_b_off))

    def gemm(self, pack, *a):
        self.eng._gemm(self.st, self.B, self.mode, ptr(self.pk, self.pk_off[pack]), *a)

    def wgrad(self, name, *args):
        """args = wn_wgrad's arguments up to relu_b, then ldc, t_lo, t_hi"""
        op = self.bw["plan"][name]
        head, (ldc, t_lo, t_hi) = args[:-3], args[-3:]
        call("wn_wgrad", *head, ptr(self.bw["slab"], op.so), ldc, op.n, t_lo, t_hi, op.chunk, self.B, self.mode, self.st)

    def bias_grad(self, name, a, a_bs, a_pitch, a_shift, rows, t_lo):
        eng = self.eng
        if eng.use_bias:
            call("wn_bias_grad", a, a_bs, a_pitch, a_shift, rows, t_lo, self.T, self.B, ptr(eng.gpack, eng.gp_bias_off[name]), self.st)

    def reduce_grads(self):
        """slabs -> gradient pack -> flat_grad (fixed summation order: bit-reproducible)"""
        eng, bw = self.eng, self.bw
        call("wn_reduce_slabs", ptr(bw["desc"]), bw["nops"], bw["vec"], ptr(bw["slab"]), ptr(eng.gpack), self.st)
        call("wn_gather_grads", ptr(eng.gpack), ptr(eng.gidx), ptr(eng.flat_grad), eng.n_gather, self.st)
        eng.mark("slab_reduce")

    def cond_expand(self, cond, t_lo, out, out_bs):
        tab, rows, Le, mode_c, q = cond
        call("wn_cond_expand", tab, rows * Le, Le, rows, t_lo, self.T, mode_c, Le, q, out, out_bs, self.pitch, self.B, self.st)

    def cond_grad(self, cond, t_lo, dy, dy_bs):
        tab, rows, Le, mode_c, q = cond
        call("wn_cond_grad", dy, dy_bs, self.pitch, rows, t_lo, self.T, mode_c, Le, q, tab, rows * Le, Le, self.B, self.st)

    # ------------------------------------------------------------------ conv with k taps
    def conv_k_fwd(self, tag, x, x_bs, x_pitch, t_in, d, K_p, out, out_bs, rows_p, rows, bias, t_lo, relu_in=0, onto_out=False):
        """out[t] (+)= sum_j W_j x[t - (k-1-j) d] (+ bias) on [t_lo, T), x valid from t_in: two taps per launch, later pairs
        accumulate through `resid`; onto_out: the first pair too (out already holds the conditioning)."""
        eng, T, pitch = self.eng, self.T, self.pitch
        for p, pair in enumerate(eng.pairs):
            s0, s1, two = eng._taps(pair, d)
            self.gemm("%s_%d" % (tag, p), x, x if two else None, x_bs, x_pitch, t_in, T, s0, s1, K_p // 32, K_p // 32 if two else 0,
                      rows_p // 16, rows, out, out_bs, pitch, 0, bias if p == 0 else None,
                      (out, out_bs, pitch, t_lo) if (p or onto_out) else NONE4, NONE3, t_lo, T, relu_in)

    def conv_k_bwd(self, tag, dy, dy_bs, rows_p, d, t_lo, x=None, x_bs=0, x_pitch=0, K_p=0, relu=0, tagT=None, out=None, out_bs=0,
                   out_pitch=0, K=0, t_in=0, resid=NONE4, mask=NONE3):
        """Backward of conv_k_fwd from dy (rows_p rows, valid on [t_lo, T)), per tap pair:
            x given:    dW_j = sum_t dy[t] (relu) x[t - (k-1-j) d]^T                 into the slabs of gradient matrix <tag>_<p>
            out given:  dx[t] = (mask) sum_j W_j^T dy[t + (k-1-j) d] + resid[t]      on [t_in, T), pack <tagT>_<p>; later pairs
                        accumulate onto `out` - unless `out` is a list, one output per pair."""
        eng, T, pitch = self.eng, self.T, self.pitch
        for p, pair in enumerate(eng.pairs):
            s0, s1, two = eng._taps(pair, d)
            if x is not None:
                self.wgrad("%s_%d" % (tag, p), dy, dy_bs, pitch, 0, pitch, x, x if two else None, x_bs, x_pitch, s0, s1, x_pitch,
                           K_p // 16, rows_p // 16, relu, (2 if two else 1) * K_p, t_lo, T)
            if out is not None:
                o, r = (out[p], NONE4) if isinstance(out, list) else (out, (out, out_bs, out_pitch, t_in) if p else resid)
                self.gemm("%s_%d" % (tagT, p), dy, dy if two else None, dy_bs, pitch, t_lo, T, -s0, -s1, rows_p // 32,
                          rows_p // 32 if two else 0, K_p // 16, K, o, out_bs, out_pitch, 0, None, r, mask, t_in, T, 0)

    # ------------------------------------------------------------------ gated block (model.py:118-124, model1.py:181-199)
    def gated_fwd(self, tag, dtag, x, x_next, R_p, R, fg, z, z_bs, D_p, d, t_in, t_lo, bias_fg, bias_d, cond=None):
        """[f; g] = (conditioning +) sum_j W_j x[t - (k-1-j) d];  z = tanh(f) sigmoid(g);  x_next = Wd z + x[t] (x_next None: the
        last block, whose output only the skip path uses)."""
        B, T, pitch, st = self.B, self.T, self.pitch, self.st
        xb, fb = R_p * pitch, 2 * D_p * pitch
        if cond is not None:
            self.cond_expand(cond, t_lo, fg, fb)
        self.conv_k_fwd(tag, x, xb, pitch, t_in, d, R_p, fg, fb, 2 * D_p, 2 * D_p, bias_fg, t_lo, 0, cond is not None)
        call("wn_gate_fwd", fg, fb, D_p, D_p, z, z_bs, pitch, t_lo, T, B, st)
        if x_next is not None:
            self.gemm(dtag, z, None, z_bs, pitch, t_lo, T, 0, 0, D_p // 32, 0, R_p // 16, R, x_next, xb, pitch, 0, bias_d,
                      (x, xb, pitch, t_lo), NONE3, t_lo, T, 0)

    def gated_bwd(self, tag, tagT, dtag, dtagT, x, dy, out, R_p, R, fg, z, dz, z_bs, D_p, d, t_in, t_lo, lo, bias_fg, bias_d,
                  cond=None):
        """Backward of gated_fwd: dy = d x_next or None, dz = the skip path's gradient of z (on [lo, T)),
        out = d x.  bias_fg = [(bias name, first row of dfg, rows)]; cond's table receives the conditioning's gradient."""
        B, T, pitch, st, bw = self.B, self.T, self.pitch, self.st, self.bw
        xb, fb = R_p * pitch, 2 * D_p * pitch
        dfg = ptr(bw["dfg"], SLACK)
        if dy is not None:                               # dz = Wd^T dy + dz_crop
            dzb = ptr(bw["dz"], SLACK)
            self.wgrad(dtag, dy, xb, pitch, 0, pitch, z, None, z_bs, pitch, 0, 0, pitch, D_p // 16, R_p // 16, 0, D_p, t_lo, T)
            self.gemm(dtagT, dy, None, xb, pitch, t_lo, T, 0, 0, R_p // 32, 0, D_p // 16, D_p, dzb, D_p * pitch, pitch, 0, None,
                      (dz, z_bs, pitch, lo), NONE3, t_lo, T, 0)
            dz, z_bs = dzb, D_p * pitch
            self.bias_grad(bias_d, dy, xb, pitch, 0, R, t_lo)
        # (else the last block's x_N is unused: only the skip path reaches z)
        call("wn_gate_bwd", fg, fb, D_p, D_p, dz, z_bs, dfg, fb, pitch, t_lo, T, B, st)
        for name, row, rows in bias_fg:
            self.bias_grad(name, ptr(bw["dfg"], SLACK + row * pitch), fb, pitch, 0, rows, t_lo)
        if cond is not None:
            self.cond_grad(cond, t_lo, dfg, fb)
        # dW[f;g]_j = sum_t [df;dg][t] x[t - (k-1-j) d]^T;  dx[t] = sum_j W_j^T [df;dg][t + (k-1-j) d] + dy[t]
        self.conv_k_bwd(tag, dfg, fb, 2 * D_p, d, t_lo, x, xb, pitch, R_p, 0, tagT, out, xb, pitch, R, t_in,
                        (dy, xb, pitch, t_lo) if dy is not None else NONE4)

    # ------------------------------------------------------------------ epilogue (model.py:127-138, model1.py:201-225)
    def epilogue_fwd(self, t1, t2, Z, z_bs, ND_p, U, H, S_p, S, O, Q_p, Q, W, lo, bias_s, bias_1, bias_2, cond=None):
        """u = sum_i Ws_i z_i;  h = W1 relu(u) (+ conditioning);  o = W2 relu(h), written compact (B, Q, W)"""
        T, pitch = self.T, self.pitch
        sb = S_p * pitch
        self.gemm("skip", Z, None, z_bs, pitch, lo, T, 0, 0, ND_p // 32, 0, S_p // 16, S, U, sb, pitch, 0, bias_s, NONE4, NONE3, lo, T, 0)
        if cond is not None:
            self.cond_expand(cond, lo, H, sb)
        self.gemm(t1, U, None, sb, pitch, lo, T, 0, 0, S_p // 32, 0, S_p // 16, S, H, sb, pitch, 0, bias_1,
                  (H, sb, pitch, lo) if cond is not None else NONE4, NONE3, lo, T, 1)
        self.gemm(t2, H, None, sb, pitch, lo, T, 0, 0, S_p // 32, 0, Q_p // 16, Q, O, Q * W, W, -lo, bias_2, NONE4, NONE3, lo, T, 1)

    def epilogue_bwd(self, t1, t2, dO, dH, dU, dZ, Z, z_bs, ND_p, U, H, S_p, S, Q_p, Q, W, lo, bias_skips, bias_1, bias_2, cond=None):
        """Backward of epilogue_fwd from dO (B, Q, W): the three weight gradients, dH, dU, and dZ for every block at once"""
        T, pitch = self.T, self.pitch
        sb = S_p * pitch
        self.wgrad(t2, dO, Q * W, W, -lo, W, H, None, sb, pitch, 0, 0, pitch, S_p // 16, Q_p // 16, 1, S_p, lo, T)
        self.gemm(t2 + "T", dO, None, Q * W, W, 0, W, -lo, 0, Q_p // 32, 0, S_p // 16, S, dH, sb, pitch, 0, None, NONE4, (H, sb, pitch),
                  lo, T, 0)
        if cond is not None:
            self.cond_grad(cond, lo, dH, sb)
        self.wgrad(t1, dH, sb, pitch, 0, pitch, U, None, sb, pitch, 0, 0, pitch, S_p // 16, S_p // 16, 1, S_p, lo, T)
        self.gemm(t1 + "T", dH, None, sb, pitch, lo, T, 0, 0, S_p // 32, 0, S_p // 16, S, dU, sb, pitch, 0, None, NONE4, (U, sb, pitch),
                  lo, T, 0)
        self.wgrad("skip", dU, sb, pitch, 0, pitch, Z, None, z_bs, pitch, 0, 0, pitch, ND_p // 16, S_p // 16, 0, ND_p, lo, T)
        self.gemm("skipT", dU, None, sb, pitch, lo, T, 0, 0, S_p // 32, 0, ND_p // 16, ND_p, dZ, z_bs, pitch, 0, None, NONE4, NONE3,
                  lo, T, 0)
        self.bias_grad(bias_2, dO, Q * W, W, -lo, Q, lo)
        self.bias_grad(bias_1, dH, sb, pitch, 0, S, lo)
        for name in bias_skips:
            self.bias_grad(name, dU, sb, pitch, 0, S, lo)
