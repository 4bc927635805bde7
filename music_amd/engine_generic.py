"""The GENERAL execution plan: every constructor argument the reference accepts (wavenet/model.py:8-15).

`engine.WaveNetEngine` drives the specialised kernels (fused residual block forward, one-launch backward block, code-aware
causal layer) and covers filter_width == 2, quantization_channels == 256 and up to 64 residual / dilation channels - every
configuration the reference ships or BASELINE.json names.  Anything else used to raise.  This engine runs the same
arithmetic for ANY filter width, quantisation channel count and channel widths out of the library's
general kernels, one product per launch:

    conv with k taps        wn_chan_gemm, two taps per launch (input shifted by -(k-1-j) d for tap j), further pairs
                            accumulate through `resid`                      (model.py:104,118-119)
    gate                    wn_gate_fwd / wn_gate_bwd (f and g are kept for the backward)   (model.py:120)
    dense + residual, skip, post-processing      wn_chan_gemm               (model.py:121-138)
    chunk softmax (+ CE)    the 256-wide kernels when Q == 256, the any-Q ones otherwise (plan_generic picks)   (model.py:142-144)
    weight gradients        wn_wgrad slabs + wn_reduce_slabs (bit-reproducible), data gradients wn_chan_gemm on W^T

Same x3 arithmetic (f16 split forward, bf16 split backward), same HBM layout (absolute time, one pitch, channels padded to
32 with zero weights), same flat parameter / gradient buffers, same workspace pool as the fast engine; 2x slower per step
at config-2 shapes (8.6 vs 4.3 ms: it is round 1's first correct structure), which is why it is only selected where the fast engine does
not apply.  The layers themselves (k-tap conv, gated block, epilogue, pack builder, slab plan) are music_amd/plan_generic.py's,
shared with the autoencoder's general plan.  PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK, _pad
from .plan_generic import GeneralPlan, PackBuilder, Pass


class GenericWaveNetEngine(GeneralPlan):
    def __init__(self, dilations, residual_channels, dilation_channels, skip_channels, quantization_channels=256,
                 filter_width=2, use_bias=False, mode_fwd="f16x3", mode_bwd="bf16x3", device=None, global_classes=0, global_channels=0,
                 phase_period=0):
        self.dil = [int(d) for d in dilations]
        self.k = int(filter_width)
        self.g_n, self.g_E = int(global_classes), int(global_channels)
        self.phase = int(phase_period)                     # phase-conditioned: the period P of the stream's stages (0: off)
        self._geometry()
        self.R, self.D, self.S, self.Q = residual_channels, dilation_channels, skip_channels, quantization_channels
        self.use_bias = bool(use_bias)
        self.RP, self.DP, self.SP, self.QP = (_pad(v, 32) for v in (self.R, self.D, self.S, self.Q))
        self.CH = self.RP                                  # rows of a residual-stream layer (fast_generate reads ws["X"])
        self.mode_fwd = _lib.MODE_NAMES[mode_fwd] if isinstance(mode_fwd, str) else mode_fwd
        self.mode_bwd = _lib.MODE_NAMES[mode_bwd] if isinstance(mode_bwd, str) else mode_bwd
        self.device = torch.device(device if device is not None else "cuda")
        _lib.load()
        self._build_spec()
        self._build_packs()
        self._init_state()

    # ------------------------------------------------------------------ packs and gradient maps
    def _build_packs(self):
        N, R, D, S, Q, RP, DP, SP, QP = self.N, self.R, self.D, self.S, self.Q, self.RP, self.DP, self.SP, self.QP
        pb = PackBuilder(self.spec, self.k, self.pairs)
        wn, bn = "dilation_layer_stack.%d.weight", "dilation_layer_stack.%d.bias"
        g_rows = DP + np.arange(D)
        pb.conv_k("causal_layer.weight", "causal", R, RP, Q, QP)              # (its transpose W_j^T per tap: input_grad)
        for i in range(N):
            # one [f | g] matrix per tap pair: forward rows [f | g] x cols per tap, backward W_j^T with cols per tap = [f | g]
            pb.conv_k(wn % (4 * i), "fg%d" % i, D, 2 * DP, R, RP, tagT="fgT%d" % i)
            pb.conv_k(wn % (4 * i + 1), "fg%d" % i, D, 2 * DP, R, RP, row_map=g_rows, tagT="fgT%d" % i)
            pb.conv_1(wn % (4 * i + 2), "d%d" % i, R, RP, D, DP, tagT="dT%d" % i)
        pb.stacked_1x1([wn % (4 * i + 3) for i in range(N)], "skip", S, SP, D, DP)
        pb.conv_1("post_process_1.weight", "p1", S, SP, S, SP)
        pb.conv_1("post_process_2.weight", "p2", Q, QP, S, SP)
        if self.use_bias:
            pb.bias_rows([n for n in self.gathered_param_names if n.endswith(".bias")], {})
        # [f | g] bias rows of every layer in the padded row order of the fg product, gathered from the flat buffer
        self._finish_packs(pb, [[(bn % (4 * i), np.arange(D)), (bn % (4 * i + 1), g_rows)] for i in range(N)], 2 * DP)

    # ------------------------------------------------------------------ workspace
    def _make_workspace(self, B, T):
        N, RP, DP, SP = self.N, self.RP, self.DP, self.SP
        ws, buf = self._new_workspace(B, T)
        ws["X"], ws["FG"] = buf((N + 1) * RP), buf(N * 2 * DP)
        ws["Z"], ws["U"], ws["H"] = buf(N * DP), buf(SP), buf(SP)
        return ws

    # ------------------------------------------------------------------ forward
    def forward_logits(self, x, ws=None, classes=None, phase_pos=None):
        """classes: one integer per clip of a class-conditional model (EngineBase.stage_classes), else None; phase_pos: the stream
        position of every clip's first target of a phase-conditioned model (EngineBase.stage_phase), else None"""
        B, Q, T = x.shape
        assert Q == self.Q and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda
        W = T - self.rf + 1
        if W <= 0:
            raise ValueError("wave sample not long enough")          # wavenet/model.py:100-101
        cls, pos = self.stage_classes(classes, B), self.stage_phase(phase_pos, B)
        ws = ws or self._ws.get(B, T)
        N, RP, DP, SP, QP, pitch = self.N, self.RP, self.DP, self.SP, self.QP, ws["pitch"]
        xin_p, xin_bs = self._stage_input(ws, x)
        ps = Pass(self, ws)
        ws["cls"], ws["pos"] = cls, pos
        cond, cond_f = (lambda i: None), None
        if pos is not None:
            # a table of P frames per clip in the tile mode (frame (t - t_lo) mod P): the phase tables' columns rotated by the clip's
            # position (wn_phase_tab_fwd), plus the class term's column where there are classes
            P, add = self.phase, (None, None, None)
            empty = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
            if cls is not None:
                add = (empty(N, B, 2 * DP), None, empty(B, self.S))
                self.gclass_fwd(cls, add[0], None, add[2], DP, ps.st)
            tab, enf = empty(N, B, 2 * DP, P), empty(B, self.S, P)
            self.phase_fwd(pos, tab, None, enf, DP, ps.st, add)
            cond = lambda i: (ptr(tab[i]), 2 * DP, P, 2, 1)
            cond_f = (ptr(enf), self.S, P, 2, 1)
            self.mark("phase_fwd")
        elif cls is not None:
            # the clips' tables, one column each: [f; g]_i += G_i emb[c] and h += G_f emb[c], constant over time - a table of one
            # frame stretched over the block's whole valid range (mode 1, q = its length)
            tab = torch.empty(N, B, 2 * DP, dtype=torch.float32, device=self.device)
            enf = torch.empty(B, self.S, dtype=torch.float32, device=self.device)
            self.gclass_fwd(cls, tab, None, enf, DP, ps.st)
            cond = lambda i: (ptr(tab[i]), 2 * DP, 1, 1, T - self.off[i + 1])
            cond_f = (ptr(enf), self.S, 1, 1, W)
            self.mark("gclass_fwd")
        x_ = lambda i: self._lay(ws, "X", i, RP)
        k0, lo, zb = self.k - 1, self.rf - 1, N * DP * pitch
        # causal conv (model.py:104): x0[t] = sum_j Wc_j in[t - (k-1-j)]
        ps.conv_k_fwd("causal", xin_p, xin_bs, T, 0, 1, QP, x_(0), RP * pitch, RP, self.R, self._bias_ptr("causal_layer.bias"), k0)
        self.mark("causal_fwd")
        bn = "dilation_layer_stack.%d.bias"
        for i, d in enumerate(self.dil):
            # [f; g] = sum_j [Wf_j; Wg_j] x_i[t - (k-1-j) d] (model.py:118-119), gate (:120), x_{i+1} = Wd z + x_i[t] (:121-124)
            ps.gated_fwd("fg%d" % i, "d%d" % i, x_(i), x_(i + 1) if i < N - 1 else None, RP, self.R, self._lay(ws, "FG", i, 2 * DP),
                         ptr(ws["Z"], SLACK + i * DP * pitch), zb, DP, d, self.off[i], self.off[i + 1],
                         ptr(self.bfg, i * 2 * DP) if self.use_bias else None, self._bias_ptr(bn % (4 * i + 2)), cond(i))
        self.mark("stack_fwd")
        bias_s = None
        if self.use_bias:
            ws["bias_skip"] = sum(self.param_view(bn % (4 * i + 3)) for i in range(N)).contiguous()
            bias_s = ptr(ws["bias_skip"])
        ps.epilogue_fwd("p1", "p2", ptr(ws["Z"], SLACK), zb, N * DP, ptr(ws["U"], SLACK), ptr(ws["H"], SLACK), SP, self.S,
                        ptr(ws["O"]), QP, Q, W, lo, bias_s, self._bias_ptr("post_process_1.bias"),
                        self._bias_ptr("post_process_2.bias"), cond_f)                             # model.py:127-138
        self.mark("epilogue_fwd")
        return ws

    def forward(self, x, classes=None, phase_pos=None):
        """wavenet/model.py:86-145 -> probabilities (B*W, Q) (fresh tensor)."""
        self.pack_weights()
        ws = self.forward_logits(x, classes=classes, phase_pos=phase_pos)
        B, W = ws["B"], ws["W"]
        probs = torch.empty(B * W, self.Q, dtype=torch.float32, device=self.device)
        self.softmax_fwd(ws["O"], probs, B * W)
        ws["probs"] = probs
        return probs, ws

    # ------------------------------------------------------------------ backward
    def _bwd_buffers(self, buf, add):
        N, RP, DP, SP, lo = self.N, self.RP, self.DP, self.SP, self.rf - 1
        for name, chunk in (("p2", 1024), ("p1", 1024), ("skip", 2048)):
            add(name, lo, chunk)
        self._add_stack(add, "fg%d", "d%d", "causal", N - 1)
        return dict(dH=buf(SP), dU=buf(SP), dZ=buf(N * DP), dX=[buf(RP), buf(RP)], dz=buf(DP), dfg=buf(2 * DP))

    def backward_from_dlogits(self, ws):
        """ws['bwd']['dO'] holds d loss / d pre-softmax (B, Q, W).  Fills self.flat_grad."""
        bw = self._bwd_workspace(ws)
        T, W, pitch = ws["T"], ws["W"], ws["pitch"]
        N, RP, DP, SP, QP, Q = self.N, self.RP, self.DP, self.SP, self.QP, self.Q
        lo, k0, zb = self.rf - 1, self.k - 1, N * DP * pitch
        self._check_input_unchanged(ws)
        ps = Pass(self, ws, bw)
        bn = "dilation_layer_stack.%d.bias"
        cls, pos, cond, cond_f = ws.get("cls"), ws.get("pos"), (lambda i: None), None
        B = ws["B"]
        if pos is not None:                      # the P-frame tables' gradients: sums of [df; dg] and of dh over each frame's samples
            P = self.phase
            d_tab = torch.zeros(N, B, 2 * DP, P, dtype=torch.float32, device=self.device)
            d_enf = torch.zeros(B, self.S, P, dtype=torch.float32, device=self.device)
            cond = lambda i: (ptr(d_tab[i]), 2 * DP, P, 2, 1)
            cond_f = (ptr(d_enf), self.S, P, 2, 1)
        elif cls is not None:                    # the tables' gradients: sums of [df; dg] and of dh over each clip's time
            d_tab = torch.zeros(N, B, 2 * DP, dtype=torch.float32, device=self.device)
            d_enf = torch.zeros(B, self.S, dtype=torch.float32, device=self.device)
            cond = lambda i: (ptr(d_tab[i]), 2 * DP, 1, 1, T - self.off[i + 1])
            cond_f = (ptr(d_enf), self.S, 1, 1, W)
        # ---- epilogue: o = P2 relu(h), h = P1 relu(u) (+ the class term), u = sum_i Ws_i z_i
        ps.epilogue_bwd("p1", "p2", ptr(bw["dO"]), ptr(bw["dH"], SLACK), ptr(bw["dU"], SLACK), ptr(bw["dZ"], SLACK),
                        ptr(ws["Z"], SLACK), zb, N * DP, ptr(ws["U"], SLACK), ptr(ws["H"], SLACK), SP, self.S, QP, Q, W, lo,
                        [bn % (4 * i + 3) for i in range(N)], "post_process_1.bias", "post_process_2.bias", cond_f)
        self.mark("epilogue_bwd")
        dX = [ptr(t, SLACK) for t in bw["dX"]]
        for i in range(N - 1, -1, -1):
            ps.gated_bwd("fg%d" % i, "fgT%d" % i, "d%d" % i, "dT%d" % i, self._lay(ws, "X", i, RP),
                         dX[(i + 1) % 2] if i < N - 1 else None, dX[i % 2], RP, self.R, self._lay(ws, "FG", i, 2 * DP),
                         ptr(ws["Z"], SLACK + i * DP * pitch), ptr(bw["dZ"], SLACK + i * DP * pitch), zb, DP, self.dil[i],
                         self.off[i], self.off[i + 1], lo, [(bn % (4 * i), 0, self.D), (bn % (4 * i + 1), DP, self.D)],
                         bn % (4 * i + 2), cond(i))
        if pos is not None:                      # behind the last table gradient: the phase tables' own, flat_grad's tail ...
            sums = (torch.empty(N, B, 2 * DP, dtype=torch.float32, device=self.device),
                    torch.empty(B, self.S, dtype=torch.float32, device=self.device)) if cls is not None else (None, None)
            self.phase_bwd(pos, d_tab, False, d_enf, DP, ps.st, sums)
            d_tab, d_enf = sums                  # (... and the sums over the frames: the class term's gradients)
        if cls is not None:                      # behind the last table gradient: the global block's own, flat_grad's tail
            self.gclass_bwd(cls, d_tab, False, d_enf, DP, ps.st)
        self.mark("stack_bwd")
        xin_p, xin_bs = ws["xin"]
        ps.conv_k_bwd("causal", dX[0], RP * pitch, RP, 1, k0, xin_p, xin_bs, T, QP)
        ps.bias_grad("causal_layer.bias", dX[0], RP * pitch, pitch, 0, self.R, k0)
        ps.reduce_grads()

    def input_grad(self, ws):
        """Gradient of the last backward w.r.t. the module's INPUT (the causal nn.Conv1d's data gradient, wavenet/model.py:104)."""
        return self._causal_input_grad(ws, [("causalT", self.RP, "dX")])

    # ------------------------------------------------------------------ fused training step (wavenet/train.py:178-181)
    def _step_forward(self, x, classes=None, phase_pos=None):
        self.mark("begin")
        self.pack_weights()
        return self.forward_logits(x, classes=classes, phase_pos=phase_pos)

    def loss_and_grad(self, x, target, want_probs=False, objective=None, windows=None, window_pos=None, classes=None, phase_pos=None,
                      weights=None, ignore_index=None, label_smoothing=0.0):
        """objective: None = self.objective (EngineBase); windows / window_pos, weights / ignore_index / label_smoothing: step_nll's;
        classes, phase_pos: as in forward_logits"""
        return self._throttled(lambda: self._fused_tail(self._step_forward(x, classes, phase_pos), target, want_probs, objective, windows,
                                                       window_pos, weights=weights, ignore_index=ignore_index,
                                                       label_smoothing=label_smoothing))

    def loss_and_grad_codes(self, codes, target, scrambled=True, want_probs=False, objective=None, windows=None, window_pos=None,
                            classes=None, phase_pos=None, weights=None, ignore_index=None, label_smoothing=0.0):
        """the fast engine's entry point on integer codes; here the one-hot is built (wn_onehot) and the dense path runs"""
        return self.loss_and_grad(self.onehot(codes, scrambled), target, want_probs, objective, windows, window_pos, classes, phase_pos,
                                  weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing)

    def onehot(self, codes, scrambled=True):
        """int32 (B,T) codes on the device -> float32 (B,Q,T) (faster_audio_data.py:62-83)."""
        B, T = codes.shape
        out = torch.empty(B, self.Q, T, dtype=torch.float32, device=self.device)
        call("wn_onehot", ptr(codes), ptr(out), B, self.Q, T, 1 if scrambled else 0, _lib.stream())
        return out
