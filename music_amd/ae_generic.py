"""The GENERAL execution plan of the autoencoder: every constructor argument the reference accepts
(wavenet_autoencoder/model1.py:14-31).

`model1._AutoencoderEngine` drives the specialised kernels (fused encoder / decoder blocks, one-launch backward blocks,
conditioning on the matrix cores) and covers filter_width == 2, quantization_channel == 256 and up to 64 residual /
dilation channels on both sides - what the reference ships and BASELINE.json names.  This engine runs the same arithmetic
(model1.py:137-268 forward, its autograd backward: SURVEY Appendix B) for ANY filter width, quantisation width and
channel counts out of the library's general kernels, one product per launch - the autoencoder counterpart of
music_amd/engine_generic.py:

    conv with k taps          wn_chan_gemm, two taps per launch (input shifted by -(k-1-j) d), further pairs accumulate
                              through `resid`; ReLU on the input / mask on the output where the encoder needs them
    conditioning (_conditon)  wn_cond_expand of the per-clip table into the conv's output buffer (the products then
                              accumulate onto it), wn_cond_grad for its gradient (bucket sums)
    gate                      wn_gate_fwd / wn_gate_bwd (rows [filter | gate]: the pack puts model1.py:188-190's halves there)
    pooled bottleneck         wn_avgpool / wn_avgpool_bwd
    chunk softmax (+ CE)      the 256-wide kernels when Q == 256, the any-Q ones otherwise (plan_generic picks)
    weight gradients          wn_wgrad slabs + wn_reduce_slabs (bit-reproducible), biases wn_bias_grad

Same x3 arithmetic, HBM layout (absolute time, one pitch, channels padded to 32 with zero weights), flat parameter /
gradient buffers and workspace pool as the fast engine.  The only arithmetic left to torch is what the fast engine leaves
there too: the N + 1 conditioning projections of the pooled encoding ((C x Bw) . (Bw x Le) per clip) and their transposes
in the backward.  The decoder with its conditioning folded away is a wavenet: its gated blocks and epilogue, the k-tap conv, the
pack builder and the slab plan are music_amd/plan_generic.py's, shared with engine_generic.py; the encoder block, the
bottleneck, the pooling and the conditioning projections have this one user and live here.  PyTorch is otherwise used for device memory and streams only.  Nothing here imports oracle/.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK, _Spec, _pad
from .plan_generic import NONE3, NONE4, GeneralPlan, PackBuilder, Pass


class GenericAutoencoderEngine(GeneralPlan):
    def __init__(self, net, device, mode="f16x3", mode_bwd="bf16x3"):
        self.net, self.device = net, device
        self.mode_fwd = _lib.MODE_NAMES[mode]
        self.mode_bwd = _lib.MODE_NAMES[mode_bwd]
        self.dil = [int(d) for d in net.dilations]
        self.k = int(net.filter_width)
        self._geometry()
        self.Q = int(net.quantization_channel)
        self.Re, self.De, self.Bw, self.pool = (net.en_residual_channel, net.en_dilation_channel, net.en_bottleneck_width,
                                                net.en_pool_kernel_size)
        self.Rd, self.Dd, self.Sd = net.de_residual_channel, net.de_dilation_channel, net.de_skip_channel
        self.ReP, self.DeP, self.BwP, self.RdP, self.DdP, self.SP, self.QP = (
            _pad(v, 32) for v in (self.Re, self.De, self.Bw, self.Rd, self.Dd, self.Sd, self.Q))
        self.use_bias = bool(net.use_bias)
        named = list(net.named_parameters())
        self.param_names = [n for n, _ in named]
        self.spec = _Spec([(n, tuple(p.shape)) for n, p in named])
        self.flat = torch.zeros(self.spec.total, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(self.spec.total, dtype=torch.float32, device=device)
        with torch.no_grad():
            for n, p in named:
                o = self.spec.off[n]
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view                                # the module's parameters now ARE the flat buffer
        self._plan_cond(net)
        self._build_packs()
        self._init_state()

    # ------------------------------------------------------------------ packs and gradient maps
    def _build_packs(self):
        N = self.N
        Re, De, Bw, Rd, Dd, Sd, Q = self.Re, self.De, self.Bw, self.Rd, self.Dd, self.Sd, self.Q
        ReP, DeP, BwP, RdP, DdP, SP, QP = self.ReP, self.DeP, self.BwP, self.RdP, self.DdP, self.SP, self.QP
        pb = PackBuilder(self.spec, self.k, self.pairs)
        # encoder (model1.py:137-156)
        pb.conv_k("en_causal_layer.weight", "en_causal", Re, ReP, Q, QP)       # (its transpose: input_grad)
        for i in range(N):
            pb.conv_k("en_dilation_layer_stack.%d.weight" % i, "en_dil%d" % i, De, DeP, Re, ReP)
            pb.conv_1("en_dense_layer_stack.%d.weight" % i, "en_dense%d" % i, Re, ReP, De, DeP)
        pb.conv_1("bottleneck_layer.weight", "bottleneck", Bw, BwP, Re, ReP)
        # decoder (model1.py:158-225): filter_gate rows are [gate (Dd) | filter (Dd)] in the reference (:188-190); the pack puts
        # filter first, gate second - the [f | g] order of wn_gate_fwd / wn_gate_bwd
        pb.conv_k("de_causal_layer.weight", "de_causal", Rd, RdP, Q, QP)
        self.fg_rows = np.concatenate([DdP + np.arange(Dd), np.arange(Dd)])          # reference row r -> pack row
        dn = "de_dilation_layer_stack.%d"
        for i in range(N):
            pb.conv_k(dn % (3 * i) + ".weight", "de_fg%d" % i, 2 * Dd, 2 * DdP, Rd, RdP, row_map=self.fg_rows)
            pb.conv_1(dn % (3 * i + 1) + ".weight", "de_d%d" % i, Rd, RdP, Dd, DdP)
        pb.stacked_1x1([dn % (3 * i + 2) + ".weight" for i in range(N)], "skip", Sd, SP, Dd, DdP)
        pb.conv_1("connection_1.weight", "c1", Sd, SP, Sd, SP)
        pb.conv_1("connection_2.weight", "c2", Q, QP, Sd, SP)
        if self.use_bias:
            # filter_gate bias: its gradient rows come in the pack's [f | g] order, each half apart
            # (not the learned conditioning projections': wn_cond_proj_bwd writes theirs)
            pb.bias_rows([n for n in self.gathered_param_names if n.endswith(".bias")],
                         {dn % (3 * i) + ".bias": (self.fg_rows, 2 * DdP) for i in range(N)})
        # the filter_gate biases of every block in the pack's padded [f | g] row order, gathered from the flat buffer
        self._finish_packs(pb, [[(dn % (3 * i) + ".bias", self.fg_rows)] for i in range(N)], 2 * DdP)

    # ------------------------------------------------------------------ workspace
    def _make_workspace(self, B, T):
        N = self.N
        ws, buf = self._new_workspace(B, T)
        ws["Xe"], ws["He"] = buf((N + 1) * self.ReP), buf(N * self.DeP)
        ws["E"] = buf(self.BwP)
        ws["Xd"], ws["FG"], ws["Z"] = buf((N + 1) * self.RdP), buf(N * 2 * self.DdP), buf(N * self.DdP)
        ws["U"], ws["R1"] = buf(self.SP), buf(self.SP)
        return ws

    def _cond_modes(self, T, Le):
        """(mode, q) of _conditon (model1.py:227-247) on every decoder block's output and on the epilogue: a length that the
        number of pooled frames divides takes the stretch branch (1, L / Le), any other the tile branch (2, -)."""
        out = []
        for i in range(self.N + 1):
            L = T - (self.off[i + 1] if i < self.N else self.rf - 1)
            out.append((1, L // Le) if L % Le == 0 else (2, 1))
        return out

    # ------------------------------------------------------------------ forward (model1.py:256-268)
    def forward(self, x, cond=None, want_probs=True, encode_only=False, classes=None, stages=None):
        """cond: the N + 1 drawn (weight, bias) pairs; None with learned conditioning (parameters of the flat buffer);
        classes: one integer per clip with global class conditioning, else None;
        stages: quantiser dropout of a residual vq bottleneck (EngineBase.vq_stage_counts): None, an int or one int per clip;
        encode_only=True stops behind the pooled (and, with a vq bottleneck, quantised) encoding: (None, enc, ws)"""
        self._check_cond(cond)
        B, Q, T = x.shape
        cls = None if encode_only and classes is None else self.stage_classes(classes, B)      # (the encoder takes no classes)
        nstage = self.vq_stage_counts(stages, B)
        assert Q == self.Q and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda
        W = T - self.rf + 1
        if W <= 0:
            raise ValueError("wave sample not long enough")
        Le = W // self.pool
        if Le < 1:
            raise RuntimeError("Output size is too small: %d samples of encoding cannot be pooled by %d" % (W, self.pool))
        ws = self._ws.get(B, T)
        ws["Le"], ws["cls"] = Le, cls
        N, pitch, dev = self.N, ws["pitch"], self.device
        ReP, DeP, BwP, RdP, DdP, SP, QP = self.ReP, self.DeP, self.BwP, self.RdP, self.DdP, self.SP, self.QP
        if not self.learned:
            cw = torch.stack([c[0][:, :, 0] for c in cond[:N]]).to(dev)      # (N, 2Dd, Bw) reference row order [gate | filter]
            cb = torch.stack([c[1] for c in cond[:N]]).to(dev)
            cfw, cfb = cond[N][0].to(dev), cond[N][1].to(dev)
        self.pack_weights()
        lo, k0 = self.rf - 1, self.k - 1
        xin_p, xin_bs = self._stage_input(ws, x)
        ps = Pass(self, ws)
        st = ps.st

        # ---------------- encoder: relu -> dilated conv -> relu -> 1x1, residual; every x_i and h_i is kept for the backward
        eb, hb = ReP * pitch, DeP * pitch
        xe = lambda i: self._lay(ws, "Xe", i, ReP)
        he = lambda i: self._lay(ws, "He", i, DeP)
        ps.conv_k_fwd("en_causal", xin_p, xin_bs, T, 0, 1, QP, xe(0), eb, ReP, self.Re, self._bias_ptr("en_causal_layer.bias"), k0)
        for i, d in enumerate(self.dil):
            t_lo = self.off[i + 1]
            ps.conv_k_fwd("en_dil%d" % i, xe(i), eb, pitch, self.off[i], d, ReP, he(i), hb, DeP, self.De,
                          self._bias_ptr("en_dilation_layer_stack.%d.bias" % i), t_lo, 1)
            ps.gemm("en_dense%d" % i, he(i), None, hb, pitch, t_lo, T, 0, 0, DeP // 32, 0, ReP // 16, self.Re, xe(i + 1), eb, pitch, 0,
                    self._bias_ptr("en_dense_layer_stack.%d.bias" % i), (xe(i), eb, pitch, t_lo), NONE3, t_lo, T, 1)
        self.mark("enc_stack_fwd")
        E = ptr(ws["E"], SLACK)
        ps.gemm("bottleneck", xe(N), None, eb, pitch, lo, T, 0, 0, ReP // 32, 0, BwP // 16, self.Bw, E, BwP * pitch, pitch, 0,
                self._bias_ptr("bottleneck_layer.bias"), NONE4, NONE3, lo, T, 0)
        enc = torch.empty(B, self.Bw, Le, dtype=torch.float32, device=dev)
        call("wn_avgpool", E, BwP * pitch, pitch, lo, self.pool, Le, self.Bw, ptr(enc), self.Bw * Le, Le, B, st)
        if self.vq:                                           # every frame -> its nearest codebook row: the decoder sees q
            enc = self.vq_fwd(ws, enc, st, nstage)
        if encode_only:
            return None, enc, ws

        # ---------------- conditioning tables en_i = Conv1d_rand(enc) (model1.py:178-179, 216-217), rows in the pack's [f | g] order
        Dd, Sd = self.Dd, self.Sd
        cmodes = self._cond_modes(T, Le)
        if self.learned:                                                               # the learned projections: one launch, every table
            tab = torch.empty(N, B, 2 * DdP, Le, dtype=torch.float32, device=dev)
            enf = torch.empty(B, Sd, Le, dtype=torch.float32, device=dev)
            self.cond_proj_fwd(enc, tab, None, enf, DdP, st, cls)
            ws.update(enc=enc, cmodes=cmodes)
        else:
            en = torch.einsum("nck,bkl->nbcl", cw, enc) + cb[:, None, :, None]         # (N, B, 2Dd, Le)
            tab = torch.zeros(N, B, 2 * DdP, Le, dtype=torch.float32, device=dev)
            tab[:, :, :Dd] = en[:, :, Dd:]
            tab[:, :, DdP:DdP + Dd] = en[:, :, :Dd]
            enf = F.conv1d(enc, cfw, cfb).contiguous()                                 # (B, Sd, Le)
            ws.update(enc=enc, cw=cw, cfw=cfw, cmodes=cmodes)

        # ---------------- decoder: the WaveNet stack and epilogue with a conditioning table under every [f; g] and under r1
        zb = N * DdP * pitch
        xd = lambda i: self._lay(ws, "Xd", i, RdP)
        ps.conv_k_fwd("de_causal", xin_p, xin_bs, T, 0, 1, QP, xd(0), RdP * pitch, RdP, self.Rd, self._bias_ptr("de_causal_layer.bias"), k0)
        bn = "de_dilation_layer_stack.%d.bias"
        for i, d in enumerate(self.dil):
            # [f; g] = conditioning (expanded over time) + sum_j W_j x_i[t - (k-1-j) d] (+ bias)
            ps.gated_fwd("de_fg%d" % i, "de_d%d" % i, xd(i), xd(i + 1) if i < N - 1 else None, RdP, self.Rd,
                         self._lay(ws, "FG", i, 2 * DdP), ptr(ws["Z"], SLACK + i * DdP * pitch), zb, DdP, d, self.off[i], self.off[i + 1],
                         ptr(self.bfg, i * 2 * DdP) if self.use_bias else None, self._bias_ptr(bn % (3 * i + 1)),
                         (ptr(tab[i]), 2 * DdP, Le) + cmodes[i])
        self.mark("dec_stack_fwd")
        bias_s = None
        if self.use_bias:
            o = self.spec.off
            ws["bias_skip"] = sum(self.flat[o[bn % (3 * i + 2)]:o[bn % (3 * i + 2)] + Sd] for i in range(N)).contiguous()
            bias_s = ptr(ws["bias_skip"])
        ps.epilogue_fwd("c1", "c2", ptr(ws["Z"], SLACK), zb, N * DdP, ptr(ws["U"], SLACK), ptr(ws["R1"], SLACK), SP, Sd, ptr(ws["O"]),
                        QP, Q, W, lo, bias_s, self._bias_ptr("connection_1.bias"), self._bias_ptr("connection_2.bias"),
                        (ptr(enf), Sd, Le) + cmodes[N])
        probs = None
        if want_probs:
            probs = torch.empty(B * W, Q, dtype=torch.float32, device=dev)
            self.softmax_fwd(ws["O"], probs, B * W)
        ws["probs"] = probs
        self.mark("epilogue_fwd")
        return probs, enc, ws

    # ------------------------------------------------------------------ backward
    def _bwd_buffers(self, buf, add):
        N, lo = self.N, self.rf - 1
        for name, chunk in (("c2", 1024), ("c1", 1024), ("skip", 2048)):
            add(name, lo, chunk)
        self._add_stack(add, "de_fg%d", "de_d%d", "de_causal", N - 1)
        add("bottleneck", lo, 512)
        self._add_stack(add, "en_dil%d", "en_dense%d", "en_causal", N)
        return dict(dR1=buf(self.SP), dU=buf(self.SP), dZ=buf(N * self.DdP), dXd=[buf(self.RdP), buf(self.RdP)], dz=buf(self.DdP),
                    dfg=buf(2 * self.DdP), dE=buf(self.BwP), dXe=[buf(self.ReP), buf(self.ReP)], dHe=buf(self.DeP))

    def input_grad(self, ws):
        """Gradient of the last backward w.r.t. the module's INPUT (the encoder's and the decoder's causal conv, model1.py:137,158)."""
        return self._causal_input_grad(ws, [("de_causalT", self.RdP, "dXd"), ("en_causalT", self.ReP, "dXe")])

    def backward_from_dlogits(self, ws):
        """bw["dO"] holds d loss / d logits (B, Q, W).  Fills self.flat_grad."""
        bw = self._bwd_workspace(ws)
        B, T, W, pitch, Le = ws["B"], ws["T"], ws["W"], ws["pitch"], ws["Le"]
        N, Q, dev = self.N, self.Q, self.device
        ReP, DeP, BwP, RdP, DdP, SP, QP = self.ReP, self.DeP, self.BwP, self.RdP, self.DdP, self.SP, self.QP
        Dd, Sd, Bw = self.Dd, self.Sd, self.Bw
        self._check_input_unchanged(ws)
        ps = Pass(self, ws, bw)
        st = ps.st
        lo, k0 = self.rf - 1, self.k - 1
        zb, eb, hb = N * DdP * pitch, ReP * pitch, DeP * pitch
        cmodes = ws["cmodes"]
        bn = "de_dilation_layer_stack.%d.bias"
        # ---- epilogue: o = C2 relu(r1), r1 = C1 relu(u) + cond, u = sum_i Ws_i z_i
        d_enf = torch.zeros(B, Sd, Le, dtype=torch.float32, device=dev)
        ps.epilogue_bwd("c1", "c2", ptr(bw["dO"]), ptr(bw["dR1"], SLACK), ptr(bw["dU"], SLACK), ptr(bw["dZ"], SLACK), ptr(ws["Z"], SLACK),
                        zb, N * DdP, ptr(ws["U"], SLACK), ptr(ws["R1"], SLACK), SP, Sd, QP, Q, W, lo,
                        [bn % (3 * i + 2) for i in range(N)], "connection_1.bias", "connection_2.bias", (ptr(d_enf), Sd, Le) + cmodes[N])
        self.mark("epilogue_bwd")
        # ---- decoder blocks
        dxd = [ptr(t, SLACK) for t in bw["dXd"]]
        d_tab = torch.zeros(N, B, 2 * DdP, Le, dtype=torch.float32, device=dev)
        for i in range(N - 1, -1, -1):
            # (the filter_gate bias gradient: rows [f | g] of the pack, the gather map un-permutes)
            ps.gated_bwd("de_fg%d" % i, "de_fg%dT" % i, "de_d%d" % i, "de_d%dT" % i, self._lay(ws, "Xd", i, RdP),
                         dxd[(i + 1) % 2] if i < N - 1 else None, dxd[i % 2], RdP, self.Rd, self._lay(ws, "FG", i, 2 * DdP),
                         ptr(ws["Z"], SLACK + i * DdP * pitch), ptr(bw["dZ"], SLACK + i * DdP * pitch), zb, DdP, self.dil[i],
                         self.off[i], self.off[i + 1], lo, [(bn % (3 * i), 0, 2 * DdP)], bn % (3 * i + 1),
                         (ptr(d_tab[i]), 2 * DdP, Le) + cmodes[i])
        self.mark("dec_stack_bwd")
        xin_p, xin_bs = ws["xin"]
        ps.conv_k_bwd("de_causal", dxd[0], RdP * pitch, RdP, 1, k0, xin_p, xin_bs, T, QP)
        ps.bias_grad("de_causal_layer.bias", dxd[0], RdP * pitch, pitch, 0, self.Rd, k0)
        # ---- conditioning projections (unregistered, no gradient of their own): d enc = sum_i cw_i^T d en_i + cfw^T d enf
        if self.learned:                     # ... parameters of their own: d enc, dW and db (flat_grad's tail) in wn_cond_proj_bwd
            d_enc = torch.empty(B, Bw, Le, dtype=torch.float32, device=dev)
            self.cond_proj_bwd(d_tab, False, d_enf, ws["enc"], d_enc, DdP, st, ws["cls"])
            if self.vq:                                       # straight through to e, + the commitment term; the codebook's gradient
                self.vq_bwd(ws, d_enc, st)
        else:
            d_en = torch.cat([d_tab[:, :, DdP:DdP + Dd], d_tab[:, :, :Dd]], 2)         # reference row order [gate | filter]
            d_enc = (torch.einsum("nck,nbcl->bkl", ws["cw"], d_en) + torch.einsum("ck,bcl->bkl", ws["cfw"][:, :, 0], d_enf)).contiguous()
        # ---- encoder: avgpool -> bottleneck -> N blocks -> causal
        dE = ptr(bw["dE"], SLACK)
        call("wn_avgpool_bwd", ptr(d_enc), Bw * Le, Le, lo, self.pool, Le, Bw, dE, BwP * pitch, pitch, T, B, st)
        xe = lambda i: self._lay(ws, "Xe", i, ReP)
        he = lambda i: self._lay(ws, "He", i, DeP)
        ps.wgrad("bottleneck", dE, BwP * pitch, pitch, 0, pitch, xe(N), None, eb, pitch, 0, 0, pitch, ReP // 16, BwP // 16, 0, ReP, lo, T)
        ps.bias_grad("bottleneck_layer.bias", dE, BwP * pitch, pitch, 0, Bw, lo)
        dxe = [ptr(t, SLACK) for t in bw["dXe"]]
        dHe = ptr(bw["dHe"], SLACK)
        ps.gemm("bottleneckT", dE, None, BwP * pitch, pitch, lo, T, 0, 0, BwP // 32, 0, ReP // 16, self.Re, dxe[N % 2], eb, pitch, 0, None,
                NONE4, NONE3, lo, T, 0)
        for i in range(N - 1, -1, -1):
            d, t_in, t_lo = self.dil[i], self.off[i], self.off[i + 1]
            y_lo = lo if i == N - 1 else t_lo                     # the top gradient only exists on the crop [rf - 1, T)
            dy = dxe[(i + 1) % 2]
            # x_{i+1} = Wdense relu(h) + x_i[t]:  dWdense = sum dy relu(h)^T,  dh = (Wdense^T dy) * [h > 0]
            ps.wgrad("en_dense%d" % i, dy, eb, pitch, 0, pitch, he(i), None, hb, pitch, 0, 0, pitch, DeP // 16, ReP // 16, 1, DeP, y_lo, T)
            ps.bias_grad("en_dense_layer_stack.%d.bias" % i, dy, eb, pitch, 0, self.Re, y_lo)
            ps.gemm("en_dense%dT" % i, dy, None, eb, pitch, y_lo, T, 0, 0, ReP // 32, 0, DeP // 16, self.De, dHe, hb, pitch, 0, None, NONE4,
                    (he(i), hb, pitch), t_lo, T, 0)
            ps.bias_grad("en_dilation_layer_stack.%d.bias" % i, dHe, hb, pitch, 0, self.De, t_lo)
            # h = sum_j Wdil_j relu(x_i)[t - (k-1-j) d]:  dWdil_j = sum dh relu(x_i)[t - (k-1-j) d]^T
            # dx_i[t] = [x_i > 0] sum_j Wdil_j^T dh[t + (k-1-j) d] + dy[t]
            ps.conv_k_bwd("en_dil%d" % i, dHe, hb, DeP, d, t_lo, xe(i), eb, pitch, ReP, 1, "en_dil%dT" % i, dxe[i % 2], eb, pitch, self.Re,
                          t_in, (dy, eb, pitch, y_lo), (xe(i), eb, pitch))
        self.mark("enc_stack_bwd")
        ps.conv_k_bwd("en_causal", dxe[0], eb, ReP, 1, k0, xin_p, xin_bs, T, QP)
        ps.bias_grad("en_causal_layer.bias", dxe[0], eb, pitch, 0, self.Re, k0)
        ps.reduce_grads()

    # ------------------------------------------------------------------ fused training step (wavenet_autoencoder/train.py:146-160)
    def loss_and_grad(self, x, target, cond=None, objective=None, classes=None, stages=None, windows=None, window_pos=None,
                      weights=None, ignore_index=None, label_smoothing=0.0):
        """objective: None = self.objective (EngineBase); stages: as in forward; windows / window_pos, weights / ignore_index /
        label_smoothing: step_nll's (the shared base)"""
        return self._throttled(lambda: self._fused_tail(self.forward(x, cond, want_probs=False, classes=classes, stages=stages)[2], target,
                                                       objective=objective, windows=windows, window_pos=window_pos,
                                                       weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing))
