"""Counterpart of the reference's ``wavenet_autoencoder/model1.py`` on the MI355X (forward path).

Same constructor kwargs, attributes, registered sub-modules and ``state_dict`` keys
(``en_dilation_layer_stack.i``, ``en_dense_layer_stack.i``, ``de_dilation_layer_stack.{3i+0..2}`` =
filter_gate / dense / skip, ``en_causal_layer``, ``bottleneck_layer``, ``de_causal_layer``,
``connection_1/2``), same ``forward`` contract (model1.py:256-268): ``(B, Q, T)`` float ->
probabilities ``(B*(T-rf+1), Q)`` with the chunk softmax.

Reference behaviours that are reproduced on purpose:
  * the conditioning projections are 31 FRESH ``nn.Conv1d(bottleneck, C, 1)`` drawn from the global
    torch CPU RNG inside every forward, with bias, never registered or trained
    (model1.py:178-179,216-217) — seed ``torch.manual_seed(s)`` right before ``forward``
    to reproduce a reference run;
  * ``_conditon`` (sic) stretches the encoding when ``len(x) % len(enc) == 0`` and tiles it
    otherwise (model1.py:227-247);
  * gate = FIRST half of the filter_gate channels, filter = second half (model1.py:188-190).
The arithmetic runs through libwavenet_hip.so only (no CPU path).  ``forward`` is differentiable
(``loss.backward()`` fills every parameter's gradient, the encoder's through the random projections
exactly as in the reference).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

try:
    from . import _lib, _losshook, vq_dropout
    from ._lib import call, ptr
    from .engine_base import SLACK, PAD_BACK, EngineBase, SlabPlan, WorkspaceHold, _Spec, _pad
    from .packs import PackSet, causal_mats, diag, epilogue_mats, full, gated_mats, pack_positions, pair_mats, transposed
    from .stack import Cond, EpiBias, GatedStack, SkipEpilogue, enc_resblock_bwd_pq, enc_resblock_fwd, hand_over
except ImportError:
    from music_amd import _lib, _losshook, vq_dropout
    from music_amd._lib import call, ptr
    from music_amd.engine_base import SLACK, PAD_BACK, EngineBase, SlabPlan, WorkspaceHold, _Spec, _pad
    from music_amd.packs import PackSet, causal_mats, diag, epilogue_mats, full, gated_mats, pack_positions, pair_mats, transposed
    from music_amd.stack import Cond, EpiBias, GatedStack, SkipEpilogue, enc_resblock_bwd_pq, enc_resblock_fwd, hand_over


class _AutoencoderEngine(EngineBase):
    """Host-side plan of the autoencoder on one MI355X: flat parameters, packed-weight index maps,
    workspaces, forward (model1.py:256-268) and backward (autograd of it)."""

    def __init__(self, net, device, mode="f16x3", mode_bwd="bf16x3"):
        self.net, self.device = net, device
        self.mode = _lib.MODE_NAMES[mode]
        self.mode_b = _lib.MODE_NAMES[mode_bwd]
        self.dil = [int(d) for d in net.dilations]
        self.N = len(self.dil)
        self.Q = net.quantization_channel
        self.fused_loss_ok = True           # _losshook.py: nn.CrossEntropyLoss on the module's output may run as wn_chunk_softmax256_ce
        if net.filter_width != 2 or self.Q != 256:
            raise NotImplementedError("HIP path implements filter_width == 2 and quantization_channel == 256")
        self.Re, self.De, self.Bw, self.pool = net.en_residual_channel, net.en_dilation_channel, net.en_bottleneck_width, net.en_pool_kernel_size
        self.Rd, self.Dd, self.Sd = net.de_residual_channel, net.de_dilation_channel, net.de_skip_channel
        self.CHe = _pad(max(self.Re, self.De), 32)
        self.CHd = _pad(max(self.Rd, self.Dd), 32)
        if self.CHd not in (32, 64):
            raise NotImplementedError("HIP path supports decoder residual/dilation channels <= 64")
        self.SP, self.BwP = _pad(self.Sd, 32), _pad(self.Bw, 32)
        self.rf = sum(self.dil) + 2
        self.off = [1]
        for d in self.dil:
            self.off.append(self.off[-1] + d)
        self.use_bias = bool(net.use_bias)
        # one launch per encoder block (wn_enc_resblock_fwd) instead of two channel GEMMs; WN_AE_FUSED_ENC=0 = the GEMMs
        self.fused_encoder = os.environ.get("WN_AE_FUSED_ENC", "1") == "1"
        # 32 / 32 channels on both sides (the reference's shipped model_params.json): even batches run BOTH stacks on the
        # 64-channel one-launch blocks, two clips per 64-row tensor with block-diagonal packs (music_amd/engine.py "pair")
        self.pair_ok = (self.CHe == 32 and self.CHd == 32 and not self.use_bias and self.mode == _lib.F16X3 and
                        self.mode_b == _lib.BF16X3 and os.environ.get("WN_PAIR32", "1") == "1")
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
                p.data = view
        self._plan_cond(net)
        self._build_packs()
        self._init_state()

        def de_bias(i):
            """the filter_gate bias is one tensor, gate rows first"""
            bias_fg = self._bias("de_dilation_layer_stack.%d" % (3 * i))
            return bias_fg + 4 * self.Dd if bias_fg is not None else None, bias_fg, self._bias("de_dilation_layer_stack.%d" % (3 * i + 1))
        # the decoder stack: its weight gradients stay on the main stream, its blocks never chain (conditioned blocks hand the pair on)
        self.decoder = GatedStack(self, "de_", self.CHd, self.Rd, self.Dd, self._fr, self._br, de_bias, self.mode, self.mode_b)
        # ... and its epilogue: o = c2(relu(r)), r = c1(relu(u)) + cond_f (the expanded final conditioning C1), u = skip(z).  The bias
        # gradients go to the small buffer of backward()'s _bias_plan, as soon as dR1 and dU exist
        skips = ["de_dilation_layer_stack.%d" % (3 * i + 2) for i in range(self.N)]
        bias = EpiBias(skips, "connection_1", "connection_2", self._bias, lambda name: ptr(self._bias_plan[2], self._bias_plan[0][name]),
                       [self.spec.off[n + ".bias"] for n in skips]) if self.use_bias else None
        self.epilogue = SkipEpilogue(self, ("skip", "c1", "c2"), ("U", "R1", "C1", "dR1"), self.CHd, self.Sd, self.SP, self._fr, self._br,
                                     self.mode, self.mode_b, bias=bias, bias_early=True)

    def _stage_cond(self, cond):
        """cond (N+1 CPU (weight, bias) pairs) -> device tensors cw (N, 2Dd, Bw), cb (N, 2Dd), cfw (Sd, Bw, 1), cfb (Sd) through one
        of three rotating pinned staging buffers (an event per buffer says when its last copy has left)."""
        N, Dd, Sd, Bw = self.N, self.Dd, self.Sd, self.Bw
        n_cw, n_cb, n_fw = N * 2 * Dd * Bw, N * 2 * Dd, Sd * Bw
        total = n_cw + n_cb + n_fw + Sd
        if getattr(self, "_cpin", None) is None or self._cpin[0][0].numel() != total:
            self._cpin = [(torch.empty(total, dtype=torch.float32).pin_memory(), None) for _ in range(3)]
            self._cpin_i = 0
        k = self._cpin_i
        self._cpin_i = (k + 1) % 3
        pin, ev = self._cpin[k]
        if ev is not None:
            ev.synchronize()
        # plain memcpys (numpy): a torch CPU op on more than 32768 elements opens an OpenMP region that wakes EVERY intra-op
        # thread (128 on an MI355X host), and in a container with a CPU quota those spinning threads get the whole process
        # throttled - 80 ms out of every 100 with the reference's shipped parameters (Bw = 512)
        pn = pin.numpy()
        pn[:n_cw].reshape(N, 2 * Dd * Bw)[...] = np.stack([c[0].numpy().reshape(-1) for c in cond[:N]])
        pn[n_cw:n_cw + n_cb].reshape(N, 2 * Dd)[...] = np.stack([c[1].numpy() for c in cond[:N]])
        pn[n_cw + n_cb:n_cw + n_cb + n_fw] = cond[N][0].numpy().reshape(-1)
        pn[n_cw + n_cb + n_fw:] = cond[N][1].numpy()
        dev = torch.empty(total, dtype=torch.float32, device=self.device)
        dev.copy_(pin, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._cpin[k] = (pin, ev)
        return (dev[:n_cw].view(N, 2 * Dd, Bw), dev[n_cw:n_cw + n_cb].view(N, 2 * Dd),
                dev[n_cw + n_cb:n_cw + n_cb + n_fw].view(Sd, Bw, 1), dev[n_cw + n_cb + n_fw:])

    def _bias(self, name):
        return ptr(self.flat, self.spec.off[name + ".bias"]) if self.use_bias else None

    def _fr(self, name):
        return ptr(self.pk, self.pk_off[name])

    def _br(self, name):
        return ptr(self.pkb, self.pkb_off[name])

    def _build_packs(self):
        sp, N, dev = self.spec, self.N, self.device
        CHe, CHd, Re, De, Dd, Bw = self.CHe, self.CHd, self.Re, self.De, self.Dd, self.Bw
        pk = PackSet(sp.total)
        self.wt_idx, self.wt = {}, {}
        for name, ch in (("en_causal", CHe), ("de_causal", CHd)):
            causal = causal_mats(sp.conv(name + "_layer.weight"), ch)
            pk.fwd(name, causal.w)
            pk.bwd(name + "T", causal.wT)
            self.wt_idx[name] = torch.from_numpy(causal.taps).to(dev)
            self.wt[name] = torch.zeros(causal.taps.size, dtype=torch.float32, device=dev)
        dn = "de_dilation_layer_stack.%d.weight"
        for i in range(N):
            wd = sp.conv("en_dilation_layer_stack.%d.weight" % i)              # [De,Re,2]
            w = pk.fwd("en_dil%d" % i, full(CHe, 2 * CHe))
            w[:De, :Re], w[:De, CHe:CHe + Re] = wd[:, :, 0], wd[:, :, 1]
            wt = pk.bwd("en_dilT%d" % i, full(CHe, 2 * CHe))                    # dx: rows Re, K = [tap1^T | tap0^T] over De
            wt[:Re, :De], wt[:Re, CHe:CHe + De] = wd[:, :, 1].T, wd[:, :, 0].T
            # [W1^T; W0^T] over dh: the one-launch backward block of the encoder
            wq = pk.bwd("en_pq%d" % i, np.concatenate([wt[:, :CHe], wt[:, CHe:]]))
            if self.pair_ok:
                pk.fwd("en_dil2_%d" % i, diag(w, 1, 2), pair=True)
                pk.bwd("en_pq2_%d" % i, diag(wq, 2, 1))
            w = pk.fwd("en_dense%d" % i, full(CHe, CHe))
            w[:Re, :De] = sp.conv("en_dense_layer_stack.%d.weight" % i)[:, :, 0]
            pk.fwd("en_dense_c%d" % i, w, chained=True, grad=False)             # chained k order: the fused encoder block
            pk.bwd("en_denseT%d" % i, transposed(w))
            if self.pair_ok:
                pk.fwd("en_dense2_%d" % i, diag(w, 1, 1), chained=True, pair=True)     # (its pack doubles as "en_dense_c2")
                pk.bwd("en_denseT2_%d" % i, diag(transposed(w), 1, 1))
            wfg = sp.conv(dn % (3 * i))                                        # [2Dd,Rd,2], gate rows first: my rows are filter then gate
            g = gated_mats(wfg[Dd:], wfg[:Dd], sp.conv(dn % (3 * i + 1))[:, :, 0], CHd)
            g2 = pair_mats(g) if self.pair_ok else None
            pk.fwd("de_fg%d" % i, g.fg)
            pk.bwd("de_fgT%d" % i, g.fgT)
            pk.bwd("de_pq%d" % i, g.pq)
            if self.pair_ok:
                pk.fwd("de_fg2_%d" % i, g2.fg, pair=True)
                pk.bwd("de_pq2_%d" % i, g2.pq)
            pk.fwd("de_d%d" % i, g.d, chained=True)
            pk.bwd("de_dT%d" % i, g.dT)
            if self.pair_ok:
                pk.fwd("de_d2_%d" % i, g2.d, chained=True, pair=True)
                pk.bwd("de_dT2_%d" % i, g2.dT)
        w = pk.fwd("bottleneck", full(self.BwP, CHe))
        w[:Bw, :Re] = sp.conv("bottleneck_layer.weight")[:, :, 0]
        pk.bwd("bottleneckT", transposed(w))
        # (no chained forward forms: the decoder's forward epilogue is the three products)
        pk.epilogue(epilogue_mats([sp.conv(dn % (3 * i + 2))[:, :, 0] for i in range(N)], sp.conv("connection_1.weight")[:, :, 0],
                                  sp.conv("connection_2.weight")[:, :, 0], CHd, self.SP), "skip", "c1", "c2", chained_fwd=False)
        self.pk_off, self.pk_idx, self.pk = pk.finish(pk.f, self.mode, dev)
        self.pkb_off, self.pkb_idx, self.pkb = pk.finish(pk.b, self.mode_b, dev)
        self.gp_off = pk.gp_off
        self.gpack = torch.zeros(pk.go, dtype=torch.float32, device=dev)
        gidx, ga, gb = pk.gather_maps()
        self.gidx = torch.from_numpy(gidx.astype(np.int32)).to(dev)          # -1 (biases) -> zero gradient
        if self.pair_ok:                                  # pair mode: a stack weight's gradient = the sum of its two copies
            self.gidx_pa = torch.from_numpy(ga.astype(np.int32)).to(dev)
            self.gidx_pb = torch.from_numpy(gb.astype(np.int32)).to(dev)

    def _make_workspace(self, B, T):
        dev = self.device
        pitch = _pad(T, 256) + 512
        W = T - self.rf + 1
        N = self.N
        buf = lambda rows: self.act_buf(B, rows, pitch)
        ws = dict(B=B, T=T, W=W, pitch=pitch, Xe=buf((N + 1) * self.CHe), He=buf(N * self.CHe), E=buf(self.BwP),
                  Xd=buf((N + 1) * self.CHd), Z=buf(N * self.CHd), U=buf(self.SP), R1=buf(self.SP),
                  C1=buf(self.SP), O=torch.zeros(B * self.Q * W + PAD_BACK, dtype=torch.float32, device=dev), bwd=None)
        return ws

    # layer i of a stacked [(N+1) or N][B][CH][pitch] buffer
    def _lay(self, t, i, ch, ws):
        return ptr(t, SLACK + i * ws["B"] * ch * ws["pitch"])

    def forward(self, x, cond=None, want_probs=True, encode_only=False, classes=None, stages=None):
        """cond: list of N+1 (weight (C,Bw,1), bias (C,)) CPU tensors (see wavenet_autoencoder.forward); None with learned
        conditioning, whose projections are parameters of the flat buffer.
        classes: one integer per clip with global class conditioning (EngineBase.stage_classes), else None.
        stages: quantiser dropout of a residual vq bottleneck - None, an int or one int per clip in [1, vq_stages]
        (EngineBase.vq_stage_counts); not None: every clip is quantised with its first n stages (wn_rvq_fwd_n).
        want_probs=False stops at the pre-softmax logits in ws["O"] (the fused training step); encode_only=True behind the pooled
        (and, with a vq bottleneck, quantised) encoding: (None, enc, ws), nothing of the decoder runs."""
        self._check_cond(cond)
        B, Q, T = x.shape
        cls = None if encode_only and classes is None else self.stage_classes(classes, B)      # (the encoder takes no classes)
        nstage = self.vq_stage_counts(stages, B)
        W = T - self.rf + 1
        Le = W // self.pool
        if Le < 1:
            raise RuntimeError("Output size is too small: %d samples of encoding cannot be pooled by %d" % (W, self.pool))
        ws = self._ws.get(B, T)
        self._gen += 1
        ws["gen"], ws["x_in"], ws["Le"], ws["cls"] = self._gen, x, Le, cls
        pair = ws["pair"] = self.pair_ok and B % 2 == 0 and Le <= 32      # decided per workspace shape (B, T fix Le)
        # the forward blocks pair only when that fills the chip (music_amd/engine.py); the backward blocks always
        pair_f = pair and (B // 2) * ((T + 511) // 512) >= 200
        # a one-hot built from integer codes (engine.onehot / the loader) carries them: both causal layers then run on the
        # codes (gather forward, scatter backward), as in music_amd/engine.py
        ws["x_codes"] = self.tagged_codes(x, B, T)
        st = _lib.stream()
        m, pitch, N, CHe, CHd, SP, BwP = self.mode, ws["pitch"], self.N, self.CHe, self.CHd, self.SP, self.BwP
        # the 31 conditioning projections (drawn on the CPU, model1.py:178,216) go to the device FIRST, in one asynchronous copy
        # from pinned memory: as four pageable .to(device) copies behind the encoder they made the host wait for the encoder
        # stack and the decoder start from an empty queue (0.35 ms for this phase at config 4)
        if not self.learned:
            cw, cb, cfw, cfb = self._stage_cond(cond)
        call("wn_pack_weights", ptr(self.flat), ptr(self.pk_idx), ptr(self.pk), self.pk_idx.numel(), m, st)
        fr, lo = self._fr, self.rf - 1
        NONE3 = (None, 0, 0)
        gemm = lambda pack, *a: self._gemm(st, B, m, fr(pack), *a)

        # ---------------- encoder (model1.py:137-156); every x_i and h_i is kept for the backward
        xe = lambda i: self._lay(ws["Xe"], i, CHe, ws)
        he = lambda i: self._lay(ws["He"], i, CHe, ws)
        E = ptr(ws["E"], SLACK)
        eb = CHe * pitch
        causal = lambda name, ch, rows, out: self.causal_fwd(ws, x, self.wt_idx[name], self.wt[name], fr(name), self._bias(name + "_layer"),
                                                             rows, ch, out, st, m)
        self.mark("begin")
        causal("en_causal", CHe, self.Re, xe(0))
        self.mark("en_causal_fwd")
        for i, d in enumerate(self.dil):
            t_lo = self.off[i + 1]
            # h = dilated_conv(relu(x));   x' = dense(relu(h)) + x[tail]
            if pair_f or self.fused_encoder:     # (pair: two clips per 64-row tensor, block-diagonal packs)
                enc_resblock_fwd(fr, i, xe(i), xe(i + 1), he(i), eb, pitch, (self._bias("en_dilation_layer_stack.%d" % i),
                                 self._bias("en_dense_layer_stack.%d" % i)), self.De, self.Re, CHe, d, t_lo, T, B, m, st, pair=pair_f)
                continue
            gemm("en_dil%d" % i, xe(i), xe(i), eb, pitch, self.off[i], T, -d, 0, CHe // 32, CHe // 32, CHe // 16, self.De,
                 he(i), eb, pitch, 0, self._bias("en_dilation_layer_stack.%d" % i), NONE3, NONE3, t_lo, T, 1)
            gemm("en_dense%d" % i, he(i), None, eb, pitch, t_lo, T, 0, 0, CHe // 32, 0, CHe // 16, self.Re,
                 xe(i + 1), eb, pitch, 0, self._bias("en_dense_layer_stack.%d" % i), (xe(i), eb, pitch, t_lo), NONE3, t_lo, T, 1)
        self.mark("enc_stack_fwd")
        gemm("bottleneck", xe(N), None, eb, pitch, lo, T, 0, 0, CHe // 32, 0, BwP // 16, self.Bw,
             E, BwP * pitch, pitch, 0, self._bias("bottleneck_layer"), NONE3, NONE3, lo, T, 0)
        enc = torch.empty(B, self.Bw, Le, dtype=torch.float32, device=self.device)
        call("wn_avgpool", E, BwP * pitch, pitch, lo, self.pool, Le, self.Bw, ptr(enc), self.Bw * Le, Le, B, st)
        if self.vq:                                           # every frame -> its nearest codebook row: the decoder sees q
            enc = self.vq_fwd(ws, enc, st, nstage)
        if encode_only:
            return None, enc, ws

        # ---------------- conditioning tables: en = Conv1d_rand(enc)  (model1.py:178-179, 216-217)
        Dd, Sd = self.Dd, self.Sd
        if self.learned:
            # the learned projections: every table straight in the layout its reader wants, in one launch (wn_cond_proj_fwd) - per
            # clip for a 32-channel or unpaired forward, as clip pairs for the pair blocks (forward if pair_f, backward always)
            empty = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
            tab_c = empty(N, B, 2 * CHd, Le) if not pair_f else None
            tab = empty(N, B // 2, 4 * CHd, Le) if pair else tab_c
            enf = empty(B, Sd, Le)
            self.cond_proj_fwd(enc, tab_c, tab if pair else None, enf, CHd, st, cls)
            ws.update(enc=enc, tab=tab)
        else:
            en = torch.einsum("nck,bkl->nbcl", cw, enc) + cb[:, None, :, None]             # (N, B, 2Dd, Le)
            tab = torch.zeros(N, B, 2 * CHd, Le, dtype=torch.float32, device=self.device)
            tab[:, :, :Dd] = en[:, :, Dd:]                                                 # my rows: filter first
            tab[:, :, CHd:CHd + Dd] = en[:, :, :Dd]
            enf = F.conv1d(enc, cfw, cfb)                                                  # (B, Sd, Le)
            ws.update(enc=enc, tab=tab, cw=cw, cfw=cfw)

        # ---------------- decoder (model1.py:158-225)
        xd = lambda i: self._lay(ws["Xd"], i, CHd, ws)
        causal("de_causal", CHd, self.Rd, xd(0))
        self.mark("bottleneck_cond_de_causal")
        cmodes = []
        for i in range(N):
            L = T - self.off[i + 1]
            cmodes.append((1, L // Le) if L % Le == 0 else (2, 0))
        ws["cmodes"] = cmodes
        cpk = cix = None
        CHp, Bp = (64, B // 2) if pair else (CHd, B)         # pair mode: 64-row tensors of two clips, rows [f: A B | g: A B]
        if not self.learned:
            tab_c = tab                                     # per clip, rows [f | g]: what the 32-channel forward block gathers from
        if pair and not self.learned:
            tab = tab.view(N, Bp, 2, 2, CHd, Le).permute(0, 1, 3, 2, 4, 5).reshape(N, Bp, 4 * CHd, Le).contiguous()
            ws["tab"] = tab
        if Le <= 32 and CHp == 64 and m == _lib.F16X3 and (pair or os.environ.get("WN_AE_COND_MFMA", "1") == "1"):
            # the conditioning bias on the matrix cores: bucket of every sample of every block as bytes (built once per
            # workspace: row i = PAD zeros, bucket(t - t_lo) for t in [t_lo, T), zeros) and, per forward, the tables as
            # packed A fragments ([2CH rows][32 buckets] per block and clip)
            if "cidx" not in ws:
                PADI = _lib.COND_IDX_PAD
                cidx = torch.zeros(N, PADI + T + 64, dtype=torch.uint8, device=self.device)
                for i in range(N):
                    L = T - self.off[i + 1]
                    trr = torch.arange(L, device=self.device)
                    mode_c, q = cmodes[i]
                    cidx[i, PADI:PADI + L] = (torch.clamp(trr // q, max=Le - 1) if mode_c == 1 else trr % Le).to(torch.uint8)
                ws["cidx"] = cidx
                row, k = pack_positions(2 * CHp // 16, 1, False)
                one = np.where(k < Le, row * Le + k, -1).astype(np.int64)                  # one [2CH][Le] table
                base = np.arange(N * Bp, dtype=np.int64)[:, None] * (2 * CHp * Le)
                ws["ctab_idx"] = torch.from_numpy(np.where(one[None, :] >= 0, base + one[None, :], -1).astype(np.int32)
                                                  .reshape(-1)).to(self.device)
                ws["ctab_pk"] = torch.empty(N * Bp * 2 * CHp * 32 * 2, dtype=torch.int16, device=self.device)
            if pair_f or not pair:                        # (the backward blocks read the fp32 table; only a 64-channel forward the pack)
                call("wn_pack_weights", ptr(tab), ptr(ws["ctab_idx"]), ptr(ws["ctab_pk"]), ws["ctab_idx"].numel(), m, st)
                cpk, cix = ws["ctab_pk"], ws["cidx"]
        cpb = 2 * CHp * 32 * 2                          # halfs of one clip's packed table (hi + lo planes)
        tab_f, n_f = (tab, Bp) if pair_f else (tab_c, B)    # the 64-row pair tables, or per clip
        cond_f = lambda i: Cond(ptr(tab_f[i]), tab_f.shape[2] * Le, Le, *cmodes[i], ptr(cpk, i * n_f * cpb) if cpk is not None else None, cpb,
                                ptr(cix[i]) if cix is not None else None)
        # z on the whole valid range: the backward's dWd reads it
        self.decoder.forward(B, T, pitch, ws["Xd"], ws["Z"], True, st, cond=cond_f, pair=pair_f)
        self.mark("dec_stack_fwd")
        bias_s = self.epilogue.skip_bias(ws)
        # final conditioning expanded over time (stretch / tile rule on the length-W sequence)
        ws["cf_mode"] = (1, W // Le) if W % Le == 0 else (2, 0)
        if not self.learned:
            enf = enf.contiguous()
        call("wn_cond_expand", ptr(enf), Sd * Le, Le, Sd, lo, T, ws["cf_mode"][0], Le, max(ws["cf_mode"][1], 1), ptr(ws["C1"], SLACK),
             SP * pitch, pitch, B, st)
        # two per-clip-group chains, the second on the side stream (stack.SkipEpilogue.forward), where the side stream is in use
        self.epilogue.forward(ws, bias_s, st, False, 2 if self.overlap_wgrad else 1)
        probs = None
        if want_probs:
            probs = torch.empty(B * W, Q, dtype=torch.float32, device=self.device)
            call("wn_chunk_softmax256_fwd", ptr(ws["O"]), ptr(probs), B * W, st)
        ws["probs"] = probs
        self.mark("epilogue_fwd")
        return probs, enc, ws

    # ------------------------------------------------------------------ backward
    def _bwd_workspace(self, ws):
        if ws["bwd"] is not None:
            return ws["bwd"]
        B, T, W, pitch, dev, N = ws["B"], ws["T"], ws["W"], ws["pitch"], self.device, self.N
        buf = lambda rows: self.act_buf(B, rows, pitch)
        bw = dict(dO=torch.zeros(B * self.Q * W + PAD_BACK, dtype=torch.float32, device=dev),
                  dR1=buf(self.SP), dU=buf(self.SP), dZ=buf(N * self.CHd), dXd=[buf(self.CHd), buf(self.CHd)],
                  dE=buf(self.BwP), dXe=[buf(self.CHe), buf(self.CHe)],
                  dHe=buf(self.CHe))
        lo = self.rf - 1
        plan = SlabPlan(self.gp_off)
        for name, t_lo, chunk in (("c2", lo, 1024), ("c1", lo, 1024), ("skip", lo, 2048), ("bottleneck", lo, 512),
                                  ("de_causal", 1, 512), ("en_causal", 1, 512)):
            plan.add(name, _lib.wgrad_slabs(t_lo, T, chunk, B), chunk)
        # decoder blocks: the channel-split block kernel (both weight gradients inside the block launch)
        # where it applies, else resblock_bwd + two wgrad launches
        pair = bw["pair"] = ws.get("pair", False)            # both stacks as clip pairs on the 64-channel one-launch blocks
        ms = pair or (self.CHd == 64 and self.mode == _lib.F16X3 and self.mode_b == _lib.BF16X3
                      and os.environ.get("WN_MS_BWD", "1") == "1")
        bw["ms"] = ms
        # ... and the data gradient inside the same launch, as the (P, Q) pair (wn_resblock_bwd_pq), without biases
        # (the conditioning gradient too, as bucket sums on the matrix cores: at most 32 pooled frames - the forward built the
        # bucket bytes then; longer encodings, and WN_AE_COND_MFMA=0, keep wn_resblock_bwd_ms + wn_cond_grad)
        bw["pq"] = pair or (ms and not self.use_bias and os.environ.get("WN_PQ_BWD", "1") == "1" and "cidx" in ws)
        if bw["pq"]:
            bw["PQ"] = [(buf(self.CHd), buf(self.CHd)), (buf(self.CHd), buf(self.CHd))]
        else:
            bw["dfg"] = buf(2 * self.CHd)               # [df;dg] in HBM: only the other block kernels write it
        # encoder blocks: wn_enc_resblock_bwd (dh + both weight gradients in one launch) where it applies
        enc_fused = pair or (self.CHe == 64 and self.mode_b == _lib.BF16X3 and self.fused_encoder)
        bw["enc_fused"] = enc_fused
        # ... and the data gradient inside the same launch, as the (P, Q) pair (wn_enc_resblock_bwd_pq), without biases
        bw["enc_pq"] = pair or (enc_fused and not self.use_bias and os.environ.get("WN_AE_ENC_PQ", "1") == "1")
        if bw["enc_pq"]:
            bw["PQe"] = (bw["PQ"] if bw["pq"] and self.CHe == self.CHd else     # the decoder's pairs are free again by then
                         [(buf(self.CHe), buf(self.CHe)), (buf(self.CHe), buf(self.CHe))])
        Bp, sfx = (B // 2, "2_") if pair else (B, "")         # pair mode: the block-diagonal gradient matrices, B / 2 "clips"
        # one-launch encoder blocks whose dilation is a multiple of 32 hand dx on WHOLE (chain form of wn_enc_resblock_bwd_pq, as
        # wn_resblock_bwd_pq's in music_amd/engine.py): 4 activation tensors per block instead of 6 - the launch is bound by its bytes
        # ... and those with d < 32 too (form 2: adjacent items walked downwards, the Q rows cross from item to item through LDS)
        want_chain = bw["enc_pq"] and os.environ.get("WN_PQ_CHAIN", "1") == "1"
        want_lch = want_chain and os.environ.get("WN_ENC_LCH", "1") == "1"
        bw["enc_chain"] = [(1 if want_chain and _lib.pq_chain_ok(self.off[i + 1], T, Bp, self.dil[i]) else
                            2 if want_lch and self.dil[i] < 32 else 0) for i in range(N)]
        for i in range(N):
            t_lo, ch = self.off[i + 1], bw["enc_chain"][i]
            # (slabs, wn_wgrad's chunk) of the decoder block's and of the encoder block's two gradients, by the kernel that writes them
            de = (_lib.ms_slabs(t_lo, T, Bp), None) if ms else (_lib.wgrad_slabs(t_lo, T, 512, B), 512)
            en = ((_lib.wgrad_slabs(t_lo, T, 512, B), 512) if not enc_fused else
                  (_lib.pq_slabs(t_lo, T, Bp, self.dil[i] if ch == 1 else 32, True), None) if ch else      # chain form: its own slab count
                  (_lib.enc_slabs(t_lo, T, Bp), None))
            plan.add("de_fg%s%d" % (sfx, i), *de)
            plan.add("en_dil%s%d" % (sfx, i), *en)
            plan.add("en_dense%s%d" % (sfx, i), *en)
            if i < N - 1:
                plan.add("de_d%s%d" % (sfx, i), *de)
        # the causal layers' weight gradients from codes (wn_causal_wgrad_codes): their own slab regions, and a second
        # reduction table in which only those two rows differ
        for name in ("de_causal", "en_causal"):
            plan.add_alternative(name, name + "_codes", _lib.causal_codes_slabs(T, B))
        bw.update(plan.finish(dev))
        ws["bwd"] = bw
        return bw

    def loss_and_grad(self, x, target, cond=None, objective=None, classes=None, stages=None, windows=None, window_pos=None,
                      weights=None, ignore_index=None, label_smoothing=0.0):
        """Fused training step body (the autoencoder counterpart of engine.loss_and_grad): forward to the logits, ONE
        kernel for chunk softmax + CrossEntropyLoss on the probabilities (wavenet_autoencoder/train.py:146-160) + both
        backward steps, then the backward.  Returns the loss (0-d device tensor); gradients land in self.flat_grad.
        objective: None = self.objective (EngineBase).  stages: as in forward (the backward then runs wn_rvq_bwd_n / _bwd_stats_n).
        windows / window_pos, weights / ignore_index / label_smoothing: step_nll's, here only because the step tail lives in the shared
        base."""
        return self._throttled(lambda: self._fused_tail(self.forward(x, cond, want_probs=False, classes=classes, stages=stages)[2], target,
                                                       objective=objective, windows=windows, window_pos=window_pos,
                                                       weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing))

    def backward_from_dlogits(self, ws):
        self.backward(ws, None)

    def input_grad(self, ws):
        """Gradient of the last backward w.r.t. the module's INPUT (model1.py:137,158: the input feeds the encoder's and the decoder's causal
        conv): din[q][s] = sum over both layers of  W[r][q][1] dx0[r][s] + W[r][q][0] dx0[r][s + 1],  dx0 living on [1, T)."""
        bw = ws["bwd"]
        if bw is None:
            raise RuntimeError("music_amd: input_grad() needs the backward of this forward to have run")
        parts = [self.causal_input_grad(ws, bw[key][0], ch, self._br(name), self.mode_b)
                 for name, ch, key in (("de_causalT", self.CHd, "dXd"), ("en_causalT", self.CHe, "dXe"))]
        return parts[0].add_(parts[1])

    def backward(self, ws, dprobs):
        """Fills self.flat_grad from d loss / d probabilities (B*W, Q); dprobs None = bw["dO"] already holds
        d loss / d logits (loss_and_grad)."""
        bw = self._bwd_workspace(ws)
        st = _lib.stream()
        # bias gradients (use_bias=True): row sums of the matching output gradient, collected in one small buffer
        # and copied to their flat-parameter positions after the weight gradients were gathered
        if self.use_bias and getattr(self, "_bias_plan", None) is None:
            names = [n for n in self.gathered_param_names if n.endswith(".bias")]
            off, o = {}, 0
            for n in names:
                off[n[:-5]] = o
                o += int(np.prod(self.spec.shape[n]))
            idx = np.concatenate([np.arange(self.spec.off[n], self.spec.off[n] + int(np.prod(self.spec.shape[n]))) for n in names])
            self._bias_plan = (off, torch.from_numpy(idx.astype(np.int64)).to(self.device),
                               torch.zeros(o, dtype=torch.float32, device=self.device))
        if self.use_bias:
            b_off, b_idx, b_grad = self._bias_plan

            def bias_grad(name, a, a_bstride, a_pitch, a_shift, rows, t_lo, t_hi, dst=0):
                call("wn_bias_grad", a, a_bstride, a_pitch, a_shift, rows, t_lo, t_hi, ws["B"], ptr(b_grad, b_off[name] + dst), st)
        else:
            def bias_grad(*a, **k):
                pass
        B, T, W, pitch, Le = ws["B"], ws["T"], ws["W"], ws["pitch"], ws["Le"]
        N, CHe, CHd, SP, BwP = self.N, self.CHe, self.CHd, self.SP, self.BwP
        Dd, Sd, Rd, Re, De, Bw = self.Dd, self.Sd, self.Rd, self.Re, self.De, self.Bw
        mb, lo = self.mode_b, self.rf - 1
        call("wn_pack_weights", ptr(self.flat), ptr(self.pkb_idx), ptr(self.pkb), self.pkb_idx.numel(), mb, st)
        br = self._br
        NONE3 = (None, 0, 0)
        gemm = lambda pack, *a: self._gemm(st, B, mb, br(pack), *a)
        plan = bw["plan"]
        wgrad = lambda name, *args: self.wgrad(bw, B, mb, st, name, *args)
        if dprobs is not None:
            dprobs = dprobs.contiguous()
            call("wn_chunk_softmax256_bwd", ptr(ws["probs"]), ptr(dprobs), ptr(bw["dO"]), B * W, st)
        sb, db, eb = SP * pitch, CHd * pitch, CHe * pitch
        # ---- decoder epilogue (its three weight gradients on the side stream as in music_amd/engine.py: config 4, 1.30 -> ~1.0 ms
        # for this phase); in the fused form connection_1's weight gradient runs on the side stream, the skip convs' on the main
        # stream, and the stack starts behind both
        epi = self.epilogue.begin_backward(ws, bw)
        cmode, cq = ws["cf_mode"]
        d_enf = torch.zeros(B, Sd, Le, dtype=torch.float32, device=self.device)
        self.epilogue.backward(epi, st, os.environ.get("WN_EPI_FUSED_BWD", "1") == "1", after_dh=lambda: call(
            "wn_cond_grad", epi.dH, sb, pitch, Sd, lo, T, cmode, Le, max(cq, 1), ptr(d_enf), Sd * Le, Le, B, st))
        self.mark("ce_epilogue_bwd")
        # ---- decoder stack
        d_tab = torch.zeros(N, B, 2 * CHd, Le, dtype=torch.float32, device=self.device)
        pair = bw["pair"]
        Bp, rows = (B // 2, 4 * CHd) if pair else (B, 2 * CHd)
        if pair:
            d_tab = torch.zeros(N, Bp, 4 * CHd, Le, dtype=torch.float32, device=self.device)     # rows [f: A B | g: A B]
        if bw["pq"] and "cslab" not in bw:
            # per-workgroup bucket sums of every block launch (one region each), added by ONE reduce behind the stack
            import ctypes
            fl = [_lib.load().wn_resblock_bwd_pq_cond_floats(self.off[i + 1], T, Bp) for i in range(N)]
            bw["cs_off"] = (ctypes.c_int64 * N)(*np.concatenate([[0], np.cumsum(fl)[:-1]]).tolist())
            bw["cs_tlo"] = (ctypes.c_int * N)(*[self.off[i + 1] for i in range(N)])
            bw["cslab"] = torch.empty(sum(fl), dtype=torch.float32, device=self.device)

        def cond(i):
            """block i's table; the one-launch block gathers by bucket bytes and leaves bucket sums of [df;dg] in its region of cslab"""
            mode_c, q = ws["cmodes"][i]
            mc = dict(cidx=ptr(ws["cidx"][i]), cslab=ptr(bw["cslab"], bw["cs_off"][i])) if bw["pq"] else {}
            return Cond(ptr(ws["tab"][i]), rows * Le, Le, mode_c, max(q, 1), **mc)

        def dfg_grads(i, dfg, dy, t_lo, s_):
            """behind a block that wrote [df;dg]: the conditioning gradient (sums over each pooled frame's samples) and the bias gradients"""
            mode_c, q = ws["cmodes"][i]
            call("wn_cond_grad", dfg, 2 * CHd * pitch, pitch, 2 * CHd, t_lo, T, mode_c, Le, max(q, 1), ptr(d_tab[i]), 2 * CHd * Le, Le, B, s_)
            if self.use_bias:
                nm = "de_dilation_layer_stack.%d" % (3 * i)
                bias_grad(nm, dfg + 4 * CHd * pitch, 2 * CHd * pitch, pitch, 0, Dd, t_lo, T)          # gate rows = dg
                bias_grad(nm, dfg, 2 * CHd * pitch, pitch, 0, Dd, t_lo, T, dst=Dd)                    # filter rows = df
                if dy is not None:
                    bias_grad("de_dilation_layer_stack.%d" % (3 * i + 1), dy, db, pitch, 0, Rd, t_lo, T)
        self.decoder.backward("pq" if bw["pq"] else "ms" if bw["ms"] else "rw", B, T, pitch, ws["Xd"], ws["Z"], bw, bw["dXd"], st,
                              chain=[False] * N, dfg=[bw["dfg"]] if "dfg" in bw else None, cond=cond, pair=pair, hook=dfg_grads)
        if bw["pq"]:
            call("wn_resblock_bwd_pq_cond_reduce", ptr(bw["cslab"]), bw["cs_off"], bw["cs_tlo"], N, T, Bp, Le, ptr(d_tab),
                 Bp * rows * Le, rows * Le, Le, st)
            if pair and not self.learned:               # back to per-clip tables, rows [f | g]
                d_tab = d_tab.view(N, Bp, 2, 2, CHd, Le).permute(0, 1, 3, 2, 4, 5).reshape(N, B, 2 * CHd, Le)
        self.mark("dec_stack_bwd")
        x_codes = self.codes_for_backward(ws)
        causal_wgrad = lambda name, dx0, ch: self.causal_wgrad(ws, bw, x_codes, name, dx0, ch, st, mb)
        causal_wgrad("de_causal", ptr(bw["dXd"][0], SLACK), CHd)
        bias_grad("de_causal_layer", ptr(bw["dXd"][0], SLACK), db, pitch, 0, Rd, 1, T)
        # ---- conditioning: en_i = cw_i enc + b (rows in the reference order: gate first), enf = cfw enc + b
        if self.learned:
            # ... and they are parameters: d enc, dW and db (into flat_grad's tail) straight from the block tables' layout
            d_enc = torch.empty(B, Bw, Le, dtype=torch.float32, device=self.device)
            self.cond_proj_bwd(d_tab, pair, d_enf, ws["enc"], d_enc, CHd, st, ws["cls"])
            if self.vq:                                       # straight through to e, + the commitment term; the codebook's gradient
                self.vq_bwd(ws, d_enc, st)
        else:
            d_en = torch.cat([d_tab[:, :, CHd:CHd + Dd], d_tab[:, :, :Dd]], 2)            # (N,B,2Dd,Le) reference row order
            d_enc = torch.einsum("nck,nbcl->bkl", ws["cw"], d_en) + torch.einsum("ck,bcl->bkl", ws["cfw"][:, :, 0], d_enf)
            d_enc = d_enc.contiguous()
        # ---- encoder: avgpool -> bottleneck -> N blocks -> causal
        dE = ptr(bw["dE"], SLACK)
        call("wn_avgpool_bwd", ptr(d_enc), Bw * Le, Le, lo, self.pool, Le, Bw, dE, BwP * pitch, pitch, T, B, st)
        xe = lambda i: self._lay(ws["Xe"], i, CHe, ws)
        he = lambda i: self._lay(ws["He"], i, CHe, ws)
        wgrad("bottleneck", dE, BwP * pitch, pitch, 0, pitch, xe(N), None, eb, pitch, 0, 0, pitch, CHe // 16, BwP // 16, 0, CHe, lo, T)
        bias_grad("bottleneck_layer", dE, BwP * pitch, pitch, 0, Bw, lo, T)
        dxe = [ptr(t, SLACK) for t in bw["dXe"]]
        dHe = ptr(bw["dHe"], SLACK)
        gemm("bottleneckT", dE, None, BwP * pitch, pitch, lo, T, 0, 0, BwP // 32, 0, CHe // 16, Re, dxe[N % 2], eb, pitch, 0, None,
             NONE3, NONE3, lo, T, 0)
        self.mark("de_causal_cond_bottleneck_bwd")
        for i in range(N - 1, -1, -1):
            d, t_lo = self.dil[i], self.off[i + 1]
            y_lo = lo if i == N - 1 else t_lo                     # the top gradient only exists on the crop
            dy = dxe[(i + 1) % 2]
            if bw["enc_pq"]:
                # the whole backward of the block in one launch; dx travels as the unshifted pair (P, Q)
                hand, chain = hand_over(i, N, bw["enc_chain"], bw["PQe"], bw["dXe"][0], self.dil, self.off), bw["enc_chain"][i]
                q_out = ptr(bw["PQe"][i % 2][1], SLACK)
                if i == N - 1:
                    hand = (dy, None, 0, y_lo, hand[4])           # the top block takes the bottleneck's data gradient, whole, on the crop
                enc_resblock_bwd_pq(br, plan, bw["slab"], i, xe(i), hand, he(i), q_out, eb, pitch, CHe, d, t_lo, T, chain, B, mb, st, pair=pair)
                if i == 0 and not chain:
                    call("wn_shift_add", hand[4], q_out, dxe[0], eb, pitch, CHe, d, t_lo, self.off[0], T, B, st)
                continue
            if bw["enc_fused"]:
                # dh, dW1 = sum dy relu(h)^T and dWdil = sum dh [relu x(t-d) | relu x(t)]^T in one launch
                call("wn_enc_resblock_bwd", xe(i), dy, he(i), dHe, eb, eb, eb, pitch, br("en_denseT%d" % i), CHe, d, t_lo, T, y_lo,
                     ptr(bw["slab"], plan["en_dil%d" % i].so), ptr(bw["slab"], plan["en_dense%d" % i].so), B, mb, st)
                bias_grad("en_dense_layer_stack.%d" % i, dy, eb, pitch, 0, Re, y_lo, T)
                bias_grad("en_dilation_layer_stack.%d" % i, dHe, eb, pitch, 0, De, t_lo, T)
                gemm("en_dilT%d" % i, dHe, dHe, eb, pitch, t_lo, T, 0, d, CHe // 32, CHe // 32, CHe // 16, Re, dxe[i % 2], eb, pitch, 0,
                     None, (dy, eb, pitch, y_lo), (xe(i), eb, pitch), self.off[i], T, 0)
                continue
            # dh = (W1^T dy) * [h > 0];  dW1 = sum dy relu(h)^T
            wgrad("en_dense%d" % i, dy, eb, pitch, 0, pitch, he(i), None, eb, pitch, 0, 0, pitch, CHe // 16, CHe // 16, 1, CHe, y_lo, T)
            bias_grad("en_dense_layer_stack.%d" % i, dy, eb, pitch, 0, Re, y_lo, T)
            gemm("en_denseT%d" % i, dy, None, eb, pitch, y_lo, T, 0, 0, CHe // 32, 0, CHe // 16, De, dHe, eb, pitch, 0, None, NONE3,
                 (he(i), eb, pitch), t_lo, T, 0)
            # dWdil = sum dh [relu(x)(t-d) | relu(x)(t)]^T
            wgrad("en_dil%d" % i, dHe, eb, pitch, 0, pitch, xe(i), xe(i), eb, pitch, -d, 0, pitch, CHe // 16, CHe // 16, 1, 2 * CHe, t_lo, T)
            bias_grad("en_dilation_layer_stack.%d" % i, dHe, eb, pitch, 0, De, t_lo, T)
            # dx_i[t] = [x_i > 0] (Wdil1^T dh[t] + Wdil0^T dh[t+d]) + dy[t]
            gemm("en_dilT%d" % i, dHe, dHe, eb, pitch, t_lo, T, 0, d, CHe // 32, CHe // 32, CHe // 16, Re, dxe[i % 2], eb, pitch, 0,
                 None, (dy, eb, pitch, y_lo), (xe(i), eb, pitch), self.off[i], T, 0)
        self.mark("enc_stack_bwd")
        causal_wgrad("en_causal", dxe[0], CHe)
        bias_grad("en_causal_layer", dxe[0], eb, pitch, 0, Re, 1, T)
        self.join_side()
        self.reduce_and_gather(bw, x_codes is not None, st)
        if self.use_bias:
            self.flat_grad.index_copy_(0, b_idx, b_grad)
        self.mark("en_causal_slab_reduce")


BOTTLENECKS = ("continuous", "vq")       # the pooled encoding as it is, or every frame replaced by its nearest codebook row (VQ-VAE)
VQ_UPDATES = ("gradient", "ema")         # what trains the codebook: its loss term's gradient, or the running mean of its frames (+ restarts)
CONDITIONING = ("random", "learned")     # the decoder's conditioning projections: drawn afresh per forward (the reference), or parameters


class _AutoencoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, grad_on, wave_sample, cond, classes, stages, *params):
        eng = net._engine_for(wave_sample.device)
        x = wave_sample.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        else:
            tag = getattr(wave_sample, "_wn_codes", None)        # one-hot built from codes (see _AutoencoderEngine.forward)
            if tag is not None and wave_sample._version == tag[2]:
                x._wn_codes = (tag[0], tag[1], x._version, tag[3])
        probs, enc, ws = eng.forward(x, cond, classes=classes) if stages is None else eng.forward(x, cond, classes=classes, stages=stages)
        net.last_encoding = enc
        ctx.eng, ctx.ws, ctx.gen = eng, ws, ws["gen"]
        ctx.loss_hook = net._last_hook = _losshook.make(eng, ws, grad_on)
        ctx.hold = WorkspaceHold(ws) if (grad_on and any(ctx.needs_input_grad)) else None      # see music_amd/model.py
        if eng.vq:
            # the quantised bottleneck: q went to the decoder (net.last_encoding); vq_loss = (1 + beta) mse is a SECOND output of this
            # node - left out of the user's loss, its upstream gradient is None and neither the codebook nor the commitment term gets any
            net.last_encoding_pre, net.vq_codes, net.last_vq = ws["enc_pre"], eng.vq_codes_of(ws), eng.last_vq
            ctx.set_materialize_grads(False)
            return probs.detach(), eng.last_vq.vq_loss
        return probs.detach()            # (an alias: the workspace's own reference must not carry the autograd node)

    @staticmethod
    def backward(ctx, dprobs, dvq=None):
        eng, ws = ctx.eng, ctx.ws
        if ws.get("gen") != ctx.gen:
            raise RuntimeError("music_amd.wavenet_autoencoder: activations were overwritten by a later forward")
        if eng.vq:
            # the upstream scalar on vq_loss goes to wn_vq_bwd as a host float (one read-back, only where vq_loss is in the loss)
            ws["vq_g"] = 0.0 if dvq is None else float(dvq)
            if dprobs is None:                                  # vq_loss alone was differentiated
                dprobs = torch.zeros(ws["B"] * ws["W"], eng.Q, dtype=torch.float32, device=eng.device)
        if not _losshook.backward(ctx.loss_hook, eng, ws, dprobs):          # (the loss ran fused: see _losshook.py)
            eng.backward(ws, dprobs)
        if ctx.hold is not None:
            ctx.hold.release()
        g = eng.flat_grad.clone()
        grads = []
        for name in eng.param_names:
            o, shp = eng.spec.off[name], eng.spec.shape[name]
            grads.append(g[o:o + int(np.prod(shp))].view(shp))
        din = eng.input_grad(ws) if ctx.needs_input_grad[2] else None       # (the reference's two causal nn.Conv1d give it, model1.py:137,158)
        return (None, None, din, None, None, None) + tuple(grads)


class wavenet_autoencoder(nn.Module):

    def __init__(self, filter_width, quantization_channel, dilations, en_residual_channel, en_dilation_channel,
                 en_bottleneck_width, en_pool_kernel_size, de_residual_channel, de_dilation_channel,
                 de_skip_channel, use_bias, conditioning="random", bottleneck="continuous", vq_codes=512, vq_beta=0.25,
                 vq_update="gradient", vq_decay=0.99, vq_eps=1e-5, vq_restart=0.0, global_classes=0, global_channels=0, vq_stages=1,
                 vq_stage_dropout=0.0):
        super(wavenet_autoencoder, self).__init__()
        if isinstance(vq_stage_dropout, bool) or not isinstance(vq_stage_dropout, (int, float)) or not 0.0 <= vq_stage_dropout <= 1.0:
            raise ValueError("music_amd.wavenet_autoencoder: vq_stage_dropout must be a number in [0, 1], not %r" % (vq_stage_dropout,))
        if vq_stage_dropout > 0 and not (isinstance(vq_stages, int) and not isinstance(vq_stages, bool) and vq_stages > 1):
            raise ValueError("music_amd.wavenet_autoencoder: vq_stage_dropout > 0 requires vq_stages > 1 (there is no stage to drop)")
        if isinstance(vq_stages, bool) or not isinstance(vq_stages, int) or not 1 <= vq_stages <= _lib.RVQ_MAX_STAGES:
            raise ValueError("music_amd.wavenet_autoencoder: vq_stages must be an integer in [1, %d], not %r"
                             % (_lib.RVQ_MAX_STAGES, vq_stages))
        if vq_stages > 1 and bottleneck != "vq":
            raise ValueError('music_amd.wavenet_autoencoder: vq_stages > 1 requires bottleneck="vq"')
        for key, val in (("global_classes", global_classes), ("global_channels", global_channels)):
            if isinstance(val, bool) or not isinstance(val, int) or val < 0:
                raise ValueError("music_amd.wavenet_autoencoder: %s must be an integer >= 0, not %r" % (key, val))
        if (global_classes > 0) != (global_channels > 0):
            raise ValueError("music_amd.wavenet_autoencoder: global_classes and global_channels must both be 0 (off) or both >= 1, "
                             "not %r and %r" % (global_classes, global_channels))
        if global_channels > _lib.GCOND_MAX_CHANNELS:
            raise ValueError("music_amd.wavenet_autoencoder: global_channels must lie in [1, %d], not %r"
                             % (_lib.GCOND_MAX_CHANNELS, global_channels))
        if global_classes > 0 and conditioning != "learned":
            raise ValueError('music_amd.wavenet_autoencoder: global_classes > 0 requires conditioning="learned" (the class term is one '
                             'more term of the learned projections\' tables)')
        if conditioning not in CONDITIONING:
            raise ValueError("music_amd.wavenet_autoencoder: conditioning must be one of %s, not %r"
                             % (", ".join('"%s"' % c for c in CONDITIONING), conditioning))
        if bottleneck not in BOTTLENECKS:
            raise ValueError("music_amd.wavenet_autoencoder: bottleneck must be one of %s, not %r"
                             % (", ".join('"%s"' % c for c in BOTTLENECKS), bottleneck))
        if bottleneck == "vq":
            if conditioning != "learned":
                raise ValueError('music_amd.wavenet_autoencoder: bottleneck="vq" requires conditioning="learned" (with projections drawn '
                                 'afresh in every forward a codebook means nothing)')
            if not 2 <= int(vq_codes) <= _lib.VQ_MAX_CODES:
                raise ValueError("music_amd.wavenet_autoencoder: vq_codes must lie in [2, %d], not %r" % (_lib.VQ_MAX_CODES, vq_codes))
            if not 1 <= int(en_bottleneck_width) <= _lib.VQ_MAX_WIDTH:
                raise ValueError('music_amd.wavenet_autoencoder: bottleneck="vq" needs en_bottleneck_width in [1, %d], not %r'
                                 % (_lib.VQ_MAX_WIDTH, en_bottleneck_width))
            if not float(vq_beta) >= 0.0:
                raise ValueError("music_amd.wavenet_autoencoder: vq_beta must be >= 0, not %r" % (vq_beta,))
        if vq_update not in VQ_UPDATES:
            raise ValueError("music_amd.wavenet_autoencoder: vq_update must be one of %s, not %r"
                             % (", ".join('"%s"' % c for c in VQ_UPDATES), vq_update))
        if vq_update == "ema":
            if bottleneck != "vq":
                raise ValueError('music_amd.wavenet_autoencoder: vq_update="ema" requires bottleneck="vq"')
            if not 0.0 < float(vq_decay) < 1.0:
                raise ValueError("music_amd.wavenet_autoencoder: vq_decay must lie in (0, 1), not %r" % (vq_decay,))
            if not float(vq_eps) >= 0.0:
                raise ValueError("music_amd.wavenet_autoencoder: vq_eps must be >= 0, not %r" % (vq_eps,))
            if not float(vq_restart) >= 0.0:
                raise ValueError("music_amd.wavenet_autoencoder: vq_restart must be >= 0, not %r" % (vq_restart,))
        self.conditioning = conditioning
        self.bottleneck, self.vq_num_codes, self.vq_beta = bottleneck, int(vq_codes), float(vq_beta)
        self.vq_stages = vq_stages       # residual quantisation: stage s quantises what the stages before it left over, with rows [sK, (s+1)K)
        # quantiser dropout (music_amd/vq_dropout.py): in training mode a share p of the clips draws its stage count from 1 .. S.  No
        # parameter, no buffer: state_dict is unchanged.  The draw hashes (vq_dropout_seed, the module's call counter, the clip's index);
        # a training loop that knows its global step and clip offset passes stages= itself (ae_train)
        self.vq_stage_dropout = float(vq_stage_dropout)
        self.vq_dropout_seed = 0
        self.vq_dropout_calls = 0
        self.vq_update, self.vq_decay, self.vq_eps, self.vq_restart = vq_update, float(vq_decay), float(vq_eps), float(vq_restart)
        self.global_classes, self.global_channels = global_classes, global_channels
        self.filter_width = filter_width
        self.quantization_channel = quantization_channel
        self.dilations = dilations
        self.en_residual_channel = en_residual_channel
        self.en_dilation_channel = en_dilation_channel
        self.en_bottleneck_width = en_bottleneck_width
        self.en_pool_kernel_size = en_pool_kernel_size
        self.de_residual_channel = de_residual_channel
        self.de_dilation_channel = de_dilation_channel
        self.de_skip_channel = de_skip_channel
        self.use_bias = use_bias
        self.receptive_field = self._calc_receptive_field()
        self.softmax = nn.Softmax(dim=1)
        # construction (= RNG draw) order of model1.py:55-58: encoder pairs, decoder triples, the
        # three input/bottleneck convs, the two output convs
        self.en_dilation_layer_stack = nn.ModuleList()
        self.en_dense_layer_stack = nn.ModuleList()
        for d in dilations:
            self.en_dilation_layer_stack.append(nn.Conv1d(en_residual_channel, en_dilation_channel, filter_width,
                                                          dilation=d, bias=use_bias))
            self.en_dense_layer_stack.append(nn.Conv1d(en_dilation_channel, en_residual_channel, 1, bias=use_bias))
        self.de_dilation_layer_stack = nn.ModuleList()
        for d in dilations:
            self.de_dilation_layer_stack.extend([
                nn.Conv1d(de_residual_channel, 2 * de_dilation_channel, filter_width, dilation=d, bias=use_bias),
                nn.Conv1d(de_dilation_channel, de_residual_channel, kernel_size=1, dilation=d, bias=use_bias),
                nn.Conv1d(de_dilation_channel, de_skip_channel, dilation=d, kernel_size=1, bias=use_bias)])
        self.en_causal_layer = nn.Conv1d(quantization_channel, en_residual_channel, filter_width, bias=use_bias)
        self.bottleneck_layer = nn.Conv1d(en_residual_channel, en_bottleneck_width, 1, bias=use_bias)
        self.de_causal_layer = nn.Conv1d(quantization_channel, de_residual_channel, filter_width, bias=use_bias)
        self.connection_1 = nn.Conv1d(de_skip_channel, de_skip_channel, 1, bias=use_bias)
        self.connection_2 = nn.Conv1d(de_skip_channel, quantization_channel, 1, bias=use_bias)
        self._engine = None
        self.last_encoding = None
        # nn.CrossEntropyLoss()(net(x), target) with its default arguments runs fused (music_amd/_losshook.py); False: torch's own
        self.fuse_loss = True
        self._last_hook = None
        # (forward, backward) arithmetic of the matrix-core products, as on `wavenet`; ("bf16x3", "bf16x3") gives the forward float32's exponent range
        # (an un-normalised ReLU encoder can leave f16's: DESIGN section 5) at 2^-17 instead of 2^-22 per product
        self.precision = ("f16x3", "bf16x3")
        if conditioning == "learned":
            # the N + 1 conditioning projections as parameters (the reference draws them afresh in every forward): registered
            # AFTER every reference submodule, so a seed gives the reference's parameters the same values in both modes and these sit at
            # the end of the flat buffer; always with a bias, rows in the reference's order (gate first), like the drawn convs
            self.de_cond_layer_stack = nn.ModuleList(nn.Conv1d(en_bottleneck_width, 2 * de_dilation_channel, 1) for _ in dilations)
            self.connection_cond = nn.Conv1d(en_bottleneck_width, de_skip_channel, 1)
        # after a forward of a vq model: vq_loss (0-d, attached to autograd: add it to the loss), vq_codes (B, Le) int64 - (B, S, Le) with
        # vq_stages = S > 1 -, last_encoding = q, last_encoding_pre = e, last_vq = the engine's VqStats
        self.vq_loss = self.vq_codes = self.last_encoding_pre = self.last_vq = None
        if bottleneck == "vq":
            # the codebook (K, Bw), registered BEHIND the learned projections: a seed gives every earlier parameter the continuous
            # model's values, and it is the last block of the flat buffer; uniform(-1/K, 1/K) (van den Oord et al. 2017)
            # (S K, Bw) with vq_stages = S: stage s owns rows [sK, (s+1)K), every row uniform(-1/K, 1/K)
            self.vq_codebook = nn.Embedding(vq_stages * self.vq_num_codes, en_bottleneck_width)
            with torch.no_grad():
                self.vq_codebook.weight.uniform_(-1.0 / self.vq_num_codes, 1.0 / self.vq_num_codes)
            if vq_update == "ema":
                # the running usage N (K) and running sums m (K, Bw) of wn_vq_ema_update, [N | m] in one vector; m / N is the
                # codebook.  A buffer: it travels with state_dict() (as the LAST key) and the module's moves, no optimizer sees it.
                # One [N | m] block per stage
                self.register_buffer("vq_ema_state", torch.empty(vq_stages * self.vq_num_codes * (en_bottleneck_width + 1)))
                self.reset_vq_ema_state()
        if global_classes > 0:
            # global class conditioning (VQ-VAE's speaker id, NSynth's instrument): en_i[b] = W_i enc[b] + b_i + G_i emb[cls[b]].  The
            # G_i (gate rows first, like de_cond_layer_stack), G_f and the embedding are registered - and drawn - BEHIND everything the
            # model has without them, the codebook included: a seed gives every earlier parameter the same value and flat offset
            self.de_gcond_layer_stack = nn.ModuleList(nn.Conv1d(global_channels, 2 * de_dilation_channel, 1, bias=False) for _ in dilations)
            self.connection_gcond = nn.Conv1d(global_channels, de_skip_channel, 1, bias=False)
            self.global_embedding = nn.Embedding(global_classes, global_channels)

    def __setstate__(self, state):
        super(wavenet_autoencoder, self).__setstate__(state)
        self.__dict__.setdefault("conditioning", "random")       # (a module pickled before the attribute existed)
        self.__dict__.setdefault("bottleneck", "continuous")
        self.__dict__.setdefault("vq_stages", 1)
        for k, v in (("vq_stage_dropout", 0.0), ("vq_dropout_seed", 0), ("vq_dropout_calls", 0)):
            self.__dict__.setdefault(k, v)
        for k, v in (("vq_update", "gradient"), ("vq_decay", 0.99), ("vq_eps", 1e-5), ("vq_restart", 0.0)):
            self.__dict__.setdefault(k, v)
        for k in ("vq_loss", "vq_codes", "last_encoding_pre", "last_vq"):
            self.__dict__.setdefault(k, None)
        self.__dict__.setdefault("global_classes", 0)
        self.__dict__.setdefault("global_channels", 0)

    def init_codebook(self, encodings, seed=0):
        """Data-dependent initialisation: K frames of `encodings` (B, Bw, Le) - pre-quantisation encodings, net.last_encoding_pre -
        become the codebook, drawn without replacement by a generator seeded with `seed`; fewer than K frames are cycled through.
        With vq_stages > 1 the stages are filled in order: stage s draws its rows (generator `seed` + s) from the residuals that the
        stages before it leave on these frames (nearest row) - of the frames no earlier stage took: a frame that BECAME a row leaves
        nothing over, and all such frames share their later residuals, rows that would tie.  Give at least S K frames."""
        if getattr(self, "bottleneck", "continuous") != "vq":
            raise ValueError('music_amd.wavenet_autoencoder: init_codebook needs bottleneck="vq"')
        w = self.vq_codebook.weight
        frames = encodings.detach().to(torch.float32).permute(0, 2, 1).reshape(-1, encodings.size(1))
        if frames.size(1) != w.size(1) or frames.size(0) < 1:
            raise ValueError("music_amd.wavenet_autoencoder: init_codebook wants (B, %d, Le) encodings, got %s"
                             % (w.size(1), tuple(encodings.shape)))
        K = self.vq_num_codes
        fresh = torch.ones(frames.size(0), dtype=torch.bool)               # frames no stage has taken as a row yet
        with torch.no_grad():
            for s in range(getattr(self, "vq_stages", 1)):
                gen = torch.Generator().manual_seed(int(seed) + s)
                pool = fresh.nonzero()[:, 0] if bool(fresh.any()) else torch.arange(frames.size(0))
                order = torch.randperm(pool.numel(), generator=gen)
                pick = pool[order[torch.arange(K) % pool.numel()]]
                fresh[pick] = False
                rows = frames[pick.to(frames.device)]
                w[s * K:(s + 1) * K].copy_(rows.to(w.device))            # (in place: the parameter may be a view of the flat buffer)
                if s + 1 < getattr(self, "vq_stages", 1):
                    frames = frames - rows[torch.cdist(frames, rows).argmin(dim=1)]
        self.reset_vq_ema_state()

    def reset_vq_ema_state(self):
        """vq_update="ema": the running state back to [1 | codebook] - usage 1 per code, sums = the rows as they are now (after the
        codebook was set by hand, init_codebook does it itself).  In place; nothing to do in gradient mode."""
        if getattr(self, "vq_update", "gradient") != "ema":
            return
        K, S = self.vq_num_codes, getattr(self, "vq_stages", 1)
        with torch.no_grad():
            state = self.vq_ema_state.view(S, -1)                      # per stage: [N | m]
            state[:, :K].fill_(1.0)
            state[:, K:].copy_(self.vq_codebook.weight.detach().reshape(S, -1))

    def state_dict(self, *args, **kwargs):
        sd = super(wavenet_autoencoder, self).state_dict(*args, **kwargs)
        key = kwargs.get("prefix", "") + "vq_ema_state"       # the module's own buffer is listed first: it goes BEHIND everything else
        if key in sd:
            sd.move_to_end(key)
        return sd

    def _cond_modules(self):
        return list(self.de_cond_layer_stack) + [self.connection_cond]

    def conditioning_projections(self):
        """The N + 1 (weight (C, Bw, 1), bias (C,)) pairs a forward conditions the decoder on: the (detached) parameters with learned
        conditioning - no RNG is consumed -, a fresh draw from the global RNG (_draw_conditioning) with random conditioning."""
        if getattr(self, "conditioning", "random") == "learned":
            return [(m.weight.detach(), m.bias.detach()) for m in self._cond_modules()]
        return self._draw_conditioning()

    def global_projections(self):
        """The N + 1 (detached) matrices G_i (2 Dd, E) - rows in the reference's order, gate first - and G_f (Sd, E) that project a
        clip's global vector into the conditioning tables."""
        self._need_global("global_projections")
        return [m.weight.detach()[:, :, 0] for m in list(self.de_gcond_layer_stack) + [self.connection_gcond]]

    def global_vectors(self, classes):
        """The (detached) embedding rows (B, E) of `classes`, B integers in [0, global_classes): what decoding takes as
        ``global_vectors=`` (a mix of two rows morphs between their classes)."""
        self._need_global("global_vectors")
        w = self.global_embedding.weight.detach()
        cls = torch.as_tensor(classes, dtype=torch.int64).reshape(-1)
        if cls.numel() and not (0 <= int(cls.min()) and int(cls.max()) < self.global_classes):
            raise ValueError("music_amd.wavenet_autoencoder: a class lies outside [0, %d) (global_classes)" % self.global_classes)
        return w[cls.to(w.device)]

    def _need_global(self, what):
        if not getattr(self, "global_classes", 0):
            raise ValueError("music_amd.wavenet_autoencoder: %s needs global_classes > 0" % what)

    def engine_cond(self, cond=None):
        """What the engine's forward / loss_and_grad take as `cond`: None with learned conditioning (a given list is refused there),
        else `cond` or a fresh draw."""
        if getattr(self, "conditioning", "random") == "learned":
            if cond is not None:
                raise ValueError('music_amd.wavenet_autoencoder: conditioning="learned": the projections are parameters, cond must be None')
            return None
        return cond if cond is not None else self._draw_conditioning()

    def load_state_dict(self, state_dict, *args, **kwargs):
        # a checkpoint of the other conditioning mode: refused whole, by name, before anything is copied
        has = any(k.startswith(("de_cond_layer_stack.", "connection_cond.")) for k in state_dict.keys())
        mine = getattr(self, "conditioning", "random")
        if has != (mine == "learned"):
            raise RuntimeError('music_amd.wavenet_autoencoder: the checkpoint was saved with conditioning="%s" but this model was built '
                               'with conditioning="%s" (the "conditioning" key of model_params.json); nothing was loaded'
                               % ("learned" if has else "random", mine))
        has_vq = any(k.startswith("vq_codebook.") for k in state_dict.keys())
        mine_vq = getattr(self, "bottleneck", "continuous")
        if has_vq != (mine_vq == "vq"):
            raise RuntimeError('music_amd.wavenet_autoencoder: the checkpoint was saved with bottleneck="%s" but this model was built '
                               'with bottleneck="%s" (the "bottleneck" key of model_params.json); nothing was loaded'
                               % ("vq" if has_vq else "continuous", mine_vq))
        has_ema = "vq_ema_state" in state_dict.keys()
        mine_ema = getattr(self, "vq_update", "gradient")
        if has_ema != (mine_ema == "ema"):
            raise RuntimeError('music_amd.wavenet_autoencoder: the checkpoint was saved with vq_update="%s" but this model was built '
                               'with vq_update="%s" (the "vq_update" key of model_params.json); nothing was loaded'
                               % ("ema" if has_ema else "gradient", mine_ema))
        if mine_vq == "vq":
            cb = state_dict.get("vq_codebook.weight", state_dict.get("module.vq_codebook.weight"))
            rows = cb.shape[0] if cb is not None and cb.dim() == 2 else 0
            mine_s = getattr(self, "vq_stages", 1)
            if rows != mine_s * self.vq_num_codes and rows % self.vq_num_codes == 0:
                raise RuntimeError("music_amd.wavenet_autoencoder: the checkpoint was saved with vq_stages=%d but this model was built "
                                   'with vq_stages=%d (the "vq_stages" key of model_params.json); nothing was loaded'
                                   % (rows // self.vq_num_codes, mine_s))
        emb = state_dict.get("global_embedding.weight", state_dict.get("module.global_embedding.weight"))
        saved = tuple(emb.shape) if emb is not None and emb.dim() == 2 else (0, 0)
        mine_g = (getattr(self, "global_classes", 0), getattr(self, "global_channels", 0))
        if saved != mine_g:
            raise RuntimeError("music_amd.wavenet_autoencoder: the checkpoint was saved with global_classes=%d, global_channels=%d but "
                               "this model was built with global_classes=%d, global_channels=%d (the keys of model_params.json); "
                               "nothing was loaded" % (saved + mine_g))
        return super(wavenet_autoencoder, self).load_state_dict(state_dict, *args, **kwargs)

    def __getstate__(self):
        # copy.deepcopy / pickle / torch.save(module): the engine (HIP streams, workspaces, ctypes plans) stays behind and is rebuilt
        # on the copy's first forward; the parameters travel as tensors
        state = self.__dict__.copy()
        state["_engine"] = None
        state["_last_hook"] = None
        state["vq_loss"] = state["last_vq"] = None           # (an autograd output and the engine's buffers of the last forward)
        return state

    def _calc_receptive_field(self):
        return (self.filter_width - 1) * (sum(self.dilations) + 1) + 1

    def _draw_conditioning(self):
        """The 31 per-forward conditioning convs, drawn on the CPU from the global RNG in the
        reference's order (model1.py:178 per layer, :216 final)."""
        # nn.Conv1d(Bw, C, 1).reset_parameters() without the module around it: the same two uniform_ draws per conv, in the same
        # order, with the bounds computed as torch.nn.init does (kaiming_uniform_(a = sqrt(5)) on the weight, then
        # U(-1/sqrt(fan_in), 1/sqrt(fan_in)) on the bias) - bit-identical tensors (tests/test_host_logic.py) at a fraction of the
        # Python objects (41 modules per forward otherwise)
        n = len(self.dilations)
        fan_in = self.en_bottleneck_width                      # kernel size 1
        gain = math.sqrt(2.0 / (1 + math.sqrt(5) ** 2))
        bound_w = math.sqrt(3.0) * (gain / math.sqrt(fan_in))
        bound_b = 1 / math.sqrt(fan_in)
        cond = []
        for i in range(n + 1):
            c_out = 2 * self.de_dilation_channel if i < n else self.de_skip_channel
            w = torch.empty(c_out, fan_in, 1).uniform_(-bound_w, bound_w)
            b = torch.empty(c_out).uniform_(-bound_b, bound_b)
            cond.append((w, b))
        return cond

    def _engine_for(self, device):
        if device.type != "cuda":
            raise RuntimeError("music_amd.wavenet_autoencoder runs on an MI355X (ROCm) device only; there is no CPU path")
        if not hasattr(self, "precision"):                   # (a module pickled before the attribute existed)
            self.precision = ("f16x3", "bf16x3")
        eng = self._engine
        p0 = next(self.parameters())
        if eng is None or eng.device != device or p0.data_ptr() != eng.flat.data_ptr() or getattr(eng, "mode_names", None) != tuple(self.precision):
            if any(p.device != device for p in self.parameters()):
                raise RuntimeError("music_amd.wavenet_autoencoder: parameters and input are on different devices")
            if any(p.dtype != torch.float32 for p in self.parameters()):
                raise TypeError("music_amd.wavenet_autoencoder: parameters must be float32 (got %s)"
                                % next(p.dtype for p in self.parameters() if p.dtype != torch.float32))
            # the specialised kernels cover filter_width 2, 256 quantisation channels and up to 64 residual / dilation channels on
            # both sides (what the reference ships and BASELINE.json names); any other constructor argument takes the general plan
            fast = (self.filter_width == 2 and self.quantization_channel == 256 and
                    max(self.en_residual_channel, self.en_dilation_channel, self.de_residual_channel, self.de_dilation_channel) <= 64)
            if fast:
                eng = _AutoencoderEngine(self, device, mode=self.precision[0], mode_bwd=self.precision[1])
            else:
                try:
                    from .ae_generic import GenericAutoencoderEngine
                except ImportError:
                    from music_amd.ae_generic import GenericAutoencoderEngine
                eng = GenericAutoencoderEngine(self, device, mode=self.precision[0], mode_bwd=self.precision[1])
            eng.mode_names = tuple(self.precision)
            self._engine = eng
        return eng

    def draw_stages(self, batch_size, step=None, first_clip=0):
        """The stage counts quantiser dropout gives `batch_size` clips (music_amd/vq_dropout.py: draw_stages with this module's
        vq_dropout_seed and vq_stage_dropout), or None where it is off.  step=None: the module's own call counter, which then advances."""
        p = getattr(self, "vq_stage_dropout", 0.0)
        if not p > 0:
            return None
        if step is None:
            step = self.vq_dropout_calls
            self.vq_dropout_calls += 1
        return vq_dropout.draw_stages(getattr(self, "vq_dropout_seed", 0), step, first_clip, batch_size, self.vq_stages, p)

    def forward(self, wave_sample, classes=None, stages=None):
        """stages: quantiser dropout of a residual vq bottleneck - None, an int n (every clip is quantised with its first n stages) or
        one int per clip, each in [1, vq_stages].  None in training mode with vq_stage_dropout > 0: the module draws them (draw_stages);
        None otherwise, eval mode included: all stages."""
        batch_size, original_channels, seq_len = wave_sample.size()
        output_width = seq_len - self.receptive_field + 1
        if output_width <= 0:
            raise ValueError("wave sample not long enough")
        if (classes is None) == bool(getattr(self, "global_classes", 0)):      # (before the engine is built and anything is drawn)
            raise ValueError("music_amd.wavenet_autoencoder: global_classes = %d: classes must be %s"
                             % (getattr(self, "global_classes", 0), "None" if classes is not None else "given, one integer per clip"))
        if stages is None and self.training:
            stages = self.draw_stages(batch_size)
        # (refused here, before the engine is built: a bool, a float, a wrong length, a value outside [1, vq_stages])
        stages = vq_dropout.stage_counts(stages, batch_size, getattr(self, "vq_stages", 1))
        self._engine_for(wave_sample.device)
        cond = self.engine_cond()
        self._last_hook = None
        out = _AutoencoderFunction.apply(self, torch.is_grad_enabled(), wave_sample, cond, classes, stages, *list(self.parameters()))
        if getattr(self, "bottleneck", "continuous") == "vq":
            out, self.vq_loss = out
        hook, self._last_hook = self._last_hook, None
        return _losshook.wrap(out, hook) if self.fuse_loss else out
