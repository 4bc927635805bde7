"""Host-side execution plan of the WaveNet hot path on one MI355X.

`WaveNetEngine` owns the flat parameter / gradient buffers, the fragment-packing index maps, the
per-(batch, length) workspaces, and sequences the C-ABI kernels of libwavenet_hip.so for

    forward   wavenet/model.py:86-145          (probabilities, chunk-softmax semantics)
    backward  autograd of the above             (SURVEY Appendix B formulas)
    train_step  wavenet/train.py:171-182        (forward + CE-on-probs + backward [+ all-reduce] + Adam)

PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .engine_base import SLACK, PAD_BACK, EngineBase, SlabPlan, WorkspaceHold, WorkspacePool, _Spec, _pad  # noqa: F401 (re-exported)
from .packs import PackSet, causal_mats, epilogue_mats, gated_mats, pack_index, pack_positions, pair_mats  # noqa: F401 (pack_* re-exported)
from .stack import Cond, EpiBias, GatedStack, SkipEpilogue


class WaveNetEngine(EngineBase):
    def __init__(self, dilations, residual_channels, dilation_channels, skip_channels,
                 quantization_channels=256, filter_width=2, use_bias=False,
                 mode_fwd="f16x3", mode_bwd="bf16x3", device=None, global_classes=0, global_channels=0, phase_period=0):
        if filter_width != 2:
            raise NotImplementedError("HIP path implements filter_width == 2 (the reference's only configuration)")
        if quantization_channels != 256:
            raise NotImplementedError("HIP path implements quantization_channels == 256 (chunk softmax width)")
        self.dil = [int(d) for d in dilations]
        self.N = len(self.dil)
        self.k = 2                                       # filter width (EngineBase._build_spec, the decoder)
        self.g_n, self.g_E = int(global_classes), int(global_channels)      # class-conditional: classes, embedding width (0, 0: off)
        self.phase = int(phase_period)                   # phase-conditioned: the period P of the stream's stages (0: off)
        self.R, self.D, self.S, self.Q = residual_channels, dilation_channels, skip_channels, quantization_channels
        self.fused_loss_ok = True           # model.py: nn.CrossEntropyLoss on the module's output may run as wn_chunk_softmax256_ce (Q = 256 here)
        self.use_bias = bool(use_bias)
        self.CH = _pad(max(self.R, self.D), 32)
        if self.CH not in (32, 64):
            raise NotImplementedError("HIP path supports residual/dilation channels <= 64")
        self.SP = _pad(self.S, 32)
        self.rf = sum(self.dil) + 2
        self.off = [1]                                   # first valid absolute time of x_i
        for d in self.dil:
            self.off.append(self.off[-1] + d)
        assert self.off[-1] == self.rf - 1
        self.mode_fwd = _lib.MODE_NAMES[mode_fwd] if isinstance(mode_fwd, str) else mode_fwd
        self.mode_bwd = _lib.MODE_NAMES[mode_bwd] if isinstance(mode_bwd, str) else mode_bwd
        # <= 32 channels: TWO clips side by side are one 64-row tensor, and with block-diagonal packs the stack runs on the
        # 64-channel block kernels (one-launch backward included) on exactly the bytes of the 32-channel tensors - the
        # zero blocks cost matrix time only.  Even batches, no biases, (f16x3, bf16x3); WN_PAIR32=0: the 32-channel kernels.
        self.pair_ok = (self.CH == 32 and not self.use_bias and self.mode_fwd == _lib.F16X3 and self.mode_bwd == _lib.BF16X3
                        and os.environ.get("WN_PAIR32", "1") == "1" and os.environ.get("WN_PQ_BWD", "1") == "1")
        self.device = torch.device(device if device is not None else "cuda")
        _lib.load()
        self._build_spec()
        self._build_packs()
        self._init_state()
        # (overlap_wgrad, on the side stream: the epilogue's three weight gradients - 2 rounds of workgroups at 80 % fill each - pack
        # into the data-gradient GEMMs' idle CUs, epilogue backward 1.25 -> 1.00 ms)
        # the forward epilogue's three products as this many per-clip-group chains, every second one on the side stream (1 = one
        # chain on the main stream; bit-identical results: tests/test_gpu_switches.py)
        self.epi_chains = 2
        # ... or all three in ONE launch per 128-column tile (wn_skip_epilogue_fwd, round 6; 256 skip / 256 quantisation channels, x3
        # modes; WN_EPI_FUSED=0 = the three launches above)
        self.epi_fused = os.environ.get("WN_EPI_FUSED", "1") == "1"
        self.epi_fused_bwd = os.environ.get("WN_EPI_FUSED_BWD", "1") == "1"
        # Channel-split backward block with both weight gradients in the launch (wn_resblock_bwd_ms):
        # 64 padded channels, (f16x3, bf16x3) only; None = whenever it applies (WN_MS_BWD=0 turns it off)
        self.ms_bwd = None
        self.fine_marks = False
        # the unfused backward reads the forward's z (stored on the full valid range) for dWd
        self.z_from_fwd = True
        bn = "dilation_layer_stack.%d.bias"
        self.stack = GatedStack(self, "", self.CH, self.R, self.D, self._fr, self._br,
                                lambda i: (self._bias_ptr(bn % (4 * i)), self._bias_ptr(bn % (4 * i + 1)), self._bias_ptr(bn % (4 * i + 2))),
                                self.mode_fwd, self.mode_bwd, fmark=self.fmark, side_wgrad=True, zero_tail=True)
        # the bias gradients are rows of the gradient pack, behind the data-gradient products
        bias = EpiBias([bn % (4 * i + 3) for i in range(self.N)], "post_process_1.bias", "post_process_2.bias", self._bias_ptr,
                       lambda name: ptr(self.gpack, self.gp_bias_off[name]),
                       [self.spec.off[bn % (4 * i + 3)] for i in range(self.N)]) if self.use_bias else None
        # (class- or phase-conditional: h gains the term as the second product's residual C1 - the three-launch forward, never the fused one)
        self.epilogue = SkipEpilogue(self, ("skip", "p1", "p2"), ("U", "H", "C1" if self.gcond or self.phase else None, "dH"), self.CH, self.S, self.SP, self._fr, self._br,
                                     self.mode_fwd, self.mode_bwd, bias=bias, fmark=self.fmark)

    def fmark(self, name):
        """Per-kernel timing marks of the epilogue (tools/kbench.py epi); off unless self.fine_marks."""
        if self.fine_marks:
            self.mark(name)

    def _bias_ptr(self, name):
        if not self.use_bias:
            return None
        return ptr(self.flat, self.spec.off[name])

    def _fr(self, name):
        return ptr(self.pk_f, self.pk_f_off[name])

    def _br(self, name):
        return ptr(self.pk_b, self.pk_b_off[name])

    # ------------------------------------------------------------------ packs
    def _build_packs(self):
        sp, CH, N, dev = self.spec, self.CH, self.N, self.device
        wn = "dilation_layer_stack.%d.weight"
        pk = PackSet(sp.total)
        causal = causal_mats(sp.conv("causal_layer.weight"), CH)
        pk.fwd("causal", causal.w)
        pk.bwd("causalT", causal.wT)
        for i in range(N):
            g = gated_mats(sp.conv(wn % (4 * i)), sp.conv(wn % (4 * i + 1)), sp.conv(wn % (4 * i + 2))[:, :, 0], CH)
            pk.fwd("fg%d" % i, g.fg)
            pk.fwd("d%d" % i, g.d, chained=True)
            pk.bwd("dT%d" % i, g.dT)
            pk.bwd("fgT%d" % i, g.fgT)
            pk.bwd("pq%d" % i, g.pq)
            if self.pair_ok:
                g2 = pair_mats(g)
                pk.fwd("fg2_%d" % i, g2.fg, pair=True)
                pk.fwd("d2_%d" % i, g2.d, chained=True, pair=True)
                pk.bwd("dT2_%d" % i, g2.dT)
                pk.bwd("pq2_%d" % i, g2.pq)
        pk.epilogue(epilogue_mats([sp.conv(wn % (4 * i + 3))[:, :, 0] for i in range(N)], sp.conv("post_process_1.weight")[:, :, 0],
                                  sp.conv("post_process_2.weight")[:, :, 0], CH, self.SP), "skip", "p1", "p2", chained_fwd=True)
        # the bias gradients: rows of the gradient pack behind the matrices (wn_bias_grad writes them)
        for name in self.param_names if self.use_bias else ():
            if name.endswith(".bias"):
                pk.bias(name, sp.off[name], sp.shape[name][0])
        self.pk_f_off, self.pk_f_idx, self.pk_f = pk.finish(pk.f, self.mode_fwd, dev)
        self.pk_b_off, self.pk_b_idx, self.pk_b = pk.finish(pk.b, self.mode_bwd, dev)
        # gradient matrices + gather map (flat parameter element -> offset in gpack)
        self.gp_off, self.gp_bias_off = pk.gp_off, pk.gp_bias_off
        self.gpack = torch.zeros(pk.go, dtype=torch.float32, device=dev)
        gidx, ga, gb = pk.gather_maps()
        assert (gidx[:self.n_gather] >= 0).all()               # (the global block, the phase tables: wn_gclass_bwd / wn_phase_tab_bwd write theirs)
        self.gidx = torch.from_numpy(gidx.astype(np.int32)).to(dev)
        if self.pair_ok:
            # pair mode: the stack's weight gradients come out of the 64-channel block kernels as block-diagonal matrices -
            # a weight's gradient is the sum of its two copies (wn_gather_grads2); everything else as above
            self.gidx_pa = torch.from_numpy(ga.astype(np.int32)).to(dev)
            self.gidx_pb = torch.from_numpy(gb.astype(np.int32)).to(dev)
        self.wt_idx = torch.from_numpy(causal.taps).to(dev)
        self.wt = torch.zeros(causal.taps.size, dtype=torch.float32, device=dev)

    def pack_weights(self):
        st = _lib.stream()
        call("wn_pack_weights", ptr(self.flat), ptr(self.pk_f_idx), ptr(self.pk_f), self.pk_f_idx.numel(), self.mode_fwd, st)
        call("wn_pack_weights", ptr(self.flat), ptr(self.pk_b_idx), ptr(self.pk_b), self.pk_b_idx.numel(), self.mode_bwd, st)

    # ------------------------------------------------------------------ workspace
    def _make_workspace(self, B, T):
        dev = self.device
        pitch = _pad(T, 256) + 512        # tiles of 512 columns may overhang T by < 512
        W = T - self.rf + 1
        buf = lambda rows: self.act_buf(B, rows, pitch)
        ws = dict(B=B, T=T, W=W, pitch=pitch)
        ws["X"] = buf((self.N + 1) * self.CH)
        ws["Z"] = buf(self.N * self.CH)
        ws["U"] = buf(self.SP)
        ws["H"] = buf(self.SP)
        ws["O"] = torch.zeros(B * self.Q * W + PAD_BACK, dtype=torch.float32, device=dev)
        if self.gcond or self.phase:
            ws["C1"] = buf(self.SP)        # the output stage's class / phase term, expanded over time
        ws["bwd"] = None
        # which backward blocks this workspace is planned for: decided ONCE here (slab layout, (P, Q) buffers, and whether
        # the forward has to store z on each block's whole range for the fallback backward) - a switch flipped later
        # takes effect with the next workspace, never half-way between a forward and its backward
        ws["ms"], ws["pq"] = self._use_ms(), self._use_pq()
        ws["pair"] = self.pair_ok and B % 2 == 0
        # the FORWARD block of the 64-channel form takes 512 columns per workgroup: below ~200 workgroups (B / 2 pairs x T / 512)
        # the 32-channel forward fills the chip better (same X / Z layout either way; the backward pairs regardless)
        ws["pair_fwd"] = ws["pair"] and (B // 2) * ((T + 511) // 512) >= 200
        return ws

    def _bwd_workspace(self, ws):
        if ws["bwd"] is not None:
            return ws["bwd"]
        B, pitch, W, dev = ws["B"], ws["pitch"], ws["W"], self.device
        buf = lambda rows: self.act_buf(B, rows, pitch)
        bw = dict(dO=torch.zeros(B * self.Q * W + PAD_BACK, dtype=torch.float32, device=dev),
                  dH=buf(self.SP), dU=buf(self.SP), dZ=buf(self.N * self.CH),
                  dX=[buf(self.CH), buf(self.CH)], dfg=[buf(2 * self.CH), buf(2 * self.CH)],
                  zs=[buf(self.CH), buf(self.CH)])
        T, lo = ws["T"], self.rf - 1
        ms = ws["ms"]
        bw["ms"] = ms
        bw["pq"] = ws["pq"]
        pair = bw["pair"] = ws["pair"]
        if bw["pq"] or pair:
            bw["PQ"] = [(buf(self.CH), buf(self.CH)), (buf(self.CH), buf(self.CH))]
        # (time chunk per workgroup of the epilogue's weight gradients; 512 / 256 / 2048-4096 measured on one box in round 5: step 4.36 /
        # 4.46 / 4.35 against 4.34 ms - shorter chunks pay in slabs to reduce, longer ones in the blocks that run beside them)
        # round 6 (the fused epilogue: the weight gradients of post_process_1 and of the skip convs now run on their own, beside each
        # other, behind the fused launch): 2048 for all three - step 4.141 against 4.19 - 4.23 at (1024, 1024, 2048), 4.22 at (512, 512, 1024),
        # 4.25 at 3264, 4.38 at 4096 (profiles/r06_ab_wgrad_chunks.json)
        ck = [int(v) for v in os.environ.get("WN_EPI_WGRAD_CHUNKS", "2048,2048,2048").split(",")]
        if "WN_EPI_WGRAD_CHUNKS" not in os.environ:
            # ... cut into EQUAL chunks of at most that: 12960 columns are 6 x 2048 + 672, and the launch takes as long as its full chunks
            # (7 x 1856: epilogue backward 0.861 -> 0.845 ms)
            span = T - (lo & ~31)

            def even(c):
                n = -(-span // c)                      # chunks per clip
                return -(-(-(-span // n)) // 32) * 32    # their common length, a multiple of the 32-sample k-step
            ck = [even(c) for c in ck]
        plan = SlabPlan(self.gp_off)
        for name, c in zip(("p2", "p1", "skip"), ck):
            plan.add(name, _lib.wgrad_slabs(lo, T, c, B), c)
        # one-launch blocks whose dilation is a multiple of 32 hand dx on WHOLE (chain form of wn_resblock_bwd_pq: the Q rows
        # of an item are the carry of the next item of its chain); decided here, once per workspace, with the slab counts
        Bp = B // 2 if pair else B
        # 0: every block hands the (P, Q) pair on (round 3's form); so do conditioned blocks (the chain form takes no table)
        want = os.environ.get("WN_PQ_CHAIN", "1") == "1" and not self.gcond and not self.phase
        bw["chain"] = [want and bool(bw["pq"] or pair) and _lib.pq_chain_ok(self.off[i + 1], T, Bp, self.dil[i]) for i in range(self.N)]
        sfx = "2_" if pair else ""                            # pair mode: the block-diagonal gradient matrices of B / 2 clip pairs
        for i in range(self.N):
            t_lo = self.off[i + 1]
            if bw["pq"] or pair:                              # one-launch block (on clips or clip pairs): one slab per workgroup of ITS plan
                ns, chunk = _lib.pq_slabs(t_lo, T, Bp, self.dil[i], bw["chain"][i]), None
            elif ms:                                          # channel-split block: one slab per workgroup
                ns, chunk = _lib.ms_slabs(t_lo, T, B), None
            else:
                ns, chunk = _lib.wgrad_slabs(t_lo, T, 512, B), 512
            plan.add("fg%s%d" % (sfx, i), ns, chunk)
            if i < self.N - 1:
                plan.add("d%s%d" % (sfx, i), ns, chunk)
        plan.add("causal", _lib.wgrad_slabs(1, T, 512, B), 512)
        # the same gradient from integer codes (wn_causal_wgrad_codes) when the input is a one-hot this engine / the
        # loader built: its own slab region and its own reduction table (only the last row differs)
        plan.add_alternative("causal", "causal_codes", _lib.causal_codes_slabs(T, B))
        bw.update(plan.finish(dev))
        ws["bwd"] = bw
        return bw

    def _use_ms(self):
        ok = self.CH == 64 and self.mode_fwd == _lib.F16X3 and self.mode_bwd == _lib.BF16X3
        if self.ms_bwd is None:
            return ok and os.environ.get("WN_MS_BWD", "1") == "1"
        if self.ms_bwd and not ok:
            raise NotImplementedError("ms_bwd needs 64 padded channels and precision (f16x3, bf16x3)")
        return bool(self.ms_bwd)

    def _use_pq(self):
        """The whole per-block backward, data gradient included, in one launch (wn_resblock_bwd_pq): wherever the
        two-role block applies and there are no biases (their gradients are sums over [df;dg], which that kernel
        never writes out).  WN_PQ_BWD=0: resblock_bwd_rw_k + chan_gemm_rw_k."""
        return self._use_ms() and not self.use_bias and os.environ.get("WN_PQ_BWD", "1") == "1"

    def _x(self, ws, i):
        return ptr(ws["X"], SLACK + i * ws["B"] * self.CH * ws["pitch"])

    # ------------------------------------------------------------------ forward
    def _cond_shape(self, ws, i):
        """(frames, mode, q) of block i's table (i = N: the output stage's): ONE frame stretched over the stage's whole range (class-
        conditional), or P frames tiled over it, frame (t - t_lo) mod P (phase-conditioned, with or without classes)"""
        if self.phase:
            return self.phase, 2, 1
        return 1, 1, (ws["T"] - self.off[i + 1] if i < self.N else ws["W"])

    def _gclass_tables(self, ws, cls, st, pos=None):
        """The clips' conditioning of one forward: every block's table [f; g]_i += G_i emb[c] and the output stage's h += G_f emb[c]
        (one launch, wn_gclass_fwd), in the forms the autoencoder's decoder runs a table of <= 32 frames in (music_amd/model1.py) -
        here ONE frame stretched over the block's whole range.  pos (a phase-conditioned model; cls may then be None): the tables have
        P frames, the phase tables' columns rotated by the clip's position plus the class column (one more launch, wn_phase_tab_fwd),
        tiled over the block's range.  Returns i -> stack.Cond; fills ws["C1"]."""
        B, T, W, pitch, N, CH = ws["B"], ws["T"], ws["W"], ws["pitch"], self.N, self.CH
        pair, pair_f, dev = ws["pair"], ws["pair_fwd"], self.device
        empty = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # per clip for a 32-channel or unpaired forward, as clip pairs for the pair blocks (forward if pair_f, backward always)
        le = self.phase or 1
        gc = (None, None, None)                       # the class term's (tab per clip, tab of pairs, enf), one frame
        if cls is not None:
            gc = (empty(N, B, 2 * CH) if not pair_f else None, empty(N, B // 2, 4 * CH) if pair else None, empty(B, self.S))
            self.gclass_fwd(cls, *gc, CH, st)
        if pos is not None:
            tab_c = empty(N, B, 2 * CH, le) if not pair_f else None
            tab = empty(N, B // 2, 4 * CH, le) if pair else tab_c
            enf = empty(B, self.S, le)
            self.phase_fwd(pos, tab_c, tab if pair else None, enf, CH, st, gc)
        else:
            tab_c, tab, enf = gc[0], gc[1] if pair else gc[0], gc[2]
        ws["tab"] = tab
        CHp, Bp = (64, B // 2) if pair else (CH, B)
        cpk = cix = None
        if CHp == 64 and self.mode_fwd == _lib.F16X3:
            # the conditioning bias on the matrix cores: the bucket of every sample as bytes (one frame: all 0; built once per
            # workspace) and, per forward, the tables as packed A fragments ([2 CH rows][32 buckets] per block and clip)
            if "cidx" not in ws:
                ws["cidx"] = torch.zeros(N, _lib.COND_IDX_PAD + T + 64, dtype=torch.uint8, device=dev)
                for i in range(N if le > 1 else 0):        # (P frames: the bucket of sample t of block i is (t - t_lo) mod P)
                    L = T - self.off[i + 1]
                    ws["cidx"][i, _lib.COND_IDX_PAD:_lib.COND_IDX_PAD + L] = (torch.arange(L, device=dev) % le).to(torch.uint8)
                row, k = pack_positions(2 * CHp // 16, 1, False)
                one = np.where(k < le, row * le + k, -1).astype(np.int64)                   # one [2 CH][le] table
                base = np.arange(N * Bp, dtype=np.int64)[:, None] * (2 * CHp * le)
                ws["ctab_idx"] = torch.from_numpy(np.where(one[None, :] >= 0, base + one[None, :], -1).astype(np.int32).reshape(-1)).to(dev)
                ws["ctab_pk"] = torch.empty(N * Bp * 2 * CHp * 32 * 2, dtype=torch.int16, device=dev)
            if pair_f or not pair:                        # (the backward blocks read the fp32 table; only a 64-channel forward the pack)
                call("wn_pack_weights", ptr(tab), ptr(ws["ctab_idx"]), ptr(ws["ctab_pk"]), ws["ctab_idx"].numel(), self.mode_fwd, st)
                cpk, cix = ws["ctab_pk"], ws["cidx"]
        cpb = 2 * CHp * 32 * 2                          # halfs of one clip's packed table (hi + lo planes)
        tab_f, n_f = (tab, Bp) if pair_f else (tab_c, B)
        _, mode_c, q = self._cond_shape(ws, N)
        call("wn_cond_expand", ptr(enf), self.S * le, le, self.S, self.rf - 1, T, mode_c, le, q, ptr(ws["C1"], SLACK), self.SP * pitch, pitch, B, st)
        return lambda i: Cond(ptr(tab_f[i]), tab_f.shape[2] * le, *self._cond_shape(ws, i),
                              ptr(cpk, i * n_f * cpb) if cpk is not None else None, cpb, ptr(cix[i]) if cix is not None else None)

    def forward_logits(self, x, ws=None, codes=None, classes=None, phase_pos=None):
        """x: (B,Q,T) float32 contiguous on the device.  Runs causal conv, the residual stack, the
        skip product and both post-process convs; leaves the pre-softmax (B,Q,W) in ws['O'].
        codes = (int32 (B,T) device tensor, scrambled) instead of x: the one-hot is never built.
        classes: one integer per clip of a class-conditional model (EngineBase.stage_classes), else None.
        phase_pos: the stream position of every clip's first target of a phase-conditioned model (EngineBase.stage_phase), else None."""
        if x is None:
            B, T = codes[0].shape
            Q = self.Q
            assert codes[0].is_cuda and codes[0].dtype == torch.int32 and codes[0].is_contiguous()
        else:
            B, Q, T = x.shape
            assert Q == self.Q and x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda
        W = T - self.rf + 1
        if W <= 0:
            raise ValueError("wave sample not long enough")          # wavenet/model.py:100-101
        cls, pos = self.stage_classes(classes, B), self.stage_phase(phase_pos, B)
        ws = ws or self._ws.get(B, T)
        st = _lib.stream()
        CH, pitch, mf = self.CH, ws["pitch"], self.mode_fwd
        ws["cls"], ws["pos"] = cls, pos
        self._gen += 1
        ws["gen"] = self._gen
        ws["x_in"] = x
        # a one-hot built from integer codes by onehot() / the loader carries them along: the backward then forms the
        # causal layer's weight gradient by scatter instead of streaming the dense tensor (still valid only while the
        # tensor has not been written to since)
        ws["x_codes"] = (codes[0], bool(codes[1])) if x is None else self.tagged_codes(x, B, T)
        # what the backward re-checks: the causal layer's weight gradient is formed later from these same tensors
        ws["x_ver"] = None if x is None else x._version
        ws["codes_ver"] = None if ws["x_codes"] is None else ws["x_codes"][0]._version
        # causal conv (wavenet/model.py:104): x0[t] = W0 in[t-1] + W1 in[t], t in [1,T)
        self.causal_fwd(ws, x, self.wt_idx, self.wt, self._fr("causal"), self._bias_ptr("causal_layer.bias"), self.R, CH, self._x(ws, 0), st, mf)
        self.mark("causal_fwd")
        # z: the skip product needs it on the crop [rf-1, T) only, and the two-role / one-launch backward blocks recompute
        # it on the CU.  Only the fallback backward (resblock_bwd_k + wgrad_k: 32 padded channels, x1 modes) reads the
        # forward's z for dWd on the block's whole valid range [off_{i+1}, T) (19 % more z; it saves that path a second
        # copy written by its recompute kernel).
        z_whole = self.z_from_fwd and not ws["ms"] and not ws["pair"]      # (pair: the one-launch backward recomputes z)
        cond = None
        if pos is not None:
            cond = self._gclass_tables(ws, cls, st, pos)
            self.mark("phase_fwd")
        elif cls is not None:
            cond = self._gclass_tables(ws, cls, st)
            self.mark("gclass_fwd")
        self.stack.forward(B, T, pitch, ws["X"], ws["Z"], z_whole, st, cond=cond, pair=ws["pair_fwd"])
        self.mark("stack_fwd")
        self.epilogue.forward(ws, self.epilogue.skip_bias(ws), st, self.epi_fused, int(self.epi_chains))
        self.mark("epilogue_fwd")
        return ws

    def forward(self, x, classes=None, phase_pos=None):
        """wavenet/model.py:86-145 -> probabilities (B*W, Q) (fresh tensor)."""
        self.pack_weights()
        ws = self.forward_logits(x, classes=classes, phase_pos=phase_pos)
        B, W = ws["B"], ws["W"]
        probs = torch.empty(B * W, self.Q, dtype=torch.float32, device=self.device)
        call("wn_chunk_softmax256_fwd", ptr(ws["O"]), ptr(probs), B * W, _lib.stream())
        ws["probs"] = probs
        return probs, ws

    # ------------------------------------------------------------------ backward
    def backward_from_dlogits(self, ws):
        """ws['bwd']['dO'] holds d loss / d pre-softmax (B,Q,W).  Fills self.flat_grad."""
        bw = self._bwd_workspace(ws)
        st = _lib.stream()
        # (WN_EPI_BWD_ORDER=0: the skip weight gradient beside the stack, on the side stream)
        a = self.epilogue.begin_backward(ws, bw)
        d_enf, after_dh = None, lambda: None
        if ws.get("cls") is not None or ws.get("pos") is not None:
            # the output stage's class / phase term: d enf = the sum of dh over each clip's time (over each frame's samples)
            le, mode_c, q = self._cond_shape(ws, self.N)
            d_enf = torch.zeros(ws["B"], self.S, *((le,) if self.phase else ()), dtype=torch.float32, device=self.device)
            after_dh = lambda: call("wn_cond_grad", a.dH, a.sb, a.pitch, self.S, self.rf - 1, a.T, mode_c, le, q, ptr(d_enf), self.S * le, le, a.B, st)
        self.epilogue.backward(a, st, self.epi_fused_bwd and not self.use_bias, side_skip=os.environ.get("WN_EPI_BWD_ORDER", "1") != "1",
                               after_dh=after_dh)
        self.mark("epilogue_bwd")
        return self._backward_stack(ws, bw, st, d_enf)

    def _backward_stack(self, ws, bw, st, d_enf=None):
        """The residual stack's backward, the causal layer's weight gradient and the slab reduction (second half of backward_from_dlogits).
        d_enf: the gradient of the output stage's class term (class-conditional), else None."""
        B, T, pitch, CH = ws["B"], ws["T"], ws["pitch"], self.CH
        N, cls, pos, cond, d_tab = self.N, ws.get("cls"), ws.get("pos"), None, None
        form = "pq" if bw["pq"] or bw["pair"] else "ms" if bw["ms"] else "rw"
        le = self.phase or 1
        conditioned = cls is not None or pos is not None
        if conditioned:
            # the block tables' gradients, sums of [df; dg] over each clip's time: inside the one-launch block as bucket sums (one
            # bucket) reduced behind the stack, else wn_cond_grad on the [df; dg] the block wrote - as the autoencoder's decoder
            Bp, rows = (B // 2, 4 * CH) if bw["pair"] else (B, 2 * CH)
            d_tab = torch.zeros(N, Bp, rows, *((le,) if self.phase else ()), dtype=torch.float32, device=self.device)
            if form == "pq" and "cslab" not in bw:
                import ctypes
                fl = [_lib.load().wn_resblock_bwd_pq_cond_floats(self.off[i + 1], T, Bp) for i in range(N)]
                bw["cs_off"] = (ctypes.c_int64 * N)(*np.concatenate([[0], np.cumsum(fl)[:-1]]).tolist())
                bw["cs_tlo"] = (ctypes.c_int * N)(*[self.off[i + 1] for i in range(N)])
                bw["cslab"] = torch.empty(sum(fl), dtype=torch.float32, device=self.device)

            def cond(i):
                mc = dict(cidx=ptr(ws["cidx"][i]), cslab=ptr(bw["cslab"], bw["cs_off"][i])) if form == "pq" else {}
                return Cond(ptr(ws["tab"][i]), rows * le, *self._cond_shape(ws, i), **mc)

        def bias_grads(i, dfg, dy, t_lo, s_):
            """row sums of [df;dg] and of dy: the gradients of block i's three biases (and of its class table)"""
            if conditioned:
                _, mode_c, q = self._cond_shape(ws, i)
                call("wn_cond_grad", dfg, 2 * CH * pitch, pitch, 2 * CH, t_lo, T, mode_c, le, q, ptr(d_tab[i]), 2 * CH * le, le, B, s_)
            if self.use_bias:
                bo, bn = self.gp_bias_off, "dilation_layer_stack.%d.bias"
                call("wn_bias_grad", dfg, 2 * CH * pitch, pitch, 0, self.D, t_lo, T, B, ptr(self.gpack, bo[bn % (4 * i)]), s_)
                call("wn_bias_grad", dfg + 4 * CH * pitch, 2 * CH * pitch, pitch, 0, self.D, t_lo, T, B, ptr(self.gpack, bo[bn % (4 * i + 1)]), s_)
                if dy is not None:
                    call("wn_bias_grad", dy, CH * pitch, pitch, 0, self.R, t_lo, T, B, ptr(self.gpack, bo[bn % (4 * i + 2)]), s_)
        # The per-layer weight-gradient products of the fallback form only feed the slab reduction at the very end, so they run on the
        # side stream next to the data-gradient chain (resblock_bwd -> dx product -> next block); dfg / z scratch is double-buffered for that.
        self.stack.backward(form, B, T, pitch, ws["X"], ws["Z"], bw, bw["dX"], st, chain=bw["chain"], dfg=bw["dfg"],
                            zs=None if self.z_from_fwd else bw["zs"], cond=cond, pair=bw["pair"], hook=bias_grads)
        if conditioned and form == "pq":
            call("wn_resblock_bwd_pq_cond_reduce", ptr(bw["cslab"]), bw["cs_off"], bw["cs_tlo"], N, T, Bp, le, ptr(d_tab), Bp * rows * le,
                 rows * le, le, st)
        self.join_side()              # everything on the side stream (epilogue weight gradients)
        if pos is not None:           # behind the last table gradient: the phase tables' own, flat_grad's tail, and the sums over the
            sums = (torch.empty(N, Bp, rows, dtype=torch.float32, device=self.device),                 # frames: the class term's
                    torch.empty(B, self.S, dtype=torch.float32, device=self.device)) if cls is not None else (None, None)
            self.phase_bwd(pos, d_tab, bw["pair"], d_enf, CH, st, sums)
            d_tab, d_enf = sums
        if cls is not None:           # behind the last table gradient: the global block's own, flat_grad's tail
            self.gclass_bwd(cls, d_tab, bw["pair"], d_enf, CH, st)
        self.mark("stack_bwd")
        # causal weight gradient: dWc[r][q][tap] = sum dx0[r][t] in[q][t-1+tap]
        dx0 = ptr(bw["dX"][0], SLACK)
        # the input and the codes it was built from must still be what the forward saw (_check_input_unchanged; onehot() documents
        # the tensor as immutable while tagged)
        self._check_input_unchanged(ws)
        x_codes = self.codes_for_backward(ws)
        self.causal_wgrad(ws, bw, x_codes, "causal", dx0, CH, st, self.mode_bwd)
        if self.use_bias:
            call("wn_bias_grad", dx0, CH * pitch, pitch, 0, self.R, 1, T, B, ptr(self.gpack, self.gp_bias_off["causal_layer.bias"]), st)
        self.mark("causal_bwd")
        self.reduce_and_gather(bw, x_codes is not None, st)
        self.mark("slab_reduce")

    def input_grad(self, ws):
        """Gradient of the last backward w.r.t. the module's INPUT (what autograd gives the reference when the input requires grad:
        the causal nn.Conv1d's data gradient, wavenet/model.py:104):  din[q][s] = sum_r W[r][q][1] dx0[r][s] + W[r][q][0] dx0[r][s + 1],
        dx0 living on [1, T).  One channel product on the first block's data gradient, which the backward leaves in its workspace."""
        bw = ws["bwd"]
        if bw is None:
            raise RuntimeError("music_amd: input_grad() needs the backward of this forward to have run")
        return self.causal_input_grad(ws, bw["dX"][0], self.CH, self._br("causalT"), self.mode_bwd)

    def backward(self, ws, dprobs):
        """dprobs: (B*W, Q) gradient w.r.t. the probabilities returned by forward()."""
        bw = self._bwd_workspace(ws)
        dprobs = dprobs.contiguous()
        call("wn_chunk_softmax256_bwd", ptr(ws["probs"]), ptr(dprobs), ptr(bw["dO"]), ws["B"] * ws["W"], _lib.stream())
        self.backward_from_dlogits(ws)

    # ------------------------------------------------------------------ fused training step
    def loss_and_grad_codes(self, codes, target, scrambled=True, want_probs=False, objective=None, windows=None, window_pos=None,
                            classes=None, phase_pos=None, weights=None, ignore_index=None, label_smoothing=0.0):
        """loss_and_grad on the integer codes themselves (int32 (B,T) on the device; `scrambled` = the loader's one-hot
        layout, faster_audio_data.py:77-81): same result as loss_and_grad(self.onehot(codes, scrambled), target), but the
        (B,256,T) float tensor is never built, written or read - the causal layer is a gather forward and
        a scatter backward."""
        return self.loss_and_grad(None, target, want_probs, codes=(codes, scrambled), objective=objective, windows=windows,
                                  window_pos=window_pos, classes=classes, phase_pos=phase_pos, weights=weights, ignore_index=ignore_index,
                                  label_smoothing=label_smoothing)

    def loss_and_grad(self, x, target, want_probs=False, codes=None, objective=None, windows=None, window_pos=None, classes=None,
                      phase_pos=None, weights=None, ignore_index=None, label_smoothing=0.0):
        """forward + CrossEntropyLoss(probs, target) + backward (wavenet/train.py:178-181).
        Returns the loss as a 0-d device tensor; gradients land in self.flat_grad.  objective: None = self.objective
        (EngineBase; "nll" = the negative log-likelihood under the per-timestep softmax instead of the reference's loss).  windows /
        window_pos: the position windows of "nll" (EngineBase.step_nll; None = self.nll_windows).  classes, phase_pos: forward_logits'.
        weights / ignore_index / label_smoothing: step_nll's masked, weighted and smoothed "nll"."""
        def step():
            self.mark("begin")
            self.pack_weights()
            self.mark("pack")
            return self._fused_tail(self.forward_logits(x, codes=codes, classes=classes, phase_pos=phase_pos), target, want_probs, objective,
                                    windows, window_pos, weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing)
        return self._throttled(step)

    def softmax_ce(self, *args):
        super().softmax_ce(*args)
        self.mark("softmax_ce")

    def adam_step(self, gscale=1.0):
        super().adam_step(gscale)
        self.mark("adam")

    def onehot(self, codes, scrambled=True):
        """int32 (B,T) codes on the device -> float32 (B,Q,T) (faster_audio_data.py:62-83).
        The result carries its codes (`_wn_codes`), and a forward on it runs the causal layer from the codes instead of
        streaming the 131 MB dense tensor.  CONTRACT: while tagged, the tensor and the codes are immutable - an in-place
        op that bumps the version counter drops the fast path (forward) or is reported (backward); a write that does
        not (`.data`, raw pointers, `out=` on the storage) is undetectable and would make the causal layer compute on
        the original codes.  A copy (`.to()`, `.contiguous()` of a non-contiguous view, `.clone()`) loses the tag and
        silently takes the dense path (+0.08 ms per step at config 2)."""
        B, T = codes.shape
        out = torch.empty(B, self.Q, T, dtype=torch.float32, device=self.device)
        call("wn_onehot", ptr(codes), ptr(out), B, self.Q, T, 1 if scrambled else 0, _lib.stream())
        self.mark("onehot")
        if codes.is_contiguous() and codes.dtype == torch.int32:
            out._wn_codes = (codes, bool(scrambled), out._version, codes._version)      # see forward_logits
        return out
