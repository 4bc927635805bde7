"""What the three training engines (engine.WaveNetEngine, model1._AutoencoderEngine, plan_generic.GeneralPlan) share on the host:
the workspace pool, the flat-parameter spec, `EngineBase` (state, timing marks, the tail of the fused step, the Adam step) and
`SlabPlan`, the bookkeeping of where every weight-gradient launch writes its slabs and what wn_reduce_slabs sums.

PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
import ctypes
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import _lib, guard, vq_dropout
from ._lib import call, ptr

SLACK = 64          # floats in front of every activation buffer
PAD_BACK = 2048     # floats behind


def _pad(n, m):
    return (n + m - 1) // m * m


class WorkspacePool:
    """(B, T) -> workspaces of that shape.  A workspace whose activations a pending autograd node still needs is HELD
    (hold() in the Function's forward, release() after its backward or when the graph dies): the next forward of the
    same shape then gets ANOTHER workspace instead of overwriting it, so a module can have several forwards in flight
    (gradient accumulation over micro-batches, the reference's autograd semantics, wavenet/model.py:86-145).  Shapes are
    evicted one at a time, least recently used first, never one that is held."""
    MAX_SHAPES = 4
    MAX_PER_SHAPE = 4

    def __init__(self, make):
        from collections import OrderedDict
        self._make = make
        self._d = OrderedDict()
        self._last = {}

    def peek(self, B, T):
        """The workspace the LAST forward of this shape used (held or not) - what a caller inspects after a step; a
        fresh one if there has been none."""
        ws = self._last.get((B, T))
        return ws if ws is not None else self.get(B, T)

    def get(self, B, T):
        """A workspace for the NEXT forward of this shape: the first one no pending backward holds, else a new one."""
        key = (B, T)
        lst = self._d.get(key)
        if lst is None:
            if len(self._d) >= self.MAX_SHAPES:
                for k, wl in self._d.items():
                    if not any(w.get("held") for w in wl):
                        del self._d[k]
                        self._last.pop(k, None)
                        break
            lst = self._d[key] = []
        self._d.move_to_end(key)
        for ws in lst:
            if not ws.get("held"):
                self._last[key] = ws
                return ws
        if len(lst) >= self.MAX_PER_SHAPE:
            # the reference never runs out (autograd just keeps allocating): take the OLDEST waiting forward's workspace over, say
            # so once, and let a backward that still arrives for it fail loudly (its generation no longer matches)
            import warnings
            warnings.warn("music_amd: %d forwards of shape %s are waiting for their backward; the oldest one's activations are "
                          "reused (run backward(), drop the outputs, or use torch.no_grad() for inference)" % (len(lst), key))
            ws = min(lst, key=lambda w: w.get("gen", 0))
            ws["held"] = False
            self._last[key] = ws
            return ws
        ws = self._make(B, T)
        lst.append(ws)
        self._last[key] = ws
        return ws

    def clear(self):
        self._d.clear()
        self._last.clear()

    def __len__(self):
        return sum(len(v) for v in self._d.values())


class WorkspaceHold:
    """Keeps a workspace out of the pool's hands while an autograd node needs it; released explicitly after backward or
    by garbage collection of the node (an output that was dropped without a backward)."""

    def __init__(self, ws):
        self.ws, self.gen = ws, ws["gen"]
        ws["held"] = True

    def release(self):
        if self.ws is not None and self.ws.get("gen") == self.gen:
            self.ws["held"] = False
        self.ws = None

    def __del__(self):
        self.release()


class _Spec:
    """Offsets of every reference parameter inside the flat buffer (state_dict order)."""

    def __init__(self, named_shapes):
        self.off, self.shape = {}, {}
        o = 0
        for name, shape in named_shapes:
            self.off[name] = o
            self.shape[name] = tuple(shape)
            o += int(np.prod(shape))
        self.total = o

    def conv(self, name):
        """int64 array [O, I, k] of flat offsets of a Conv1d weight."""
        shp = self.shape[name]
        return self.off[name] + np.arange(int(np.prod(shp)), dtype=np.int64).reshape(shp)


OBJECTIVES = ("reference", "nll")     # what a fused step minimises: the reference's loss, or the true NLL per sample


class WindowTable:
    """A table of position windows (include/wavenet_hip.h): 1..16 ``(lo, hi)`` pairs with 0 <= lo < hi <= Q; stream position p is
    sampled, or scored, inside pair ``p % len(windows)``.  THE place the pairs are parsed and checked and the host array the entry
    points read is built: the decoder's and the sampler's table (fast_generate._Windows) and the "nll" objective's (NllWindows) are
    this class with their own ``tail``."""

    def __init__(self, windows, Q):
        try:
            pairs = [(int(lo), int(hi)) for lo, hi in windows]
        except (TypeError, ValueError):
            raise ValueError("windows must be a sequence of (lo, hi) pairs") from None
        if not 1 <= len(pairs) <= 16:
            raise ValueError("windows must hold 1..16 (lo, hi) pairs, got %d" % len(pairs))
        for lo, hi in pairs:
            if not 0 <= lo < hi <= Q:
                raise ValueError("every window needs 0 <= lo < hi <= Q = %d, got (%d, %d)" % (Q, lo, hi))
        self.pairs = pairs
        self.host = (ctypes.c_int32 * (2 * len(pairs)))(*[v for pr in pairs for v in pr])

    def at(self, pos):
        """The pair of stream position ``pos``."""
        return self.pairs[pos % len(self.pairs)]


class NllWindows(WindowTable):
    """The position windows of the "nll" objective (wn_win_step_nll): the samplers' table (fast_generate.stage_windows); the column
    at stream position p is scored inside pair ``p % len(windows)``."""
    pos = None                           # the per-clip positions of the last tail(), kept alive for the launch

    def tail(self, window_pos, B, device):
        """The arguments the windowed entries take behind those of wn_step_nll / wn_step_softmax (before the stream): win_host,
        win_period, win_pos, win_pos0.  window_pos: None (every clip starts at position 0), an int (all clips), or one per clip - a
        host sequence, or an int64 device tensor, which travels as it is (no host synchronisation)."""
        pos, pos0 = None, 0
        if isinstance(window_pos, torch.Tensor) and window_pos.dim() > 0:
            pos = window_pos.reshape(-1)
            if pos.dtype != torch.int64:
                raise ValueError("window_pos as a tensor is int64, one stream position per clip, got %s" % pos.dtype)
            pos = pos.to(device).contiguous()
        elif window_pos is not None and not isinstance(window_pos, (int, np.integer, torch.Tensor)):
            vals = [int(v) for v in window_pos]
            if any(v < 0 for v in vals):
                raise ValueError("window_pos (the stream position of a clip's first target) must be >= 0, got %d" % min(vals))
            pos = torch.tensor(vals, dtype=torch.int64).to(device)
        elif window_pos is not None:
            pos0 = int(window_pos)
            if pos0 < 0:
                raise ValueError("window_pos (the stream position of a clip's first target) must be >= 0, got %d" % pos0)
        if pos is not None and pos.numel() != B:
            raise ValueError("window_pos holds %d positions for %d clips" % (pos.numel(), B))
        self.pos = pos
        return ctypes.cast(self.host, ctypes.c_void_p), len(self.pairs), ptr(pos), pos0


SlabOp = namedtuple("SlabOp", "so n chunk ns")      # first slab element, elements per slab, wn_wgrad's chunk (or None), slabs


class SlabPlan:
    """Weight-gradient slabs: every weight-gradient workgroup writes its partial C with plain stores into a region of its own,
    one batched kernel (wn_reduce_slabs) then sums the slabs of all ops in a fixed order - deterministic.  The ORDER of the add()
    calls fixes the slab offsets and the order of that sum.  The caller passes the slab count of the kernel it has chosen for the op
    (_lib.wgrad_slabs / ms_slabs / pq_slabs / enc_slabs / causal_codes_slabs); `chunk` is what wn_wgrad is handed, None for an op
    that another kernel writes."""

    def __init__(self, gp_off):
        self.gp_off, self.ops, self.desc, self.row, self.alt = gp_off, {}, [], {}, []
        self.so = self.vs = 0

    def __getitem__(self, name):
        return self.ops[name]

    def _region(self, name, n, chunk, ns):
        op = self.ops[name] = SlabOp(self.so, n, chunk, ns)
        self.so += ns * n
        return op

    def add(self, name, ns, chunk=None, grad=None):
        """`ns` slabs of gradient matrix `grad or name`, and its row [vs, so, ns, n, go, n] of the reduction table."""
        go, r, c = self.gp_off[grad or name]
        op = self._region(name, r * c, chunk, ns)
        self.row[name] = len(self.desc)
        self.desc.append([self.vs, op.so, ns, op.n, go, op.n])
        self.vs += (op.n + 3) // 4

    def add_alternative(self, of, name, ns):
        """Another kernel for the gradient of `of` (a causal layer from integer codes): a slab region of its own, and [so, ns] in the
        row of `of` in a second reduction table that is otherwise the first."""
        op = self._region(name, self.ops[of].n, None, ns)
        self.alt.append((self.row[of], [op.so, ns]))

    def finish(self, device):
        """The backward workspace's entries: slab tensor, this plan, reduction table(s), vector count and op count of the reduction."""
        out = dict(slab=torch.empty(self.so, dtype=torch.float32, device=device), plan=self, vec=self.vs, nops=len(self.desc),
                   desc=torch.tensor(self.desc, dtype=torch.int64, device=device))
        if self.alt:
            rows = [list(r) for r in self.desc]
            for i, so_ns in self.alt:
                rows[i][1:3] = so_ns
            out["desc_codes"] = torch.tensor(rows, dtype=torch.int64, device=device)
        return out


class VqStats:
    """What one forward's wn_vq_fwd left on the device, read on demand (nothing here runs in the step): `mse` and `perplexity` are
    0-d device tensors, `vq_loss` = (1 + beta) mse - beta mse with EMA codebook updates, where the codebook term is gone (`coef`) -,
    `codes_used` the number of codes at least one frame chose.

    With a residual chain of S > 1 stages (wn_rvq_fwd) `part` is (S, partials) and `counts` (S, K): `stage_mse` (S,) holds every
    stage's sum (r_s - q_s)^2 / (C Bw), `mse` is the LAST stage's - the error of q against e -, `vq_loss` = coef x their sum, and
    `stage_perplexity` / `stage_codes_used` (S,) stand beside `perplexity` / `codes_used`, which describe stage 0.

    `stage_frames` (S,) = counts.sum(1), the frames that took part in each stage: all of them without quantiser dropout, the ACTIVE
    ones of a forward with stage counts (wn_rvq_fwd_n, `final_res` given).  There `stage_mse` keeps the fixed denominator C Bw (its
    sum x coef is vq_loss, the batch expectation), `stage_mse_active` = stage_mse C / stage_frames is the stage's error per frame it
    saw (0 where it saw none), `stage_perplexity` is taken over the stage's own active frames, and `mse` - q against e - comes from
    `final_res`, every frame's residual behind ITS last active stage."""

    def __init__(self, part, counts, frames, beta, coef=None, final_res=None):
        self.part, self.counts, self.frames, self.beta = part, counts, frames, beta
        self.coef = 1.0 + beta if coef is None else coef
        self.final_res = final_res

    @property
    def stage_frames(self):
        return self.counts.reshape(-1, self.counts.shape[-1]).sum(dim=1)

    @property
    def stage_mse_active(self):
        n = self.stage_frames.to(torch.float32)
        return torch.where(n > 0, self.stage_mse * float(self.frames) / n.clamp_min(1.0), torch.zeros_like(n))

    @property
    def stage_mse(self):
        return self.part.reshape(-1, self.part.shape[-1]).sum(dim=1)

    @property
    def stage_perplexity(self):
        if self.final_res is not None:                        # quantiser dropout: every stage over the frames it saw
            p = self.counts.to(torch.float64) / self.stage_frames.clamp_min(1).to(torch.float64)[:, None]
            return torch.exp(-(p * torch.log(p.clamp_min(1e-300))).sum(dim=1)).float()
        p = self.counts.reshape(-1, self.counts.shape[-1]).to(torch.float64) / self.frames
        return torch.exp(-(p * torch.log(p.clamp_min(1e-300))).sum(dim=1)).float()

    @property
    def stage_codes_used(self):
        return (self.counts.reshape(-1, self.counts.shape[-1]) > 0).sum(dim=1)

    @property
    def mse(self):
        if self.final_res is not None:
            return self.final_res.square().sum() / self.final_res.numel()
        return self.part.sum() if self.part.dim() == 1 else self.part[-1].sum()

    @property
    def vq_loss(self):
        return self.part.sum() * self.coef

    @property
    def perplexity(self):
        p = (self.counts if self.counts.dim() == 1 else self.counts[0]).to(torch.float64) / self.frames
        return torch.exp(-(p * torch.log(p.clamp_min(1e-300))).sum()).float()

    @property
    def codes_used(self):
        return ((self.counts if self.counts.dim() == 1 else self.counts[0]) > 0).sum()


class EngineBase:
    """Host state and the steps every engine runs the same way.  An engine sets `device`, `Q`, `spec`, `flat`, `flat_grad`, calls
    _init_state(), and provides _make_workspace(), _bwd_workspace() and backward_from_dlogits()."""

    # the loss of loss_and_grad(..., objective=None): "reference" = chunk softmax + CrossEntropyLoss on the probabilities, as the
    # reference trains; "nll" = the negative log-likelihood under the per-timestep softmax the decoder samples from
    objective = "reference"
    # the position windows of the "nll" objective: None, or 1..16 (lo, hi) pairs (NllWindows) - step_nll, score_logits, step_probs
    # and the fused step then run wn_win_step_nll / wn_win_step_softmax, the softmax of a column taken inside its position's pair
    nll_windows = None

    # ------------------------------------------------------------------ parameters (the WaveNet engines': reference state_dict order)
    def _build_spec(self):
        """The flat layout of a WaveNet with filter width self.k, and the zeroed flat parameter / gradient buffers."""
        k = self.k
        names = [("causal_layer.weight", (self.R, self.Q, k))]
        if self.use_bias:
            names.append(("causal_layer.bias", (self.R,)))
        for i in range(self.N):
            for j, shp in enumerate([(self.D, self.R, k), (self.D, self.R, k), (self.R, self.D, 1), (self.S, self.D, 1)]):
                names.append(("dilation_layer_stack.%d.weight" % (4 * i + j), shp))
                if self.use_bias:
                    names.append(("dilation_layer_stack.%d.bias" % (4 * i + j), (shp[0],)))
        names.append(("post_process_1.weight", (self.S, self.S, 1)))
        if self.use_bias:
            names.append(("post_process_1.bias", (self.S,)))
        names.append(("post_process_2.weight", (self.Q, self.S, 1)))
        if self.use_bias:
            names.append(("post_process_2.bias", (self.Q,)))
        names += self.gclass_names(self.N, self.D, self.S, self.g_n, self.g_E)       # (class-conditional: the global block, last)
        names += self.phase_names(self.N, self.D, self.S, getattr(self, "phase", 0))  # (phase-conditioned: the N + 1 tables behind it)
        self.spec = _Spec(names)
        self.param_names = [n for n, _ in names]
        self._plan_phase(getattr(self, "phase", 0))
        self._plan_gclass(self.g_n, self.g_E)
        self.flat = torch.zeros(self.spec.total, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros(self.spec.total, dtype=torch.float32, device=self.device)

    def param_view(self, name, grad=False):
        o, shp = self.spec.off[name], self.spec.shape[name]
        n = int(np.prod(shp))
        return (self.flat_grad if grad else self.flat)[o:o + n].view(shp)

    def load_state_dict_tensors(self, sd):
        with torch.no_grad():
            for n in self.param_names:
                self.param_view(n).copy_(sd[n])

    def _init_state(self):
        self._ws = WorkspacePool(self._make_workspace)
        self._gen = 0
        self.adam_state = None
        self.marks = None            # list of (name, torch.cuda.Event) when profiling is on
        self.mark_only = None        # optional set of mark names to keep
        self._throttle = _lib.StepThrottle()   # at most WN_MAX_STEPS_IN_FLIGHT fused steps in flight
        # weight-gradient launches that only feed the final slab reduction run on a second HIP stream (on_side): their half-empty
        # last rounds of workgroups pack into the data-gradient launches beside them
        self._side = None
        self.overlap_wgrad = True

    def mark(self, name):
        """Record a timing event on the current stream (only when self.marks is a list; self.mark_only, if set, limits
        the events to those names - every event costs a marker packet between two kernels)."""
        if self.marks is not None and (self.mark_only is None or name in self.mark_only):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def workspace(self, B, T):
        """The workspace the last forward of this shape used (what callers inspect after a step; WorkspacePool.peek).  A
        forward takes its own through WorkspacePool.get: the first one no pending backward holds."""
        return self._ws.peek(B, T)

    def act_buf(self, B, rows, pitch):
        """A zeroed [clip][rows][pitch] activation buffer between its SLACK and PAD_BACK floats."""
        return torch.zeros(SLACK + B * rows * pitch + PAD_BACK, dtype=torch.float32, device=self.device)

    def _gemm(self, st, B, mode, wpack, in0, in1, in_bs, in_pitch, in_lo, in_hi, s0, s1, ks0, ks1, mt, m_valid, out, out_bs,
              out_pitch, out_shift, bias, resid, mask, t_lo, t_hi, relu_in):
        """wn_chan_gemm with `resid` (pointer, clip stride, pitch[, first valid column]) and `mask` (pointer, clip stride, pitch) as tuples"""
        call("wn_chan_gemm", in0, in1, in_bs, in_pitch, in_lo, in_hi, s0, s1, ks0, ks1, wpack, mt, m_valid,
             out, out_bs, out_pitch, out_shift, bias, resid[0], resid[1], resid[2], resid[3] if len(resid) > 3 else 0,
             mask[0], mask[1], mask[2], t_lo, t_hi, relu_in, B, mode, st)

    def _check_input_unchanged(self, ws):
        """The dense input must still be what the forward saw: in-place writes that bump the version counter are caught here
        (autograd's own rule for saved tensors); writes that do not (x.data.zero_(), a raw-pointer kernel) cannot be."""
        if ws.get("x_ver") is not None and ws["x_in"]._version != ws["x_ver"]:
            raise RuntimeError("music_amd: the input of this forward was modified in place before backward()")

    # ------------------------------------------------------------------ learned conditioning projections (the autoencoder's engines)
    learned = False              # net.conditioning == "learned": the N + 1 projections are parameters at the END of the flat buffer
    n_cond = 0                   # their floats: wn_cond_proj_bwd writes that tail of flat_grad, the gather everything in front of it

    vq = False                   # net.bottleneck == "vq": the codebook (K, Bw) is the LAST parameter of the flat buffer, behind the projections
    n_vq = 0                     # its floats: wn_vq_bwd writes that tail of flat_grad
    last_vq = None               # VqStats of the last forward (vq only)
    vq_S = 1                     # net.vq_stages: S > 1 = a residual chain, the codebook is (S K, Bw) and the wn_rvq_* entries run it
    vq_ema = False               # net.vq_update == "ema": wn_vq_bwd_stats in place of wn_vq_bwd, wn_vq_ema_update behind the optimizer
    gcond = False                # net.global_classes > 0: the global block [G_0 .. G_N-1 | G_f | embedding] ends the flat buffer, behind the codebook
    n_gcond = 0                  # its floats: wn_gcond_proj_bwd writes that tail of flat_grad (and the projections' in front of the codebook)
    phase = 0                    # net.phase_period (the WaveNet engines): the N + 1 phase tables end the flat buffer, behind the global block
    n_phase = 0                  # their floats: wn_phase_tab_bwd writes that tail of flat_grad

    @property
    def n_gather(self):
        """Leading elements of flat_grad that the gather of the gradient pack fills."""
        return self.spec.total - self.n_cond - self.n_vq - self.n_gcond - self.n_phase

    @property
    def gathered_param_names(self):
        """The parameters whose gradients come out of the gradient pack: all but the learned projections' 2 (N + 1), the codebook,
        the global block's N + 2 and the phase tables' N + 1, the last ones."""
        N = len(self.dil)
        return self.param_names[:len(self.param_names) - (2 * (N + 1) if self.learned else 0) - (1 if self.vq else 0)
                                - (N + 2 if self.gcond else 0) - (N + 1 if self.phase else 0)]

    def _plan_cond(self, net):
        """Learned mode: where wn_cond_proj_fwd / wn_cond_proj_bwd find the projections in the flat buffers; the vq bottleneck's
        codebook behind them, the global class conditioning's block behind that: the tail of flat / flat_grad is
        [projections | codebook | global block]."""
        self.learned = getattr(net, "conditioning", "random") == "learned"
        self.vq = getattr(net, "bottleneck", "continuous") == "vq"
        self.gcond = int(getattr(net, "global_classes", 0)) > 0
        if self.gcond:
            if not self.learned:
                raise ValueError('music_amd: global_classes > 0 requires conditioning="learned"')
            o, N = self.spec.off, len(self.dil)
            E, n = self.g_E, self.g_n = int(net.global_channels), int(net.global_classes)
            gw0, gwf, emb = o["de_gcond_layer_stack.0.weight"], o["connection_gcond.weight"], o["global_embedding.weight"]
            gstride = 2 * self.Dd * E
            # registered last, in stage order: one constant stage stride, the final stage's G and the embedding behind the stages'
            assert all(o["de_gcond_layer_stack.%d.weight" % i] == gw0 + i * gstride for i in range(N)) and gwf == gw0 + N * gstride \
                and emb == gwf + self.Sd * E and emb + n * E == self.spec.total
            self.gcond_off = (gw0, gstride, gwf, emb)
            self.n_gcond = self.spec.total - gw0
        if self.vq:
            if not self.learned:
                raise ValueError('music_amd: bottleneck="vq" requires conditioning="learned"')
            S = self.vq_S = int(getattr(net, "vq_stages", 1))
            self.vq_K, self.vq_beta = int(net.vq_codebook.num_embeddings) // S, float(net.vq_beta)
            self.vq_off = self.spec.off["vq_codebook.weight"]
            self.n_vq = S * self.vq_K * self.Bw
            assert self.spec.shape["vq_codebook.weight"] == (S * self.vq_K, self.Bw) and self.vq_off + self.n_vq == self.spec.total - self.n_gcond
            self.vq_ema = getattr(net, "vq_update", "gradient") == "ema"
            if self.vq_ema:
                # [n | s] of the last backward, the update's scratch and its restart counters; the running state is the MODULE's buffer
                self.vq_decay, self.vq_eps, self.vq_restart = float(net.vq_decay), float(net.vq_eps), float(net.vq_restart)
                # (one block of each per stage, the stats of all stages in ONE tensor: a data-parallel run reduces it in one call)
                self.vq_stat = torch.zeros(S * self.vq_K * (self.Bw + 1), dtype=torch.float32, device=self.device)
                self.vq_ema_work = torch.zeros(S * _lib.VQ_EMA_WORK_BYTES // 4, dtype=torch.int32, device=self.device)
                self.vq_ema_info = torch.zeros(2 * S, dtype=torch.int32, device=self.device)
                self._vq_net = weakref.ref(net)
        if not self.learned:
            return
        o, N = self.spec.off, len(self.dil)
        w0, b0 = o["de_cond_layer_stack.0.weight"], o["de_cond_layer_stack.0.bias"]
        stride = 2 * self.Dd * self.Bw + 2 * self.Dd
        wf, bf = o["connection_cond.weight"], o["connection_cond.bias"]
        # registered last (the codebook and the global block alone behind them), in stage order (weight, bias per stage): one constant stage stride
        assert all(o["de_cond_layer_stack.%d.weight" % i] == w0 + i * stride and o["de_cond_layer_stack.%d.bias" % i] == b0 + i * stride
                   for i in range(N)) and wf == w0 + N * stride and bf + self.Sd == self.spec.total - self.n_vq - self.n_gcond
        self.cond_off = (w0, b0, stride, wf, bf)
        self.n_cond = self.spec.total - self.n_vq - self.n_gcond - w0

    # ------------------------------------------------------------------ vector-quantised bottleneck (the autoencoder's engines)
    def vq_stage_counts(self, stages, B):
        """`stages` of forward / loss_and_grad -> None (the launches without dropout) or the clips' stage counts as (B,) int32 on the
        device (music_amd/vq_dropout.py: stage_counts validates on the host, a ValueError before any launch)."""
        n = vq_dropout.stage_counts(stages, B, self.vq_S if self.vq else 1)
        return None if n is None else torch.from_numpy(n).to(self.device, non_blocking=True)      # (ONE small copy per step, as stage_classes')

    def vq_fwd(self, ws, enc, st, nstage=None):
        """The pooled encoding e (B, Bw, Le) -> q, every frame its nearest codebook row (wn_vq_fwd, one launch); ws keeps enc_pre = e,
        vq_idx, vq_counts and the loss partials (fresh tensors per forward: the module hands them out), self.last_vq reads them.
        nstage (vq_stage_counts; S > 1 only): quantiser dropout, clip b takes part in its first nstage[b] stages (wn_rvq_fwd_n, still
        one launch); ws keeps it for the backward, vq_idx holds -1 where a clip took no part."""
        B, _, Le = enc.shape
        dev = self.device
        # S > 1: the residual chain, still one launch: idx (S, B, Le), counts (S, K), the loss partials per stage, and res[s] = what
        # stage s left over, which the backward reads.  S = 1: the one-stage entry, no stage axis, no res, no stage counts
        S, chain = self.vq_S, self.vq_S > 1
        lead = (S,) if chain else ()
        nstage = nstage if chain else None
        q = torch.empty_like(enc)
        idx = torch.empty(lead + (B, Le), dtype=torch.int32, device=dev)
        counts = torch.empty(lead + (self.vq_K,), dtype=torch.int32, device=dev)
        part = torch.empty(lead + (_lib.VQ_NUM_PARTIALS,), dtype=torch.float32, device=dev)
        res = torch.empty(lead + tuple(enc.shape), dtype=torch.float32, device=dev) if chain else None
        call("wn_vq_fwd" if not chain else "wn_rvq_fwd" if nstage is None else "wn_rvq_fwd_n",
             ptr(enc), ptr(self.flat), self.vq_off, *([ptr(nstage)] if nstage is not None else []), ptr(q), ptr(idx), ptr(counts),
             *([ptr(res)] if chain else []), ptr(part), *([S] if chain else []), self.vq_K, self.Bw, Le, B, st)
        ws.update(enc_pre=enc, vq_idx=idx, vq_counts=counts, vq_part=part, vq_g=1.0, **(dict(vq_res=res, vq_nstage=nstage) if chain else {}))
        self.last_vq = VqStats(part, counts, B * Le, self.vq_beta, self.vq_loss_coef, final_res=None if nstage is None else res[S - 1])
        return q

    def vq_bwd(self, ws, d_q, st):
        """d_q (what wn_cond_proj_bwd wrote as d enc) -> d e in place, and the codebook's gradient into the tail of flat_grad (wn_vq_bwd,
        one launch); ws["vq_g"]: the upstream scalar on vq_loss (1 in the fused step, autograd's in the module's backward)."""
        B, _, Le = d_q.shape
        # a chain hands over res and S; a forward that ran with stage counts the counts: the same launch over the ACTIVE stages of every
        # frame (idx = -1 matches no code); EMA mode: the same d e, the frames' counts and sums per code into vq_stat, zeros as the
        # codebook's gradient
        chain = self.vq_S > 1
        nstage = ws.get("vq_nstage") if chain else None
        call(("wn_rvq_bwd" if chain else "wn_vq_bwd") + ("_stats" if self.vq_ema else "") + ("_n" if nstage is not None else ""),
             ptr(ws["enc_pre"]), ptr(ws["vq_idx"]), *([ptr(ws["vq_res"])] if chain else []), *([ptr(nstage)] if nstage is not None else []),
             ptr(d_q), ptr(self.flat), self.vq_off, self.vq_beta, float(ws.get("vq_g", 1.0)), ptr(d_q), ptr(self.flat_grad),
             *([ptr(self.vq_stat)] if self.vq_ema else []), *([self.vq_S] if chain else []), self.vq_K, self.Bw, Le, B, st)

    @property
    def vq_loss_coef(self):
        """vq_loss / mse: codebook term + beta x commitment term; the commitment term alone where the codebook follows its frames' mean."""
        return self.vq_beta if self.vq_ema else 1.0 + self.vq_beta

    def vq_codes_of(self, ws):
        """The codes of a forward's workspace as the module hands them out: (B, Le) int64, (B, S, Le) with S > 1 stages - with -1
        where a forward with stage counts left a clip out of a stage, as they are."""
        idx = ws["vq_idx"].to(torch.int64)
        return idx if self.vq_S == 1 else idx.permute(1, 0, 2)

    def vq_ema_state(self):
        """The module's running state [N | m] (its `vq_ema_state` buffer, which checkpoints carry), on this engine's device."""
        net = self._vq_net()
        state = None if net is None else getattr(net, "vq_ema_state", None)
        if state is None or state.device != self.flat.device or state.dtype != torch.float32 or state.numel() != self.vq_stat.numel():
            raise RuntimeError("music_amd: the model's vq_ema_state buffer is gone, or not where its parameters are")
        return state

    def vq_ema_step(self, guard=None):
        """wn_vq_ema_update (two launches) on the stats of the last backward: the module's running state and the codebook's rows of
        the flat buffer, in place.  Behind the optimizer's update - which leaves those rows alone, their gradient being 0 - and in
        front of the EMA shadow's.  `guard`: the GradGuard that decided the step; a skipped step changes nothing."""
        chain = self.vq_S > 1               # every stage on its own block of stat, state, work and info; still two launches
        call("wn_rvq_ema_update" if chain else "wn_vq_ema_update", ptr(self.flat), self.vq_off, ptr(self.vq_stat), ptr(self.vq_ema_state()),
             ptr(self.vq_ema_work), ptr(self.vq_ema_info), *([self.vq_S] if chain else []), self.vq_K, self.Bw, self.vq_decay, self.vq_eps,
             self.vq_restart, None if guard is None else guard.state_ptr(), _lib.stream())

    def vq_restarted(self):
        """Codes restarted since the last call (reads the device's counter back and zeroes it)."""
        n = int(self.vq_ema_info[0::2].sum().item())                   # (info is [S][2]: the stages' counters)
        self.vq_ema_info[0::2] = 0
        return n

    def vq_backward_scaled(self, ws, dloss, dvq):
        """backward_from_dlogits of a vq model for upstream gradients `dloss` (0-d device tensor or None) on the reconstruction loss whose
        d loss / d logits the workspace holds, and `dvq` (likewise) on vq_loss.  The backward is not linear in dloss alone, so
        d loss / d logits is scaled (and restored behind the backward) rather than the result; dvq reaches wn_vq_bwd as a host float -
        one read-back, only where vq_loss is part of the loss."""
        ws["vq_g"] = 0.0 if dvq is None else float(dvq)
        d_o = self._bwd_workspace(ws)["dO"][:ws["B"] * ws["W"] * self.Q]
        keep = d_o.clone()
        if dloss is None:
            d_o.zero_()
        else:
            d_o.mul_(dloss)
        self.backward_from_dlogits(ws)
        d_o.copy_(keep)

    def vq_lookup(self, codes):
        """codes (B, Le) integer -> q (B, Bw, Le) out of the codebook (wn_vq_lookup); a code outside [0, K) raises.  With S > 1 stages:
        codes (B, n, Le), 1 <= n <= S, the first n stages' codes -> the sum of their rows in stage order (wn_rvq_lookup).  Codes with
        -1 in a clip's absent stages (what a forward with stage counts hands out; vq_dropout.counts_of_codes checks the pattern on the
        host) -> every clip the sum of ITS stages' rows (wn_rvq_lookup_n)."""
        S, chain, dev = self.vq_S, self.vq_S > 1, self.device
        nstage = None
        if chain:
            if codes.dim() != 3 or not 1 <= codes.shape[1] <= S:
                raise ValueError("music_amd: vq_stages = %d: codes must be (B, n, Le) with 1 <= n <= %d, not %s" % (S, S, tuple(codes.shape)))
            nstage = None if codes.is_floating_point() else vq_dropout.counts_of_codes(codes, S)
        elif codes.dim() != 2:
            raise ValueError("music_amd: codes must be (B, Le), not %s" % (tuple(codes.shape),))
        idx = codes.to(device=dev, dtype=torch.int32)
        if chain:
            idx = idx.permute(1, 0, 2)                                     # (n, B, Le): the stage in front, as the forward's vq_idx
        n = idx.shape[0] if chain else 1
        if nstage is not None:                                             # all S stages, -1 behind the n given ones
            full = torch.full((S,) + tuple(idx.shape[1:]), -1, dtype=torch.int32, device=dev)
            full[:n] = idx
            idx, nstage = full, torch.from_numpy(nstage).to(dev)
        idx = idx.contiguous()
        B, Le = idx.shape[-2:]
        q = torch.empty(B, self.Bw, Le, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        call("wn_vq_lookup" if not chain else "wn_rvq_lookup" if nstage is None else "wn_rvq_lookup_n",
             ptr(idx), *([ptr(nstage)] if nstage is not None else []), ptr(self.flat), self.vq_off, ptr(q), ptr(bad), *([S] if chain else []),
             *([n] if chain and nstage is None else []), self.vq_K, self.Bw, Le, B, _lib.stream())
        if int(bad.item()):
            raise ValueError("music_amd: a code lies outside [0, %d)" % self.vq_K)
        return q

    def _check_cond(self, cond):
        """`cond` of forward / loss_and_grad: the drawn projections in random mode, None in learned mode - nothing is ignored silently."""
        if self.learned and cond is not None:
            raise ValueError('music_amd: conditioning="learned": the projections are the model\'s parameters, pass cond=None')
        if not self.learned and cond is None:
            raise ValueError('music_amd: conditioning="random": pass the drawn projections (net.conditioning_projections()) as cond')

    def stage_classes(self, classes, B):
        """`classes` of forward / loss_and_grad -> what the workspace keeps as ws["cls"]: None with the mode off (a given vector is
        refused), else the (B,) int32 class vector on the device - ONE copy per step; values that are still on the host are checked
        against [0, n) here, before anything is launched (a device tensor's are the kernel's to turn into NaN)."""
        if not self.gcond:
            if classes is not None:
                raise ValueError("music_amd: global_classes is 0: this model takes no classes, pass classes=None")
            return None
        if classes is None:
            raise ValueError("music_amd: global_classes = %d: pass classes, one integer in [0, %d) per clip" % (self.g_n, self.g_n))
        cls = classes if torch.is_tensor(classes) else torch.as_tensor(list(classes))
        if cls.dim() != 1 or cls.numel() != B or cls.is_floating_point() or cls.is_complex() or cls.dtype == torch.bool:
            raise ValueError("music_amd: classes must be %d integers, one per clip, not %s of shape %s" % (B, cls.dtype, tuple(cls.shape)))
        if cls.device.type == "cpu" and B and not (0 <= int(cls.min()) and int(cls.max()) < self.g_n):
            raise ValueError("music_amd: a class lies outside [0, %d) (global_classes)" % self.g_n)
        return cls.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()

    def _gcond_args(self, cls):
        return (ptr(cls),) + self.gcond_off + (self.g_E, self.g_n)

    def cond_proj_fwd(self, enc, tab, tab_pair, enf, ch, st, cls=None):
        """All N + 1 projections of enc (B, Bw, Le) out of the flat buffer in one launch: the block tables (per clip and / or as clip
        pairs, padding rows included) and the final table enf (B, Sd, Le); with global class conditioning plus every clip's
        G emb[cls[b]] (wn_gcond_proj_fwd, `cls` = stage_classes' vector)."""
        B, _, Le = enc.shape
        args = (ptr(enc), ptr(self.flat)) + self.cond_off + (ptr(tab), ptr(tab_pair), ptr(enf), len(self.dil), self.Dd, ch, self.Sd, self.Bw,
                                                            Le, B)
        if self.gcond:
            return call("wn_gcond_proj_fwd", *args, *self._gcond_args(cls), st)
        call("wn_cond_proj_fwd", *args, st)

    def cond_proj_bwd(self, d_tab, pair, d_enf, enc, d_enc, ch, st, cls=None):
        """d enc and the projections' own gradients (into the tail of flat_grad) from the block tables' and the final table's gradients;
        with global class conditioning the global block's too (wn_gcond_proj_bwd)."""
        B, _, Le = enc.shape
        args = (ptr(d_tab), 1 if pair else 0, ptr(d_enf), ptr(enc), ptr(self.flat)) + self.cond_off + (
            ptr(d_enc), ptr(self.flat_grad), len(self.dil), self.Dd, ch, self.Sd, self.Bw, Le, B)
        if self.gcond:
            return call("wn_gcond_proj_bwd", *args, *self._gcond_args(cls), st)
        call("wn_cond_proj_bwd", *args, st)

    # ------------------------------------------------------------------ class-conditional WaveNet (the two WaveNet engines)
    @staticmethod
    def gclass_names(N, D, S, n, E):
        """(name, shape) of the global block of a class-conditional WaveNet, in the order it ends the flat buffer"""
        return ([("gcond_layer_stack.%d.weight" % i, (2 * D, E, 1)) for i in range(N)] + [("connection_gcond.weight", (S, E, 1))] +
                [("global_embedding.weight", (n, E))]) if n > 0 else []

    def _plan_gclass(self, n, E):
        """Where wn_gclass_fwd / wn_gclass_bwd find G_i (2 D x E, gate rows first), G_f (S x E) and the embedding (n x E): the tail
        of flat / flat_grad, behind everything the model has without them (self.D, self.S: the engine's channel counts)."""
        self.gcond = n > 0
        if not self.gcond:
            return
        o, N = self.spec.off, len(self.dil)
        self.g_E, self.g_n = E, n
        n_phase = getattr(self, "n_phase", 0)                 # (the phase tables, behind the global block)
        gw0, gwf, emb = o["gcond_layer_stack.0.weight"], o["connection_gcond.weight"], o["global_embedding.weight"]
        gstride = 2 * self.D * E
        assert all(o["gcond_layer_stack.%d.weight" % i] == gw0 + i * gstride for i in range(N)) and gwf == gw0 + N * gstride \
            and emb == gwf + self.S * E and emb + n * E == self.spec.total - n_phase
        self.gcond_off = (gw0, gstride, gwf, emb)
        self.n_gcond = self.spec.total - n_phase - gw0

    def gclass_fwd(self, cls, tab, tab_pair, enf, ch, st):
        """Every block's table (per clip and / or as clip pairs, padding rows included; one column per clip) and the output stage's
        enf (B, S) of the clips' classes, in one launch"""
        call("wn_gclass_fwd", ptr(self.flat), ptr(tab), ptr(tab_pair), ptr(enf), len(self.dil), self.D, ch, self.S, cls.numel(),
             *self._gcond_args(cls), st)

    def gclass_bwd(self, cls, d_tab, pair, d_enf, ch, st):
        """dG_i, dG_f and every row of d emb into the tail of flat_grad, from the tables' gradients"""
        call("wn_gclass_bwd", ptr(d_tab), 1 if pair else 0, ptr(d_enf), ptr(self.flat), ptr(self.flat_grad), len(self.dil), self.D, ch,
             self.S, cls.numel(), *self._gcond_args(cls), st)

    # ------------------------------------------------------------------ phase-conditioned WaveNet (the two WaveNet engines)
    @staticmethod
    def phase_names(N, D, S, P):
        """(name, shape) of the phase tables of a phase-conditioned WaveNet, in the order they end the flat buffer"""
        return ([("phase_layer_stack.%d" % i, (2 * D, P)) for i in range(N)] + [("connection_phase", (S, P))]) if P > 0 else []

    def _plan_phase(self, P):
        """Where wn_phase_tab_fwd / wn_phase_tab_bwd find T_i (2 D x P, gate rows first) and T_f (S x P): the tail of flat / flat_grad,
        behind the global block; and the stages' rotations.  Output column c of a clip whose first target sits at stream position
        pos predicts position pos + c and sits at absolute time rf - 1 + c; block i's table is read at frame (t - t_lo_i) mod P, so its
        frame l is the parameter's column (l + pos + t_lo_i - (rf - 1)) mod P: rot[i] = (off[i + 1] - (rf - 1)) mod P, 0 for the
        output stage, whose table is expanded from rf - 1."""
        self.phase = int(P)
        if not self.phase:
            return
        o, N = self.spec.off, len(self.dil)
        pw0, pwf = o["phase_layer_stack.0"], o["connection_phase"]
        pstride = 2 * self.D * P
        assert all(o["phase_layer_stack.%d" % i] == pw0 + i * pstride for i in range(N)) and pwf == pw0 + N * pstride \
            and pwf + self.S * P == self.spec.total
        self.phase_off = (pw0, pstride, pwf)
        self.n_phase = self.spec.total - pw0
        self.phase_rot = torch.tensor([(self.off[i + 1] - (self.rf - 1)) % P for i in range(N)] + [0], dtype=torch.int32, device=self.device)

    def stage_phase(self, phase_pos, B):
        """`phase_pos` of forward / loss_and_grad -> what the workspace keeps as ws["pos"]: None with the mode off (a given value is
        refused), else the (B,) int64 vector of the clips' stream positions on the device - ONE copy per step.  One int for all clips,
        one per clip, or a device tensor; values still on the host are checked here, before anything is launched (a device tensor's
        negative entries are the kernel's to turn into NaN)."""
        if not self.phase:
            if phase_pos is not None:
                raise ValueError("music_amd: phase_period is 0: this model takes no phase_pos, pass phase_pos=None")
            return None
        if phase_pos is None:
            raise ValueError("music_amd: phase_period = %d: pass phase_pos, the stream position of every clip's first target "
                             "(one integer >= 0 per clip)" % self.phase)
        if isinstance(phase_pos, (int, np.integer)) and not isinstance(phase_pos, bool):
            phase_pos = [int(phase_pos)] * B
        pos = phase_pos if torch.is_tensor(phase_pos) else torch.as_tensor(list(phase_pos))
        if pos.dim() != 1 or pos.numel() != B or pos.is_floating_point() or pos.is_complex() or pos.dtype == torch.bool:
            raise ValueError("music_amd: phase_pos must be %d integers, one per clip, not %s of shape %s" % (B, pos.dtype, tuple(pos.shape)))
        if pos.device.type == "cpu" and B and int(pos.min()) < 0:
            raise ValueError("music_amd: a phase_pos is negative (%d): stream positions are >= 0" % int(pos.min()))
        return pos.to(device=self.device, dtype=torch.int64, non_blocking=True).contiguous()

    def phase_fwd(self, pos, tab, tab_pair, enf, ch, st, add=(None, None, None), rot=None):
        """Every block's table of P frames (per clip and / or as clip pairs, padding rows included) and the output stage's enf
        (B, S, P) of the clips' positions, in one launch; add = wn_gclass_fwd's (tab, tab_pair, enf): the class term, added per frame;
        rot: the stages' rotations (default: the forward's, self.phase_rot; the decoder's tables take zeros)"""
        call("wn_phase_tab_fwd", ptr(self.flat), *self.phase_off, ptr(pos), ptr(self.phase_rot if rot is None else rot), *(ptr(a) for a in add), ptr(tab),
             ptr(tab_pair), ptr(enf), len(self.dil), self.D, ch, self.S, self.phase, pos.numel(), st)

    def phase_bwd(self, pos, d_tab, pair, d_enf, ch, st, sums=(None, None)):
        """dT_i and dT_f into the tail of flat_grad, from the tables' gradients; sums = (sum_tab, sum_enf): their sums over the
        frames, what wn_gclass_bwd takes as the class term's gradients"""
        call("wn_phase_tab_bwd", ptr(d_tab), 1 if pair else 0, ptr(d_enf), ptr(self.flat_grad), *self.phase_off, ptr(pos),
             ptr(self.phase_rot), *(ptr(a) for a in sums), len(self.dil), self.D, ch, self.S, self.phase, pos.numel(), st)

    # ------------------------------------------------------------------ the second stream
    def _side_stream(self):
        """THE side stream of this device (_lib.side_stream: high priority = a hardware queue of its own), created at first use."""
        if self._side is None:
            self._side = _lib.side_stream(self.device)
        return self._side

    def on_side(self, fn):
        """fn(stream) on the side stream, behind everything enqueued so far on the main stream; overlap_wgrad off: on the main stream."""
        if not self.overlap_wgrad:
            return fn(_lib.stream())
        side, ev = self._side_stream(), torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        side.wait_event(ev)
        with torch.cuda.stream(side):
            fn(_lib.stream())

    def join_side(self):
        """The main stream waits for everything enqueued so far on the side stream."""
        if self.overlap_wgrad:
            ev = torch.cuda.Event()
            ev.record(self._side_stream())
            torch.cuda.current_stream().wait_event(ev)

    # ------------------------------------------------------------------ weight gradients: slabs, reduction, gather
    def wgrad(self, bw, B, mode, st, name, *args):
        """wn_wgrad into the slabs of op `name` of bw["plan"]; args = everything of wn_wgrad up to and including relu_b, then ldc, t_lo, t_hi"""
        op = bw["plan"][name]
        head, (ldc, t_lo, t_hi) = args[:-3], args[-3:]
        call("wn_wgrad", *head, ptr(bw["slab"], op.so), ldc, op.n, t_lo, t_hi, op.chunk, B, mode, st)

    def wgrad_s(self, bw, B, mode, name, *args):
        """... on the side stream, as soon as its operands exist"""
        self.on_side(lambda s2: self.wgrad(bw, B, mode, s2, name, *args))

    def reduce_and_gather(self, bw, from_codes, st):
        """slabs -> gradient pack (one batched sum in a fixed order; the second table where a causal layer's gradient came from codes) ->
        flat_grad (pair mode: a stack weight's gradient is the sum of its two copies in the block-diagonal matrix)"""
        call("wn_reduce_slabs", ptr(bw["desc_codes"] if from_codes else bw["desc"]), bw["nops"], bw["vec"], ptr(bw["slab"]), ptr(self.gpack), st)
        if bw["pair"]:
            call("wn_gather_grads2", ptr(self.gpack), ptr(self.gidx_pa), ptr(self.gidx_pb), ptr(self.flat_grad), self.n_gather, st)
        else:
            call("wn_gather_grads", ptr(self.gpack), ptr(self.gidx), ptr(self.flat_grad), self.n_gather, st)

    # ------------------------------------------------------------------ the causal layer(s): from integer codes, else dense
    @staticmethod
    def tagged_codes(x, B, T):
        """(codes, scrambled) of a one-hot that onehot() / the loader built from integer codes and that still is what it was then (the
        tensor and the codes are immutable while tagged: an in-place op that bumps a version counter drops the tag's fast path), else None"""
        tag = getattr(x, "_wn_codes", None) if x is not None else None
        if tag is not None:
            codes, scrambled, version, cversion = tag
            if (x._version == version and codes._version == cversion and codes.is_cuda and codes.dtype == torch.int32 and
                    codes.is_contiguous() and tuple(codes.shape) == (B, T)):
                return codes, scrambled
        return None

    def causal_fwd(self, ws, x, wt_idx, wt, wpack, bias, R, CH, out, st, mode):
        """x0[t] = W0 in[t-1] + W1 in[t] on [1, T): a gather of weight columns where the input is the one-hot of known codes
        (ws["x_codes"]; the dense tensor is not read), else the channel product over the dense input"""
        B, T, pitch, Q = ws["B"], ws["T"], ws["pitch"], self.Q
        if ws["x_codes"] is None:
            return call("wn_chan_gemm", ptr(x), ptr(x), Q * T, T, 0, T, -1, 0, Q // 32, Q // 32, wpack, CH // 16, R, out, CH * pitch, pitch, 0, bias,
                        None, 0, 0, 0, None, 0, 0, 1, T, 0, B, mode, st)
        codes, scrambled = ws["x_codes"]
        call("wn_gather_grads", ptr(self.flat), ptr(wt_idx), ptr(wt), wt.numel(), st)
        call("wn_causal_fwd_codes", ptr(codes), 1 if scrambled else 0, ptr(wt), bias, R, out, CH * pitch, pitch, CH, Q, T, B, st)

    def codes_for_backward(self, ws):
        """ws["x_codes"] if the codes are still what the forward saw (where it noted their version); changed codes beside an intact dense
        input: None, the dense weight-gradient product"""
        x_codes, cv = ws.get("x_codes"), ws.get("codes_ver")
        if x_codes is not None and cv is not None and x_codes[0]._version != cv:
            if ws["x_in"] is None:
                raise RuntimeError("music_amd: the integer codes of this forward were modified in place before backward()")
            return None
        return x_codes

    def causal_wgrad(self, ws, bw, x_codes, name, dx0, CH, st, mode):
        """dWc[r][q][tap] = sum dx0[r][t] in[q][t-1+tap] into the slabs of `name`: a scatter from the codes (slabs `name`_codes), else dense"""
        B, T, pitch, Q, x = ws["B"], ws["T"], ws["pitch"], self.Q, ws["x_in"]
        if x_codes is not None:
            return call("wn_causal_wgrad_codes", ptr(x_codes[0]), 1 if x_codes[1] else 0, dx0, None, 0, 0, CH * pitch, pitch, CH, Q, T, B,
                        ptr(bw["slab"], bw["plan"][name + "_codes"].so), st)
        self.wgrad(bw, B, mode, st, name, dx0, CH * pitch, pitch, 0, pitch, ptr(x), ptr(x), Q * T, T, -1, 0, T, Q // 16, CH // 16, 0, 2 * Q, 1, T)

    def causal_input_grad(self, ws, dx0, CH, wpackT, mode):
        """din[q][s] = sum_r W[r][q][1] dx0[r][s] + W[r][q][0] dx0[r][s + 1], dx0 (the first block's data gradient, which the backward
        leaves in its workspace) living on [1, T): one channel product with the transposed causal weight"""
        B, T, pitch, Q = ws["B"], ws["T"], ws["pitch"], self.Q
        din = torch.empty(B, Q, T, dtype=torch.float32, device=self.device)
        dx0 = ptr(dx0, SLACK)
        call("wn_chan_gemm", dx0, dx0, CH * pitch, pitch, 1, T, 0, 1, CH // 32, CH // 32, wpackT, Q // 16, Q,
             ptr(din), Q * T, T, 0, None, None, 0, 0, 0, None, 0, 0, 0, T, 0, B, mode, _lib.stream())
        return din

    # ------------------------------------------------------------------ fused training step
    def softmax_ce(self, logits, target, probs, dlogits, loss_part, n):
        """loss partials and d loss / d logits of the MEAN cross entropy over n rows of 256 (probs None: not wanted)"""
        call("wn_chunk_softmax256_ce", ptr(logits), ptr(target), ptr(probs), ptr(dlogits), ptr(loss_part), n, 1.0 / n, _lib.stream())

    def _resolve_objective(self, objective):
        objective = self.objective if objective is None else objective
        if objective not in OBJECTIVES:
            raise ValueError("music_amd: objective must be one of %s, not %r" % (", ".join(OBJECTIVES), objective))
        return objective

    def _resolve_windows(self, windows, window_pos=None):
        """NllWindows of `windows`, else of self.nll_windows, else None (then window_pos must be unset too)"""
        windows = self.nll_windows if windows is None else windows
        if windows is None:
            if window_pos is not None:
                raise ValueError("music_amd: window_pos is the position inside a window table: pass windows= (or set nll_windows) with it")
            return None
        return windows if isinstance(windows, NllWindows) else NllWindows(windows, self.Q)

    def _resolve_wnll(self, ws, weights=None, ignore_index=None, label_smoothing=0.0):
        """None with all three at their defaults (today's launch), else wn_wstep_nll's tail: (weight tensor or None, ignore_index,
        smoothing).  weights: (B, W) or (B W,) floats on the device or the host, one per target; ignore_index: the target value
        of an absent column (None: no target is absent); label_smoothing in [0, 1)."""
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise ValueError("music_amd: label_smoothing must lie in [0, 1), got %r" % (label_smoothing,))
        if weights is None and ignore_index is None and eps == 0.0:
            return None
        if weights is not None:
            weights = torch.as_tensor(weights).reshape(-1)
            if weights.numel() != ws["B"] * ws["W"]:
                raise ValueError("music_amd: %d weights for %d clips of %d targets" % (weights.numel(), ws["B"], ws["W"]))
            if not weights.is_floating_point():
                raise ValueError("music_amd: weights are floats, one per target, got %s" % weights.dtype)
            weights = weights.to(device=self.device, dtype=torch.float32).contiguous()
        # (no ignore_index: the one value no stream can hold - it lies outside [0, Q) for every Q)
        return weights, -(1 << 63) if ignore_index is None else int(ignore_index), eps

    def step_nll(self, ws, target, dlogits=None, probs=None, row_nll=None, row_hit=None, windows=None, window_pos=None, weights=None,
                 ignore_index=None, label_smoothing=0.0):
        """wn_step_nll on the compact logits ws["O"] (pitch W, clip stride Q W): loss partials of the MEAN negative log-likelihood under
        the per-timestep softmax into ws["loss_part"]; d loss / d logits in the logits' own layout, the (B W, Q) probabilities, the
        per-column nll and hit flags where a tensor is given.  windows (None: self.nll_windows) / window_pos: the one launch is
        wn_win_step_nll, column c of clip b scored inside the pair of stream position window_pos[b] + c (NllWindows.tail).
        weights / ignore_index / label_smoothing (_resolve_wnll), any of them set: the launch is wn_wstep_nll - the weighted mean over
        the columns that carry a target, a column of weight 0 or with target == ignore_index skipped; ws["nll_den"] then holds the sum
        of the weights and its reciprocal on the device."""
        B, W, Q = ws["B"], ws["W"], self.Q
        win = self._resolve_windows(windows, window_pos)
        wt = self._resolve_wnll(ws, weights, ignore_index, label_smoothing)
        if "loss_part" not in ws:
            ws["loss_part"] = torch.zeros(_lib.CE_NUM_PARTIALS, dtype=torch.float32, device=self.device)
        if wt is not None:
            if "nll_den" not in ws:
                ws["nll_den"] = torch.zeros(2, dtype=torch.float32, device=self.device)
            ws["nll_win"], ws["nll_weight"] = win, wt[0]      # (alive as long as the workspace's last launch)
            tail = (None, 0, None, 0) if win is None else win.tail(window_pos, B, self.device)
            call("wn_wstep_nll", ptr(ws["O"]), Q * W, W, ptr(target), ptr(dlogits), Q * W, W, ptr(probs), ptr(row_nll), ptr(row_hit),
                 ptr(ws["loss_part"]), W, Q, B, *tail, ptr(wt[0]), wt[1], wt[2], ptr(ws["nll_den"]), _lib.stream())
        elif win is None:
            call("wn_step_nll", ptr(ws["O"]), Q * W, W, ptr(target), ptr(dlogits), Q * W, W, ptr(probs), ptr(row_nll), ptr(row_hit),
                 ptr(ws["loss_part"]), W, Q, B, 1.0 / (B * W), _lib.stream())
        else:
            ws["nll_win"] = win                 # (the host table and the positions live as long as the workspace's last launch)
            call("wn_win_step_nll", ptr(ws["O"]), Q * W, W, ptr(target), ptr(dlogits), Q * W, W, ptr(probs), ptr(row_nll), ptr(row_hit),
                 ptr(ws["loss_part"]), W, Q, B, 1.0 / (B * W), *win.tail(window_pos, B, self.device), _lib.stream())
        self.mark("step_nll")

    def score_logits(self, ws, target, windows=None, window_pos=None, weights=None, ignore_index=None, label_smoothing=0.0):
        """(row_nll float32 (B W,), row_hit int32 (B W,)) of the logits a forward left in ws["O"]: nats of every target sample under
        the per-timestep softmax, and whether the first-index argmax is the target.  Forward only: no gradient is formed.  weights /
        ignore_index (step_nll): a skipped column reports 0 and 0; row_nll is unsmoothed under any label_smoothing."""
        n = ws["B"] * ws["W"]
        target = target.reshape(-1)
        assert target.numel() == n and target.dtype == torch.int64 and target.is_cuda
        row_nll = torch.empty(n, dtype=torch.float32, device=self.device)
        row_hit = torch.empty(n, dtype=torch.int32, device=self.device)
        self.step_nll(ws, target, row_nll=row_nll, row_hit=row_hit, windows=windows, window_pos=window_pos, weights=weights,
                      ignore_index=ignore_index, label_smoothing=label_smoothing)
        return row_nll, row_hit

    def step_probs(self, ws, windows=None, window_pos=None):
        """(B W, Q) per-timestep probabilities of the logits in ws["O"] (wn_step_softmax): row b W + w is the distribution the
        decoder draws sample w of clip b from - under windows (wn_win_step_softmax), the one a windowed decode draws from"""
        B, W, Q = ws["B"], ws["W"], self.Q
        win = self._resolve_windows(windows, window_pos)
        probs = torch.empty(B * W, Q, dtype=torch.float32, device=self.device)
        if win is None:
            call("wn_step_softmax", ptr(ws["O"]), Q * W, W, ptr(probs), W, Q, B, _lib.stream())
        else:
            ws["nll_win"] = win
            call("wn_win_step_softmax", ptr(ws["O"]), Q * W, W, ptr(probs), W, Q, B, *win.tail(window_pos, B, self.device), _lib.stream())
        return probs

    def _throttled(self, step):
        """step() between the throttle's enter and leave (_lib.StepThrottle)."""
        self._throttle.enter()
        out = step()
        self._throttle.leave()
        return out

    def _fused_tail(self, ws, target, want_probs=False, objective=None, windows=None, window_pos=None, weights=None, ignore_index=None,
                    label_smoothing=0.0):
        """Everything of a fused step behind the forward that left the logits in ws["O"]: softmax + CrossEntropyLoss on the
        probabilities in one kernel (objective "nll": the per-timestep softmax and its negative log-likelihood, step_nll), the
        backward, the loss as a 0-d device tensor.  Gradients land in self.flat_grad.  windows / window_pos: step_nll's; the
        reference's loss has no per-column softmax to window.  weights / ignore_index / label_smoothing: step_nll's, "nll" only too."""
        objective = self._resolve_objective(objective)
        win = self._resolve_windows(windows, window_pos)
        if win is not None and objective != "nll":
            raise ValueError('music_amd: position windows (nll_windows) apply to objective "nll" only, not %r' % objective)
        if objective != "nll" and self._resolve_wnll(ws, weights, ignore_index, label_smoothing) is not None:
            raise ValueError('music_amd: weights, ignore_index and label_smoothing apply to objective "nll" only, not %r' % objective)
        bw = self._bwd_workspace(ws)
        n = ws["B"] * ws["W"]
        target = target.reshape(-1)
        assert target.numel() == n and target.dtype == torch.int64 and target.is_cuda
        if "loss_part" not in ws:
            ws["loss_part"] = torch.zeros(_lib.CE_NUM_PARTIALS, dtype=torch.float32, device=self.device)
        probs = None
        if want_probs:
            probs = torch.empty(n, self.Q, dtype=torch.float32, device=self.device)
            ws["probs"] = probs
        if objective == "nll":
            self.step_nll(ws, target, bw["dO"], probs, windows=win, window_pos=window_pos, weights=weights, ignore_index=ignore_index,
                          label_smoothing=label_smoothing)
        else:
            self.softmax_ce(ws["O"], target, probs, bw["dO"], ws["loss_part"], n)
        if self.vq:                         # reconstruction loss + vq_loss, under either objective; its upstream scalar is 1
            ws["vq_g"] = 1.0
            self.backward_from_dlogits(ws)
            return torch.add(ws["loss_part"].sum(), ws["vq_part"].sum(), alpha=self.vq_loss_coef)
        self.backward_from_dlogits(ws)
        return ws["loss_part"].sum()

    # ------------------------------------------------------------------ optimizer
    def adam_init(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                  ema_warmup=False):
        """max_grad_norm / skip_nonfinite: the guarded step (music_amd/guard.py) - the gradient is clipped to that global L2 norm and
        a non-finite one is skipped, both decided on the device; unset, adam_step is the one wn_adam_flat launch.  ema_decay /
        ema_warmup: the step ends with the wn_ema_flat launch on a shadow of the flat buffer taken here (music_amd/ema.py, `ema`)."""
        from . import ema
        self.adam_state = dict(m=torch.zeros_like(self.flat), v=torch.zeros_like(self.flat), t=0,
                               lr=lr, b1=betas[0], b2=betas[1], eps=eps)
        guard.adam_init_guard(self.adam_state, self.flat.device, max_grad_norm, skip_nonfinite)
        shadow = self.adam_state["ema"] = ema.make(ema_decay, ema_warmup)
        if shadow is not None:
            shadow.bind_engine(self)

    @property
    def ema(self):
        """The ShadowParams of the fused step (adam_init(ema_decay=...)), else None."""
        return None if self.adam_state is None else self.adam_state.get("ema")

    def guard_report(self):
        """The guard's state block read back (the only sync of the guarded step): norm / coef / taken / clipped / skipped /
        nonfinite, adam_state["t"] set to the steps taken; None without a guard."""
        return guard.engine_guard_report(self)

    def adam_step(self, gscale=1.0):
        """torch.optim.Adam semantics on the flat parameter buffer (guarded with adam_init's options; the codebook's EMA update and
        the shadow's follow the update: guard.flat_step)."""
        guard.engine_adam_step(self, gscale)
