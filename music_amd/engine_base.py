"""What the three training engines (engine.WaveNetEngine, model1._AutoencoderEngine, plan_generic.GeneralPlan) share on the host:
the workspace pool, the flat-parameter spec, `EngineBase` (state, timing marks, the tail of the fused step, the Adam step) and
`SlabPlan`, the bookkeeping of where every weight-gradient launch writes its slabs and what wn_reduce_slabs sums.

PyTorch is used for device memory and streams only.  Nothing here imports oracle/.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, guard
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


class EngineBase:
    """Host state and the steps every engine runs the same way.  An engine sets `device`, `Q`, `spec`, `flat`, `flat_grad`, calls
    _init_state(), and provides _make_workspace(), _bwd_workspace() and backward_from_dlogits()."""

    def _init_state(self):
        self._ws = WorkspacePool(self._make_workspace)
        self._gen = 0
        self.adam_state = None
        self.marks = None            # list of (name, torch.cuda.Event) when profiling is on
        self.mark_only = None        # optional set of mark names to keep
        self._throttle = _lib.StepThrottle()   # at most WN_MAX_STEPS_IN_FLIGHT fused steps in flight

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

    # ------------------------------------------------------------------ fused training step
    def softmax_ce(self, logits, target, probs, dlogits, loss_part, n):
        """loss partials and d loss / d logits of the MEAN cross entropy over n rows of 256 (probs None: not wanted)"""
        call("wn_chunk_softmax256_ce", ptr(logits), ptr(target), ptr(probs), ptr(dlogits), ptr(loss_part), n, 1.0 / n, _lib.stream())

    def _throttled(self, step):
        """step() between the throttle's enter and leave (_lib.StepThrottle)."""
        self._throttle.enter()
        out = step()
        self._throttle.leave()
        return out

    def _fused_tail(self, ws, target, want_probs=False):
        """Everything of a fused step behind the forward that left the logits in ws["O"]: softmax + CrossEntropyLoss on the
        probabilities in one kernel, the backward, the loss as a 0-d device tensor.  Gradients land in self.flat_grad."""
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
        self.softmax_ce(ws["O"], target, probs, bw["dO"], ws["loss_part"], n)
        self.backward_from_dlogits(ws)
        return ws["loss_part"].sum()

    # ------------------------------------------------------------------ optimizer
    def adam_init(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        """max_grad_norm / skip_nonfinite: the guarded step (music_amd/guard.py) - the gradient is clipped to that global L2 norm and
        a non-finite one is skipped, both decided on the device; unset, adam_step is the one wn_adam_flat launch."""
        self.adam_state = dict(m=torch.zeros_like(self.flat), v=torch.zeros_like(self.flat), t=0,
                               lr=lr, b1=betas[0], b2=betas[1], eps=eps)
        guard.adam_init_guard(self.adam_state, self.flat.device, max_grad_norm, skip_nonfinite)

    def guard_report(self):
        """The guard's state block read back (the only sync of the guarded step): norm / coef / taken / clipped / skipped /
        nonfinite, adam_state["t"] set to the steps taken; None without a guard."""
        return guard.engine_guard_report(self)

    def adam_step(self, gscale=1.0):
        """torch.optim.Adam semantics on the flat parameter buffer."""
        s = self.adam_state
        if s.get("guard") is not None:
            return guard.adam_step_guarded(self, gscale)
        s["t"] += 1
        call("wn_adam_flat", ptr(self.flat), ptr(self.flat_grad), ptr(s["m"]), ptr(s["v"]), self.spec.total,
             s["lr"], s["b1"], s["b2"], s["eps"], 1.0 - s["b1"] ** s["t"], 1.0 - s["b2"] ** s["t"], gscale, _lib.stream())
