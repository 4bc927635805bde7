"""Counterpart of the reference's ``wavenet/fast_generate.py`` (cached-queue autoregressive decode).

``predict_next(net, note, state_queue=None)`` keeps the reference's contract
(wavenet/fast_generate.py:13-141): the first call takes a ``(1, Q, receptive_field)`` one-hot piece,
runs the full forward (HIP path) and snapshots the per-layer queues; later calls take one
``(1, Q, 1)`` column and advance every queue by one sample.  It returns ``(LongTensor(1,), queue)``
where ``queue`` behaves like the reference's ``OrderedDict`` ('causal_layer' -> (1,Q,1),
'block_i' -> (1,R,d_i), oldest column first).

As WRITTEN in the reference each block pushes its OUTPUT into its own queue instead of its input
(fast_generate.py:128-129), so fast generation differs from naive generation; that
recurrence is reproduced by default.  ``correct_queue=True`` selects the fast-wavenet recurrence.

Any filter width k >= 1: block i keeps the last (k-1) d_i columns of its input ('block_i' -> (1, R, (k-1) d_i)) and the
causal layer the last k-1 input columns ('causal_layer' -> (1, Q, k-1)).  The as-written push is undefined for k != 2 (its
``[state | note]`` input is too short for k >= 3): there only ``correct_queue=True`` exists, ``False`` raises ValueError.

``generate()`` (fast_generate.py:144-179) runs the whole greedy loop as ONE persistent kernel launch
(``wn_decode``) instead of one Python iteration per sample, and writes the wav with scipy (librosa,
which the reference uses for that, is not a dependency here).  Unlike the reference module this one
has no import-time side effect (the reference calls ``generate(...)`` at import, :182-186).
"""
from collections import OrderedDict
import ctypes
import json
import os

import numpy as np
import torch

try:
    from . import _lib
    from ._lib import call, ptr
    from .audio_func import mu_law_decode
    from .engine import SLACK, pack_index
    from .engine_base import WindowTable
    from .model import wavenet
    from .train import load_model
except ImportError:
    from music_amd import _lib
    from music_amd._lib import call, ptr
    from music_amd.audio_func import mu_law_decode
    from music_amd.engine import SLACK, pack_index
    from music_amd.engine_base import WindowTable
    from music_amd.model import wavenet
    from music_amd.train import load_model


def _mfma_decode(eng):
    """True when the matrix-core decode kernels serve this model (wn_decode_batch_pk): up to 64 residual / dilation channels -
    fewer are PADDED to 64 with zero rows and columns (the decoder is bound by latency, not traffic: the padding is free) -,
    256 or 512 skip channels, 256 quantisation channels, f16x3 forward mode; biases are fine.  WN_DEC_MFMA=0: never.
    Decided ONCE per engine (the queue column width of every DecodeState and the layout of the weight pack follow from it:
    a switch flipped inside a process must not make them disagree)."""
    v = getattr(eng, "_dec_mfma", None)
    if v is None:
        k = eng.k
        if k == 2:
            v = bool(os.environ.get("WN_DEC_MFMA", "1") == "1" and eng.R <= 64 and
                     eng.D <= 64 and eng.S in (256, 512) and eng.Q == 256 and eng.mode_fwd == _lib.F16X3 and
                     "fg0" in getattr(eng, "pk_f_off", {}))
        else:
            # filter widths 3 / 4 (general-plan engines; _DecodePack builds the [2 x 64][64 k] fg packs itself): the history
            # taps are summed a sample ahead, so the tap-0-ahead form is required (WN_DEC_T0=0: the fp32 kernel)
            v = bool(os.environ.get("WN_DEC_MFMA", "1") == "1" and os.environ.get("WN_DEC_T0", "1") != "0" and k in (3, 4) and
                     eng.R <= 64 and eng.D <= 64 and eng.S in (256, 512) and eng.Q == 256 and eng.mode_fwd == _lib.F16X3)
        eng._dec_mfma = v
    return v


def _ring_width(eng):
    """Floats per queue column: the (padded) residual channel count the decode kernels run with."""
    return 64 if _mfma_decode(eng) else eng.R


class _DecodePack:
    """fp32 weights in the layout wn_decode reads (rebuilt from the engine's flat buffer), and for the matrix-core kernels
    the same weights as packed f16 hi/lo fragments.  With fewer than 64 residual / dilation channels on that path every
    matrix is laid out for Rp = Dp = 64 channels with structural zeros (index -1)."""

    def __init__(self, eng):
        sp, R, D, S, Q, N = eng.spec, eng.R, eng.D, eng.S, eng.Q, eng.N
        k = self.k = eng.k
        self.mfma = _mfma_decode(eng)
        Rp = Dp = self.Rp = self.Dp = 64 if self.mfma else None
        if not self.mfma:
            Rp, Dp = self.Rp, self.Dp = R, D

        def pad(m, rows, cols):
            out = np.full((rows, cols), -1, dtype=np.int64)
            out[:m.shape[0], :m.shape[1]] = m
            return out

        def padv(v, n):
            out = np.full(n, -1, dtype=np.int64)
            out[:len(v)] = v
            return out
        parts, mats = [], {}
        wc = sp.conv("causal_layer.weight")                                 # [R,Q,k]
        self.o_causal = 0
        parts.append(pad(np.concatenate([wc[:, :, j] for j in range(k)], 1), Rp, k * Q).reshape(-1))     # k = [tap0 | .. | tap k-1]
        self.layer_stride = 2 * Dp * k * Rp + Rp * Dp + S * Dp
        self.o_layers = sum(len(p) for p in parts)
        for i in range(N):
            wf = sp.conv("dilation_layer_stack.%d.weight" % (4 * i))        # [D,R,k]
            wg = sp.conv("dilation_layer_stack.%d.weight" % (4 * i + 1))
            wd = sp.conv("dilation_layer_stack.%d.weight" % (4 * i + 2))[:, :, 0]
            ws = sp.conv("dilation_layer_stack.%d.weight" % (4 * i + 3))[:, :, 0]
            blk = lambda w, taps: np.concatenate([pad(w[:, :, j], Dp, Rp) for j in taps], 1)
            fg = np.concatenate([blk(wf, range(k - 1, -1, -1)),                        # k = [tap k-1 (cur) | tap k-2 | .. | tap0 (oldest)]
                                 blk(wg, range(k - 1, -1, -1))], 0)
            parts += [fg.reshape(-1), pad(wd, Rp, Dp).reshape(-1), pad(ws, S, Dp).reshape(-1)]
            # the packed forms: [f; g] rows, K = [tap0 | tap1 | ..] in natural order; dense in chained order (as wn_resblock_fwd)
            mats["fg%d" % i] = (np.concatenate([blk(wf, range(k)), blk(wg, range(k))], 0), False)
            mats["d%d" % i] = (pad(wd, Rp, Dp), True)
            mats.setdefault("skip_cols", []).append(pad(ws, S, Dp))
        self.o_p1 = sum(len(p) for p in parts)
        parts.append(sp.conv("post_process_1.weight")[:, :, 0].reshape(-1))
        self.o_p2 = sum(len(p) for p in parts)
        parts.append(sp.conv("post_process_2.weight")[:, :, 0].reshape(-1))
        self.o_bias = None
        if eng.use_bias:
            self.o_bias = sum(len(p) for p in parts)
            b = lambda n: sp.off[n] + np.arange(sp.shape[n][0])
            self.ob_causal = self.o_bias
            parts.append(padv(b("causal_layer.bias"), Rp))
            self.ob_layers = sum(len(p) for p in parts)
            for i in range(N):
                parts += [padv(b("dilation_layer_stack.%d.bias" % (4 * i + k)), n) for k, n in enumerate((Dp, Dp, Rp, S))]
            self.ob_p1 = sum(len(p) for p in parts)
            parts.append(b("post_process_1.bias"))
            self.ob_p2 = sum(len(p) for p in parts)
            parts.append(b("post_process_2.bias"))
        idx = np.concatenate(parts).astype(np.int32)
        self.idx = torch.from_numpy(idx).to(eng.device)
        self.buf = torch.empty(len(idx), dtype=torch.float32, device=eng.device)
        self.eng = eng
        self.pk = None
        if self.mfma:
            # packed fragments: per block "fg" then "d" at a fixed stride, then skip, p1, p2 (offsets in halfs, hi + lo planes)
            lst = []
            for i in range(N):
                lst += [("fg%d" % i,) + mats["fg%d" % i], ("d%d" % i,) + mats["d%d" % i]]
            lst += [("skip", np.concatenate(mats["skip_cols"], 1), False),
                    ("p1", sp.conv("post_process_1.weight")[:, :, 0], False), ("p2", sp.conv("post_process_2.weight")[:, :, 0], False)]
            offs, o, pidx = {}, 0, []
            for name, m, chained in lst:
                offs[name] = 2 * o
                pi = pack_index(m.astype(np.int64), chained)
                pidx.append(pi)
                o += len(pi)
            self.pk_off = offs
            self.pk_stride = offs["fg1"] - offs["fg0"] if N > 1 else 0
            self.pk_idx = torch.from_numpy(np.concatenate(pidx).astype(np.int32)).to(eng.device)
            self.pk = torch.zeros(2 * o, dtype=torch.int16, device=eng.device)

    def refresh(self):
        call("wn_gather_grads", ptr(self.eng.flat), ptr(self.idx), ptr(self.buf), self.idx.numel(), _lib.stream())
        if self.pk is not None:
            call("wn_pack_weights", ptr(self.eng.flat), ptr(self.pk_idx), ptr(self.pk), self.pk_idx.numel(), _lib.F16X3, _lib.stream())

    def p(self, off):
        return None if off is None else ptr(self.buf, off)

    def weights(self):
        """(w_causal, b_causal, w_layers, layer stride, b_layers, w_p1, b_p1, w_p2, b_p2) as every decode entry takes them."""
        ob = (self.ob_causal, self.ob_layers, self.ob_p1, self.ob_p2) if self.o_bias is not None else (None,) * 4
        return (self.p(self.o_causal), self.p(ob[0]), self.p(self.o_layers), self.layer_stride, self.p(ob[1]),
                self.p(self.o_p1), self.p(ob[2]), self.p(self.o_p2), self.p(ob[3]))

    def chain(self):
        """(pk pointer, fg offset, d offset, per-block stride, skip, p1, p2 offsets) for wn_decode_batch_pk, or Nones / -1."""
        if self.pk is None:
            return None, 0, 0, 0, -1, -1, -1
        o = self.pk_off
        return ptr(self.pk), o["fg0"], o["d0"], self.pk_stride, o["skip"], o["p1"], o["p2"]


def _taps(eng):
    """k - 1: the previous input columns every layer keeps (filter_width - 1)."""
    return eng.k - 1


def _check_recurrence(eng, correct_queue):
    if _taps(eng) != 1 and not correct_queue:
        raise ValueError("the reference's as-written queue push (wavenet/fast_generate.py:128-129) is defined for filter_width "
                         "== 2 only; pass correct_queue=True for filter_width %d" % (_taps(eng) + 1))


def _ptr_or_none(t):
    """Device pointer, or None for an empty tensor (filter_width 1: no previous input columns)."""
    return ptr(t) if t is not None and t.numel() else None


def _ring_offsets(eng):
    """Float offset of every block's ring - (k-1) d_i columns of _ring_width floats each -, then the floats of all of them: N + 1
    values.  THE place the ring layout is computed (DecodeState, the launcher, decode_batch_cond's check, zero_state)."""
    return np.cumsum([0] + [_taps(eng) * d * _ring_width(eng) for d in eng.dil]).astype(np.int64)


def zero_state(eng, B):
    """The queues of B utterances that have seen nothing, as ``decode_batch_cond`` takes them: (rings (B, ring floats), prev (B, k-1,
    Q)), zeros on the engine's device.  (filter_width 1 keeps no queues, but the entry point wants a queue buffer: one unused float.)"""
    return (torch.zeros(B, max(1, int(_ring_offsets(eng)[-1])), dtype=torch.float32, device=eng.device),
            torch.zeros(B, _taps(eng), eng.Q, dtype=torch.float32, device=eng.device))


class DecodeState(OrderedDict):
    """The per-layer FIFO queues of the decoder.  Internally every block's queue is a ring buffer of (k-1) d_i columns in
    time-major layout on the device (k = filter_width); indexing by the reference's keys materialises the
    time-ordered ``(1, C, (k-1) d)`` tensor (``'causal_layer'``: ``(1, Q, k-1)``), oldest column first."""

    def __init__(self, eng, rings, prev, steps=0):
        super().__init__()
        self.eng, self.rings, self.prev, self.steps = eng, rings, prev, steps
        self.rw = _ring_width(eng)                # floats per queue column (64 on the matrix-core kernels, zeros beyond eng.R)
        self.q_off = _ring_offsets(eng)
        for k in ["causal_layer"] + ["block_%d" % (i + 1) for i in range(eng.N)]:
            OrderedDict.__setitem__(self, k, None)

    def _ring(self, i):
        L = _taps(self.eng) * self.eng.dil[i]
        return self.rings[self.q_off[i]:self.q_off[i] + L * self.rw].view(L, self.rw)[:, :self.eng.R]

    def __getitem__(self, key):
        K1 = _taps(self.eng)
        if key == "causal_layer":
            Q = self.eng.Q
            return self.prev.view(K1, Q).t().contiguous().view(1, Q, K1).clone()
        i = int(key.split("_")[1]) - 1
        L = K1 * self.eng.dil[i]
        ring = self._ring(i)
        if L:
            ring = torch.roll(ring, -(self.steps % L), 0)              # oldest column first
        return ring.t().contiguous().view(1, self.eng.R, L)

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    @staticmethod
    def from_tensors(eng, queue):
        """Build the ring form from reference-style tensors (time-ordered, oldest first)."""
        rw, K1 = _ring_width(eng), _taps(eng)
        rings = torch.cat([torch.nn.functional.pad(queue["block_%d" % (i + 1)].to(eng.device).float().reshape(eng.R, K1 * eng.dil[i]).t(),
                                                   (0, rw - eng.R)).reshape(-1) for i in range(eng.N)])
        prev = queue["causal_layer"].to(eng.device).float().reshape(eng.Q, K1).t().contiguous().reshape(-1)
        return DecodeState(eng, rings.contiguous(), prev, 0)


def _per_row(v, U, spread=False):
    """A setting that is a scalar or one value per utterance (tensor / ndarray / list / tuple) -> None for a scalar, the list of its U
    values otherwise.  ``spread``: a scalar comes back U times and a sequence as it is - the caller checks what it holds."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    if isinstance(v, np.ndarray):
        v = v.tolist()
    if not isinstance(v, (list, tuple)):
        return [v] * U if spread else None
    if len(v) != U and not spread:
        raise ValueError("per-utterance sampling settings must have one entry per utterance (%d), got %d" % (U, len(v)))
    return list(v)


class _Sampling:
    """The sampling arguments of one decode launch of U utterances (or of ``sample_logits`` over U rows).  ``temperature``,
    ``top_k``, ``top_p`` and ``seed`` may each be a scalar or a length-U sequence / tensor; ``streams`` are the random-number
    stream ids (default ``arange(U)``: the utterance index, today's key).  Scalars travel as the entry point's scalar
    arguments; the device table of ``wn_sampling`` entries is built only when something is per-utterance.
    ``plain``: nothing here needs ``wn_decode_batch_samp`` (no filter, no table)."""

    def __init__(self, U, temperature, top_k, top_p, seed, streams, dev, default_stream=None):
        seq = lambda v: _per_row(v, U)
        per = {"temperature": seq(temperature), "top_k": seq(top_k), "top_p": seq(top_p), "seed": seq(seed)}
        st = seq(streams)
        if streams is not None and st is None:
            raise ValueError("streams must be a sequence of one stream id per utterance")
        if st is not None and default_stream is None and [int(v) for v in st] == list(range(U)):
            st = None                                     # the default key
        val = lambda name, v: per[name] if per[name] is not None else [v] * U
        T = [0.0 if t is None else float(t) for t in val("temperature", temperature)]
        K = [0 if k is None else int(k) for k in val("top_k", top_k)]
        P = [1.0 if q is None else float(q) for q in val("top_p", top_p)]
        for k in K:
            if k < 0:
                raise ValueError("top_k must be >= 0 (0 / None: no top-k filter), got %d" % k)
        for q in P:
            if not (0.0 < q <= 1.0):
                raise ValueError("top_p must lie in (0, 1] (1 / None: no nucleus filter), got %r" % (q,))
        self.table = None
        if st is not None or any(v is not None for v in per.values()):
            sd = [int(v) for v in val("seed", seed)]
            if st is None:
                st = [default_stream] * U if default_stream is not None else list(range(U))
            tab = np.zeros(U, dtype=np.dtype([("temperature", "<f4"), ("top_p", "<f4"), ("top_k", "<i4"), ("stream", "<u4"), ("seed", "<u8")]))
            assert tab.dtype.itemsize == ctypes.sizeof(_lib.Sampling)
            tab["temperature"], tab["top_p"], tab["top_k"], tab["stream"] = T, P, K, [int(v) for v in st]
            tab["seed"] = [v & 0xFFFFFFFFFFFFFFFF for v in sd]
            self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
            self.temperature, self.top_k, self.top_p, self.seed = 0.0, 0, 1.0, 0
        else:
            self.temperature, self.top_k, self.top_p, self.seed = T[0] if T[0] > 0 else 0.0, K[0], P[0], int(seed)
        self.filtered = any(k > 0 for k in K) or any(q < 1.0 for q in P)
        self.plain = self.table is None and not self.filtered

    def tail(self):
        """The arguments wn_decode_batch_samp takes behind wn_decode_batch_cond's (before the stream)."""
        return ptr(self.table), int(self.top_k), float(self.top_p)


_NO_COND = (None, 0, None, 0, None, None, 1, 0)       # wn_decode_batch_cond's table arguments of an unconditioned launch
last_error_flags = None        # the error flag word of every utterance of the last decode_batch_cond launch (device tensor)


def _corrected_only(correct_queue, what, entry):
    """THE refusal of the as-written recurrence: `what` exists on the corrected one only, served by `entry`."""
    if not correct_queue:
        raise ValueError("%s on the corrected recurrence only (%s): pass correct_queue=True" % (what, entry))


def _need_corrected(smp, correct_queue):
    if not smp.plain:
        _corrected_only(correct_queue, "top_k / top_p and per-utterance sampling settings run", "wn_decode_batch_samp")


def stage_windows(stages, K):
    """The window table of a residual quantiser's frame-major token stream (tools/vq_codes_dataset.py: token = s K + code at
    stream position p with s = p mod stages): ``[(s K, (s + 1) K) for s in range(stages)]``."""
    return [(s * int(K), (s + 1) * int(K)) for s in range(int(stages))]


class _Windows(WindowTable):
    """The position windows of one launch (engine_base.WindowTable; include/wavenet_hip.h, wn_win_decode_batch) and ``pos``, the
    stream position of the launch's first step (row); step s samples inside pair ``(pos + s) % len(windows)``.  ``_windows_of``
    gives None for ``windows=None``."""

    def __init__(self, windows, pos, Q):
        super().__init__(windows, Q)
        if int(pos) < 0:
            raise ValueError("window_pos (the stream position of the first code) must be >= 0, got %d" % int(pos))
        self.pos = int(pos)

    def tail(self, ahead=0):
        """The arguments wn_win_decode_batch / wn_win_sample_logits take behind the entry they extend (before the stream), for a
        launch whose first step sits ``ahead`` positions behind ``pos``."""
        return ctypes.cast(self.host, ctypes.c_void_p), len(self.pairs), self.pos + ahead


def _windows_of(windows, window_pos, Q, correct_queue=True):
    """``windows=`` / ``window_pos=`` of a generator -> _Windows or None; ``correct_queue``: the recurrence the caller runs on."""
    if windows is None:
        if window_pos:
            raise ValueError("window_pos is the position inside a window table: pass windows= with it")
        return None
    win = _Windows(windows, window_pos, Q)
    _corrected_only(correct_queue, "position windows run", "wn_win_decode_batch")
    return win


def _first_in_window(probs, win):
    """First-index argmax of every row of the init forward's probabilities (U, Q) inside the window of position ``win.pos``,
    taken on the host; reported in the full alphabet."""
    lo, hi = win.at(win.pos)
    return torch.from_numpy(lo + np.argmax(probs.detach().float().cpu().numpy()[:, lo:hi], axis=1)).to(probs.device)


def _check_classes(net, classes):
    """classes are refused by a model without the mode (or without the notion) and required by one with it, before any launch"""
    check = getattr(net, "check_classes", None)
    if check is not None:
        check(classes)
    elif classes is not None:
        raise ValueError("music_amd.fast_generate: this model takes no classes, pass classes=None")


def _check_phase(net, phase_pos):
    """phase_pos is refused by a model without the mode (or without the notion) and required by one with it, before any launch; the
    generators take ONE stream position for the launch, as they take one window_pos"""
    check = getattr(net, "check_phase", None)
    if check is not None:
        check(phase_pos)
    elif phase_pos is not None:
        raise ValueError("music_amd.fast_generate: this model takes no phase_pos, pass phase_pos=None")
    if phase_pos is not None and (isinstance(phase_pos, bool) or not isinstance(phase_pos, (int, np.integer))):
        raise ValueError("music_amd.fast_generate: phase_pos is one integer >= 0, the stream position of the first token the launch "
                         "chooses, not %r" % (phase_pos,))


def _phase_cond(net, eng, cls, U, pos0):
    """The decode tables of a phase-conditioned WaveNet: cond_fg (U, N, P, 2 Dp) rows [f | g] and cond_p1 (U, P, S), frame l = the
    phase tables' column l (plus the utterance's class column where there are classes: wn_gclass_fwd, then wn_phase_tab_fwd at position
    0 without rotation), under a schedule with c_shift = 0, c_q = 0 (the tile rule: column c mod P) and le = P.  pos0: the stream
    position of the launch's first step - priming steps may lie in front of stream position 0, where the entry would read column 0;
    the tile rule is periodic, so the launch is given pos0 mod P (the mathematical one: a multiple of P added), never negative."""
    pack = _pack_for(net, eng)
    N, D, S, Dp, P, dev = eng.N, eng.D, eng.S, pack.Dp, eng.phase, eng.device
    ch = -(-D // 32) * 32
    empty = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    st, add = _lib.stream(), (None, None, None)
    if cls is not None:
        add = (empty(N, U, 2 * ch), None, empty(U, S))
        eng.gclass_fwd(cls, add[0], None, add[2], ch, st)
    tab, enf = empty(N, U, 2 * ch, P), empty(U, S, P)
    zero_pos, zero_rot = torch.zeros(U, dtype=torch.int64, device=dev), torch.zeros(N + 1, dtype=torch.int32, device=dev)
    eng.phase_fwd(zero_pos, tab, None, enf, ch, st, add, rot=zero_rot)
    cond_fg = torch.zeros(U, N, P, 2 * Dp, dtype=torch.float32, device=dev)
    cond_fg[:, :, :, :D] = tab[:, :, :D].permute(1, 0, 3, 2)
    cond_fg[:, :, :, Dp:Dp + D] = tab[:, :, ch:ch + D].permute(1, 0, 3, 2)
    cond_p1 = enf.transpose(1, 2).contiguous()
    shift = (ctypes.c_int32 * (N + 1))(*([0] * (N + 1)))
    qs = (ctypes.c_int32 * (N + 1))(*([0] * (N + 1)))
    cond = (ptr(cond_fg), cond_fg[0].numel(), ptr(cond_p1), cond_p1[0].numel(), ctypes.cast(shift, ctypes.c_void_p),
            ctypes.cast(qs, ctypes.c_void_p), P, int(pos0) % P)
    return cond, (cond_fg, cond_p1, shift, qs)


def _class_cond(net, eng, classes, U, correct_queue, phase_pos0=None):
    """The conditioning arguments of a class-conditional WaveNet's decode launch (None with the mode off): the U utterances' tables
    - cond_fg (U, N, 1, 2 Dp) rows [f | g], cond_p1 (U, 1, S) - built on the device from wn_gclass_fwd's output, under a schedule
    of one frame that every position reads.  Classes are refused with the mode off and required with it on (EngineBase.stage_classes);
    corrected recurrence only.  phase_pos0: the stream position of the launch's first step for a phase-conditioned model, whose tables
    have P frames (``_phase_cond``, with or without classes).  Returns (wn_decode_batch_cond's eight table arguments, the tensors
    they point into)."""
    if getattr(eng, "phase", 0):
        _corrected_only(correct_queue, "a phase-conditioned model decodes", "wn_decode_batch_cond")
        return _phase_cond(net, eng, eng.stage_classes(classes, U), U, phase_pos0)
    if classes is None and not getattr(eng, "gcond", False):
        return None, None
    cls = eng.stage_classes(classes, U)
    if cls is None:
        return None, None
    _corrected_only(correct_queue, "a class-conditional model decodes", "wn_decode_batch_cond")
    pack = _pack_for(net, eng)
    N, D, S, Dp, dev = eng.N, eng.D, eng.S, pack.Dp, eng.device
    ch = -(-D // 32) * 32                                         # the table's rows per half: D padded to 32
    tab = torch.empty(N, U, 2 * ch, dtype=torch.float32, device=dev)
    enf = torch.empty(U, S, dtype=torch.float32, device=dev)
    eng.gclass_fwd(cls, tab, None, enf, ch, _lib.stream())
    cond_fg = torch.zeros(U, N, 1, 2 * Dp, dtype=torch.float32, device=dev)
    cond_fg[:, :, 0, :D] = tab[:, :, :D].transpose(0, 1)
    cond_fg[:, :, 0, Dp:Dp + D] = tab[:, :, ch:ch + D].transpose(0, 1)
    cond_p1 = enf.view(U, 1, S)
    shift = (ctypes.c_int32 * (N + 1))(*([0] * (N + 1)))          # one frame, the tile rule: every position reads frame 0
    qs = (ctypes.c_int32 * (N + 1))(*([0] * (N + 1)))
    cond = (ptr(cond_fg), cond_fg[0].numel(), ptr(cond_p1), S, ctypes.cast(shift, ctypes.c_void_p), ctypes.cast(qs, ctypes.c_void_p), 1, 0)
    return cond, (cond_fg, cond_p1, shift, qs)


def _guidance_of(net, guidance, U, correct_queue, classes):
    """``guidance=`` of the generators -> None, or U floats (a scalar serves every utterance).  Classifier-free guidance needs a
    class-conditional model whose parameters name a ``null_class``, classes, and the corrected recurrence: refused here, before
    anything is launched."""
    if guidance is None:
        return None
    if not getattr(net, "global_classes", 0) or classes is None:
        raise ValueError("music_amd.fast_generate: guidance= extrapolates from the unconditional towards the class-conditional "
                         "distribution: it needs a model with global_classes > 0 and classes=")
    if getattr(net, "null_class", None) is None:
        raise ValueError('music_amd.fast_generate: guidance= needs a model with "null_class" (the class that stands for "no class", '
                         'trained with "class_dropout")')
    _corrected_only(correct_queue, "guidance runs", "wn_cfg_decode_batch")
    g = _per_row(guidance, U, spread=True)
    if len(g) != U or any(isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf") for v in g):
        raise ValueError("guidance must be None, a finite number or %d finite numbers (one per utterance)" % U)
    return [float(v) for v in g]


def _first_codes(probs, win=None, guide=None):
    """The first code of every utterance from the init forward's probabilities: the first-index argmax of its row, inside the
    window of position ``win.pos`` when there is a table (``_first_in_window``).  ``guide`` (U scales): the rows are (2U, Q), [c, u]
    interleaved, and the code is the first-index argmax of log p_c + (s - 1)(log p_c - log p_u) inside the window (the rule of the
    launch on log-probabilities, which differ from the logits by a constant per row: the argmax is the same), taken on the host in
    float64."""
    if guide is None:
        return probs.argmax(1) if win is None else _first_in_window(probs, win)
    lp = np.log(np.maximum(probs.detach().double().cpu().numpy(), 1e-300))
    lo, hi = win.at(win.pos) if win is not None else (0, lp.shape[1])
    s = np.asarray(guide, dtype=np.float64)[:, None]
    comb = lp[0::2, lo:hi] + (s - 1.0) * (lp[0::2, lo:hi] - lp[1::2, lo:hi])
    return torch.from_numpy(lo + np.argmax(comb, axis=1)).to(probs.device)


def check_keep(keep, U, note_num, Q, win=None):
    """The pure checks of ``keep=`` (no device): ``keep`` is (U, note_num) - or (note_num,) for one utterance - integers, every entry
    a token in [0, Q) that IS the code at its position, or -1: the sampler's choice.  ``win`` (a ``_Windows`` or None): a kept token at
    position j must lie inside the window of stream position ``win.pos + j``.  Returns the (U, note_num) int64 host tensor."""
    k = torch.as_tensor(keep)
    if k.is_floating_point() or k.is_complex() or k.dtype == torch.bool:
        raise ValueError("keep must hold integers (a token, or -1 for the sampler's choice), got %s" % k.dtype)
    if k.dim() == 1 and U == 1:
        k = k.reshape(1, -1)
    if tuple(k.shape) != (U, note_num):
        raise ValueError("keep must be (%d, %d) integers, one per utterance and position, got %s" % (U, note_num, tuple(k.shape)))
    k = k.detach().to(device="cpu", dtype=torch.int64)
    wrong = (k < -1) | (k >= Q)
    if bool(wrong.any()):
        u, j = (int(v) for v in wrong.nonzero()[0])
        raise ValueError("keep: token %d of utterance %d at position %d is neither -1 nor a token in [0, %d)" % (int(k[u, j]), u, j, Q))
    if win is not None:
        lo = torch.tensor([win.at(win.pos + j)[0] for j in range(note_num)], dtype=torch.int64)
        hi = torch.tensor([win.at(win.pos + j)[1] for j in range(note_num)], dtype=torch.int64)
        wrong = (k >= 0) & ((k < lo) | (k >= hi))
        if bool(wrong.any()):
            u, j = (int(v) for v in wrong.nonzero()[0])
            raise ValueError("keep: token %d of utterance %d at position %d (stream position %d) lies outside that position's range "
                             "[%d, %d)" % (int(k[u, j]), u, j, win.pos + j, int(lo[j]), int(hi[j])))
    return k


def _check_forced(forced, Q, what):
    """``forced=`` of a launch: entries >= Q are refused where the tensor lives on the host (a device tensor travels as it is: no
    synchronisation); negative entries free their step (include/wavenet_hip.h, wn_decode)."""
    if forced is not None and not forced.is_cuda and forced.numel() and int(forced.max()) >= Q:
        raise ValueError("%s: forced holds a code >= Q = %d (a negative entry frees its step)" % (what, Q))


def _keep_of(keep, U, note_num, Q, win, correct_queue):
    """``keep=`` of a generator -> None, or the checked (U, note_num) int64 host tensor; corrected recurrence only."""
    if keep is None:
        return None
    _corrected_only(correct_queue, "keep= (partially forced decode) runs", "wn_decode_batch")
    return check_keep(keep, U, int(note_num), Q, win)


def _resolved(kept, codes):
    """The fed stream: the kept code where there is one, else the launch's own (``codes``: a device tensor of ``kept``'s shape)."""
    k = kept.to(codes.device)
    return torch.where(k >= 0, k, codes.to(torch.int64))


def _note0(first, rows, Q, dev):
    """The first input column of a launch, (rows U, Q): the one-hot of every utterance's first code, once per row of the utterance."""
    idx = first.to(dev).repeat_interleave(rows)
    note0 = torch.zeros(idx.numel(), Q, dtype=torch.float32, device=dev)
    note0[torch.arange(idx.numel(), device=dev), idx] = 1.0
    return note0


def _pack_for(net, eng):
    """The decode weight pack of `eng`, kept on the net (built on first use; refreshed by the launcher)."""
    pack = getattr(net, "_decode_pack", None)
    if pack is None or pack.eng is not eng:
        pack = net._decode_pack = _DecodePack(eng)
    return pack


_NO_WIN = (None, 0, 0)                                # wn_win_decode_batch's window arguments of a launch without a table


def _decode_call(shape, dil, qoff, queues, weights, io, step0, n_steps, push_input, sync, U, queues_ustride, smp, pk, cond=None,
                 win=None, guide=None):
    """(entry point, its arguments without the stream) of one decode launch: THE place the argument list is written and the
    entry chosen.  Plain values and pointers only (no device work).  ``shape``: (filter_width, N, Rp, Dp, S, Q); ``weights``:
    ``_DecodePack.weights()``; ``io``: note0, prev0, note_out, prev_out, forced, codes, probs; ``pk``: ``_DecodePack.chain()``;
    ``cond``: the eight table arguments of wn_decode_batch_cond when the launch came in through ``decode_batch_cond``;
    ``win``: the three window arguments (``_Windows.tail``) - only then is the entry wn_win_decode_batch, whatever the sampling;
    ``guide``: the device pointer of the guidance table (U / 2 floats) - only then is the entry wn_cfg_decode_batch."""
    args = (*shape, dil, qoff, queues, *weights, *io, step0, n_steps, push_input, sync, U, queues_ustride,
            smp.temperature, smp.seed, *pk)
    if guide is not None:
        return "wn_cfg_decode_batch", (args + (_NO_COND if cond is None else tuple(cond)) + smp.tail() +
                                       (_NO_WIN if win is None else tuple(win)) + (guide,))
    if win is not None:
        return "wn_win_decode_batch", args + (_NO_COND if cond is None else tuple(cond)) + smp.tail() + tuple(win)
    if smp.plain and cond is None:
        return "wn_decode_batch_fw", args
    args += _NO_COND if cond is None else tuple(cond)
    if smp.plain:
        return "wn_decode_batch_cond", args
    return "wn_decode_batch_samp", args + smp.tail()


def _launch_decode(net, eng, smp, rings, note0, prev0, U, n_steps, step0, push_input, timeout_msg, check=True, forced=None,
                   want_probs=False, sync=None, cond=None, win=None, guide=None):
    """One persistent decode launch of U utterances: ``rings`` ((U, ring floats), or 1-D for one utterance) is advanced in
    place.  ``win``: the window arguments of the launch's first step (``_Windows.tail``), or None.  ``guide``: the guidance table
    (U / 2 floats on the device; the rows are then (conditional, unconditional) pairs), or None.  ``sync``: the hand-off scratch (default: fresh and zeroed); ``check``: read the error flags back and raise
    ``timeout_msg`` if one is set.  Returns (codes int32 (U, n_steps), probabilities (U, n_steps, Q) or None, note_out (U, Q),
    prev_out (U, k-1, Q))."""
    global last_error_flags
    pack = _pack_for(net, eng)
    pack.refresh()
    dev, N, Q, K1 = eng.device, eng.N, eng.Q, pack.k - 1
    dil = (ctypes.c_int32 * N)(*eng.dil)
    qoff = (ctypes.c_int64 * N)(*[int(v) for v in _ring_offsets(eng)[:N]])
    forced_t = forced.to(device=dev, dtype=torch.int32).contiguous() if forced is not None else None
    codes = torch.empty(U, n_steps, dtype=torch.int32, device=dev)
    probs = torch.empty(U, n_steps, Q, dtype=torch.float32, device=dev) if want_probs else None
    note_out = torch.empty(U, Q, dtype=torch.float32, device=dev)
    prev_out = torch.empty(U, K1, Q, dtype=torch.float32, device=dev)
    if sync is None:
        sync = torch.zeros(U * _lib.decode_sync_granules(N, pack.Dp, eng.S), dtype=torch.int64, device=dev)
    qbuf = rings if rings.numel() else torch.zeros(1, dtype=torch.float32, device=dev)     # (filter_width 1: zero_state)
    name, args = _decode_call((pack.k, N, pack.Rp, pack.Dp, eng.S, Q), ctypes.cast(dil, ctypes.c_void_p),
                              ctypes.cast(qoff, ctypes.c_void_p), ptr(qbuf), pack.weights(),
                              (ptr(note0), _ptr_or_none(prev0), ptr(note_out), _ptr_or_none(prev_out), ptr(forced_t), ptr(codes),
                               ptr(probs)), int(step0), n_steps, push_input, ptr(sync), U, rings.size(1) if rings.dim() == 2 else 0,
                              smp, pack.chain(), cond, win, ptr(guide) if guide is not None else None)
    call(name, *args, _lib.stream())
    flags = sync.view(U, -1)[:, -1]                          # the error flag word of every utterance
    if cond is not None:
        last_error_flags = flags
    if check and int(flags.abs().max().item()) != 0:
        raise _lib.WavenetHipError(timeout_msg)
    return codes, probs, note_out, prev_out


def _decode(net, state, note0, n_steps, forced=None, want_probs=False, correct_queue=False, temperature=None, seed=0,
            top_k=None, top_p=None, win=None, cond=None):
    """One launch of one utterance on ``state``.  ``forced`` (n_steps,): the next input codes; a negative entry frees its step (the
    launch's own code is fed), an entry >= Q is refused when the tensor is a host tensor."""
    eng = state.eng
    _check_recurrence(eng, correct_queue)
    _check_forced(forced, eng.Q, "wn_decode")
    smp = _Sampling(1, temperature, top_k, top_p, seed, None, eng.device)
    _need_corrected(smp, correct_queue)
    pack = _pack_for(net, eng)
    if state.rw != pack.Rp:
        raise RuntimeError("music_amd.fast_generate: this DecodeState holds %d floats per queue column, the weight pack is laid "
                           "out for %d (built for another engine or decode kernel form)" % (state.rw, pack.Rp))
    sync = getattr(net, "_decode_sync", None)
    n_sync = _lib.decode_sync_granules(eng.N, pack.Dp, eng.S)
    if sync is None or sync.device != eng.device or sync.numel() != n_sync:
        sync = net._decode_sync = torch.zeros(n_sync, dtype=torch.int64, device=eng.device)
    codes, probs, note_out, prev_out = _launch_decode(
        net, eng, smp, state.rings, note0, state.prev, 1, n_steps, state.steps, 1 if correct_queue else 0,
        "wn_decode: a hand-off between the two decode workgroups timed out", check=n_steps >= 4, forced=forced,
        want_probs=want_probs, sync=sync, win=win, cond=cond)
    state.prev = prev_out.view(-1)
    state.steps += n_steps
    return codes[0], probs[0] if want_probs else None, note_out[0]


def _rings_from_workspace(eng, U, T):
    """(U, ring floats) from the workspace of the forward just run over (U, Q, T): the ring of block i of utterance u = the
    last (k-1) d_i columns of that block's INPUT (fast_generate.py:42-47 for k = 2), time-major."""
    ws = eng.workspace(U, T)
    pitch, CH, R, N = ws["pitch"], eng.CH, eng.R, eng.N
    X = ws["X"][SLACK:SLACK + (N + 1) * U * CH * pitch].view(N + 1, U, CH, pitch)
    rw, K1 = _ring_width(eng), _taps(eng)
    return torch.cat([torch.nn.functional.pad(X[i, :, :R, T - K1 * d:T].transpose(1, 2), (0, rw - R)).reshape(U, K1 * d * rw)
                      for i, d in enumerate(eng.dil)], 1).contiguous()


def _prime(net, start_pieces, classes=None, rows=1, phase_pos=None):
    """THE prompt stage of every generator: the full forward over the U start pieces ``(U, Q, receptive_field)`` and the state it
    leaves -> (engine, probabilities (rows U, Q), rings (rows U, ring floats), prev0 (rows U, k-1, Q): the causal layer's queue =
    the last k-1 input columns, oldest first, the classes of the rows).  ``rows`` = 2 is guidance: every utterance becomes a pair of
    rows, as its class and as ``net.null_class``, [c_u, null_class] interleaved, for the forward and for the class tables.
    ``phase_pos``: the stream position of the code the forward predicts (a phase-conditioned model), the same for every row."""
    assert start_pieces.dim() == 3 and start_pieces.size(2) == net.receptive_field
    dev = start_pieces.device if start_pieces.is_cuda else torch.device("cuda")
    x = start_pieces.detach().to(dev).float()
    if rows == 2:
        cls = classes.detach().cpu().tolist() if isinstance(classes, torch.Tensor) else [int(c) for c in classes]
        if len(cls) != x.size(0):
            raise ValueError("music_amd: classes must be %d integers, one per clip" % x.size(0))
        classes = [v for c in cls for v in (int(c), int(net.null_class))]
        x = x.repeat_interleave(2, 0)
    x = x.contiguous()
    with torch.no_grad():
        kw = {} if phase_pos is None else {"phase_pos": int(phase_pos)}
        probs = net(x, **kw) if classes is None else net(x, classes=classes, **kw)     # (rows U, Q): W == 1
    eng, n, T = net._engine, x.size(0), x.size(2)
    return eng, probs.view(n, -1), _rings_from_workspace(eng, n, T), x[:, :, T - _taps(eng):T].transpose(1, 2).contiguous(), classes


def _init_forward(net, note, classes=None, phase_pos=None):
    """The full forward over a ``(1, Q, receptive_field)`` piece: (probabilities (1, Q), the queues it leaves)."""
    eng, probs, rings, prev0, _ = _prime(net, note, classes, phase_pos=phase_pos)
    return probs, DecodeState(eng, rings[0], prev0.view(-1), 0)


def predict_next(net, note, state_queue=None, correct_queue=False):
    """wavenet/fast_generate.py:13-141."""
    if state_queue is None:
        probs, state = _init_forward(net, note)
        _, predict = torch.topk(probs.view(-1), 1)
        return predict.to(note.device), state
    assert note.size()[2] == 1
    eng = net._engine_for(note.device if note.is_cuda else torch.device("cuda"))
    if not isinstance(state_queue, DecodeState):
        state_queue = DecodeState.from_tensors(eng, state_queue)
    note0 = note.detach().to(eng.device).float().reshape(-1).contiguous()
    codes, _, _ = _decode(net, state_queue, note0, 1, correct_queue=correct_queue)
    return codes.to(torch.int64).to(note.device), state_queue


def generate_codes(net, start_piece, note_num, correct_queue=False, temperature=None, seed=0, top_k=None, top_p=None,
                   windows=None, window_pos=0, classes=None, guidance=None, keep=None, phase_pos=None):
    """The greedy loop of fast_generate.py:162-172 as one init forward + ONE persistent launch.
    Returns the note_num generated codes (int64, on the device).
    ``temperature`` (the reference is greedy only): if given and > 0, every code after the
    first is SAMPLED from softmax(logits / temperature), reproducibly for a given ``seed``.
    ``top_k`` / ``top_p``: the distribution is truncated first (include/wavenet_hip.h, wn_decode_batch_samp: the top_k largest
    logits, then the smallest head whose mass reaches top_p, ties kept); corrected recurrence only.
    ``windows`` / ``window_pos``: 1..16 ``(lo, hi)`` pairs and the stream position of the first code returned; the code at
    position p is chosen inside pair ``p % len(windows)`` only, renormalised there (include/wavenet_hip.h,
    wn_win_decode_batch; ``stage_windows`` for a residual quantiser's token stream).  The first code is the first-index argmax
    of the init forward inside its window.  Corrected recurrence only.
    ``classes``: ``[c]``, the class to generate as, for a class-conditional model (required there, refused elsewhere): the init
    forward runs with it and the launch is the conditioned one (wn_decode_batch_cond).  Corrected recurrence only.
    ``guidance``: a scale s, classifier-free guidance (``generate_codes_batch``; the one-utterance batch of it).
    ``keep``: (note_num,) or (1, note_num) integers - partially forced decode (``generate_codes_batch``).
    ``phase_pos``: the stream position of the first code returned, for a phase-conditioned model (required there, refused
    elsewhere; ``window_pos``'s convention): the code at position p is conditioned on phase p mod phase_period.  The start piece's
    positions lie in front of it, mod the period - also where that is in front of stream position 0.  Corrected recurrence only."""
    if guidance is not None:
        return generate_codes_batch(net, start_piece, note_num, correct_queue=correct_queue, temperature=temperature, seed=seed,
                                    top_k=top_k, top_p=top_p, windows=windows, window_pos=window_pos, classes=classes,
                                    guidance=guidance, **({} if keep is None else {"keep": keep}),
                                    **({} if phase_pos is None else {"phase_pos": phase_pos}))[0]
    win = _windows_of(windows, window_pos, net.quantization_channels, correct_queue)
    _check_classes(net, classes)
    _check_phase(net, phase_pos)
    if phase_pos is not None:
        _corrected_only(correct_queue, "a phase-conditioned model decodes", "wn_decode_batch_cond")
    kept = _keep_of(keep, 1, note_num, net.quantization_channels, win, correct_queue)
    probs, state = _init_forward(net, start_piece, classes, phase_pos)
    # (the plain call picks as predict_next does, with the reference's topk: the argmax, whatever either makes of a tie)
    first = torch.topk(probs.view(-1), 1)[1] if win is None and classes is None and phase_pos is None else _first_codes(probs, win)
    eng = state.eng
    cond, tables = _class_cond(net, eng, classes, 1, correct_queue, None if phase_pos is None else phase_pos + 1)
    if kept is not None and note_num >= 1:
        first = _resolved(kept[:, 0], first)
    if note_num <= 1:
        return first[:note_num]
    codes, _, _ = _decode(net, state, _note0(first, 1, eng.Q, eng.device)[0], note_num - 1, correct_queue=correct_queue,
                          temperature=temperature, seed=seed, top_k=top_k, top_p=top_p, win=win.tail(1) if win is not None else None,
                          cond=cond, **({} if kept is None else {"forced": kept[0, 1:].to(torch.int32)}))
    codes = codes.to(torch.int64)
    return torch.cat([first.to(torch.int64), codes if kept is None else _resolved(kept[0, 1:], codes)])


def generate_codes_batch(net, start_pieces, note_num, correct_queue=False, temperature=None, seed=0, top_k=None, top_p=None,
                         streams=None, windows=None, window_pos=0, classes=None, guidance=None, keep=None, phase_pos=None):
    """SURVEY 8f2 (batched utterances; the reference generates one at a time): greedy generation of
    ``note_num`` codes for U independent start pieces ``(U, Q, receptive_field)`` in ONE persistent
    launch - on the matrix-core path eight utterances to a workgroup pair, one pair of MFMA result columns each (else one
    pair per utterance), the weights are shared.  Returns int64
    ``(U, note_num)`` on the device; row u equals ``generate_codes(net, start_pieces[u:u+1], note_num)``.
    ``temperature``, ``top_k``, ``top_p`` and ``seed`` may each be a scalar or one value per utterance (a sweep of settings
    over one prompt, N takes of one prompt); ``streams``: the random-number stream id of every utterance (default: its
    index; row u is then the single-utterance launch with ``streams=[u]``, bit for bit when both run the same kernel form,
    see WN_DEC_KS).  Truncation and per-utterance settings run on the corrected recurrence only.
    ``windows`` / ``window_pos``: as in ``generate_codes``; one table and one position for the whole launch.
    ``classes``: one class per utterance for a class-conditional model, every utterance with its own tables.
    ``guidance``: None, a scale s or one per utterance - classifier-free guidance (include/wavenet_hip.h, wn_cfg_decode_batch) on a
    model with ``null_class``: every utterance is decoded as a PAIR of rows, as its class and as null_class, each on its own queues
    and tables; the ONE code per step is picked from l_c + (s - 1)(l_c - l_u) with the utterance's settings and fed to both.  s = 1
    is the conditional model, s > 1 more of the class, s = 0 the unconditional model; half as many utterances fit a launch.
    Corrected recurrence only; None is the call without the argument, launch for launch.
    ``keep``: (U, note_num) integers - partially forced decode (include/wavenet_hip.h, wn_decode: a negative ``forced`` entry frees its
    step).  ``keep[u][j] >= 0`` IS the code returned at position j and what the model is fed there; -1 is the sampler's choice
    (position 0: the init forward's pick).  The launch still draws at every step - a stream's random numbers do not move with the
    mask - and the function returns the fed stream, ``where(keep >= 0, keep, codes)``.  Under ``windows`` a kept token outside the
    window of its position ``window_pos + j`` is a ValueError before any launch (``check_keep``); under ``guidance`` both rows of a
    pair are fed the utterance's row.  Fill the absent stages of a residual-VQ stream, continue a prompt of any length, regenerate
    single positions - in the one launch.  Corrected recurrence only; None is the call without the argument.
    ``phase_pos``: as in ``generate_codes``; one position for the whole launch.  Under ``guidance`` the unconditional member's table
    is the null class's column plus the phase column."""
    assert start_pieces.dim() == 3 and start_pieces.size(2) == net.receptive_field
    _check_classes(net, classes)
    _check_phase(net, phase_pos)
    if phase_pos is not None:
        _corrected_only(correct_queue, "a phase-conditioned model decodes", "wn_decode_batch_cond")
    win = _windows_of(windows, window_pos, net.quantization_channels, correct_queue)
    U = start_pieces.size(0)
    kept = _keep_of(keep, U, note_num, net.quantization_channels, win, correct_queue)
    guide = _guidance_of(net, guidance, U, correct_queue, classes)
    rows = 1 if guide is None else 2                                # guided: every utterance is a pair of rows [c_u, null_class]
    if rows * U > 1024:
        raise ValueError("at most 1024 utterances per launch (128 off the matrix-core path)" if guide is None else
                         "at most 512 guided utterances per launch (64 off the matrix-core path): every one is a pair of rows")
    eng, probs, rings, prev0, row_classes = _prime(net, start_pieces, classes, rows, phase_pos)
    cond, tables = _class_cond(net, eng, row_classes, rows * U, correct_queue, None if phase_pos is None else phase_pos + 1)
    first = _first_codes(probs, win, guide)
    if kept is not None and note_num >= 1:
        first = _resolved(kept[:, 0], first)
    if note_num <= 1:
        return first.view(U, 1)[:, :note_num]
    _check_recurrence(eng, correct_queue)
    dev = eng.device
    if guide is not None:
        # both members of a pair carry the utterance's settings and stream id (the launch reads the conditional member's)
        pair = lambda v: v if _per_row(v, U) is None else [e for e in _per_row(v, U) for _ in (0, 1)]
        temperature, top_k, top_p, seed = pair(temperature), pair(top_k), pair(top_p), pair(seed)
        streams = pair(list(range(U)) if streams is None else streams)
    smp = _Sampling(rows * U, temperature, top_k, top_p, seed, streams, dev)
    _need_corrected(smp, correct_queue)
    codes, _, _, _ = _launch_decode(net, eng, smp, rings, _note0(first, rows, eng.Q, dev), prev0, rows * U, note_num - 1, 0,
                                    1 if correct_queue else 0, "%s: a hand-off between two decode workgroups timed out"
                                    % ("wn_decode_batch" if guide is None else "wn_cfg_decode_batch"), check=note_num - 1 >= 4,
                                    win=win.tail(1) if win is not None else None, cond=cond,
                                    guide=None if guide is None else torch.tensor(guide, dtype=torch.float32, device=dev),
                                    **({} if kept is None else {"forced": kept[:, 1:].to(torch.int32).repeat_interleave(rows, 0)}))
    codes = codes[0::rows].to(torch.int64)
    return torch.cat([first.view(U, 1).to(torch.int64), codes if kept is None else _resolved(kept[:, 1:], codes)], 1)


def decode_batch_cond(net, rings, prev0, note0, n_steps, step0=0, pos0=0, forced=None, want_probs=False, temperature=None,
                      seed=0, cond_fg=None, cond_p1=None, schedule=None, top_k=None, top_p=None, streams=None, windows=None,
                      window_pos=0, guidance=None, phase_pos=None, classes=None):
    """One persistent launch of wn_decode_batch_cond (corrected recurrence) for U utterances from explicit state: ``rings``
    (U, ring floats) is advanced in place, ``prev0`` (U, k-1, Q) / ``note0`` (U, Q) are the causal layer's history and the
    first input column.  ``cond_fg`` (U, N, Le, 2 Dp) rows [f | g] and ``cond_p1`` (U, Le, S) are the per-utterance
    conditioning tables (Dp = the decode pack's dilation width), ``schedule`` the N + 1 (shift, q, Le) triples of
    ``ae_generate.cond_schedule``; step s is output position pos0 + s.  ``forced`` (U, n_steps): the next input codes; a
    negative entry frees its step - the launch's own code is fed, as without ``forced`` (include/wavenet_hip.h, wn_decode) -, an entry
    >= Q is refused when the tensor is a host tensor (a device tensor travels as it is, no synchronisation).
    ``temperature`` / ``top_k`` / ``top_p`` / ``seed``: scalars or one value per utterance, ``streams`` the random-number stream
    ids (default: the utterance index); anything beyond a scalar temperature and seed goes through wn_decode_batch_samp.
    ``windows`` / ``window_pos``: position windows shared by the launch, step s samples inside pair ``(window_pos + s) %
    len(windows)`` (wn_win_decode_batch; independent of ``step0`` and ``pos0``).
    ``guidance``: (U / 2,) scales - the rows are (conditional, unconditional) pairs with equal ``note0`` / ``prev0`` / ``forced``
    rows, decoded by wn_cfg_decode_batch; every output comes back for all U rows.
    ``phase_pos``: for a phase-conditioned model (required there, refused elsewhere) the stream position of output position 0 - step
    s chooses the token at stream position phase_pos + pos0 + s - with ``classes``, one per row, where the model has classes too; the
    tables are built here (``cond_fg`` / ``cond_p1`` / ``schedule`` stay None).  Priming steps (pos0 < 0) may lie in front of stream
    position 0: the phase is periodic.
    Returns (codes int32 (U, n_steps), probabilities (U, n_steps, Q) or None, note_out, prev_out)."""
    eng = net._engine_for(rings.device)
    pack = _pack_for(net, eng)
    dev, N, U = eng.device, eng.N, rings.size(0)
    n_ring = max(1, int(_ring_offsets(eng)[-1]))
    if rings.dim() != 2 or rings.size(1) != n_ring or not rings.is_contiguous():
        raise ValueError("decode_batch_cond: rings must be (U, %d) contiguous floats" % n_ring)
    if U > (1024 if pack.mfma else 128):
        raise ValueError("at most 1024 utterances per launch (128 off the matrix-core path)")
    smp = _Sampling(U, temperature, top_k, top_p, seed, streams, dev)
    win = _windows_of(windows, window_pos, eng.Q)
    _check_phase(net, phase_pos)
    if phase_pos is None and classes is not None:
        raise ValueError("decode_batch_cond: classes= comes with phase_pos= (a class-conditional model's own tables are the caller's)")
    le = 1
    shift = qs = None
    if cond_fg is not None or cond_p1 is not None:
        if schedule is None or len(schedule) != N + 1:
            raise ValueError("decode_batch_cond: conditioning tables need a schedule of N + 1 (shift, q, Le) triples")
        le = int(schedule[0][2])
        if cond_fg is not None and (tuple(cond_fg.shape) != (U, N, le, 2 * pack.Dp) or not cond_fg.is_contiguous()):
            raise ValueError("decode_batch_cond: cond_fg must be (U, N, Le, %d) contiguous" % (2 * pack.Dp))
        if cond_p1 is not None and (tuple(cond_p1.shape) != (U, le, eng.S) or not cond_p1.is_contiguous()):
            raise ValueError("decode_batch_cond: cond_p1 must be (U, Le, S) contiguous")
        shift = ctypes.cast((ctypes.c_int32 * (N + 1))(*[int(t[0]) for t in schedule]), ctypes.c_void_p)
        qs = ctypes.cast((ctypes.c_int32 * (N + 1))(*[int(t[1]) for t in schedule]), ctypes.c_void_p)
    assert forced is None or tuple(forced.shape) == (U, n_steps)
    _check_forced(forced, eng.Q, "decode_batch_cond")
    gtab = None
    if guidance is not None:
        gtab = torch.as_tensor(guidance, dtype=torch.float32).to(dev).contiguous()
        if U % 2 or tuple(gtab.shape) != (U // 2,):
            raise ValueError("decode_batch_cond: guidance must hold one scale per pair of rows (U / 2 = %s of them, U even)" % (U / 2,))
    cond = (ptr(cond_fg), cond_fg[0].numel() if cond_fg is not None else 0, ptr(cond_p1),
            cond_p1[0].numel() if cond_p1 is not None else 0, shift, qs, le, int(pos0))
    if phase_pos is not None:
        if cond_fg is not None or cond_p1 is not None or schedule is not None:
            raise ValueError("decode_batch_cond: with phase_pos= the tables are the model's own: pass no cond_fg, cond_p1 or schedule")
        _check_classes(net, classes)
        cond, tables = _class_cond(net, eng, classes, U, True, int(phase_pos) + int(pos0))
    return _launch_decode(net, eng, smp, rings, note0, prev0, U, n_steps, step0, 1,
                          "wn_decode_batch_cond: a hand-off between two decode workgroups timed out", forced=forced,
                          want_probs=want_probs, cond=cond, win=win.tail() if win is not None else None, guide=gtab)


def sample_logits(logits, temperature=1.0, top_k=None, top_p=None, seed=0, step0=0, u=None, want_probs=False, streams=None,
                  windows=None, window_pos=0, guidance=None, logits_u=None):
    """The decoder's sampler (the same device function, wn_sample_logits) on a matrix of pre-softmax logits ``(n, Q)``,
    Q <= 1024: row i is drawn as "step" ``step0 + i``.  ``temperature`` (<= 0 / None: greedy argmax), ``top_k``, ``top_p`` and
    ``seed`` may each be a scalar or one value per row (``streams``: the rows' random-number stream ids, default 0);
    ``u`` (n,) replaces the generated uniform numbers.  ``windows`` / ``window_pos``: row i samples inside pair ``(window_pos +
    i) % len(windows)`` of the table (wn_win_sample_logits), independent of ``step0``.  Returns the codes (int64, on the device), with ``want_probs`` also the
    distributions drawn from ``(n, Q)``.  This is what a one-forward-per-sample generator calls on the forward's logits.
    ``guidance`` (a scale or one per row) with ``logits_u`` (n, Q): classifier-free guidance - ``logits`` are the conditional
    model's, ``logits_u`` the unconditional one's, row i is drawn from l_c + (s_i - 1)(l_c - l_u) (wn_cfg_sample_logits)."""
    if logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("sample_logits: logits must be a (n, Q) device tensor")
    x = logits.detach().float()
    if x.size(1) > 0 and x.stride(1) != 1:
        x = x.contiguous()
    n, Q = x.shape
    if not 1 <= Q <= 1024:
        raise ValueError("sample_logits: 1 <= Q <= 1024")
    smp = _Sampling(n, temperature, top_k, top_p, seed, streams, x.device, default_stream=0)
    win = _windows_of(windows, window_pos, Q)
    u_t = None
    if u is not None:
        u_t = torch.as_tensor(u, dtype=torch.float32).to(x.device).contiguous()
        if tuple(u_t.shape) != (n,):
            raise ValueError("sample_logits: u must hold one number per row")
    codes = torch.empty(n, dtype=torch.int32, device=x.device)
    probs = torch.empty(n, Q, dtype=torch.float32, device=x.device) if want_probs else None
    if (guidance is None) != (logits_u is None):
        raise ValueError("sample_logits: guidance= and logits_u= come together (the scales and the unconditional model's logits)")
    if guidance is not None:
        if not isinstance(logits_u, torch.Tensor) or tuple(logits_u.shape) != (n, Q) or logits_u.device != x.device:
            raise ValueError("sample_logits: logits_u must be a (%d, %d) tensor on the device of logits" % (n, Q))
        x, xu = x.contiguous(), logits_u.detach().float().contiguous()
        g = torch.as_tensor(guidance, dtype=torch.float32).reshape(-1)
        g = (g.expand(n) if g.numel() == 1 else g).to(x.device).contiguous()
        if tuple(g.shape) != (n,) or not bool(torch.isfinite(g).all()):
            raise ValueError("sample_logits: guidance must be a finite number or one per row")
    args = (ptr(x), n, Q, x.stride(0) if n > 1 else max(Q, x.stride(0)), ptr(smp.table), smp.temperature, smp.seed, int(smp.top_k),
            float(smp.top_p), int(step0), ptr(u_t), ptr(codes), ptr(probs))
    if guidance is not None:
        call("wn_cfg_sample_logits", *args, *(win.tail() if win is not None else _NO_WIN), ptr(xu), ptr(g), _lib.stream())
    elif win is None:
        call("wn_sample_logits", *args, _lib.stream())
    else:
        call("wn_win_sample_logits", *args, *win.tail(), _lib.stream())
    codes = codes.to(torch.int64)
    return (codes, probs) if want_probs else codes


def generate(model_path, model_name, generate_path, generate_name, start_piece=None, sr=16000, duration=10, temperature=None,
             seed=0, top_k=None, top_p=None, classes=None, guidance=None, phase_pos=None):
    """wavenet/fast_generate.py:144-179.  ``temperature`` / ``top_k`` / ``top_p`` / ``seed``: sample instead of the greedy
    argmax; a filter selects the corrected queue recurrence (the only one truncated sampling runs on).  ``classes``: ``[c]``, the
    class to generate as (a model whose parameters set "global_classes"; corrected recurrence).  ``guidance``: a classifier-free
    guidance scale (``generate_codes``; the model's parameters set "null_class").  ``phase_pos``: the stream position of the first
    code generated (a model whose parameters set "phase_period"; corrected recurrence)."""
    if os.path.exists(generate_path) is False:
        os.makedirs(generate_path)
    with open('./params/wavenet_params.json', 'r') as f:
        params = json.load(f)
    net = wavenet(**params)
    net = load_model(net, model_path, model_name)
    if net is None:
        raise FileNotFoundError(model_path + model_name)
    net = net.cuda()
    if start_piece is None:
        Q = net.quantization_channels
        start_piece = torch.zeros(1, Q, net.receptive_field)
        start_piece[:, Q // 2, :] = 1.0
    # the as-written queue push exists for filter_width 2 only; every other width runs the corrected recurrence
    generated_piece = generate_codes(net, start_piece.cuda(), duration * sr,
                                     correct_queue=(net.filter_width != 2 or top_k is not None or top_p is not None
                                                    or classes is not None or guidance is not None or phase_pos is not None),
                                     temperature=temperature, seed=seed, top_k=top_k, top_p=top_p, classes=classes, guidance=guidance,
                                     **({} if phase_pos is None else {"phase_pos": phase_pos}))
    print(generated_piece.tolist()[:32], "...")
    audio = mu_law_decode(generated_piece, net.quantization_channels).cpu().numpy()
    from scipy.io import wavfile
    wavfile.write(generate_path + generate_name, sr, audio.astype(np.float32))
    return generated_piece
