"""The complete launch trace of a fast engine's step, recorded on the CPU (tests/test_launch_trace.py compares it with
tests/golden/launch_traces.json and, for the forms of the skip epilogue that file does not reach, launch_traces_epilogue.json;
tools/record_launch_trace.py writes those files and dumps the trace of any checkout).

Nothing is launched and no device is touched: the engines are built on device="cpu" with `call` replaced
(test_engine_base.patch_calls), `ptr` replaced by a marker that remembers its tensor, and the streams, events, the step throttle
and the autoencoder's pinned staging stubbed.  A trace is the ordered list of

    ["call", entry point, stream label, canonical arguments]     "main" / "side": what _lib.stream() returned for the launch
    ["record" | "wait", stream label, event number]             events are numbered in the order they are created
    ["mark", name]                                              with fine_marks on

A pointer is written as [owner key, element offset]: the owner is the first tensor among the engine's attributes, `ws` and `bw`
(lists, tuples and dicts included, keys sorted) whose memory holds the address; a tensor no owner holds any more (d_tab, d_enf,
a replaced table) is "tmp<k>" in order of first appearance.  None stays None, ctypes arrays are written out as lists."""
import ctypes
import hashlib
import json
import re
import sys
from contextlib import contextmanager

import numpy as np
import torch

from tests.test_engine_base import CASES, _ae_net, patch_calls

SWITCHES = ("WN_PQ_BWD", "WN_MS_BWD", "WN_PAIR32", "WN_PQ_CHAIN", "WN_ENC_LCH", "WN_AE_ENC_PQ", "WN_AE_FUSED_ENC", "WN_EPI_WGRAD_CHUNKS",
            "WN_EPI_FUSED", "WN_EPI_FUSED_BWD", "WN_EPI_BWD_ORDER", "WN_AE_COND_MFMA", "WN_MAX_STEPS_IN_FLIGHT")
WN_DIL, WN_T, AE_T = [1, 2, 4, 32, 64], 1200, 400
SIX, AE_SIX = WN_DIL + [1], [1, 2, 32, 33, 1, 2]


class OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda with True (the engines assert it of their inputs)."""
    is_cuda = property(lambda self: True)


def on_device(t):
    return t.as_subclass(OnDevice)


class Ptr:
    """What ptr(t, offset) returns here: the tensor (kept alive, so that no two temporaries share an address) and the byte address."""

    def __init__(self, t, addr):
        self.t, self.addr = t, addr

    def __add__(self, nbytes):
        return Ptr(self.t, self.addr + nbytes)

    __radd__ = __add__


def _ptr(t, offset=0):
    return None if t is None else Ptr(t, t.data_ptr() + offset * t.element_size())


class _Stream:
    def __init__(self, label, trace):
        self.label, self.trace = label, trace

    def wait_event(self, ev):
        self.trace.append(("wait", self.label, ev.n))


def install(monkeypatch):
    """Replace everything that would touch a device -> the trace list the launches, events and marks are appended to."""
    from music_amd import _lib, engine_base, model1
    trace = patch_calls(monkeypatch)
    real_ptr = _lib.ptr
    for name, mod in list(sys.modules.items()):
        if name.startswith("music_amd") and getattr(mod, "ptr", None) is real_ptr:
            monkeypatch.setattr(mod, "ptr", _ptr)
    main, side = _Stream("main", trace), _Stream("side", trace)
    current, events = [main], [0]

    class Event:
        def __init__(self, enable_timing=False):
            self.n = events[0]
            events[0] += 1

        def record(self, stream=None):
            trace.append(("record", (stream or current[-1]).label, self.n))

        def synchronize(self):
            pass

    @contextmanager
    def use(stream):
        current.append(stream)
        try:
            yield
        finally:
            current.pop()

    class Throttle:
        def enter(self):
            pass

        leave = enter

    def stage_cond(self, cond):
        N = self.N
        return (torch.stack([c[0][:, :, 0] for c in cond[:N]]), torch.stack([c[1] for c in cond[:N]]), cond[N][0].clone(), cond[N][1].clone())

    def mark(self, name):
        if self.marks is not None and (self.mark_only is None or name in self.mark_only):
            trace.append(("mark", name))

    monkeypatch.setattr(_lib, "stream", lambda: current[-1].label)
    monkeypatch.setattr(_lib, "side_stream", lambda device: side)
    monkeypatch.setattr(_lib, "StepThrottle", Throttle)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: current[-1])
    monkeypatch.setattr(torch.cuda, "stream", use)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(engine_base.EngineBase, "mark", mark)
    monkeypatch.setattr(model1._AutoencoderEngine, "_stage_cond", stage_cond)
    return trace


# ---------------------------------------------------------------- canonical form
def _tensors(obj, key, out):
    if isinstance(obj, torch.Tensor):
        out.append((key, obj))
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            _tensors(obj[k], "%s.%s" % (key, k), out)
    elif isinstance(obj, (list, tuple)):
        for k, v in enumerate(obj):
            _tensors(v, "%s.%d" % (key, k), out)


def owners(eng, ws):
    out = []
    _tensors(vars(eng), "eng", out)
    _tensors({k: v for k, v in ws.items() if k != "bwd"}, "ws", out)
    _tensors(ws.get("bwd") or {}, "bw", out)
    return [(key, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for key, t in out if t.numel()]


def canonical(trace, eng, ws):
    own, tmp = owners(eng, ws), {}

    def arg(a):
        if isinstance(a, Ptr):
            size = a.t.element_size()
            for key, lo, hi in own:
                if lo <= a.addr < hi:
                    return [key, (a.addr - lo) // size]
            base = a.t.untyped_storage().data_ptr()
            return [tmp.setdefault(base, "tmp%d" % len(tmp)), (a.addr - base) // size]
        if isinstance(a, ctypes.Array):
            return list(a)
        assert a is None or isinstance(a, (int, float, str)), a
        assert not isinstance(a, int) or abs(a) < 1 << 40, "a raw address among the arguments: %r" % (a,)
        return a

    out = []
    for item in trace:
        if item[0] in ("record", "wait", "mark"):
            out.append(list(item))
        else:
            name, args = item
            labels = [a for a in args if isinstance(a, str)]
            out.append(["call", name, labels[-1] if labels else None, [arg(a) for a in args]])
    return out


PACK_KEYS = r"pk\w*_(idx|off)|gp_off|gidx\w*|wt_idx"
PACK_KEYS_ALL = PACK_KEYS + r"|bfg_idx|gp_bias_off"       # the second file's: the bias maps too


def pack_maps(eng, keys=PACK_KEYS):
    """SHA-256 of every index map _build_packs produces (pk*_idx, pk*_off, gp_off, gidx*, wt_idx)."""
    def plain(v):
        if isinstance(v, torch.Tensor):
            a = v.numpy()
            return [str(a.dtype), list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()]
        if isinstance(v, dict):
            return {str(k): plain(v[k]) for k in sorted(v)}
        return v
    maps = {k: plain(v) for k, v in sorted(vars(eng).items()) if re.fullmatch(keys, k)}
    return {k: hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest() for k, v in maps.items()}


# ---------------------------------------------------------------- the cases
def _wn(ch, dil=WN_DIL, **kw):
    from music_amd.engine import WaveNetEngine
    return WaveNetEngine(dil, ch, ch, 256, device="cpu", **kw)


def _ae(en, de, **kw):
    from music_amd.model1 import _AutoencoderEngine
    net = _ae_net(en, de, **kw)
    eng = _AutoencoderEngine(net, torch.device("cpu"))
    torch.manual_seed(3)
    eng.cond = None if eng.learned else [tuple(c) for c in net._draw_conditioning()]
    return eng


def _with(eng, **attrs):
    """the engine with the switches a test or tool sets as attributes"""
    for k, v in attrs.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    return eng


def _input(eng, B, T):
    W = T - eng.rf + 1
    return on_device(torch.zeros(B, 256, T)), on_device(torch.zeros(B * W, dtype=torch.int64))


def _wn_step(B, how="dense"):
    def run(eng):
        if how == "pair_fwd":
            # the forward pairs only where that fills the chip (100 000 samples at this batch): planned by hand on the pooled workspace
            ws = eng._ws.get(B, WN_T)
            assert ws["pair"] and not ws["pair_fwd"]
            ws["pair_fwd"] = True
        x, target = _input(eng, B, WN_T)
        codes = on_device(torch.zeros(B, WN_T, dtype=torch.int32))
        if how == "codes":
            eng.loss_and_grad_codes(codes, target)
        elif how == "tagged":
            x = on_device(eng.onehot(codes))                 # (the subclass view does not carry the tag over: the same tag again)
            x._wn_codes = (codes, True, x._version, codes._version)
            eng.loss_and_grad(x, target)
        else:
            eng.loss_and_grad(x, target)
        return eng._ws.peek(B, WN_T)
    return run


def _wn_fwd_bwd(B):
    def run(eng):
        probs, ws = eng.forward(_input(eng, B, WN_T)[0])
        eng.backward(ws, torch.zeros_like(probs))
        return ws
    return run


def _ae_step(B):
    def run(eng):
        x, target = _input(eng, B, AE_T)
        eng.loss_and_grad(x, target, eng.cond)
        return eng._ws.peek(B, AE_T)
    return run


def _ae_fwd_bwd(B):
    def run(eng):
        probs, _, ws = eng.forward(_input(eng, B, AE_T)[0], eng.cond)
        eng.backward(ws, torch.zeros_like(probs))
        return ws
    return run


def _env(name):
    return CASES[name][0]


# name -> (environment switches, engine builder, run -> workspace).  The ten fast-engine cases of test_engine_base.CASES with
# their dilations, T and batch (the long encoding is a real one here: pool 8 gives 41 pooled frames, above the 32 buckets of
# `cidx`), the one-launch case of each engine once more as forward() + backward(dprobs), the WaveNet pair case once more with
# the forward blocks paired too, and four further forms
TRACE_CASES = {
    "wavenet64": (_env("wavenet64"), lambda: _wn(64), _wn_step(2)),
    "wavenet64_fwd_bwd": (_env("wavenet64"), lambda: _wn(64), _wn_fwd_bwd(2)),
    "wavenet64_channel_split": (_env("wavenet64_channel_split"), lambda: _wn(64), _wn_step(2)),
    "wavenet64_chunk512": (_env("wavenet64_chunk512"), lambda: _wn(64), _wn_step(2)),
    "wavenet32_pair": (_env("wavenet32_pair"), lambda: _wn(32), _wn_step(2)),
    "wavenet32_pair_fwd": (_env("wavenet32_pair"), lambda: _wn(32), _wn_step(2, "pair_fwd")),
    "wavenet32_odd_batch": (_env("wavenet32_odd_batch"), lambda: _wn(32), _wn_step(3)),
    "autoencoder32_pair": (_env("autoencoder32_pair"), lambda: _ae(32, 32), _ae_step(2)),
    "autoencoder32_odd_batch": (_env("autoencoder32_odd_batch"), lambda: _ae(32, 32), _ae_step(3)),
    "autoencoder64": (_env("autoencoder64"), lambda: _ae(64, 64), _ae_step(2)),
    "autoencoder64_fwd_bwd": (_env("autoencoder64"), lambda: _ae(64, 64), _ae_fwd_bwd(2)),
    "autoencoder64_long_encoding": (_env("autoencoder64_long_encoding"), lambda: _ae(64, 64, en_pool_kernel_size=8), _ae_step(2)),
    "autoencoder_en32_de64": (_env("autoencoder_en32_de64"), lambda: _ae(32, 64), _ae_step(2)),
    "wavenet64_bias": ({}, lambda: _wn(64, use_bias=True), _wn_step(2)),
    "autoencoder64_bias": ({}, lambda: _ae(64, 64, use_bias=True), _ae_step(2)),
    "wavenet64_codes": ({}, lambda: _wn(64), _wn_step(2, "codes")),
    "wavenet64_onehot_tag": ({}, lambda: _wn(64), _wn_step(2, "tagged")),
}

# The forms of the skip epilogue (and learned conditioning) that none of the cases above runs, same shapes: recorded into
# tests/golden/launch_traces_epilogue.json, with every pack map hashed (PACK_KEYS_ALL)
EPILOGUE_CASES = {
    "wavenet64_epi3": ({"WN_EPI_FUSED": "0"}, lambda: _wn(64), _wn_step(2)),                       # two chains on two streams
    "wavenet64_epi3_one_chain": ({"WN_EPI_FUSED": "0"}, lambda: _with(_wn(64), epi_chains=1), _wn_step(2)),
    "wavenet64_bias_epi3": ({"WN_EPI_FUSED": "0"}, lambda: _wn(64, use_bias=True), _wn_step(2)),   # the summed skip bias enters the chain
    "wavenet64_epi_bwd3": ({"WN_EPI_FUSED_BWD": "0"}, lambda: _wn(64), _wn_step(2)),
    "wavenet64_epi_bwd_order0": ({"WN_EPI_BWD_ORDER": "0"}, lambda: _wn(64), _wn_step(2)),
    "autoencoder64_epi_bwd3": ({"WN_EPI_FUSED_BWD": "0"}, lambda: _ae(64, 64), _ae_step(2)),
    "autoencoder64_bias_epi_bwd3": ({"WN_EPI_FUSED_BWD": "0"}, lambda: _ae(64, 64, use_bias=True), _ae_step(2)),
    "autoencoder64_no_overlap": ({}, lambda: _with(_ae(64, 64), overlap_wgrad=False), _ae_step(2)),   # one forward chain, all on main
    "autoencoder64_learned": ({}, lambda: _ae(64, 64, conditioning="learned"), _ae_step(2)),
    # wn_skip_epilogue_bwd takes the skip product's 16-row tiles three at a time: five (or the autoencoder's four) blocks of 64
    # channels never reach it, whatever the switches say - the four cases above with WN_EPI_FUSED_BWD / WN_EPI_BWD_ORDER run the
    # three launches.  Six blocks do, the autoencoder with 256 skip channels
    "wavenet64_six_blocks": ({}, lambda: _wn(64, SIX), _wn_step(2)),
    "wavenet64_six_blocks_bwd_order0": ({"WN_EPI_BWD_ORDER": "0"}, lambda: _wn(64, SIX), _wn_step(2)),
    "wavenet64_six_blocks_epi_bwd3": ({"WN_EPI_FUSED_BWD": "0"}, lambda: _wn(64, SIX), _wn_step(2)),
    "autoencoder64_six_blocks": ({}, lambda: _ae(64, 64, dilations=AE_SIX, de_skip_channel=256), _ae_step(2)),
    "autoencoder64_six_blocks_bias": ({}, lambda: _ae(64, 64, dilations=AE_SIX, de_skip_channel=256, use_bias=True), _ae_step(2)),
    "autoencoder64_six_blocks_epi_bwd3": ({"WN_EPI_FUSED_BWD": "0"}, lambda: _ae(64, 64, dilations=AE_SIX, de_skip_channel=256), _ae_step(2)),
}
# ... and of the two general engines the pack maps alone (they are built from the same pack builder): name -> builder of (engine, _)
PACK_CASES = {name: CASES[name] for name in ("general_wavenet", "general_autoencoder")}


def record_packs(name, monkeypatch):
    """-> pack-map hashes (PACK_KEYS_ALL) of one general engine."""
    env, build = PACK_CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    patch_calls(monkeypatch)
    return pack_maps(build()[0], PACK_KEYS_ALL)


def record(name, monkeypatch):
    """-> (canonical trace, pack-map hashes, forms of the workspace) of one case."""
    env, build, run = TRACE_CASES[name] if name in TRACE_CASES else EPILOGUE_CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trace = install(monkeypatch)
    eng = build()
    eng.marks = []
    eng.fine_marks = True
    del trace[:]
    ws = run(eng)
    bw = ws["bwd"]
    forms = {k: v for k, v in list(ws.items()) + list(bw.items())
             if k in ("pair", "pair_fwd", "ms", "pq", "chain", "enc_chain", "enc_pq", "enc_fused")}
    forms["cidx"] = "cidx" in ws
    return canonical(trace, eng, ws), pack_maps(eng, PACK_KEYS if name in TRACE_CASES else PACK_KEYS_ALL), forms


def digest(trace):
    return hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()
