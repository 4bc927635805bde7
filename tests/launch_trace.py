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
a replaced table) is "tmp<k>" in order of first appearance.  None stays None, ctypes arrays are written out as lists.  A raw
address (the data_ptr() integers the flat optimizers and GradGuard pass) inside an owner's memory is written exactly as a pointer is,
so code may pass either; any other integer of 2^40 or more fails the recording.

A third set, the optimizer steps (OPTIMIZER_CASES, record_optimizer, tests/golden/launch_traces_optimizers.json), and a fourth, the
generators (DECODE_CASES, record_decode, tests/golden/launch_traces_decode.json), are at the end."""
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


def _span(key, t):
    return key, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), t.element_size()


def owners(eng, ws):
    out = []
    _tensors(vars(eng), "eng", out)
    _tensors({k: v for k, v in ws.items() if k != "bwd"}, "ws", out)
    _tensors(ws.get("bwd") or {}, "bw", out)
    return [_span(key, t) for key, t in out if t.numel()]


def canonical(trace, eng, ws, own=None, tmp=None):
    """`own`: the owners (default: the engine's and the workspace's); `tmp`: the names of tensors no owner holds, carried over where
    a case is canonicalised in pieces.  A raw address (an int, what data_ptr() gives) inside an owner's memory is named as a Ptr is."""
    own, tmp = owners(eng, ws) if own is None else own, {} if tmp is None else tmp

    def arg(a):
        if isinstance(a, Ptr):
            size = a.t.element_size()
            for key, lo, hi, _ in own:
                if lo <= a.addr < hi:
                    return [key, (a.addr - lo) // size]
            base = a.t.untyped_storage().data_ptr()
            return [tmp.setdefault(base, "tmp%d" % len(tmp)), (a.addr - base) // size]
        if isinstance(a, ctypes.Array):
            return list(a)
        assert a is None or isinstance(a, (int, float, str)), a
        if isinstance(a, int):
            for key, lo, hi, size in own:
                if lo <= a < hi:
                    return [key, (a - lo) // size]
            assert abs(a) < 1 << 40, "a raw address among the arguments: %r" % (a,)
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


# ---------------------------------------------------------------- the optimizer steps (tests/golden/launch_traces_optimizers.json)
# What ends a training step: the flat optimizers of music_amd/train.py and the fused step's adam_step, plain and guarded, with and
# without an EMA shadow, on a model whose codebook follows EMA updates or not.  The engines are built on the CPU as in
# test_vq_ema_model_cpu (net._engine = Engine(net, cpu); parameters and gradients are views of eng.flat / eng.flat_grad), the guard is
# the real GradGuard on device="cpu".  No launch runs, so the recorder plays the device's one part the host later reads back: every
# wn_grad_guard issued counts as a step TAKEN (the gradients here are finite) in the guard's state block.
GUARD = dict(max_grad_norm=1.0, skip_nonfinite=True)
SHADOW = dict(ema_decay=0.99, ema_warmup=True)
OPT_DIL, OPT_K = [1, 2], 24
STANDARD = ("flat", "flat", "foreign", "flat", "reload", "flat")


def _opt_net(ae=False):
    """-> (module, its engine on the CPU), the parameters being views of eng.flat"""
    if ae:
        from music_amd.model1 import _AutoencoderEngine
        net = _ae_net(64, 64, conditioning="learned", bottleneck="vq", vq_codes=OPT_K, vq_update="ema")
        eng = net._engine = _AutoencoderEngine(net, torch.device("cpu"))
    else:
        from music_amd.engine import WaveNetEngine
        from music_amd.model import wavenet
        torch.manual_seed(0)
        net = wavenet(2, OPT_DIL, 32, 32, 32, 256, False)
        eng = net._engine = WaveNetEngine(OPT_DIL, 32, 32, 32, device="cpu")
    assert [n for n, _ in net.named_parameters()] == eng.param_names
    for n, p in net.named_parameters():
        o = eng.spec.off[n]
        eng.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
        p.data = eng.flat[o:o + p.numel()].view(p.shape)
    eng.flat_grad.fill_(0.01)
    return net, eng


def _flat_grads(net, eng):
    for n, p in net.named_parameters():
        o = eng.spec.off[n]
        p.grad = eng.flat_grad[o:o + p.numel()].view(p.shape)


def _optimizer(kind, momentum=0.9, ae=False, **kw):
    def build():
        from music_amd import train
        net, eng = _opt_net(ae)
        return net, eng, train.get_optimizer(net, kind, 1e-3, momentum, **kw)
    return build


def _fused(ae=False, **kw):
    def build():
        net, eng = _opt_net(ae)
        eng.adam_init(lr=1e-3, **kw)
        return net, eng, None
    return build


def _mixed_steps(net, eng, opt):
    """a state dict in which the first parameter's `step` differs, loaded"""
    sd = opt.state_dict()
    sd["state"][0]["step"] = sd["state"][0]["step"] + 3
    opt.load_state_dict(sd)


def _some_buffers(net, eng, opt):
    """only the first parameter holds a momentum_buffer"""
    p = opt.param_groups[0]["params"][0]
    opt.state[p]["momentum_buffer"] = torch.zeros_like(p)


def _second_group(net, eng, opt):
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})


def _weight_decay(net, eng, opt):
    opt.param_groups[0]["weight_decay"] = 1e-2


# name -> (builder of (module, engine, optimizer or None), the scripted sequence).  "flat": a step with the gradients on the flat
# buffer; "foreign": with p.grad = p.grad.clone() (torch's path); "closure": step(closure); "reload": load_state_dict(state_dict());
# "fused": eng.adam_step(); a function: called with (module, engine, optimizer) between two steps
OPTIMIZER_CASES = {}
for _kind in ("adam", "sgd", "rmsprop"):
    for _g, _gkw in (("plain", {}), ("guarded", GUARD)):
        for _s, _skw in (("", {}), ("_shadow", SHADOW)):
            OPTIMIZER_CASES["%s_%s%s" % (_kind, _g, _s)] = (_optimizer(_kind, **_gkw, **_skw), STANDARD)
        OPTIMIZER_CASES["%s_vq_ema_%s_shadow" % (_kind, _g)] = (_optimizer(_kind, ae=True, **_gkw, **SHADOW), ("flat", "flat"))
for _g, _gkw in (("plain", {}), ("guarded", GUARD)):
    for _s, _skw in (("", {}), ("_shadow", SHADOW)):
        OPTIMIZER_CASES["fused_%s%s" % (_g, _s)] = (_fused(**_gkw, **_skw), ("fused", "fused"))
    OPTIMIZER_CASES["fused_vq_ema_%s_shadow" % _g] = (_fused(ae=True, **_gkw, **SHADOW), ("fused", "fused"))
OPTIMIZER_CASES.update({
    "sgd_momentum0": (_optimizer("sgd", 0.0), ("flat", "flat")),
    "sgd_momentum0_guarded": (_optimizer("sgd", 0.0, **GUARD), ("flat", "flat")),
    "rmsprop_momentum0": (_optimizer("rmsprop", 0.0), ("flat", "flat")),
    "rmsprop_momentum0_guarded": (_optimizer("rmsprop", 0.0, **GUARD), ("flat", "flat")),
    "adam_closure": (_optimizer("adam", **SHADOW), ("flat", "closure", "flat")),
    "adam_mixed_steps": (_optimizer("adam"), ("flat", _mixed_steps, "flat", "flat")),
    "adam_mixed_steps_guarded": (_optimizer("adam", **GUARD), ("flat", _mixed_steps, "flat", "flat")),
    "sgd_some_momentum_buffers": (_optimizer("sgd"), (_some_buffers, "flat", "flat")),
    "adam_second_group": (_optimizer("adam"), ("flat", _second_group, "flat")),
    "sgd_second_group": (_optimizer("sgd"), ("flat", _second_group, "flat")),
    "adam_weight_decay": (_optimizer("adam"), ("flat", _weight_decay, "flat")),
    "sgd_weight_decay": (_optimizer("sgd"), ("flat", _weight_decay, "flat")),
    "rmsprop_weight_decay": (_optimizer("rmsprop"), ("flat", _weight_decay, "flat")),
})
del _kind, _g, _gkw, _s, _skw


def _optimizer_owners(eng, opt, keep):
    """The engine's tensors, then the optimizer's state tensors by storage (`opt.<state key>`, numbered where the parameters'
    tensors do not share one), the guard's state and partials and the shadow's flat buffer.  `keep` holds every tensor ever named,
    so that no address is handed out twice within a case."""
    out = []
    _tensors(vars(eng), "eng", out)
    out = [_span(key, t) for key, t in out if t.numel()]
    gd, shadow = (opt._guard, opt.ema) if opt is not None else (eng.adam_state.get("guard"), eng.ema)
    if opt is not None:
        seen = {}
        for p in (p for grp in opt.param_groups for p in grp["params"]):
            for key, t in sorted(opt.state[p].items()):
                if torch.is_tensor(t) and t.numel() and t.dim():
                    st = t.untyped_storage()
                    if (key, st.data_ptr()) not in seen:
                        n = sum(k == key for k, _ in seen)
                        seen[key, st.data_ptr()] = ("opt.%s" % key if n == 0 else "opt.%s.%d" % (key, n), st.data_ptr(), st.data_ptr() + st.nbytes(),
                                                    t.element_size())
                    keep.append(t)
        out += list(seen.values())
    if gd is not None:
        out += [_span("guard.state", gd.state), _span("guard.partials", gd.partials)]
    if shadow is not None and shadow.flat is not None:
        out.append(_span("shadow.flat", shadow.flat))
    keep.extend(t for t in (getattr(gd, "state", None), getattr(gd, "partials", None), getattr(shadow, "flat", None)) if t is not None)
    return out


def _optimizer_forms(eng, opt, prev):
    """after a step: every parameter's `step`, the sorted state keys, per state tensor whether it is a view of ONE flat buffer
    at the parameter's offset ("1"), a tensor of its own ("0") or None ("-"), one character per parameter, and `fresh`: the keys
    whose (first) tensor lies in other memory than after the step before (`prev`) - the state was adopted anew"""
    if opt is None:
        return {"t": eng.adam_state["t"]}
    params = [p for grp in opt.param_groups for p in grp["params"]]
    keys = sorted({k for p in params for k in opt.state[p]})
    forms = {"keys": keys, "step": [float(opt.state[p]["step"]) if opt.state[p].get("step") is not None else None for p in params],
             "fresh": []}
    for key in keys:
        if key == "step":
            continue
        ts = [opt.state[p].get(key) for p in params]
        base = next((t.untyped_storage().data_ptr() for t in ts if t is not None), None)
        if prev.get(key) != base:
            forms["fresh"].append(key)
        prev[key] = base
        forms[key] = "".join("-" if t is None else
                             "1" if n in eng.spec.off and t.untyped_storage().data_ptr() == base and t.storage_offset() == eng.spec.off[n]
                             and t.untyped_storage().nbytes() == 4 * eng.spec.total else "0"
                             for n, t in zip(eng.param_names + [None] * len(ts), ts))
    return forms


def record_optimizer(name, monkeypatch):
    """-> (canonical trace, {}, forms: one entry per item of the sequence) of one case of OPTIMIZER_CASES; a step that launched
    nothing leaves no trace item, ["step", k] items separate the sequence's."""
    from music_amd.guard import _TAKEN
    build, script = OPTIMIZER_CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = install(monkeypatch)
    net, eng, opt = build()
    del trace[:]
    out, forms, keep, tmp, prev = [], [], [], {}, {}
    for k, what in enumerate(script):
        if what == "fused":
            eng.adam_step()
        elif what == "reload":
            opt.load_state_dict(opt.state_dict())
        elif callable(what):
            what(net, eng, opt)
        else:
            _flat_grads(net, eng)
            if what == "foreign":
                for p in net.parameters():
                    p.grad = p.grad.clone()
            opt.step(*([lambda: None] if what == "closure" else []))
        gd = opt._guard if opt is not None else eng.adam_state.get("guard")
        if gd is not None:                  # the device's part: every guard launch saw a finite gradient, the step was taken
            gd.state[_TAKEN] += sum(item[0] == "wn_grad_guard" for item in trace)
        out.append(["step", k])
        out += canonical(trace, eng, None, _optimizer_owners(eng, opt, keep), tmp)
        forms.append(_optimizer_forms(eng, opt, prev))
        del trace[:]
    return out, {}, {"steps": forms}


# ---------------------------------------------------------------- the generators (tests/golden/launch_traces_decode.json)
# What music_amd/fast_generate.py and ae_generate.py launch between a prompt and the persistent decode kernel: the init forward, the
# class tables, the weight pack's refresh and the decode entry with every argument, for each public way in.  Beyond install():
# wavenet._engine_for builds its engine on the CPU (the module's own choice between the fast and the general one), ctypes.cast hands
# a host array through (it is then written out by value: dilations, ring offsets, window pairs, schedules), .cuda() is the identity.
# Owners: the engine, every workspace of its pool ("ws<B>x<T>"), the decode weight pack and the cached hand-off scratch.  The init
# forward's probabilities are never written here, so the first code is arbitrary: it enters no launch argument.
DEC_DIL, DEC_U, DEC_N = [1, 2, 4], 3, 12
DEC_CLASSES = [0, 1, 2]


def _halves(Q):
    return [(0, Q // 2), (Q // 2, Q)]


def _dec_net(kind):
    from music_amd.model import wavenet
    torch.manual_seed(0)
    if kind == "general":                                    # filter_width 3, Q = 100: the general plan and the fp32 decode kernel
        return wavenet(3, DEC_DIL, 40, 48, 96, 100, False)
    extra = dict(global_classes=4, global_channels=8, null_class=3) if kind == "classes" else {}
    return wavenet(2, DEC_DIL, 64, 64, 256, 256, kind == "bias", **extra)      # the matrix-core pack


def _prompt(net, U):
    return on_device(torch.zeros(U, net.quantization_channels, net.receptive_field))


def _gen(batch, note_nums=(DEC_N,), **kw):
    def run(fg, net):
        for n in note_nums:
            out = (fg.generate_codes_batch if batch else fg.generate_codes)(net, _prompt(net, DEC_U if batch else 1), n, **kw)
            assert tuple(out.shape) == ((DEC_U, n) if batch else (n,)) and out.dtype == torch.int64
    return run


def _predict(fg, net):
    Q = net.quantization_channels
    col = lambda: on_device(torch.zeros(1, Q, 1))
    _, state = fg.predict_next(net, _prompt(net, 1))
    corrected = net.filter_width != 2
    fg.predict_next(net, col(), state, correct_queue=corrected)
    fg.predict_next(net, col(), state, correct_queue=True)
    fg.predict_next(net, col(), dict(state.items()), correct_queue=True)       # reference-style tensors: DecodeState.from_tensors


def _explicit(U, **kw):
    """decode_batch_cond from explicit state: zero rings of the pack's ring size, five steps"""
    def run(fg, net):
        from music_amd.ae_generate import cond_schedule
        eng = net._engine_for(torch.device("cpu"))
        pack, K1, n = fg._pack_for(net, eng), net.filter_width - 1, 5
        rings = torch.zeros(U, max(1, sum(K1 * d * pack.Rp for d in eng.dil)))
        a = dict(kw)
        if a.pop("tables", False):
            a.update(cond_fg=torch.zeros(U, eng.N, 2, 2 * pack.Dp), cond_p1=torch.zeros(U, 2, eng.S),
                     schedule=cond_schedule((net.filter_width, eng.dil), n, 2), forced=torch.zeros(U, n, dtype=torch.int64))
        fg.decode_batch_cond(net, rings, torch.zeros(U, K1, eng.Q), torch.zeros(U, eng.Q), n, step0=2, pos0=1, **a)
    return run


def _sampler(**kw):
    def run(fg, net):
        a = dict(kw)
        if a.pop("with_u", False):
            a["logits_u"] = on_device(torch.zeros(5, 256))
        fg.sample_logits(on_device(torch.zeros(5, 256)), **a)
    return run


def _ae_resynthesize(fg, net):
    from music_amd import ae_generate
    torch.manual_seed(3)
    ae_generate.resynthesize(net, torch.zeros(2, 256, net.receptive_field + 99), temperature=0.9, seed=2)


def _ae_decode_codes(fg, net):
    from music_amd import ae_generate
    ae_generate.decode_codes(net, torch.zeros(2, 2, dtype=torch.int64), 80, temperature=0.9, seed=2)


_W256 = dict(correct_queue=True, windows=_halves(256), window_pos=5)
_TABLES = dict(correct_queue=True, temperature=[0.5, 0.8, 1.0], top_k=[0, 40, 5], seed=[1, 2, 3], streams=[4, 5, 6])
_CLS1, _CLS = dict(correct_queue=True, classes=[1]), dict(correct_queue=True, classes=DEC_CLASSES)
# name -> (model of _dec_net, or a builder of the module, or None; run(fast_generate, module))
DECODE_CASES = {
    "one": ("fast", _gen(False)),
    "one_sampled": ("fast", _gen(False, correct_queue=True, temperature=0.9, top_k=20, seed=3)),
    "one_windows": ("fast", _gen(False, **_W256)),
    "batch": ("fast", _gen(True)),
    "batch_tables": ("fast", _gen(True, **_TABLES)),
    "batch_windows": ("fast", _gen(True, **_W256)),
    "batch_bias": ("bias", _gen(True)),
    "classes_one": ("classes", _gen(False, **_CLS1)),
    "classes_batch": ("classes", _gen(True, **_CLS)),
    "guided_one": ("classes", _gen(False, guidance=2.0, temperature=0.9, seed=3, **_CLS1, **{k: v for k, v in _W256.items() if k != "correct_queue"})),
    "guided_batch_scalar": ("classes", _gen(True, guidance=2.0, streams=[4, 5, 6], temperature=0.9, seed=3, classes=DEC_CLASSES, **_W256)),
    "guided_batch": ("classes", _gen(True, guidance=[0.5, 1.0, 2.5], classes=DEC_CLASSES, windows=_halves(256), window_pos=5, **_TABLES)),
    "guidance_none_one": ("classes", _gen(False, guidance=None, **_CLS1)),
    "guidance_none_batch": ("classes", _gen(True, guidance=None, **_CLS)),
    "general_one": ("general", _gen(False, correct_queue=True)),
    "general_batch": ("general", _gen(True, correct_queue=True)),
    "short_one": ("fast", _gen(False, (0, 1))),
    "short_batch": ("fast", _gen(True, (0, 1))),
    "short_guided": ("classes", _gen(True, (0, 1), guidance=2.0, **_CLS)),
    "predict_next": ("fast", _predict),
    "predict_next_general": ("general", _predict),
    "explicit": ("fast", _explicit(3)),
    "explicit_tables": ("fast", _explicit(3, tables=True, want_probs=True, temperature=0.9, top_p=0.8, seed=4)),
    "explicit_guided": ("fast", _explicit(4, tables=True, guidance=[1.5, 0.5], windows=_halves(256), window_pos=2)),
    "explicit_general": ("general", _explicit(3)),
    "sample_logits": (None, _sampler(temperature=0.8, top_k=5, seed=2, step0=3)),
    "sample_logits_windows": (None, _sampler(temperature=[0.5, 0.6, 0.7, 0.8, 0.9], windows=_halves(256), window_pos=3)),
    "sample_logits_guided": (None, _sampler(guidance=[0.5, 1.0, 1.5, 2.0, 2.5], with_u=True, windows=_halves(256), window_pos=3)),
    "ae_resynthesize": (lambda: _ae_net(64, 64), _ae_resynthesize),
    "ae_decode_codes": (lambda: _ae_net(64, 64, conditioning="learned", bottleneck="vq", vq_codes=OPT_K), _ae_decode_codes),
}


def _cpu_engine_for(self, device=None):
    """model.wavenet._engine_for on device="cpu": the same choice of engine, the parameters views of its flat buffer"""
    from music_amd.engine import WaveNetEngine
    from music_amd.engine_generic import GenericWaveNetEngine
    if self._engine is None:
        fast = self.filter_width == 2 and self.quantization_channels == 256 and max(self.residual_channels, self.dilation_channels) <= 64
        eng = (WaveNetEngine if fast else GenericWaveNetEngine)(
            self.dilations, self.residual_channels, self.dilation_channels, self.skip_channels, self.quantization_channels, self.filter_width,
            self.use_bias, mode_fwd=self.precision[0], mode_bwd=self.precision[1], device="cpu",
            **(dict(global_classes=self.global_classes, global_channels=self.global_channels) if self.global_classes else {}))
        eng.mode_names = tuple(self.precision)
        with torch.no_grad():
            for name, p in self._named_ref_params():
                view = eng.param_view(name)
                view.copy_(p.data)
                p.data = view
        self._engine = eng
    return self._engine


def _decode_owners(nets):
    out = []
    for j, net in enumerate(nets):
        eng, tag = net._engine, "" if j == 0 else str(j)
        if eng is None:
            continue
        _tensors(vars(eng), "eng" + tag, out)
        for (B, T), lst in eng._ws._d.items():
            for k, ws in enumerate(lst):
                _tensors({key: v for key, v in ws.items() if key != "bwd"}, "ws%s_%dx%d_%d" % (tag, B, T, k), out)
        pack = getattr(net, "_decode_pack", None)
        _tensors({k: getattr(pack, k, None) for k in ("buf", "idx", "pk", "pk_idx")} if pack is not None else {}, "pack" + tag, out)
        _tensors(getattr(net, "_decode_sync", None), "sync" + tag, out)
    return [_span(key, t) for key, t in out if t.numel()]


def _values(trace, own):
    """What a pointer's name does not say, per launch: shape and dtype of every tensor no owner holds (note0, prev0, the rings, the
    class tables, the outputs), the bytes of a sampling table (the one uint8 tensor) as a hash, and the floats of a guidance table
    (the last pointer of the wn_cfg_* entries)."""
    out = []
    for n, item in enumerate(trace):
        if item[0] in ("record", "wait", "mark"):
            continue
        name, args = item
        ptrs = [(j, a) for j, a in enumerate(args) if isinstance(a, Ptr)]
        vals = {}
        for j, a in ptrs:
            if not any(lo <= a.addr < hi for _, lo, hi, _ in own):
                vals[str(j)] = [list(a.t.shape), str(a.t.dtype)]
                if a.t.dtype == torch.uint8:
                    vals[str(j)].append(hashlib.sha256(a.t.numpy().tobytes()).hexdigest())
        if name.startswith("wn_cfg_"):
            vals["guidance"] = [float(v) for v in ptrs[-1][1].t.tolist()]
        if vals:
            out.append([n, name, vals])
    return out


def _decode_pack_maps(pack):
    """the decode weight pack's index maps by hash and its offsets by value"""
    if pack is None:
        return {}
    h = lambda t: None if t is None else hashlib.sha256(t.numpy().tobytes()).hexdigest()
    out = {k: getattr(pack, k, None) for k in ("k", "mfma", "Rp", "Dp", "o_causal", "o_layers", "layer_stride", "o_p1", "o_p2", "o_bias",
                                               "pk_off", "pk_stride")}
    return dict(out, idx=h(pack.idx), pk_idx=h(getattr(pack, "pk_idx", None)))


def record_decode(name, monkeypatch):
    """-> (canonical trace, pack-map hashes of the engine and the decode pack, {"values": what the trace cannot name}) of one case."""
    from music_amd import ae_generate, fast_generate as fg, model, model1  # noqa: F401 (imported so that install() patches them)
    build, run = DECODE_CASES[name]
    for k in SWITCHES + ("WN_DEC_MFMA", "WN_DEC_T0"):
        monkeypatch.delenv(k, raising=False)
    trace = install(monkeypatch)
    real_cast = ctypes.cast
    monkeypatch.setattr(ctypes, "cast", lambda a, t: a if isinstance(a, ctypes.Array) and t is ctypes.c_void_p else real_cast(a, t))
    monkeypatch.setattr(model.wavenet, "_engine_for", _cpu_engine_for)
    # the autoencoder's cases: the clips and both modules stay where they are, the engine is built on the CPU
    made = []
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: on_device(self))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: made.append(self) or self)

    def ae_engine_for(self, device=None):
        if self._engine is None:
            self._engine = model1._AutoencoderEngine(self, torch.device("cpu"))
        return self._engine
    monkeypatch.setattr(model1.wavenet_autoencoder, "_engine_for", ae_engine_for)
    net = None if build is None else _dec_net(build) if isinstance(build, str) else build()
    del trace[:]
    with np.errstate(all="ignore"), torch.no_grad():
        run(fg, net)
    nets = [] if net is None else [net] + [m for m in made if m is not net]
    own = _decode_owners(nets)
    packs = {}
    for j, m in enumerate(nets):
        if m._engine is not None:
            packs["engine%d" % j] = pack_maps(m._engine, PACK_KEYS_ALL)
            packs["decode%d" % j] = _decode_pack_maps(getattr(m, "_decode_pack", None))
    return canonical(trace, None, None, own), packs, {"values": _values(trace, own)}
