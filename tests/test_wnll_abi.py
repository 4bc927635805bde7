"""CPU checks of the masked / weighted / smoothed objective's entry wn_wstep_nll (include/wavenet_hip.h, music_amd/csrc/wn_nll.hip) -
declared, exported, bound with matching arity and types, the ABI still 9, every refusal reported by entry and argument name before
anything is launched, empty calls accepted - and of the host surface above it that needs no device: the weights= / ignore_index= /
label_smoothing= keywords of every step tail (with all three at their defaults the launch is the one from before, recorded with
tests/launch_trace.py), and the JSON keys "ignore_token" / "label_smoothing" / "nll_stage_weights".  No device is touched; pointers
below are never dereferenced (the window table is a host array and IS read)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.helpers import ROOT

P = 1 << 20            # "some non-NULL address"
_KEEP = []
ARGS = ("x", "x_bstride", "x_pitch", "target", "dx", "dx_bstride", "dx_pitch", "probs", "row_nll", "row_hit", "loss_part", "w", "q",
        "batch", "win_host", "win_period", "win_pos", "win_pos0", "weight", "ignore_index", "smoothing", "den", "stream")
KEYWORDS = ("weights", "ignore_index", "label_smoothing")


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def _table(pairs):
    t = (ctypes.c_int32 * (2 * len(pairs)))(*[v for pr in pairs for v in pr])
    _KEEP.append(t)
    return ctypes.cast(t, ctypes.c_void_p)


def test_the_entry_is_declared_exported_and_bound():
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint wn_wstep_nll\s*\((.*?)\);", src, flags=re.S)
    assert decl, "wn_wstep_nll is not declared"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wn_wstep_nll")
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == ARGS and len(_lib.SIGNATURES["wn_wstep_nll"]) == len(ARGS)
    assert _lib.load().wn_wstep_nll.argtypes == _lib.SIGNATURES["wn_wstep_nll"]
    for a, typ in zip(decl.group(1).split(","), _lib.SIGNATURES["wn_wstep_nll"]):
        want = (ctypes.c_void_p if ("*" in a or "wn_stream_t" in a) else ctypes.c_int64 if "int64_t" in a
                else ctypes.c_float if "float" in a else ctypes.c_int)
        assert typ is want, a
    # wn_win_step_nll's arguments without inv_n, then weight, ignore_index, smoothing, den
    p, l, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    sig = _lib.SIGNATURES["wn_win_step_nll"]
    assert sig[14] is f and _lib.SIGNATURES["wn_wstep_nll"] == sig[:14] + sig[15:-1] + [p, l, f, p] + sig[-1:]
    assert len(_lib.SIGNATURES["wn_step_nll"]) == 16 and len(sig) == 20                  # the entries before it keep theirs


def test_the_version_stays_9_and_the_kernel_is_not_a_fork():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()
    src = open(os.path.join(ROOT, "music_amd", "csrc", "wn_nll.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bvoid step_nll_k\(", src)) == 1 and "nll_den_k" in src
    assert "atomic" not in src.lower().replace("no float atomics", "")


def _refused(ok, arg, **kw):
    from music_amd import _lib
    lib = _lib.load()
    a = list(ok)
    for k, v in kw.items():
        a[ARGS.index(k)] = v
    rc = lib.wn_wstep_nll(*a)
    msg = lib.wn_last_error().decode()
    assert rc == -4 and msg.startswith("wn_wstep_nll:") and "'%s'" % arg in msg, (arg, rc, msg)
    return msg


def test_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    w, q = 70, 256
    ok = [P, q * w, w, P, P, q * w, w, P, P, P, P, w, q, 2, _table([(0, 128), (128, 256)]), 2, P, 0, P, -1, 0.1, P, None]
    bad = lambda arg, **kw: _refused(ok, arg, **kw)
    # its own
    for v in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        bad("smoothing", smoothing=v)
    bad("den", den=None)
    bad("smoothing", smoothing=1.0, batch=0)                             # refused whether or not there is work to do
    # everything wn_win_step_nll refuses, under this entry's name
    bad("win_period", win_period=-1)
    bad("win_period", win_period=17)
    bad("win_host", win_host=None)
    bad("win_host", win_host=_table([(0, 8), (-1, 4)]))
    bad("win_host", win_host=_table([(0, q + 1), (0, 4)]))
    assert "pair 1" in bad("win_host", win_host=_table([(0, 4), (9, 3)]))
    bad("win_pos0", win_pos0=-1)
    bad("win_period", win_period=17, batch=0)
    for name in ("x", "target", "loss_part"):
        bad(name, **{name: None})
    for v in (0, -1, 1025):
        bad("q", q=v)
    bad("x_pitch", x_pitch=w - 1)
    bad("dx_pitch", dx_pitch=w - 1)
    bad("x_bstride", x_bstride=q * w - 1)
    bad("dx_bstride", dx_bstride=q * w - 1)
    bad("batch", batch=-1)
    bad("w", w=-1)
    # weight, the window table with period 0, win_pos and the optional outputs may be NULL: refused only for the next thing wrong
    bad("den", weight=None, win_host=None, win_period=0, win_pos=None, dx=None, probs=None, row_nll=None, row_hit=None, den=None)
    # empty calls return 0 with NULLs (den included), with and without a table
    tab = _table([(0, 64)] * 16)
    for tail in ((tab, 16, None, 2 ** 40), (None, 0, None, 0)):
        assert lib.wn_wstep_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 256, 4, *tail, None, -1, 0.0, None, None) == 0
        assert lib.wn_wstep_nll(None, 256 * 5, 5, None, None, 0, 0, None, None, None, None, 5, 256, 0, *tail, None, -1, 0.5, None, None) == 0
    # ... but the shapes of an empty call are still checked
    assert lib.wn_wstep_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 0, 0, None, 0, None, 0, None, -1, 0.0, None, None) == -4
    assert "'q'" in lib.wn_last_error().decode()


# ---------------------------------------------------------------- engines
def test_every_step_tail_takes_the_three_keywords():
    from music_amd import ae_generate, ae_generic, engine, engine_base, engine_generic, model1, objective
    fns = [engine_base.EngineBase.step_nll, engine_base.EngineBase.score_logits, engine_base.EngineBase._fused_tail,
           engine.WaveNetEngine.loss_and_grad, engine.WaveNetEngine.loss_and_grad_codes,
           engine_generic.GenericWaveNetEngine.loss_and_grad, engine_generic.GenericWaveNetEngine.loss_and_grad_codes,
           model1._AutoencoderEngine.loss_and_grad, ae_generic.GenericAutoencoderEngine.loss_and_grad,
           objective.nll_loss, objective.score, ae_generate.prior_score]
    for fn in fns:
        par = inspect.signature(fn).parameters
        assert [par[k].default for k in KEYWORDS] == [None, None, 0.0], fn.__qualname__


def _step_calls(monkeypatch, **kw):
    """the launches of one fused "nll" step of a small fast WaveNet engine recorded on the CPU: [(entry, arguments)]"""
    from tests import launch_trace
    from music_amd.engine import WaveNetEngine
    if not _TRACE or _TRACE[0] is not monkeypatch:               # (one recorder per test: install() replaces `call` once)
        _TRACE[:] = [monkeypatch, launch_trace.install(monkeypatch)]
    trace = _TRACE[1]
    eng = WaveNetEngine([1, 2], 32, 32, 256, device="cpu")
    eng.objective = "nll"
    T = eng.rf + 69
    x = launch_trace.on_device(torch.zeros(2, 256, T))
    target = launch_trace.on_device(torch.zeros(2 * 70, dtype=torch.int64))
    del trace[:]
    eng.loss_and_grad(x, target, **kw)
    ws = eng._ws.peek(2, T)
    return eng, ws, [item for item in trace if item[0].startswith("wn_") and "step_nll" in item[0]], target


_TRACE = []


def test_defaults_launch_the_entry_from_before_with_its_arguments(monkeypatch):
    eng, ws, calls, target = _step_calls(monkeypatch)
    assert [c[0] for c in calls] == ["wn_step_nll"] and "nll_den" not in ws
    a = calls[0][1]
    W, Q, B = 70, 256, 2
    assert [v.addr if hasattr(v, "addr") else v for v in a] == [
        ws["O"].data_ptr(), Q * W, W, target.data_ptr(), ws["bwd"]["dO"].data_ptr(), Q * W, W, None, None, None,
        ws["loss_part"].data_ptr(), W, Q, B, 1.0 / (B * W), "main"]
    # explicit defaults are the defaults
    _, _, calls, _ = _step_calls(monkeypatch, weights=None, ignore_index=None, label_smoothing=0.0)
    assert [c[0] for c in calls] == ["wn_step_nll"]
    _, _, calls, _ = _step_calls(monkeypatch, windows=[(0, 128), (128, 256)], window_pos=3)
    assert [c[0] for c in calls] == ["wn_win_step_nll"] and len(calls[0][1]) == 20


@pytest.mark.parametrize("kw", [dict(ignore_index=-1), dict(label_smoothing=0.1), dict(weights=torch.ones(2, 70)),
                                dict(weights=[1.0] * 140, ignore_index=7, label_smoothing=0.25)], ids=["ignore", "smoothing", "weights", "all"])
def test_any_keyword_launches_the_weighted_entry(monkeypatch, kw):
    eng, ws, calls, target = _step_calls(monkeypatch, **kw)
    assert [c[0] for c in calls] == ["wn_wstep_nll"]
    a = [v.addr if hasattr(v, "addr") else v for v in calls[0][1]]
    W, Q, B = 70, 256, 2
    wt = ws["nll_weight"]
    assert (wt is None) == ("weights" not in kw) and (wt is None or (wt.dtype == torch.float32 and wt.numel() == B * W))
    assert a == [ws["O"].data_ptr(), Q * W, W, target.data_ptr(), ws["bwd"]["dO"].data_ptr(), Q * W, W, None, None, None,
                 ws["loss_part"].data_ptr(), W, Q, B, None, 0, None, 0, None if wt is None else wt.data_ptr(),
                 kw.get("ignore_index", -(1 << 63)), kw.get("label_smoothing", 0.0), ws["nll_den"].data_ptr(), "main"]
    assert ws["nll_den"].shape == (2,) and ws["nll_den"].dtype == torch.float32
    # under windows the table travels in the same launch
    _, _, calls, _ = _step_calls(monkeypatch, windows=[(0, 128), (128, 256)], window_pos=3, **kw)
    assert [c[0] for c in calls] == ["wn_wstep_nll"] and calls[0][1][15:18:2] == (2, 3)


def test_keywords_are_checked_on_the_host(monkeypatch):
    for kw, match in ((dict(label_smoothing=1.0), "label_smoothing"), (dict(label_smoothing=-0.1), "label_smoothing"),
                      (dict(label_smoothing=float("nan")), "label_smoothing"), (dict(weights=torch.ones(139)), "139 weights"),
                      (dict(weights=torch.ones(140, dtype=torch.int64)), "floats")):
        with pytest.raises(ValueError, match=match):
            _step_calls(monkeypatch, **kw)
    # the reference's loss has no per-column term to weight
    from tests import launch_trace
    from music_amd.engine import WaveNetEngine
    eng = WaveNetEngine([1, 2], 32, 32, 256, device="cpu")
    x = launch_trace.on_device(torch.zeros(2, 256, eng.rf + 69))
    target = launch_trace.on_device(torch.zeros(140, dtype=torch.int64))
    with pytest.raises(ValueError, match='objective "nll" only'):
        eng.loss_and_grad(x, target, ignore_index=-1)


# ---------------------------------------------------------------- the JSON keys
def test_json_keys_are_parsed_and_refused_by_name():
    from music_amd import objective
    ds = {"token_positions": True}
    nll = {"objective": "nll"}
    assert objective.wnll_option(nll, ds) is None and objective.wnll_option({}, {}) is None
    assert objective.wnll_option(dict(nll, ignore_token=-1), {}) == {"ignore_index": -1, "label_smoothing": 0.0, "stage_weights": None}
    assert objective.wnll_option(dict(nll, label_smoothing=0.1), {}) == {"ignore_index": None, "label_smoothing": 0.1, "stage_weights": None}
    assert objective.wnll_option(dict(nll, nll_stage_weights=[2, 1.0, 0]), ds)["stage_weights"] == [2.0, 1.0, 0.0]
    for key, value in (("ignore_token", -1), ("label_smoothing", 0.1), ("nll_stage_weights", [1.0, 0.5])):
        for tp in ({key: value}, {key: value, "objective": "reference"}):
            with pytest.raises(ValueError, match=r'"%s" needs "objective": "nll"' % key):
                objective.wnll_option(tp, ds)
    for bad_ds in ({}, {"token_positions": False}):
        with pytest.raises(ValueError, match=r'"nll_stage_weights" needs "token_positions": true'):
            objective.wnll_option(dict(nll, nll_stage_weights=[1.0]), bad_ds)
    for v in (1.5, "x", True, [1]):
        with pytest.raises(ValueError, match='"ignore_token" must be an integer'):
            objective.wnll_option(dict(nll, ignore_token=v), ds)
    for v in (1.0, -0.1, "x", True, float("nan")):
        with pytest.raises(ValueError, match=r'"label_smoothing" must be a number in \[0, 1\)'):
            objective.wnll_option(dict(nll, label_smoothing=v), ds)
    for v in ([], [1.0] * 17, [1.0, -0.5], [float("inf")], [float("nan")], 1.0, ["a"], [True]):
        with pytest.raises(ValueError, match='"nll_stage_weights" must be a list of 1..16 non-negative numbers'):
            objective.wnll_option(dict(nll, nll_stage_weights=v), ds)


def test_stage_weights_follow_the_stream_position():
    from music_amd import objective
    opt = objective.wnll_option({"objective": "nll", "nll_stage_weights": [4.0, 1.0, 0.0], "ignore_token": -1}, {"token_positions": True})
    kw = objective.wnll_kwargs(opt, {"audio_pos": torch.tensor([0, 5])}, 4, torch.device("cpu"))
    assert kw["ignore_index"] == -1 and kw["label_smoothing"] == 0.0
    assert kw["weights"].dtype == torch.float32 and kw["weights"].tolist() == [[4.0, 1.0, 0.0, 4.0], [0.0, 4.0, 1.0, 0.0]]
    # the table and the column offsets are made once per device and width, not per batch
    held = opt["_device"][torch.device("cpu"), 4]
    kw = objective.wnll_kwargs(opt, {"audio_pos": torch.tensor([1, 2])}, 4, "cpu")
    assert opt["_device"][torch.device("cpu"), 4] is held and len(opt["_device"]) == 1 and kw["weights"][:, 0].tolist() == [1.0, 0.0]
    assert objective.wnll_kwargs(None, {}, 4, torch.device("cpu")) == {}
    opt = objective.wnll_option({"objective": "nll", "label_smoothing": 0.2}, {})
    assert objective.wnll_kwargs(opt, {}, 4, torch.device("cpu")) == {"ignore_index": None, "label_smoothing": 0.2}
