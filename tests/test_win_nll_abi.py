"""CPU checks of the windowed objective's entries wn_win_step_softmax and wn_win_step_nll (include/wavenet_hip.h) - declared, exported,
bound with matching arity, the ABI still 9, every refusal reported by entry and argument name before anything is launched - and of
the host surface above them that needs no device: EngineBase.nll_windows and the windows= / window_pos= arguments of the step tail,
the JSON keys "nll_windows" / "token_positions", and the loader's 'audio_pos'.  No device is touched; pointers below are never
dereferenced (the window table is a host array and IS read)."""
import ctypes
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.cpu_model import onehot_oracle
from tests.helpers import ROOT

P = 1 << 20            # "some non-NULL address"
_KEEP = []
NLL_ARGS = ("x", "x_bstride", "x_pitch", "target", "dx", "dx_bstride", "dx_pitch", "probs", "row_nll", "row_hit", "loss_part", "w", "q",
            "batch", "inv_n", "win_host", "win_period", "win_pos", "win_pos0", "stream")
SM_ARGS = ("x", "x_bstride", "x_pitch", "probs", "w", "q", "batch", "win_host", "win_period", "win_pos", "win_pos0", "stream")


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def _table(pairs):
    if pairs is None:
        return None
    t = (ctypes.c_int32 * max(1, 2 * len(pairs)))(*[v for pr in pairs for v in pr])
    _KEEP.append(t)
    return ctypes.cast(t, ctypes.c_void_p)


@pytest.mark.parametrize("name,names,base", [("wn_win_step_softmax", SM_ARGS, "wn_step_softmax"), ("wn_win_step_nll", NLL_ARGS, "wn_step_nll")])
def test_entries_are_declared_exported_and_bound(name, names, base):
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == names and len(_lib.SIGNATURES[name]) == len(names)
    assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name]
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    sig = _lib.SIGNATURES[base]
    assert _lib.SIGNATURES[name] == sig[:-1] + [p, i, p, l] + sig[-1:]
    # the entries they extend keep their signatures
    assert len(_lib.SIGNATURES["wn_step_softmax"]) == 8 and len(_lib.SIGNATURES["wn_step_nll"]) == 16


def test_the_version_stays_9():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()


def _refused(fn, names, ok, arg, **kw):
    from music_amd import _lib
    lib = _lib.load()
    a = list(ok)
    for k, v in kw.items():
        a[names.index(k)] = v
    rc = getattr(lib, fn)(*a)
    msg = lib.wn_last_error().decode()
    assert rc == -4 and msg.startswith(fn + ":") and "'%s'" % arg in msg, (fn, arg, rc, msg)
    return msg


def _window_refusals(bad, q):
    bad("win_period", win_period=-1)
    bad("win_period", win_period=17)
    bad("win_period", win_host=_table([(0, 1)] * 17), win_period=17)
    bad("win_host", win_host=None)
    bad("win_host", win_host=_table([(0, 8), (-1, 4)]))
    bad("win_host", win_host=_table([(0, q + 1), (0, 4)]))
    bad("win_host", win_host=_table([(7, 7), (0, 4)]))
    assert "pair 1" in bad("win_host", win_host=_table([(0, 4), (9, 3)]))
    bad("win_pos0", win_pos0=-1)
    bad("win_pos0", win_pos0=-2 ** 40)
    # refused whether or not there is work to do
    bad("win_period", win_period=17, batch=0)
    bad("win_pos0", win_pos0=-1, w=0, x_pitch=0, x_bstride=0)
    bad("win_host", win_host=_table([(0, q + 1), (0, 4)]), batch=0)


def test_win_step_nll_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    w, q = 70, 256
    ok = [P, q * w, w, P, P, q * w, w, P, P, P, P, w, q, 2, 0.5, _table([(0, 128), (128, 256)]), 2, P, 0, None]
    bad = lambda arg, **kw: _refused("wn_win_step_nll", NLL_ARGS, ok, arg, **kw)
    _window_refusals(bad, q)
    # everything wn_step_nll refuses, under this entry's name
    for name in ("x", "target", "loss_part"):
        bad(name, **{name: None})
    for v in (0, -1, 1025):
        bad("q", q=v)
    bad("x_pitch", x_pitch=w - 1)
    bad("dx_pitch", dx_pitch=w - 1)
    bad("x_bstride", x_bstride=q * w - 1)
    bad("dx_bstride", dx_bstride=q * w - 1)
    bad("x_bstride", x_pitch=w + 3)
    bad("batch", batch=-1)
    bad("w", w=-1)
    # empty calls return 0 with NULLs, with a table, with period 0 (NULL table and positions), with a large position
    tab = _table([(0, 64)] * 16)
    for tail in ((tab, 16, None, 2 ** 40), (None, 0, None, 0), (tab, 16, P, 0)):
        assert lib.wn_win_step_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 256, 4, 1.0, *tail, None) == 0
        assert lib.wn_win_step_nll(None, 256 * 5, 5, None, None, 0, 0, None, None, None, None, 5, 256, 0, 1.0, *tail, None) == 0
    # ... but the shapes of an empty call are still checked
    assert lib.wn_win_step_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 0, 0, 1.0, None, 0, None, 0, None) == -4
    assert "'q'" in lib.wn_last_error().decode()
    # the entry it extends still reports under its own name
    assert lib.wn_step_nll(P, q * w, w, P, P, q * w, w - 1, P, P, P, P, w, q, 2, 0.5, None) == -4
    assert lib.wn_last_error().decode().startswith("wn_step_nll:")


def test_win_step_softmax_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    w, q = 33, 100
    ok = [P, q * w, w, P, w, q, 3, _table([(0, 10), (10, 100)]), 2, None, 0, None]
    bad = lambda arg, **kw: _refused("wn_win_step_softmax", SM_ARGS, ok, arg, **kw)
    _window_refusals(bad, q)
    bad("x", x=None)
    bad("probs", probs=None)
    for v in (0, 1025):
        bad("q", q=v)
    bad("x_pitch", x_pitch=w - 1)
    bad("x_bstride", x_bstride=q * w - 1)
    assert lib.wn_win_step_softmax(None, q * w, w, None, w, q, 0, _table([(0, 10)]), 1, None, 7, None) == 0
    assert lib.wn_win_step_softmax(None, 0, 0, None, 0, q, 3, None, 0, None, 0, None) == 0


# ---------------------------------------------------------------- engines
def test_windows_are_an_engine_attribute_and_every_step_tail_takes_them():
    from music_amd import ae_generic, engine, engine_base, engine_generic, model1
    eb = engine_base.EngineBase
    assert eb.nll_windows is None
    for fn in (eb.step_nll, eb.score_logits, eb.step_probs, eb._fused_tail):
        sig = inspect.signature(fn).parameters
        assert sig["windows"].default is None and sig["window_pos"].default is None, fn
    for cls in (engine.WaveNetEngine, engine_generic.GenericWaveNetEngine, model1._AutoencoderEngine, ae_generic.GenericAutoencoderEngine):
        fns = [cls.loss_and_grad] + ([cls.loss_and_grad_codes] if hasattr(cls, "loss_and_grad_codes") else [])
        for fn in fns:
            sig = inspect.signature(fn).parameters
            assert sig["windows"].default is None and sig["window_pos"].default is None, fn
        assert not {"step_nll", "score_logits", "step_probs", "_fused_tail", "_resolve_windows"} & set(cls.__dict__)      # one copy, in the base
    e = eb.__new__(eb)
    e.Q = 256
    assert e._resolve_windows(None) is None
    assert e._resolve_windows([(0, 128), (128, 256)]).pairs == [(0, 128), (128, 256)]
    e.nll_windows = [(0, 64)] * 16
    assert len(e._resolve_windows(None).pairs) == 16 and e._resolve_windows([(3, 9)]).pairs == [(3, 9)]
    for bad, what in (([], "1..16"), ([(0, 1)] * 17, "1..16"), ([(0, 257)], "lo < hi <= Q"), ([(5, 5)], "lo < hi"), ([(-1, 5)], "0 <= lo"),
                      (7, "pairs"), ([(1, 2, 3)], "pairs")):
        with pytest.raises(ValueError, match=what):
            e._resolve_windows(bad)
    e.nll_windows = None
    with pytest.raises(ValueError, match="window_pos"):
        e._resolve_windows(None, 3)
    win = engine_base.NllWindows([(0, 128), (128, 256)], 256)
    for bad, what in ((-1, ">= 0"), ([0, -2], ">= 0"), ([0, 1, 2], "3 positions for 2 clips"), (torch.zeros(2, dtype=torch.int32), "int64"),
                      (torch.zeros(3, dtype=torch.int64), "3 positions for 2 clips")):
        with pytest.raises(ValueError, match=what):
            win.tail(bad, 2, "cpu")


def _patched_engine(monkeypatch, calls, B, W, Q):
    from music_amd import _lib, engine_base
    monkeypatch.setattr(engine_base, "call", lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(_lib, "stream", lambda: 77)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    class Eng(engine_base.EngineBase):
        device = "cpu"

        def __init__(self):
            self.Q = Q
            self.marks = self.mark_only = None
            self.bw = {"dO": torch.zeros(B * Q * W)}

        def _bwd_workspace(self, ws):
            return self.bw

        def backward_from_dlogits(self, ws):
            calls.append(("backward",))
    return Eng()


def _table_of(arg, period):
    return list(ctypes.cast(arg, ctypes.POINTER(ctypes.c_int32))[:2 * period])


def test_fused_tail_launches_the_windowed_entry_only_when_windows_are_set(monkeypatch):
    """_fused_tail with the launches patched out.  Windows unset under "nll": exactly wn_step_nll with the arguments from before the
    windows.  Windows set (argument or attribute): exactly ONE wn_win_step_nll - the same head, then the table, the period, the
    positions and the first position.  Windows under "reference" raise before anything is launched."""
    calls = []
    B, W, Q = 2, 5, 256
    eng = _patched_engine(monkeypatch, calls, B, W, Q)
    ws = {"B": B, "W": W, "O": torch.zeros(B * Q * W)}
    tgt = torch.zeros(B, W, dtype=torch.int64)
    eng._fused_tail(ws, tgt, want_probs=True, objective="nll")
    assert [c[0] for c in calls] == ["wn_step_nll", "backward"]
    a = calls[0][1:]
    assert len(a) == 16
    assert a[0] == ws["O"].data_ptr() and a[1:3] == (Q * W, W) and a[4] == eng.bw["dO"].data_ptr() and a[5:7] == (Q * W, W)
    assert a[7] == ws["probs"].data_ptr() and a[8] is None and a[9] is None and a[10] == ws["loss_part"].data_ptr()
    assert a[11:14] == (W, Q, B) and a[14] == 1.0 / (B * W) and a[15] == 77
    head = a[:15]
    win = [(0, 64), (64, 128), (128, 192), (192, 256)]
    flat = [v for pr in win for v in pr]
    # per-clip positions on the "device": the tensor itself travels, no copy
    pos = torch.tensor([3, 8], dtype=torch.int64)
    del calls[:]
    eng._fused_tail(ws, tgt, want_probs=True, objective="nll", windows=win, window_pos=pos)
    assert [c[0] for c in calls] == ["wn_win_step_nll", "backward"]
    a = calls[0][1:]
    assert len(a) == 20 and a[:7] == head[:7] and a[7] == ws["probs"].data_ptr() and a[8:15] == head[8:15] and a[19] == 77
    assert a[16] == 4 and _table_of(a[15], 4) == flat and a[17] == pos.data_ptr() and a[18] == 0
    # the attribute, an int for all clips
    eng.objective, eng.nll_windows = "nll", win
    del calls[:]
    eng._fused_tail(ws, tgt, window_pos=6)
    assert [c[0] for c in calls] == ["wn_win_step_nll", "backward"]
    a = calls[0][1:]
    assert a[7] is None and a[16] == 4 and _table_of(a[15], 4) == flat and a[17] is None and a[18] == 6
    # a host sequence becomes the int64 array; None is position 0
    del calls[:]
    eng._fused_tail(ws, tgt, window_pos=[1, 2])
    a = calls[0][1:]
    assert a[17] == ws["nll_win"].pos.data_ptr() and ws["nll_win"].pos.tolist() == [1, 2] and ws["nll_win"].pos.dtype == torch.int64 and a[18] == 0
    del calls[:]
    eng._fused_tail(ws, tgt)
    assert calls[0][0] == "wn_win_step_nll" and calls[0][18] is None and calls[0][19] == 0
    # the argument wins over the attribute
    del calls[:]
    eng._fused_tail(ws, tgt, windows=[(0, 256)])
    assert calls[0][17] == 1 and _table_of(calls[0][16], 1) == [0, 256]
    # the softmax and the scores
    del calls[:]
    eng.step_probs(ws, window_pos=pos)
    eng.score_logits(ws, tgt, window_pos=pos)
    assert [c[0] for c in calls] == ["wn_win_step_softmax", "wn_win_step_nll"]
    assert len(calls[0]) == 13 and calls[0][9] == 4 and calls[0][10] == pos.data_ptr() and calls[1][18] == pos.data_ptr() and calls[1][5] is None
    # the reference's loss has no per-column softmax to window
    del calls[:]
    with pytest.raises(ValueError, match="objective"):
        eng._fused_tail(ws, tgt, objective="reference")
    eng.objective = "reference"
    with pytest.raises(ValueError, match="objective"):
        eng._fused_tail(ws, tgt)
    assert calls == []
    # and with everything unset again: the launches from before the windows
    eng.nll_windows = None
    eng._fused_tail(ws, tgt)
    eng.step_probs(ws)
    assert [c[0] for c in calls] == ["wn_chunk_softmax256_ce", "backward", "wn_step_softmax"] and len(calls[2]) == 9


def test_an_engine_built_without_init_keeps_issuing_the_plain_call(monkeypatch):
    from music_amd import _lib, engine_base
    calls = []
    monkeypatch.setattr(engine_base, "call", lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(_lib, "stream", lambda: 5)
    e = engine_base.EngineBase.__new__(engine_base.EngineBase)
    e.Q, e.device, e.marks, e.mark_only = 96, "cpu", None, None
    ws = {"B": 1, "W": 4, "O": torch.zeros(96 * 4)}
    e.step_nll(ws, torch.zeros(4, dtype=torch.int64))
    assert [c[0] for c in calls] == ["wn_step_nll"] and len(calls[0]) == 17


# ---------------------------------------------------------------- JSON keys
def test_json_keys_of_the_training_loop():
    from music_amd import objective
    from music_amd.fast_generate import stage_windows
    ds = {"token_positions": True, "quantization_channels": 64}
    tp = {"objective": "nll"}
    assert objective.nll_windows_option({}, {}) is None and objective.nll_windows_option(tp, ds) is None
    got = objective.nll_windows_option(dict(tp, nll_windows={"stages": 2, "codes": 32}), ds)
    assert got == stage_windows(2, 32) == [(0, 32), (32, 64)]
    assert objective.nll_windows_option(dict(tp, nll_windows=[[0, 10], [10, 11], [5, 64]]), ds) == [(0, 10), (10, 11), (5, 64)]
    assert objective.nll_windows_option(dict(tp, nll_windows=[[0, 100]]), ds, 128) == [(0, 100)]         # (the model's Q where it is given)
    for bad_tp in ({"nll_windows": {"stages": 2, "codes": 32}}, {"objective": "reference", "nll_windows": [[0, 4]]}):
        with pytest.raises(ValueError, match='"objective": "nll"'):
            objective.nll_windows_option(bad_tp, ds)
    for bad_ds in ({}, {"token_positions": False}):
        with pytest.raises(ValueError, match="token_positions"):
            objective.nll_windows_option(dict(tp, nll_windows=[[0, 4]]), bad_ds)
    for spec in ({"stages": 3, "codes": 32}, [[0, 65]], [[0, 32], [32, 129]]):
        with pytest.raises(ValueError, match="Q = 64"):
            objective.nll_windows_option(dict(tp, nll_windows=spec), ds)
    for spec in ({"stages": 2}, {"stages": 2, "codes": 8, "more": 1}, [], [[4, 4]], {"stages": 17, "codes": 1}):
        with pytest.raises(ValueError, match="nll_windows"):
            objective.nll_windows_option(dict(tp, nll_windows=spec), ds)
    # validation: off unless both of its keys are set, whatever the windows say
    assert objective.Validation.make(dict(tp, nll_windows=[[0, 4]], log_dir="./log/"), ds) is None
    for fn in (objective.nll_loss, objective.step_probs, objective.score):
        sig = inspect.signature(fn).parameters
        assert sig["windows"].default is None and sig["window_pos"].default is None, fn


# ---------------------------------------------------------------- loader
RF, WIN = 9, 20


def _pickle(tmp_path, lengths):
    rng = np.random.default_rng(1)
    items = [rng.integers(0, 64, size=(n,)).astype(np.int32) for n in lengths]
    path = str(tmp_path / "np_tokens.pkl")
    pickle.dump(items, open(path, "wb"))
    return items, dict(batch_size=2, shuffle=False, num_workers=0, pin_memory=False, audio_path=path, receptive_field=RF, window_length=WIN,
                       cuda_available=False, quantization_channels=64)


def test_audio_pos_is_the_offset_of_the_first_target_in_its_item(tmp_path):
    """An item of four windows plus a tail longer than rf (the re-append quirk: the last piece is appended again and keeps its
    position), then a second item of unequal length: its positions start over."""
    from music_amd import faster_audio_data as fad
    items, kw = _pickle(tmp_path, (90, 53))
    kw = {k: v for k, v in kw.items() if k not in ("batch_size", "shuffle", "num_workers", "pin_memory")}
    data = fad.audio_dataset(token_positions=True, **kw)
    want = [(0, 9), (0, 29), (0, 49), (0, 69), (0, 69), (1, 9), (1, 29)]       # 90 -> 4 windows, 10 left > rf: quirk; 53 -> 2 windows, 13 left > rf
    want.append((1, 29))
    assert [p["audio_pos"] for p in data.data] == [pos for _, pos in want]
    for piece, (n, pos) in zip(data.data, want):
        assert sorted(piece) == ["audio_piece", "audio_pos", "audio_target"]
        item = torch.from_numpy(items[n]).long()
        assert torch.equal(piece["audio_target"], item[pos:pos + WIN]) and int(piece["audio_target"][0]) == int(item[pos])
        assert torch.equal(piece["audio_piece"].long(), item[pos - RF:pos + WIN - 1])
    # unset: the pieces of before, with exactly their keys
    plain = fad.audio_dataset(**kw)
    assert len(plain.data) == len(data.data)
    for a, b in zip(plain.data, data.data):
        assert sorted(a) == ["audio_piece", "audio_target"]
        assert torch.equal(a["audio_piece"], b["audio_piece"]) and torch.equal(a["audio_target"], b["audio_target"])


@pytest.mark.parametrize("positions", [True, False, None])
def test_a_batch_carries_audio_pos_only_when_asked(tmp_path, monkeypatch, positions):
    from music_amd import faster_audio_data as fad
    monkeypatch.setattr(fad, "onehot_device", lambda codes, quantization_channels=256, scrambled=True: onehot_oracle(codes, quantization_channels, scrambled))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _, kw = _pickle(tmp_path, (90, 53))
    if positions is not None:
        kw["token_positions"] = positions
    batches = list(fad.audio_data_loader(**kw))
    assert len(batches) == 4
    if positions:
        assert [sorted(b) for b in batches] == [["audio_piece", "audio_pos", "audio_target"]] * 4
        got = torch.cat([b["audio_pos"] for b in batches])
        assert got.dtype == torch.int64 and all(tuple(b["audio_pos"].shape) == (2,) for b in batches)
        assert got.tolist() == [9, 29, 49, 69, 69, 9, 29, 29]
    else:
        assert [sorted(b) for b in batches] == [["audio_piece", "audio_target"]] * 4
