"""CPU checks of the per-timestep softmax / negative log-likelihood entry points wn_step_softmax and wn_step_nll
(include/wavenet_hip.h, music_amd/csrc/wn_nll.hip) - declared, exported, bound with matching arity, every refusal reported by name
before anything is launched - and of the host surface above them that needs no device: the `objective` switch of the engines, the
JSON keys of train() / ae_train, and the loader's one_hot layout.  No device is touched."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.cpu_model import onehot_oracle
from tests.helpers import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,arity", [("wn_step_softmax", 8), ("wn_step_nll", 16)])
def test_entries_are_declared_exported_and_bound(name, arity):
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]) == arity


def test_the_version_stays_9():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
NLL_ARGS = ("x", "x_bstride", "x_pitch", "target", "dx", "dx_bstride", "dx_pitch", "probs", "row_nll", "row_hit", "loss_part", "w", "q",
            "batch", "inv_n", "stream")
SM_ARGS = ("x", "x_bstride", "x_pitch", "probs", "w", "q", "batch", "stream")


def _refused(fn, names, ok, arg, **kw):
    from music_amd import _lib
    lib = _lib.load()
    a = list(ok)
    for k, v in kw.items():
        a[names.index(k)] = v
    rc = getattr(lib, fn)(*a)
    msg = lib.wn_last_error().decode()
    assert rc == -4 and fn in msg and "'%s'" % arg in msg, (fn, arg, rc, msg)


def test_step_nll_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    w, q = 70, 256
    ok = [P, q * w, w, P, P, q * w, w, P, P, P, P, w, q, 2, 0.5, None]
    bad = lambda arg, **kw: _refused("wn_step_nll", NLL_ARGS, ok, arg, **kw)
    for name in ("x", "target", "loss_part"):
        bad(name, **{name: None})
    for v in (0, -1, 1025):
        bad("q", q=v)
    bad("x_pitch", x_pitch=w - 1)
    bad("dx_pitch", dx_pitch=w - 1)
    bad("x_bstride", x_bstride=q * w - 1)
    bad("dx_bstride", dx_bstride=q * w - 1)
    bad("x_bstride", x_pitch=w + 3)                     # (the stride no longer holds q rows of that pitch)
    bad("batch", batch=-1)
    bad("w", w=-1)
    # dx not wanted: its stride and pitch are not looked at; empty calls return 0 with NULLs (loss_part NULL: nothing to zero)
    assert lib.wn_step_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 256, 4, 1.0, None) == 0
    assert lib.wn_step_nll(None, 256 * 5, 5, None, None, 0, 0, None, None, None, None, 5, 256, 0, 1.0, None) == 0
    # ... but the shapes of an empty call are still checked
    assert lib.wn_step_nll(None, 0, 0, None, None, 0, 0, None, None, None, None, 0, 0, 0, 1.0, None) == -4
    assert "'q'" in lib.wn_last_error().decode()


def test_step_softmax_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    w, q = 33, 100
    ok = [P, q * w, w, P, w, q, 3, None]
    bad = lambda arg, **kw: _refused("wn_step_softmax", SM_ARGS, ok, arg, **kw)
    bad("x", x=None)
    bad("probs", probs=None)
    for v in (0, 1025):
        bad("q", q=v)
    bad("x_pitch", x_pitch=w - 1)
    bad("x_bstride", x_bstride=q * w - 1)
    assert lib.wn_step_softmax(None, q * w, w, None, w, q, 0, None) == 0
    assert lib.wn_step_softmax(None, 0, 0, None, 0, q, 3, None) == 0


def test_objective_switch_of_the_engines():
    """`objective` is a class attribute of EngineBase with the default "reference"; None resolves to it, anything else is refused;
    every engine's loss_and_grad (and loss_and_grad_codes) takes objective=None."""
    import inspect
    from music_amd import ae_generic, engine, engine_base, engine_generic, model1
    eb = engine_base.EngineBase
    assert eb.objective == "reference" and engine_base.OBJECTIVES == ("reference", "nll")
    e = eb.__new__(eb)
    assert e._resolve_objective(None) == "reference" and e._resolve_objective("nll") == "nll"
    e.objective = "nll"
    assert e._resolve_objective(None) == "nll" and e._resolve_objective("reference") == "reference"
    with pytest.raises(ValueError, match="objective"):
        e._resolve_objective("mse")
    for cls in (engine.WaveNetEngine, engine_generic.GenericWaveNetEngine, model1._AutoencoderEngine, ae_generic.GenericAutoencoderEngine):
        assert issubclass(cls, eb)
        fns = [cls.loss_and_grad] + ([cls.loss_and_grad_codes] if hasattr(cls, "loss_and_grad_codes") else [])
        for fn in fns:
            assert inspect.signature(fn).parameters["objective"].default is None, fn
        assert "step_nll" not in cls.__dict__ and "score_logits" not in cls.__dict__          # one copy, in the base


def test_fused_tail_launches_step_nll_only_under_nll(monkeypatch):
    """_fused_tail with the launches patched out: "reference" (and unset) goes through softmax_ce exactly as before, "nll" issues ONE
    wn_step_nll on ws["O"] / bw["dO"] with pitch W and clip stride Q W, 1 / (B W), and the probabilities when they are wanted."""
    from music_amd import _lib, engine_base
    calls = []
    monkeypatch.setattr(engine_base, "call", lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(_lib, "stream", lambda: 77)
    B, W, Q = 2, 5, 256

    class Eng(engine_base.EngineBase):
        device, Q = "cpu", 256

        def __init__(self):
            self.marks = self.mark_only = None
            self.bw = {"dO": torch.zeros(B * Q * W)}

        def _bwd_workspace(self, ws):
            return self.bw

        def backward_from_dlogits(self, ws):
            calls.append(("backward",))
    eng = Eng()
    ws = {"B": B, "W": W, "O": torch.zeros(B * Q * W)}
    tgt = torch.zeros(B, W, dtype=torch.int64)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for objective in (None, "reference"):
        del calls[:]
        eng._fused_tail(ws, tgt, objective=objective)
        assert [c[0] for c in calls] == ["wn_chunk_softmax256_ce", "backward"]
    del calls[:]
    eng._fused_tail(ws, tgt, want_probs=True, objective="nll")
    assert [c[0] for c in calls] == ["wn_step_nll", "backward"]
    a = calls[0][1:]
    assert a[0] == ws["O"].data_ptr() and a[1:3] == (Q * W, W) and a[4] == eng.bw["dO"].data_ptr() and a[5:7] == (Q * W, W)
    assert a[7] == ws["probs"].data_ptr() and a[8] is None and a[9] is None and a[10] == ws["loss_part"].data_ptr()
    assert a[11:14] == (W, Q, B) and a[14] == 1.0 / (B * W) and a[15] == 77 and tuple(ws["probs"].shape) == (B * W, Q)
    eng.objective = "nll"
    del calls[:]
    eng._fused_tail(ws, tgt)
    assert [c[0] for c in calls] == ["wn_step_nll", "backward"] and calls[0][8] is None          # (no probabilities this time)


def test_json_keys_of_the_training_loops():
    from music_amd import objective
    assert objective.objective_option({}) == "reference" and objective.objective_option({"objective": "nll"}) == "nll"
    with pytest.raises(ValueError, match="objective"):
        objective.objective_option({"objective": "NLL"})
    # validation is off unless BOTH keys are set: nothing is built (the path is not even opened)
    for tp in ({}, {"valid_audio_path": "/nowhere.pkl"}, {"validate_every": 5}, {"valid_audio_path": "/nowhere.pkl", "validate_every": 0}):
        assert objective.Validation.make(dict(tp, log_dir="./log/"), {}) is None


def _pieces(tmp_path):
    rng = np.random.default_rng(1)
    path = str(tmp_path / "np_audio.pkl")
    pickle.dump([rng.integers(0, 256, size=(90,)).astype(np.int32)], open(path, "wb"))
    return dict(batch_size=2, shuffle=False, num_workers=0, pin_memory=False, audio_path=path, receptive_field=9, window_length=20,
                cuda_available=False, quantization_channels=256)


@pytest.mark.parametrize("one_hot,scrambled", [(None, True), ("scrambled", True), ("canonical", False)])
def test_loader_one_hot_key_reaches_the_collate(tmp_path, monkeypatch, one_hot, scrambled):
    """audio_data_loader(one_hot=...) (the "one_hot" key of dataset_params.json) -> _Collate -> onehot_device(scrambled=...); unset,
    the loader's layout is the scrambled one, as before."""
    from music_amd import faster_audio_data as fad
    seen = []

    def spy(codes, quantization_channels=256, scrambled=True):
        seen.append(scrambled)
        return onehot_oracle(codes, quantization_channels, scrambled)
    monkeypatch.setattr(fad, "onehot_device", spy)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    kw = _pieces(tmp_path)
    if one_hot is not None:
        kw["one_hot"] = one_hot
    loader = fad.audio_data_loader(**kw)
    assert loader.collate_fn.scrambled is scrambled
    batch = next(iter(loader))
    assert seen == [scrambled] and tuple(batch["audio_piece"].shape) == (2, 256, 28)
    codes = torch.stack([loader.dataset[i]["audio_piece"] for i in range(2)])
    assert torch.equal(batch["audio_piece"], onehot_oracle(codes, 256, scrambled))
    if not scrambled:                                     # the true one-hot: x[b][code[t]][t] = 1
        assert torch.equal(batch["audio_piece"].argmax(1), codes.long())


def test_loader_refuses_an_unknown_layout(tmp_path):
    from music_amd import faster_audio_data as fad
    with pytest.raises(ValueError, match="one_hot"):
        fad.audio_data_loader(one_hot="proper", **_pieces(tmp_path))
    assert fad._Collate(256).scrambled is True and fad._Collate(256, (0, 2)).scrambled is True
