"""CPU checks of music_amd/engine_base.py: the slab plans of all four engines pinned to the tables the engines built before they
shared `SlabPlan` (tests/golden/engine_base_plans.json, recorded from those hand-written loops), the properties a slab plan must
have, and the optimizer step / timing marks every engine inherits from `EngineBase`.

No device is touched: the engines are constructed on device="cpu" with `call` replaced in every music_amd module (nothing is
launched) and `_lib.stream` stubbed; the slab-count functions are host code of the library.  The autoencoder engines are
constructed from a module on the CPU; their backward workspace is planned on a fresh workspace in which `pair` and `cidx` - the
two decisions the forward leaves there - are set by the case."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_base_plans.json")
AE_DIL = [1, 2, 32, 33]          # encoder chain forms 2, 2, 1 and 0: below 32, a multiple of 32, neither


def patch_calls(monkeypatch):
    """Every launch of every music_amd module recorded instead of made -> the list of (entry point, arguments)."""
    from music_amd import _lib, ae_generic, engine, engine_generic, model1  # noqa: F401 (imported so that they are patched)
    calls, real = [], _lib.call
    for name, mod in list(sys.modules.items()):             # the engines bind the name at import (from ._lib import call)
        if name.startswith("music_amd") and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "stream", lambda: None)
    return calls


def _wavenet(ch, B, T=1200):
    from music_amd.engine import WaveNetEngine
    eng = WaveNetEngine([1, 2, 4, 32, 64], ch, ch, 256, device="cpu")
    return eng, eng._make_workspace(B, T)


def _general():
    from music_amd.engine_generic import GenericWaveNetEngine
    eng = GenericWaveNetEngine([1, 2, 4], 48, 40, 96, quantization_channels=100, filter_width=3, device="cpu")
    return eng, eng._make_workspace(2, 300)


def _ae_net(en, de, **kw):
    from music_amd.model1 import wavenet_autoencoder
    cfg = dict(filter_width=2, quantization_channel=256, dilations=AE_DIL, en_residual_channel=en, en_dilation_channel=en,
               en_bottleneck_width=8, en_pool_kernel_size=40, de_residual_channel=de, de_dilation_channel=de, de_skip_channel=32,
               use_bias=False)
    cfg.update(kw)
    torch.manual_seed(0)
    return wavenet_autoencoder(**cfg)


def _autoencoder(en, de, B, pair, cidx):
    from music_amd.model1 import _AutoencoderEngine
    eng = _AutoencoderEngine(_ae_net(en, de), torch.device("cpu"))
    ws = eng._make_workspace(B, 400)
    assert eng.pair_ok or not pair
    ws["pair"] = pair
    if cidx:
        ws["cidx"] = None        # (only its presence is read: the forward built the bucket bytes of the conditioning)
    return eng, ws


def _ae_general():
    from music_amd.ae_generic import GenericAutoencoderEngine
    net = _ae_net(24, 40, filter_width=3, quantization_channel=100, dilations=[1, 2, 4])
    eng = GenericAutoencoderEngine(net, torch.device("cpu"))
    return eng, eng._make_workspace(2, 300)


# name -> (environment switches, builder of (engine, fresh workspace))
CASES = {
    "wavenet64": ({}, lambda: _wavenet(64, 2)),                                  # one-launch blocks, chain = [F, F, F, T, T]
    "wavenet64_channel_split": ({"WN_PQ_BWD": "0"}, lambda: _wavenet(64, 2)),
    "wavenet64_chunk512": ({"WN_MS_BWD": "0"}, lambda: _wavenet(64, 2)),
    "wavenet32_pair": ({}, lambda: _wavenet(32, 2)),
    "wavenet32_odd_batch": ({}, lambda: _wavenet(32, 3)),
    "general_wavenet": ({}, _general),
    "autoencoder32_pair": ({}, lambda: _autoencoder(32, 32, 2, True, True)),
    "autoencoder32_odd_batch": ({}, lambda: _autoencoder(32, 32, 3, False, False)),
    "autoencoder64": ({}, lambda: _autoencoder(64, 64, 2, False, True)),         # one-launch blocks on both sides
    "autoencoder64_long_encoding": ({}, lambda: _autoencoder(64, 64, 2, False, False)),
    "autoencoder_en32_de64": ({}, lambda: _autoencoder(32, 64, 2, False, True)),
    "general_autoencoder": ({}, _ae_general),
}


def snapshot(bw):
    """What pins a slab plan: both reduction tables, the counts wn_reduce_slabs takes, the slab tensor's size, the kernel forms,
    and where every launch writes ((so, n) and the chunk wn_wgrad is handed; None for an op another kernel writes)."""
    plan = bw["plan"]
    return dict(desc=bw["desc"].tolist(), desc_codes=bw["desc_codes"].tolist() if "desc_codes" in bw else None,
                vec=bw["vec"], nops=bw["nops"], slab=bw["slab"].numel(),
                forms={k: bw[k] for k in ("chain", "pq", "ms", "pair", "enc_chain", "enc_pq", "enc_fused") if k in bw},
                plan={name: [op.so, op.n, op.chunk] for name, op in plan.ops.items()})


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def planned(request, monkeypatch):
    """(engine, backward workspace) of the case named by the test's parameter."""
    env, build = CASES[request.param]
    patch_calls(monkeypatch)
    for k in ("WN_PQ_BWD", "WN_MS_BWD", "WN_PAIR32", "WN_PQ_CHAIN", "WN_ENC_LCH", "WN_AE_ENC_PQ", "WN_AE_FUSED_ENC", "WN_EPI_WGRAD_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng, ws = build()
    return eng, eng._bwd_workspace(ws)


@pytest.mark.parametrize("planned", list(CASES), indirect=True)
def test_slab_plan_is_the_one_the_hand_written_loops_built(planned, golden, request):
    want = golden[request.node.callspec.params["planned"]]
    got = json.loads(json.dumps(snapshot(planned[1])))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_recorded_tables_are_the_known_ones(golden):
    """A few figures of the recorded tables that were worked out independently of the recording, and the kernel forms the cases are there for."""
    g = golden["wavenet64"]
    assert (g["nops"], g["vec"], g["slab"]) == (13, 86016, 7168000) and g["forms"]["chain"] == [False, False, False, True, True]
    assert g["desc"][0] == [0, 0, 2, 65536, 282624, 65536]
    assert (golden["general_wavenet"]["nops"], golden["general_wavenet"]["vec"]) == (13, 36608)
    assert golden["autoencoder64"]["forms"]["enc_chain"] == [2, 2, 1, 0]
    assert golden["wavenet32_pair"]["forms"]["pair"] and not golden["wavenet32_odd_batch"]["forms"]["pair"]
    assert golden["autoencoder32_pair"]["forms"]["pair"] and not golden["autoencoder32_odd_batch"]["forms"]["pair"]


@pytest.mark.parametrize("planned", list(CASES), indirect=True)
def test_slab_plan_properties(planned):
    eng, bw = planned
    plan, desc = bw["plan"], bw["desc"].tolist()
    # the slab regions of all ops, alternatives included, are disjoint and cover [0, total) exactly
    at = 0
    for so, size in sorted((op.so, op.ns * op.n) for op in plan.ops.values()):
        assert so == at and size > 0
        at += size
    assert at == bw["slab"].numel()
    # the reduction table: one row per add() in order, vs advancing by the float4 vectors of the row before
    named = [name for name in plan.ops if name in plan.row]
    assert [plan.row[name] for name in named] == list(range(len(desc))) and bw["nops"] == len(desc)
    vs = 0
    for name, row in zip(named, desc):
        op, (go, r, c) = plan[name], eng.gp_off[name]
        assert row == [vs, op.so, op.ns, op.n, go, op.n] and op.n == r * c
        vs += (op.n + 3) // 4
    assert vs == bw["vec"]
    # the alternative table differs from the main one in columns 1-2 of the named rows only
    alt = [name for name in plan.ops if name not in plan.row]
    assert ("desc_codes" in bw) == bool(alt)
    if alt:
        codes = bw["desc_codes"].tolist()
        rows = {plan.row[name[:-len("_codes")]]: plan[name] for name in alt}
        for i, (a, b) in enumerate(zip(desc, codes)):
            if i in rows:
                assert b[1:3] == [rows[i].so, rows[i].ns] and b[1] != a[1] and a[:1] + a[3:] == b[:1] + b[3:]
                assert rows[i].n == a[3] and rows[i].chunk is None
            else:
                assert a == b
    # wn_wgrad is only ever handed a real chunk length
    assert all(op.chunk is None or op.chunk > 0 for op in plan.ops.values())


def test_slab_plan_on_its_own():
    from music_amd.engine_base import SlabPlan
    plan = SlabPlan({"a": (100, 3, 5), "b": (0, 2, 2)})
    plan.add("a", 4, 512)
    plan.add("b", 1)
    plan.add("b_again", 3, grad="b")                       # a second launch into the same gradient matrix
    plan.add_alternative("a", "a_codes", 7)
    out = plan.finish("cpu")
    assert out["desc"].tolist() == [[0, 0, 4, 15, 100, 15], [4, 60, 1, 4, 0, 4], [5, 64, 3, 4, 0, 4]]
    assert out["desc_codes"].tolist() == [[0, 76, 7, 15, 100, 15], [4, 60, 1, 4, 0, 4], [5, 64, 3, 4, 0, 4]]
    assert (out["vec"], out["nops"], out["slab"].numel()) == (6, 3, 76 + 7 * 15) and out["plan"] is plan
    assert tuple(plan["a"]) == (0, 15, 512, 4) and plan["a_codes"].chunk is None and plan["b"].chunk is None
    assert "desc_codes" not in SlabPlan({}).finish("cpu")


# ---------------------------------------------------------------- EngineBase: optimizer step and marks
def _stub():
    from music_amd.engine_base import EngineBase

    class Stub(EngineBase):
        def _make_workspace(self, B, T):
            return dict(B=B, T=T)
    eng = Stub()
    eng.device = torch.device("cpu")
    eng.flat, eng.flat_grad = torch.zeros(10), torch.zeros(10)
    eng.spec = type("S", (), {"total": 10})()
    eng._init_state()
    return eng


ENGINES = {"stub": _stub, "wavenet": lambda: _wavenet(64, 2)[0], "general_wavenet": lambda: _general()[0],
           "autoencoder": lambda: _autoencoder(64, 64, 2, False, True)[0], "general_autoencoder": lambda: _ae_general()[0]}


@pytest.fixture
def engine(request, monkeypatch):
    calls = patch_calls(monkeypatch)
    return ENGINES[request.param](), calls


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
def test_adam_step_is_one_launch_or_the_guarded_pair(engine):
    eng, calls = engine
    assert eng.adam_state is None and eng.guard_report() is None
    assert eng._throttle is not None and eng.marks is None and eng.mark_only is None
    eng.adam_init(lr=1e-3, betas=(0.8, 0.95))
    assert eng.guard_report() is None
    for t in (1, 2, 3):
        del calls[:]
        eng.adam_step(gscale=0.5)
        (name, a), = calls
        assert name == "wn_adam_flat" and len(a) == 13 and a[4] == eng.spec.total
        assert a[:4] == tuple(x.data_ptr() for x in (eng.flat, eng.flat_grad, eng.adam_state["m"], eng.adam_state["v"]))
        assert a[5:9] == (1e-3, 0.8, 0.95, 1e-8) and a[9] == 1.0 - 0.8 ** t and a[10] == 1.0 - 0.95 ** t and a[11] == 0.5
        assert eng.adam_state["t"] == t
    # with a guard set: wn_grad_guard + the guarded update through music_amd/guard.py, never the plain entry
    eng.adam_init(lr=1e-3, max_grad_norm=2.0, skip_nonfinite=True)
    del calls[:]
    eng.adam_step(gscale=0.25)
    assert [c[0] for c in calls] == ["wn_grad_guard", "wn_adam_flat_guarded"] and eng.adam_state["t"] == 1
    assert calls[0][1][2:5] == (0.25, 2.0, 1) and calls[1][1][-2] == eng.adam_state["guard"].state_ptr()
    eng.adam_state["guard"].seed_taken(5)
    assert eng.guard_report()["taken"] == 5 and eng.adam_state["t"] == 5


class _Event:
    def __init__(self, enable_timing=False):
        assert enable_timing

    def record(self):
        pass


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
def test_mark_honours_mark_only_and_only_the_wavenet_engine_marks_adam(engine, monkeypatch, request):
    eng, _ = engine
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    eng.mark("a")                                          # marks is None: nothing is recorded, no event is made
    eng.marks = []
    eng.mark("a")
    eng.mark("b")
    eng.mark_only = {"b", "adam"}
    eng.mark("a")
    eng.mark("b")
    assert [n for n, _ in eng.marks] == ["a", "b", "b"] and all(isinstance(e, _Event) for _, e in eng.marks)
    eng.marks, eng.mark_only = [], None
    eng.adam_init()
    eng.adam_step()
    assert [n for n, _ in eng.marks] == (["adam"] if request.node.callspec.params["engine"] == "wavenet" else [])
