"""CPU checks of the phase-conditioned prior's surface (no device is touched): the model's parameters and their place in the
parameter order, the checkpoint refusals, phase_pos's checks, the K-ary token stream of tools/vq_codes_dataset.py --layout phase with
split_code_stream / join_code_stream(layout="phase"), the detection of such a prior by sample_code_stream / prior_score, train()'s
start-up refusal, and the engine's flat layout and rotations against tests/phase_ref.py."""
import importlib.util
import math
import os
import types

import pytest
import torch

from tests import phase_ref as ref
from tests.helpers import ROOT

CFG = dict(filter_width=2, dilations=[1, 2, 4], dilation_channels=6, residual_channels=5, skip_channels=7, quantization_channels=16,
           use_bias=True)


def _tool():
    spec = importlib.util.spec_from_file_location("vq_codes_dataset", os.path.join(ROOT, "tools", "vq_codes_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---------------------------------------------------------------- the model surface
def test_the_tables_are_the_last_parameters_and_every_earlier_draw_is_the_parents():
    from music_amd.model import wavenet
    for extra in ({}, dict(global_classes=3, global_channels=4)):
        torch.manual_seed(5)
        plain = wavenet(**CFG, **extra)
        torch.manual_seed(5)
        net = wavenet(**CFG, **extra, phase_period=3)
        names = [n for n, _ in net.named_parameters()]
        before = [n for n, _ in plain.named_parameters()]
        assert names == before + ["phase_layer_stack.%d" % i for i in range(3)] + ["connection_phase"]
        assert [p is q for p, (_, q) in zip(net.parameters(), net.named_parameters())] == [True] * len(names)
        assert set(net.state_dict()) == set(names)
        for n, p in plain.named_parameters():
            assert torch.equal(p, dict(net.named_parameters())[n]), n
        assert tuple(net.connection_phase.shape) == (7, 3) and tuple(net.phase_layer_stack[1].shape) == (12, 3)
        # gcond_layer_stack's rule (nn.Conv1d's default) at fan-in P: U(-1 / sqrt(P), 1 / sqrt(P))
        for p in list(net.phase_layer_stack) + [net.connection_phase]:
            assert p.requires_grad and 0.3 / math.sqrt(3) < float(p.detach().abs().max()) <= 1 / math.sqrt(3)
    for bad in (-1, 17, 2.0, True, "3"):
        with pytest.raises(ValueError, match="phase_period"):
            wavenet(**CFG, phase_period=bad)
    torch.manual_seed(5)
    assert list(wavenet(**CFG, phase_period=0).state_dict()) == list(wavenet(**CFG, phase_period=None).state_dict()) \
        == list(wavenet(**CFG).state_dict())
    assert wavenet(**CFG, phase_period=16).phase_period == 16


def test_a_checkpoint_loads_only_into_the_same_mode_and_period():
    from music_amd.model import wavenet
    off, p3, p4 = wavenet(**CFG), wavenet(**CFG, phase_period=3), wavenet(**CFG, phase_period=4)
    with pytest.raises(RuntimeError, match=r"saved with phase_period=3 .* built with phase_period=0"):
        off.load_state_dict(p3.state_dict())
    with pytest.raises(RuntimeError, match=r"saved with phase_period=0 .* built with phase_period=4"):
        p4.load_state_dict(off.state_dict())
    with pytest.raises(RuntimeError, match=r"saved with phase_period=3 .* built with phase_period=4"):
        p4.load_state_dict({"module." + k: v for k, v in p3.state_dict().items()})
    again = wavenet(**CFG, phase_period=3)
    again.load_state_dict(p3.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), p3.parameters()))


def test_phase_pos_is_checked_before_anything_is_built():
    from music_amd.engine_base import EngineBase
    from music_amd.model import wavenet
    on, off = wavenet(**CFG, phase_period=3), wavenet(**CFG)
    x = torch.zeros(2, 16, on.receptive_field + 3)
    with pytest.raises(ValueError, match="phase_pos must be given"):
        on(x)
    with pytest.raises(ValueError, match="negative"):
        on(x, phase_pos=[4, -1])
    with pytest.raises(ValueError, match="phase_pos must be None"):
        off(x, phase_pos=[0, 0])
    assert on._engine is None and off._engine is None
    eng = types.SimpleNamespace(phase=3, device="cpu")
    assert EngineBase.stage_phase(eng, 7, 2).tolist() == [7, 7]
    got = EngineBase.stage_phase(eng, [2 ** 40 + 1, 0], 2)
    assert got.dtype == torch.int64 and got.tolist() == [2 ** 40 + 1, 0]
    assert EngineBase.stage_phase(eng, torch.tensor([1, 2], dtype=torch.int32), 2).dtype == torch.int64
    for bad, what in (([0, -3], "negative"), ([0], "one per clip"), ([0.0, 1.0], "one per clip"), (None, "pass phase_pos")):
        with pytest.raises(ValueError, match=what):
            EngineBase.stage_phase(eng, bad, 2)
    with pytest.raises(ValueError, match="takes no phase_pos"):
        EngineBase.stage_phase(types.SimpleNamespace(phase=0), [0, 1], 2)
    assert EngineBase.stage_phase(types.SimpleNamespace(phase=0), None, 2) is None


def test_engine_layout_puts_the_tables_at_the_tail_and_the_rotations_are_the_references():
    from music_amd.engine_base import EngineBase, _Spec
    names = [("a.weight", (3, 2, 2))] + EngineBase.gclass_names(3, 4, 6, 5, 7) + EngineBase.phase_names(3, 4, 6, 5)
    off = [1, 2, 4, 8]
    eng = types.SimpleNamespace(spec=_Spec(names), dil=[1, 2, 4], D=4, S=6, off=off, rf=9, device="cpu")
    EngineBase._plan_phase(eng, 5)
    EngineBase._plan_gclass(eng, 5, 7)
    total = eng.spec.total
    assert eng.phase == 5 and eng.n_phase == (3 * 8 + 6) * 5 and eng.phase_off == (total - 150, 40, total - 30)
    assert eng.gcond_off[0] == 12 and eng.n_gcond == total - 150 - 12
    assert eng.phase_rot.tolist() == ref.rotations([1, 2, 4], 2, 5) == [(2 - 8) % 5, (4 - 8) % 5, 0, 0]
    assert EngineBase.phase_names(3, 4, 6, 0) == []
    # the rotation turns the rule on output columns into the tile rule on each block's own columns
    P, rf, pos = 5, 9, 2 ** 40 + 3
    for i in range(3):
        for t in range(off[i + 1], 40):
            assert ((t - off[i + 1]) % P + pos + ref.rotations([1, 2, 4], 2, P)[i]) % P == (pos + t - (rf - 1)) % P


def test_the_float64_model_is_the_class_conditional_one_plus_the_phase_columns():
    """tests/phase_ref.logits against tests/class_cond_ref.logits: with P = 1 the phase term is one column, a bias - folded into the
    class term's embedding-free part it must give the same logits; with P > 1 a shift by P changes nothing, a shift by 1 does"""
    from tests import class_cond_ref as cref
    cfg = dict(CFG, use_bias=False, global_classes=3, global_channels=4)
    net = cref.build(dict(cfg, phase_period=1), 9, scale=2.0)
    p = {k: v.detach().double() for k, v in net.state_dict().items()}
    x = torch.nn.functional.one_hot(torch.randint(0, 16, (2, net.receptive_field + 6), generator=torch.Generator().manual_seed(1)), 16)
    x = x.permute(0, 2, 1).double()
    cls = torch.tensor([2, 0])
    got = ref.logits(p, cfg["dilations"], x, [5, 0], cls)
    # one more embedding channel that is 1 for every class, its G column the phase column: the same network
    q = {k: v for k, v in p.items() if "phase" not in k}
    for i in range(3):
        q["gcond_layer_stack.%d.weight" % i] = torch.cat([p["gcond_layer_stack.%d.weight" % i], p["phase_layer_stack.%d" % i][:, :, None]], 1)
    q["connection_gcond.weight"] = torch.cat([p["connection_gcond.weight"], p["connection_phase"][:, :, None]], 1)
    q["global_embedding.weight"] = torch.cat([p["global_embedding.weight"], torch.ones(3, 1, dtype=torch.float64)], 1)
    want = cref.logits(q, cfg["dilations"], x, cls)
    assert float((got - want).abs().max()) < 1e-12
    net3 = cref.build(dict(CFG, phase_period=3), 9, scale=2.0)
    p3 = {k: v.detach().double() for k, v in net3.state_dict().items()}
    a, b, c = (ref.logits(p3, CFG["dilations"], x, pos) for pos in ([1, 7], [4, 7 + 3 * 2 ** 35], [2, 7]))
    assert torch.equal(a, b) and torch.equal(a[1], c[1]) and not torch.equal(a[0], c[0])


# ---------------------------------------------------------------- the token stream
def test_split_and_join_round_trip_in_both_layouts():
    from music_amd.ae_generate import join_code_stream, split_code_stream
    g = torch.Generator().manual_seed(2)
    S, K, Le = 4, 512, 7
    codes = torch.randint(0, K, (3, S, Le), generator=g)
    for layout in ("interleaved", "phase"):
        tok = join_code_stream(codes, K, layout)
        assert tok.shape == (3, Le * S) and torch.equal(split_code_stream(tok, S, K, layout), codes)
        assert int(tok.max()) < (K if layout == "phase" else S * K)
        part = codes.clone()
        part[:, 2:] = -1
        assert torch.equal(join_code_stream(part, K, layout) == -1, (part == -1).permute(0, 2, 1).reshape(3, -1))
    assert torch.equal(join_code_stream(codes, K), join_code_stream(codes, K, "interleaved"))
    assert torch.equal(join_code_stream(codes, K, "phase"), codes.permute(0, 2, 1).reshape(3, -1))          # frame-major, token = code
    with pytest.raises(ValueError, match=r"range \[0, 512\)"):
        split_code_stream(join_code_stream(codes, K), S, K, "phase")
    for fn, args in ((split_code_stream, (torch.zeros(8, dtype=torch.int64), 4, 512)), (join_code_stream, (codes, 512))):
        with pytest.raises(ValueError, match="layout"):
            fn(*args, layout="stacked")


def test_the_dataset_tool_takes_four_stages_of_512_codes_in_the_phase_layout_only():
    tool = _tool()
    tool.check_alphabet(4, 512, "phase")
    tool.check_alphabet(8, 1024, "phase")
    with pytest.raises(ValueError, match="4 x 512 = 2048"):
        tool.check_alphabet(4, 512)
    with pytest.raises(ValueError, match="4 x 512 = 2048"):
        tool.check_alphabet(4, 512, "interleaved")
    with pytest.raises(ValueError, match='"vq_codes" = 2048'):
        tool.check_alphabet(1, 2048, "phase")
    with pytest.raises(ValueError, match="layout"):
        tool.check_alphabet(2, 8, "stacked")
    with pytest.raises(SystemExit):
        tool.main(["--model-params", "m", "--checkpoint", "c", "--audio", "a", "--out", "o", "--layout", "stacked"])
    assert "layout" in tool.encode_pieces.__code__.co_varnames


def test_a_phase_prior_is_detected_and_any_other_combination_is_refused_by_name():
    from music_amd import ae_generate
    prior = lambda P, Q: types.SimpleNamespace(phase_period=P, quantization_channels=Q)
    assert ae_generate._phase_prior(prior(4, 512), 4, 512, "f") is True
    assert ae_generate._phase_prior(prior(0, 2048), 4, 512, "f") is False
    assert ae_generate._phase_prior(types.SimpleNamespace(quantization_channels=64), 2, 32, "f") is False
    for P, Q in ((4, 2048), (2, 512), (8, 512), (4, 256)):
        with pytest.raises(ValueError, match="sample_code_stream: the prior has phase_period = %d and quantization_channels = %d" % (P, Q)):
            ae_generate._phase_prior(prior(P, Q), 4, 512, "sample_code_stream")
    from music_amd.model import wavenet
    net = wavenet(**dict(CFG, quantization_channels=8), phase_period=2)
    start = torch.zeros(1, net.receptive_field + 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="phase_period = 2 and quantization_channels = 8"):
        ae_generate.sample_code_stream(net, 4, 8, 2, start)
    with pytest.raises(ValueError, match="phase_period = 2 and quantization_channels = 8"):
        ae_generate.prior_score(net, torch.zeros(1, net.receptive_field + 4, dtype=torch.int64), 2, 4)


# ---------------------------------------------------------------- train()
def test_train_refuses_at_start_a_phase_model_whose_dataset_hands_out_no_positions(monkeypatch, tmp_path):
    from music_amd import train
    tp = {"restore_model": None, "device_ids": None, "log_dir": str(tmp_path) + "/", "seed": 1}
    seen = []

    class Reached(Exception):
        pass

    def make(cls, *a):
        seen.append("validation")
        raise Reached()
    monkeypatch.setattr(train.wdist, "init_from_env", lambda: (0, 1, 0))
    monkeypatch.setattr(train.wobjective.Validation, "make", classmethod(make))
    for ds in ({}, {"token_positions": False}):
        monkeypatch.setattr(train, "get_arguments", lambda: (dict(tp), dict(CFG, phase_period=4), dict(ds)))
        with pytest.raises(ValueError, match=r'"phase_period": 4.*"token_positions": true'):
            train.train()
    assert seen == []
    # with the positions, and for a plain model without them, start-up goes on (to the stub that ends it here)
    for wp, ds in ((dict(CFG, phase_period=4), {"token_positions": True}), (dict(CFG), {})):
        monkeypatch.setattr(train, "get_arguments", lambda: (dict(tp), wp, dict(ds)))
        with pytest.raises(Reached):
            train.train()
    assert seen == ["validation", "validation"]
