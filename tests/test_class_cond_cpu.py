"""The class-conditional WaveNet without a device: tests/class_cond_ref.py (the float64 restatement the GPU tests compare against) is
held to the oracle by one identity - clip b of the conditioned model IS the oracle's biased WaveNet on clip b alone with G_i emb[c]
added to block i's dilated-conv biases (gate rows first) and G_f emb[c] to post_process_1's bias - and the model surface: parameter
order and values under one seed, the JSON keys, the host-side refusals, the labels the token tool writes, and the float64 top-2
margins of the greedy roll-outs the decode tests repeat on the device."""
import json
import os
import sys
import types

import pytest
import torch

from oracle import wavenet_oracle as wo
from tests import class_cond_ref as ref
from tests.helpers import ROOT

CFG = dict(filter_width=2, dilations=[1, 2, 4], dilation_channels=8, residual_channels=6, skip_channels=10, quantization_channels=12,
           use_bias=False)
ON = dict(global_classes=5, global_channels=7)


def _params64(net):
    return {k: v.detach().double() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("use_bias,k", [(False, 2), (True, 2), (True, 3)])
def test_the_restatement_is_the_oracles_wavenet_with_the_class_terms_folded_into_biases(use_bias, k):
    cfg = dict(CFG, use_bias=use_bias, filter_width=k, **ON)
    net = ref.build(cfg, 3, scale=2.0)
    p, dil, Q = _params64(net), cfg["dilations"], cfg["quantization_channels"]
    rf = ref.receptive_field(k, dil)
    B, T = 3, rf + 9
    g = torch.Generator().manual_seed(5)
    x = torch.nn.functional.one_hot(torch.randint(0, Q, (B, T), generator=g), Q).permute(0, 2, 1).double()
    target = torch.randint(0, Q, (B, T - rf + 1), generator=g)
    classes = torch.tensor([4, 1, 4])
    lg = ref.logits(p, dil, x, classes, k)
    G, Gf, emb = ref.global_block(p, len(dil))
    D = cfg["dilation_channels"]
    plain = {n: v for n, v in p.items() if "gcond" not in n and "global_embedding" not in n}
    losses = []
    for b in range(B):
        q = dict(plain)
        v = emb[classes[b]]
        for name in list(plain):
            if name.endswith(".weight") and name[:-7] + ".bias" not in q:
                q[name[:-7] + ".bias"] = torch.zeros(plain[name].shape[0], dtype=torch.float64)
        for i in range(len(dil)):
            c = G[i] @ v
            q["dilation_layer_stack.%d.bias" % (4 * i)] = q["dilation_layer_stack.%d.bias" % (4 * i)] + c[D:]          # filter
            q["dilation_layer_stack.%d.bias" % (4 * i + 1)] = q["dilation_layer_stack.%d.bias" % (4 * i + 1)] + c[:D]  # gate
        q["post_process_1.bias"] = q["post_process_1.bias"] + Gf @ v
        inter = {}
        probs = wo.wavenet_forward(q, dil, x[b:b + 1], filter_width=k, quantization_channels=Q, intermediates=inter)
        assert torch.allclose(inter["pre_softmax"][0], lg[b], rtol=0, atol=1e-12)
        assert torch.allclose(probs, ref.chunk_probs(lg[b:b + 1]), rtol=0, atol=1e-13)
        losses.append(wo.ce_on_probs(probs, target[b]))
    val, _ = ref.loss(p, dil, x, target, classes, "reference", k)
    assert abs(float(val) - float(torch.stack(losses).mean())) < 1e-12
    # the nll objective: the mean negative log of the per-timestep softmax, and under windows the softmax inside the position's pair
    nll, _ = ref.loss(p, dil, x, target, classes, "nll", k)
    want = -torch.log_softmax(lg, 1).gather(1, target[:, None, :]).mean()
    assert abs(float(nll) - float(want)) < 1e-12
    win = [(0, 6), (6, 12)]
    pw = ref.step_probs(lg, win, [0, 1, 3]).view(B, -1, Q)
    assert torch.allclose(pw.sum(2), torch.ones(B, T - rf + 1, dtype=torch.float64)) and float(pw[0, 0, 6:].abs().max()) == 0.0 \
        and float(pw[1, 0, :6].abs().max()) == 0.0 and float(pw[2, 1, 6:].abs().max()) == 0.0
    # autograd reaches the whole global block, and a class nobody has gets an exactly zero embedding gradient
    _, _, grads = ref.loss_and_grads(p, dil, x, target, classes, objective="nll", filter_width=k)
    assert float(grads["global_embedding.weight"][[0, 2, 3]].abs().max()) == 0.0
    assert all(float(grads[n].abs().max()) > 0 for n in grads if "gcond" in n or "global_embedding" in n)


def test_parameters_of_the_parent_come_first_and_the_global_block_is_the_tail():
    from music_amd.model import wavenet
    for use_bias in (False, True):
        cfg = dict(CFG, use_bias=use_bias)
        torch.manual_seed(7)
        parent = wavenet(**cfg)
        torch.manual_seed(7)
        off = wavenet(**cfg, global_classes=0, global_channels=0)
        torch.manual_seed(7)
        on = wavenet(**cfg, **ON)
        sd_p, sd_off, sd_on = parent.state_dict(), off.state_dict(), on.state_dict()
        names = ["causal_layer"] + ["dilation_layer_stack.%d" % j for j in range(12)] + ["post_process_1", "post_process_2"]
        want = [n + s for n in names for s in ((".weight", ".bias") if use_bias else (".weight",))]
        assert list(sd_p) == want == list(sd_off)
        assert all(torch.equal(sd_p[n], sd_off[n]) for n in want)
        tail = ["gcond_layer_stack.%d.weight" % i for i in range(3)] + ["connection_gcond.weight", "global_embedding.weight"]
        assert list(sd_on) == want + tail
        assert all(torch.equal(sd_p[n], sd_on[n]) for n in want)                          # one seed: the parent's values
        assert [tuple(sd_on[n].shape) for n in tail] == [(16, 7, 1)] * 3 + [(10, 7, 1), (5, 7)]
        assert [n for n, _ in on.named_parameters()] == want + tail and not any("bias" in n for n in tail)
        # the global block is initialised as the autoencoder's: Conv1d's and Embedding's defaults, in registration order
        torch.manual_seed(7)
        wavenet(**cfg)
        convs = [torch.nn.Conv1d(7, 16, 1, bias=False) for _ in range(3)] + [torch.nn.Conv1d(7, 10, 1, bias=False)]
        embed = torch.nn.Embedding(5, 7)
        assert all(torch.equal(c.weight, sd_on[n]) for c, n in zip(convs, tail)) and torch.equal(embed.weight, sd_on[tail[-1]])
        assert torch.equal(on.global_vectors([4, 0]), sd_on[tail[-1]][[4, 0]])


def test_json_keys_round_trip_and_bad_values_are_refused():
    from music_amd import _lib
    from music_amd.model import wavenet
    cfg = json.loads(json.dumps(dict(CFG, **ON)))
    net = wavenet(**cfg)
    assert (net.global_classes, net.global_channels) == (5, 7)
    again = wavenet(**json.loads(json.dumps({k: getattr(net, k) for k in cfg})))
    assert list(again.state_dict()) == list(net.state_dict())
    assert wavenet(**CFG).global_classes == 0 and wavenet(**CFG).global_channels == 0
    for bad in (dict(global_classes=3), dict(global_channels=3), dict(global_classes=-1, global_channels=2),
                dict(global_classes=2, global_channels=_lib.GCOND_MAX_CHANNELS + 1), dict(global_classes=True, global_channels=1),
                dict(global_classes=2.0, global_channels=2)):
        with pytest.raises(ValueError, match="global_c"):
            wavenet(**CFG, **bad)
    wavenet(**CFG, global_classes=1, global_channels=_lib.GCOND_MAX_CHANNELS)


def test_a_checkpoint_loads_only_into_its_own_mode_and_sizes():
    from music_amd.model import wavenet
    off, on, other_n, other_e = (wavenet(**CFG), wavenet(**CFG, **ON), wavenet(**CFG, global_classes=4, global_channels=7),
                                 wavenet(**CFG, global_classes=5, global_channels=8))
    on.load_state_dict(on.state_dict())
    off.load_state_dict(off.state_dict())
    for dst, src in ((off, on), (on, off), (on, other_n), (on, other_e)):
        before = {k: v.clone() for k, v in dst.state_dict().items()}
        with pytest.raises(RuntimeError, match="global_classes=.*nothing was loaded"):
            dst.load_state_dict(src.state_dict())
        assert all(torch.equal(v, dst.state_dict()[k]) for k, v in before.items())


def test_host_side_refusals():
    from music_amd import objective
    from music_amd.engine_base import EngineBase
    from music_amd.model import wavenet
    off, on = wavenet(**CFG), wavenet(**CFG, **ON)
    x = torch.zeros(2, 12, 20)
    with pytest.raises(ValueError, match="global_classes = 0: classes must be None"):
        off(x, classes=[0, 1])
    with pytest.raises(ValueError, match="global_classes = 5: classes must be given"):
        on(x)
    for fn in (lambda: objective.nll_loss(off, x, torch.zeros(2, 6, dtype=torch.int64), classes=[0, 1]),
               lambda: objective.step_probs(on, x), lambda: objective.score(on, x, torch.zeros(2, 6, dtype=torch.int64))):
        with pytest.raises(ValueError, match="global_classes"):
            fn()
    with pytest.raises(ValueError, match="global_vectors needs"):
        off.global_vectors([0])
    with pytest.raises(ValueError, match="outside"):
        on.global_vectors([5])
    # the engines' check (EngineBase.stage_classes): shape, dtype and range, on the host before anything is launched
    eng = types.SimpleNamespace(gcond=True, g_n=5, device=torch.device("cpu"))
    assert EngineBase.stage_classes(eng, [4, 0], 2).dtype == torch.int32
    for bad, what in (([5, 0], "outside"), ([-1, 0], "outside"), ([0], "one per clip"), ([0, 1, 2], "one per clip"),
                      ([0.0, 1.0], "one per clip"), (torch.zeros(2, 1, dtype=torch.int64), "one per clip")):
        with pytest.raises(ValueError, match=what):
            EngineBase.stage_classes(eng, bad, 2)
    with pytest.raises(ValueError, match="pass classes"):
        EngineBase.stage_classes(eng, None, 2)
    with pytest.raises(ValueError, match="takes no classes"):
        EngineBase.stage_classes(types.SimpleNamespace(gcond=False), [0, 1], 2)


def test_engine_layout_puts_the_global_block_at_the_tail_of_the_flat_buffer():
    from music_amd.engine_base import EngineBase, _Spec
    names = [("a.weight", (3, 2, 2))] + EngineBase.gclass_names(2, 4, 6, 5, 7)
    eng = types.SimpleNamespace(spec=_Spec(names), dil=[1, 2], D=4, S=6)
    EngineBase._plan_gclass(eng, 5, 7)
    assert eng.gcond and eng.gcond_off == (12, 56, 12 + 112, 12 + 112 + 42) and eng.n_gcond == 112 + 42 + 35 == eng.spec.total - 12
    assert EngineBase.gclass_names(2, 4, 6, 0, 0) == []


def test_the_token_tool_hands_every_item_the_label_of_its_source_piece():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vq_codes_dataset as tool
    codes = [np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(2, np.int32)]
    assert tool.item_labels([3, 1, 2], codes) == [3, 1, 2]
    assert tool.item_labels([3, 1, 2], codes, drop_empty=True) == [3, 2]
    for bad in ([3, 1], [3, 1, -2], [3, 1, 2.5], [3, True, 2]):
        with pytest.raises(ValueError):
            tool.item_labels(bad, codes)


@pytest.mark.parametrize("name", sorted(ref.DECODE_CASES))
def test_greedy_roll_outs_have_a_margin(name):
    case = ref.DECODE_CASES[name]
    cfg = case["cfg"]
    net = ref.build(cfg, case["seed"])
    rf, Q, U = net.receptive_field, cfg["quantization_channels"], len(case["classes"])
    codes, margin = ref.greedy_rollout(net.state_dict(), cfg["dilations"], ref.seed_codes(U, rf, Q, case["seed"]),
                                       torch.tensor(case["classes"]), case["steps"], Q, cfg["filter_width"])
    print("  %s: smallest top-2 margin %.3e" % (name, margin))
    assert codes.shape == (U, case["steps"]) and margin > 1e-4
    # two utterances share a class and a third has another: the class changes what is generated
    other, _ = ref.greedy_rollout(net.state_dict(), cfg["dilations"], ref.seed_codes(U, rf, Q, case["seed"]),
                                  torch.full((U,), (case["classes"][0] + 1) % cfg["global_classes"]),
                                  case["steps"], Q, cfg["filter_width"])
    assert not torch.equal(codes[0], other[0])
