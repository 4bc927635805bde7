"""CPU check that a host-side change leaves what the fast engines LAUNCH alone: every launch of a step of music_amd/engine.py
and music_amd/model1.py - entry point, argument values, stream, position in the order - every event recorded or waited on and
every timing mark, compared with the trace recorded at the commit named in tests/golden/launch_traces.json (written once by
tools/record_launch_trace.py --write, never regenerated), and the index maps _build_packs produces compared by hash.

A second file, tests/golden/launch_traces_epilogue.json (tools/record_launch_trace.py --write --set epilogue, at the commit it names),
pins the forms of the skip epilogue the first one does not reach - the three-launch forward, one chain, the fused backward and its
switches, learned conditioning - and the pack maps of the two general engines.

A third file, tests/golden/launch_traces_optimizers.json (--set optimizers), pins what ENDS a step: the launches of the three flat
optimizers of music_amd/train.py and of the fused step's adam_step - plain and guarded, with and without an EMA shadow and an
EMA-updated codebook - over short scripted sequences, with the steps that launch nothing (torch's path) and the optimizer's state
after every step.

A fourth file, tests/golden/launch_traces_decode.json (--set decode), pins the generators: what fast_generate.py and ae_generate.py
launch between a prompt and the persistent decode kernel, every public way in.

The recording itself (what is stubbed, how pointers are named) is tests/launch_trace.py.  No device is touched."""
import json
import os

import pytest

from tests import launch_trace as lt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")
GOLDEN_EPILOGUE = os.path.join(os.path.dirname(GOLDEN), "launch_traces_epilogue.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden_epilogue():
    with open(GOLDEN_EPILOGUE) as f:
        return json.load(f)


def _same(want, trace, packs, forms):
    trace = json.loads(json.dumps(trace))
    assert forms == want["forms"]
    assert packs == want["packs"]
    for k, (got, exp) in enumerate(zip(trace, want["trace"])):
        assert got == exp, "item %d of %d" % (k, len(want["trace"]))
    assert len(trace) == len(want["trace"])


def test_the_recorded_cases_are_the_cases(golden):
    assert len(golden["recorded_at"]) == 40 and sorted(golden["cases"]) == sorted(lt.TRACE_CASES)
    # the forms the cases are there for
    forms = {name: case["forms"] for name, case in golden["cases"].items()}
    assert forms["wavenet64"]["pq"] and forms["wavenet64"]["chain"] == [False, False, False, True, True]
    assert forms["wavenet64_channel_split"]["ms"] and not forms["wavenet64_channel_split"]["pq"] and not forms["wavenet64_chunk512"]["ms"]
    assert forms["wavenet64_bias"]["ms"] and not forms["wavenet64_bias"]["pq"]
    assert forms["wavenet32_pair"]["pair"] and not forms["wavenet32_pair"]["pair_fwd"] and forms["wavenet32_pair_fwd"]["pair_fwd"]
    assert not forms["wavenet32_odd_batch"]["pair"] and not forms["wavenet32_odd_batch"]["ms"]
    assert forms["autoencoder32_pair"]["pair"] and not forms["autoencoder32_odd_batch"]["pair"]
    assert forms["autoencoder64"]["pq"] and forms["autoencoder64"]["enc_pq"] and forms["autoencoder64"]["enc_chain"] == [2, 2, 1, 0]
    assert forms["autoencoder64_long_encoding"]["ms"] and not forms["autoencoder64_long_encoding"]["pq"] and not forms["autoencoder64_long_encoding"]["cidx"]
    assert forms["autoencoder_en32_de64"]["pq"] and not forms["autoencoder_en32_de64"]["enc_fused"]
    assert forms["autoencoder64_bias"]["ms"] and forms["autoencoder64_bias"]["enc_fused"] and not forms["autoencoder64_bias"]["enc_pq"]
    entries = lambda name: [i[1] for i in golden["cases"][name]["trace"] if i[0] == "call"]
    assert "wn_causal_fwd_codes" in entries("wavenet64_codes") and "wn_causal_wgrad_codes" in entries("wavenet64_onehot_tag")
    assert "wn_causal_fwd_codes" not in entries("wavenet64") and "wn_chunk_softmax256_bwd" in entries("autoencoder64_fwd_bwd")
    assert any(i[:2] == ["call", "wn_wgrad"] and i[2] == "side" for i in golden["cases"]["wavenet64"]["trace"])


@pytest.mark.parametrize("name", list(lt.TRACE_CASES))
def test_launch_trace_is_the_recorded_one(name, golden, monkeypatch):
    want = golden["cases"][name]
    trace, packs, forms = lt.record(name, monkeypatch)
    trace = json.loads(json.dumps(trace))
    assert forms == want["forms"]
    assert packs == want["packs"]
    for k, (got, exp) in enumerate(zip(trace, want["trace"])):
        assert got == exp, "item %d of %d" % (k, len(want["trace"]))
    assert len(trace) == len(want["trace"])


def test_the_recorded_epilogue_cases_are_the_cases(golden_epilogue):
    g = golden_epilogue
    assert len(g["recorded_at"]) == 40 and sorted(g["cases"]) == sorted(lt.EPILOGUE_CASES) and sorted(g["packs_only"]) == sorted(lt.PACK_CASES)
    assert all("gp_bias_off" in p and "gidx" in p for p in g["packs_only"].values())
    items = lambda name: g["cases"][name]["trace"]
    calls = lambda name, entry=None: [i for i in items(name) if i[0] == "call" and entry in (None, i[1])]
    on = lambda name, entry: [i[2] for i in calls(name, entry)]
    # the three-launch forward: two chains on two streams, one chain on the main stream, the summed skip bias as the first product's bias
    for name in ("wavenet64_epi3", "wavenet64_epi3_one_chain", "wavenet64_bias_epi3"):
        assert not calls(name, "wn_skip_epilogue_fwd")
    fwd3 = lambda name: [i for i in calls(name, "wn_chan_gemm") if i[3][10][0] in ("eng.pk_f", "eng.pk")][-6:]
    assert [i[2] for i in fwd3("wavenet64_epi3")] == ["main"] * 3 + ["side"] * 3
    assert [i[2] for i in fwd3("wavenet64_epi3_one_chain")][-3:] == ["main"] * 3 and "side" not in on("wavenet64_epi3_one_chain", "wn_chan_gemm")
    assert fwd3("wavenet64_bias_epi3")[0][3][17][0] == "ws.bias_skip" and fwd3("wavenet64_epi3")[0][3][17] is None
    # five blocks of 64 channels never take the fused backward; six do, and the autoencoder with 256 skip channels, biases or not
    for name in ("wavenet64_epi_bwd3", "wavenet64_epi_bwd_order0", "autoencoder64_epi_bwd3", "autoencoder64_bias_epi_bwd3",
                 "wavenet64_six_blocks_epi_bwd3", "autoencoder64_six_blocks_epi_bwd3"):
        assert not calls(name, "wn_skip_epilogue_bwd")
    for name in ("wavenet64_six_blocks", "wavenet64_six_blocks_bwd_order0", "autoencoder64_six_blocks", "autoencoder64_six_blocks_bias"):
        assert len(calls(name, "wn_skip_epilogue_bwd")) == 1
    assert on("wavenet64_six_blocks", "wn_wgrad")[:3] == ["side", "side", "main"]
    assert on("wavenet64_six_blocks_bwd_order0", "wn_wgrad")[:3] == ["side", "side", "side"]
    # the conditioning gradient directly behind the launch that produces dR1, in both forms
    for name, entry in (("autoencoder64_six_blocks", "wn_skip_epilogue_bwd"), ("autoencoder64_six_blocks_epi_bwd3", "wn_chan_gemm")):
        seq = [i[1] for i in calls(name)]
        k = seq.index("wn_cond_grad")
        assert seq[k - 1] == entry
    assert calls("autoencoder64_bias_epi_bwd3", "wn_bias_grad") and calls("autoencoder64_six_blocks_bias", "wn_bias_grad")
    assert "side" not in [i[2] for i in calls("autoencoder64_no_overlap")] and not [i for i in items("autoencoder64_no_overlap") if i[0] != "call" and i[0] != "mark"]
    assert len(calls("autoencoder64_learned", "wn_cond_proj_fwd")) == 1 and len(calls("autoencoder64_learned", "wn_cond_proj_bwd")) == 1


@pytest.mark.parametrize("name", list(lt.EPILOGUE_CASES))
def test_epilogue_launch_trace_is_the_recorded_one(name, golden_epilogue, monkeypatch):
    _same(golden_epilogue["cases"][name], *lt.record(name, monkeypatch))


@pytest.mark.parametrize("name", list(lt.PACK_CASES))
def test_general_engine_pack_maps_are_the_recorded_ones(name, golden_epilogue, monkeypatch):
    assert lt.record_packs(name, monkeypatch) == golden_epilogue["packs_only"][name]


# ---------------------------------------------------------------- the optimizer steps
GOLDEN_OPTIMIZERS = os.path.join(os.path.dirname(GOLDEN), "launch_traces_optimizers.json")


@pytest.fixture(scope="module")
def golden_optimizers():
    with open(GOLDEN_OPTIMIZERS) as f:
        return json.load(f)


def test_the_recorded_optimizer_cases_are_the_cases(golden_optimizers):
    g = golden_optimizers
    assert len(g["recorded_at"]) == 40 and sorted(g["cases"]) == sorted(lt.OPTIMIZER_CASES)
    assert os.path.getsize(GOLDEN_OPTIMIZERS) < 1 << 20


def test_the_recorded_optimizer_cases_hold_the_forms_they_are_there_for(golden_optimizers):
    """What the third file pins (tests/golden/launch_traces_optimizers.json, tools/record_launch_trace.py --write --set optimizers at
    the commit it names): the launches that END a step - the update, plain or behind wn_grad_guard, then the codebook's EMA update,
    then the shadow's - of the three flat optimizers and of the fused step, and which steps launch nothing (torch's path).  The guard
    is the real GradGuard on the CPU; the one piece played for the device is its count of steps taken, which the recorder bumps
    per wn_grad_guard issued (tests/launch_trace.py, record_optimizer)."""
    cases = golden_optimizers["cases"]

    def steps(name):                                          # the entry points of every item of the case's sequence
        out = []
        for item in cases[name]["trace"]:
            if item[0] == "step":
                out.append([])
            else:
                out[-1].append(item[1])
        return out
    forms = lambda name: cases[name]["forms"]["steps"]
    args = lambda name, entry: [i[3] for i in cases[name]["trace"] if i[0] == "call" and i[1] == entry]
    for kind, keys in (("adam", ["exp_avg", "exp_avg_sq"]), ("sgd", ["momentum_buffer"]), ("rmsprop", ["momentum_buffer", "square_avg"])):
        entry = "wn_%s_flat" % kind
        for g, head in (("plain", [entry]), ("guarded", ["wn_grad_guard", entry + "_guarded"])):
            for s, tail in (("", []), ("_shadow", ["wn_ema_flat"])):
                # flat, flat, foreign gradients (torch's path: no launch), flat, load_state_dict(state_dict()), flat
                assert steps("%s_%s%s" % (kind, g, s)) == [head + tail, head + tail, [], head + tail, [], head + tail], (kind, g, s)
                f = forms("%s_%s%s" % (kind, g, s))
                assert all(all(st[k] == "1" * 11 for k in keys) for st in f)                 # views of the flat buffers throughout
                assert [st["fresh"] for st in f] == [keys, [], [], [], [], keys]              # ... adopted anew after a load, only then
            assert steps("%s_vq_ema_%s_shadow" % (kind, g)) == [head + ["wn_vq_ema_update", "wn_ema_flat"]] * 2
        assert all(a[11] is None for a in args(kind + "_vq_ema_plain_shadow", "wn_vq_ema_update"))
        assert all(a[11] == ["guard.state", 0] for a in args(kind + "_vq_ema_guarded_shadow", "wn_vq_ema_update"))
        assert steps(kind + "_weight_decay")[1:] == [[], []]
    # the step counters: bumped by the host on the plain path, the device's count (read back by state_dict()) on the guarded one
    assert [st["step"][0] for st in forms("adam_plain")] == [1.0, 2.0, 3.0, 4.0, 4.0, 5.0]
    assert [st["step"][0] for st in forms("adam_guarded")] == [0.0, 0.0, 3.0, 3.0, 4.0, 4.0]
    assert [st["step"][0] for st in forms("rmsprop_guarded")] == [0.0, 0.0, 3.0, 3.0, 4.0, 4.0]
    # SGD's first step, and the momentum buffer only with momentum
    assert [a[7] for a in args("sgd_plain", "wn_sgd_flat")] == [1, 0, 0, 0] and [a[7] for a in args("sgd_momentum0", "wn_sgd_flat")] == [0, 0]
    assert all(a[2] == ["opt.momentum_buffer", 0] for a in args("sgd_plain", "wn_sgd_flat"))
    for name, entry, at in (("sgd_momentum0", "wn_sgd_flat", 2), ("sgd_momentum0_guarded", "wn_sgd_flat_guarded", 2),
                            ("rmsprop_momentum0", "wn_rmsprop_flat", 3), ("rmsprop_momentum0_guarded", "wn_rmsprop_flat_guarded", 3)):
        assert len(args(name, entry)) == 2 and all(a[at] is None for a in args(name, entry))
        assert "momentum_buffer" not in forms(name)[-1]["keys"]
    # torch's path: a closure, parameters at different step counts, some momentum buffers, a second group, weight decay
    assert steps("adam_closure") == [["wn_adam_flat", "wn_ema_flat"], [], ["wn_adam_flat", "wn_ema_flat"]]
    assert [a[5] for a in args("adam_closure", "wn_ema_flat")] == [1, 3]           # the update on the host counted
    assert steps("adam_mixed_steps") == [["wn_adam_flat"], [], [], []] and forms("adam_mixed_steps")[-1]["step"][:2] == [6.0, 3.0]
    assert steps("sgd_some_momentum_buffers") == [[], [], ["wn_sgd_flat"]]
    assert [st["momentum_buffer"] for st in forms("sgd_some_momentum_buffers")] == ["0" + "-" * 10, "0" * 11, "1" * 11]
    assert steps("adam_second_group")[1:] == [[], []] and steps("sgd_second_group")[1:] == [[], []]
    # the fused step
    for g, head in (("plain", ["wn_adam_flat"]), ("guarded", ["wn_grad_guard", "wn_adam_flat_guarded"])):
        assert steps("fused_" + g) == [head] * 2 and steps("fused_%s_shadow" % g) == [head + ["wn_ema_flat"]] * 2
        assert steps("fused_vq_ema_%s_shadow" % g) == [head + ["wn_vq_ema_update", "wn_ema_flat"]] * 2
        assert [st["t"] for st in forms("fused_" + g)] == [1, 2]


@pytest.mark.parametrize("name", list(lt.OPTIMIZER_CASES))
def test_optimizer_launch_trace_is_the_recorded_one(name, golden_optimizers, monkeypatch):
    want = golden_optimizers["cases"][name]
    trace, packs, forms = lt.record_optimizer(name, monkeypatch)
    if name in ("adam_mixed_steps", "adam_mixed_steps_guarded"):
        # `fresh` of these two cases alone: at the recorded commit FlatAdam left its cache unfinished when the parameters' step
        # counts differ and adopted the moments into new buffers at EVERY such step; its moments now go through _flat_views like
        # the other two optimizers', which adopts them once.  Same values, same views, no launch either way.
        want = dict(want, forms={"steps": [dict(st, fresh=None) for st in want["forms"]["steps"]]})
        forms = {"steps": [dict(st, fresh=None) for st in forms["steps"]]}
    _same(want, trace, packs, forms)


# ---------------------------------------------------------------- the generators
GOLDEN_DECODE = os.path.join(os.path.dirname(GOLDEN), "launch_traces_decode.json")


@pytest.fixture(scope="module")
def golden_decode():
    with open(GOLDEN_DECODE) as f:
        return json.load(f)


def test_the_recorded_decode_cases_hold_the_forms_they_are_there_for(golden_decode):
    """What the fourth file pins (tests/golden/launch_traces_decode.json, tools/record_launch_trace.py --write --set decode at the commit
    it names): everything music_amd/fast_generate.py and ae_generate.py launch between a prompt and the persistent decode kernel, for
    every public way in - and what no pointer's name says (the shapes of note0 / prev0 / rings / tables, the sampling table's bytes,
    the guidance scales) by value, under "forms"."""
    g = golden_decode
    assert len(g["recorded_at"]) == 40 and sorted(g["cases"]) == sorted(lt.DECODE_CASES) and os.path.getsize(GOLDEN_DECODE) < 1 << 20
    entries = lambda name: [i[1] for i in g["cases"][name]["trace"] if i[0] == "call"]
    args = lambda name: [i[3] for i in g["cases"][name]["trace"] if i[0] == "call"][-1]
    values = lambda name: g["cases"][name]["forms"]["values"][-1][2]
    decode = lambda name: [e for e in entries(name) if "decode" in e]
    assert entries("batch")[-3:] == ["wn_gather_grads", "wn_pack_weights", "wn_decode_batch_fw"] and len(g["cases"]["batch"]["trace"]) == 11
    assert len(g["cases"]["guided_batch"]["trace"]) == 24
    for name, entry in (("one", "wn_decode_batch_fw"), ("one_sampled", "wn_decode_batch_samp"), ("one_windows", "wn_win_decode_batch"),
                        ("batch_tables", "wn_decode_batch_samp"), ("batch_windows", "wn_win_decode_batch"), ("batch_bias", "wn_decode_batch_fw"),
                        ("classes_one", "wn_decode_batch_cond"), ("classes_batch", "wn_decode_batch_cond"), ("guided_one", "wn_cfg_decode_batch"),
                        ("guided_batch", "wn_cfg_decode_batch"), ("guided_batch_scalar", "wn_cfg_decode_batch"),
                        ("general_one", "wn_decode_batch_fw"), ("general_batch", "wn_decode_batch_fw"), ("explicit", "wn_decode_batch_cond"),
                        ("explicit_tables", "wn_decode_batch_samp"), ("explicit_guided", "wn_cfg_decode_batch"),
                        ("ae_resynthesize", "wn_decode_batch_cond"), ("ae_decode_codes", "wn_decode_batch_cond")):
        assert decode(name) and set(decode(name)) == {entry}, name
    for name in ("guidance_none_one", "guidance_none_batch"):          # None is the call without the argument
        assert g["cases"][name]["trace"] == g["cases"][name.replace("guidance_none", "classes")]["trace"]
    for name in ("short_one", "short_batch", "short_guided"):          # note_num 0 and 1: two init forwards, no decode launch
        assert not decode(name) and entries(name)
    assert entries("predict_next").count("wn_decode_batch_fw") == 3 and entries("predict_next_general").count("wn_decode_batch_fw") == 3
    assert [entries(n) for n in ("sample_logits", "sample_logits_windows", "sample_logits_guided")] == [
        ["wn_sample_logits"], ["wn_win_sample_logits"], ["wn_cfg_sample_logits"]]
    # one utterance: the cached scratch and no utterance stride; the matrix-core pack, the fp32 kernel's absence of one
    assert args("one")[28] == ["sync", 0] and args("one")[29:31] == [1, 0] and args("batch")[28][0].startswith("tmp") and args("batch")[29:31] == [3, 448]
    assert args("batch")[33][0] == "pack.pk" and args("general_batch")[33] is None and args("general_batch")[:6] == [3, 3, 48, 40, 96, 100]
    # by value: the guidance scales, one per utterance, and the doubled rows; the sampling table only where something is per-utterance
    assert values("guided_batch")["guidance"] == [0.5, 1.0, 2.5] and values("guided_batch_scalar")["guidance"] == [2.0] * 3
    assert values("guided_one")["guidance"] == [2.0] and args("guided_batch")[29] == 6 and args("guided_one")[29] == 2
    hashed = lambda name: [v for v in values(name).values() if isinstance(v, list) and len(v) == 3 and v[1] == "torch.uint8"]
    assert [v[0] for v in hashed("batch_tables")] == [[72]] and [v[0] for v in hashed("guided_batch")] == [[144]] and not hashed("batch_windows")
    assert hashed("guided_batch")[0][2] != hashed("guided_batch_scalar")[0][2]


@pytest.mark.parametrize("name", list(lt.DECODE_CASES))
def test_decode_launch_trace_is_the_recorded_one(name, golden_decode, monkeypatch):
    _same(golden_decode["cases"][name], *lt.record_decode(name, monkeypatch))
