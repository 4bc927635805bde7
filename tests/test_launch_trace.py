"""CPU check that a host-side change leaves what the fast engines LAUNCH alone: every launch of a step of music_amd/engine.py
and music_amd/model1.py - entry point, argument values, stream, position in the order - every event recorded or waited on and
every timing mark, compared with the trace recorded at the commit named in tests/golden/launch_traces.json (written once by
tools/record_launch_trace.py --write, never regenerated), and the index maps _build_packs produces compared by hash.

The recording itself (what is stubbed, how pointers are named) is tests/launch_trace.py.  No device is touched."""
import json
import os

import pytest

from tests import launch_trace as lt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


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
