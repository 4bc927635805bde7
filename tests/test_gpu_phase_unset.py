"""With "phase_period" unset nothing of the phase-conditioned prior exists: the launch list of a training step is the one recorded at
the parent (tests/golden/launch_traces.json through tests/launch_trace.py, an engine built with phase_period=0 included), and on the
device the state_dict keys, a training step's loss and its flat gradient are bit-equal between a model built without the keyword and
one built with phase_period=0 - on the fast plan (pairs and not), the general plan, and a class-conditional model.  Run with -m gpu."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import launch_trace as lt
from tests.test_launch_trace import _same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")


@pytest.mark.parametrize("name", ["wavenet64", "wavenet32_pair", "wavenet32_odd_batch", "wavenet64_bias"])
def test_the_launch_list_is_the_parents(name):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][name]
    env, build, run = lt.TRACE_CASES[name]
    with pytest.MonkeyPatch.context() as mp:
        trace, packs, forms = lt.record(name, mp)
    _same(want, trace, packs, forms)
    assert not any(item[0] == "call" and "phase" in item[1] for item in trace)
    # ... and the keyword at 0 is the keyword absent
    ch = 32 if "32" in name else 64
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(lt.TRACE_CASES, name, (env, lambda: lt._wn(ch, phase_period=0, **({"use_bias": True} if "bias" in name else {})), run))
        again = lt.record(name, mp)
    assert again[0] == trace and again[1] == packs and again[2] == forms


CASES = {
    "fast64": (dict(filter_width=2, dilations=[1, 2, 4, 1], dilation_channels=64, residual_channels=64, skip_channels=256,
                    quantization_channels=256, use_bias=False), 2, {}),
    "fast32_pair": (dict(filter_width=2, dilations=[1, 2, 4, 1], dilation_channels=32, residual_channels=32, skip_channels=256,
                         quantization_channels=256, use_bias=False), 2, {}),
    "general": (dict(filter_width=3, dilations=[1, 2, 4, 1], dilation_channels=24, residual_channels=20, skip_channels=36,
                     quantization_channels=40, use_bias=True), 3, {}),
    "classes": (dict(filter_width=2, dilations=[1, 2, 4, 1], dilation_channels=64, residual_channels=64, skip_channels=256,
                     quantization_channels=256, use_bias=False, global_classes=3, global_channels=5), 2, {"classes": [2, 0]}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_dict_loss_and_flat_gradient_are_bit_equal_to_a_model_without_the_keyword(name):
    from music_amd.model import wavenet
    cfg, B, kw = CASES[name]
    out = []
    for extra in ({}, {"phase_period": 0}):
        torch.manual_seed(4)
        net = wavenet(**cfg, **extra).cuda()
        Q, T = cfg["quantization_channels"], net.receptive_field + 120
        g = torch.Generator().manual_seed(1)
        x = torch.nn.functional.one_hot(torch.randint(0, Q, (B, T), generator=g), Q).permute(0, 2, 1).float().contiguous().cuda()
        target = torch.randint(0, Q, (B * (T - net.receptive_field + 1),), generator=g).cuda()
        with torch.no_grad():
            probs = net(x, **kw).clone()
        eng = net._engine
        losses = [eng.loss_and_grad(x, target, objective=o, **kw).clone() for o in ("reference", "nll")]
        out.append((list(net.state_dict()), [n for n, _ in net.named_parameters()], probs, losses, eng.flat_grad.clone(), eng.flat.clone(),
                    eng.spec.total, eng.n_gather, sorted(k for k in eng._ws.peek(B, T) if k != "bwd")))
        assert eng.phase == 0 and eng.n_phase == 0 and not hasattr(eng, "phase_rot") and not any("phase" in n for n in eng.param_names)
        with pytest.raises(ValueError, match="phase_pos must be None"):
            net(x, phase_pos=[0] * B, **kw)
    a, b = out
    assert a[0] == b[0] and a[1] == b[1] and a[6:] == b[6:]
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a[3], b[3]))
    assert torch.equal(a[4].view(torch.int32), b[4].view(torch.int32)) and torch.equal(a[5], b[5])
