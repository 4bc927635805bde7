"""The class-conditional WaveNet on the device (music_amd.model.wavenet with global_classes / global_channels, wn_gclass_fwd /
wn_gclass_bwd), both plans against the float64 restatement tests/class_cond_ref.py (held to the oracle by
tests/test_class_cond_cpu.py): probabilities within 1e-3, every gradient tensor within 3e-4 of its max-abs - the project's bars - with
the global tail of flat_grad checked on its own, under both objectives and, for one case, under position windows.

    fast a / b / c    filter width 2, Q = 256, dilations 1, 2, 4:  64 / 64 / 256 (the one-launch conditioned blocks), 32 / 32 / 256 (an
                      even batch as clip pairs with tab_pair, an odd one on the 32-channel kernels), 64 / 64 / 256 with biases (the
                      channel-split blocks + wn_cond_grad)
    general a / b     filter width 3 at 48 / 48 / 100, Q = 100;  filter width 2 at Q = 512
T = receptive field + 70; batches of 2 and 3 (two clips share a class, a class is absent); E = 7 and 64.  Run with -m gpu."""
import functools
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_cond_ref as ref
from tests.helpers import nonvacuous

PROB_TOL, GRAD_RTOL = 1e-3, 3e-4
NC = 5
DIL = [1, 2, 4]


def _cfg(k, D, R, S, Q, bias, E):
    return dict(filter_width=k, dilations=DIL, dilation_channels=D, residual_channels=R, skip_channels=S, quantization_channels=Q,
                use_bias=bias, global_classes=NC, global_channels=E)


# name -> (model, batch, plan, what the workspace must say about clip pairs)
CASES = OrderedDict([
    ("fast_a_b3", (_cfg(2, 64, 64, 256, 256, False, 7), 3, "fast", False)),
    ("fast_a_b2", (_cfg(2, 64, 64, 256, 256, False, 64), 2, "fast", False)),
    ("fast_b_b2", (_cfg(2, 32, 32, 256, 256, False, 64), 2, "fast", True)),
    ("fast_b_b3", (_cfg(2, 32, 32, 256, 256, False, 7), 3, "fast", False)),
    ("fast_c_b2", (_cfg(2, 64, 64, 256, 256, True, 7), 2, "fast", False)),
    ("fast_c_b3", (_cfg(2, 32, 32, 256, 256, True, 64), 3, "fast", False)),
    ("general_a_b3", (_cfg(3, 48, 48, 100, 100, True, 64), 3, "general", None)),
    ("general_b_b2", (_cfg(2, 16, 16, 32, 512, False, 7), 2, "general", None)),
])
WINDOWED = "general_a_b3"
WINDOWS = [(0, 50), (50, 100)]


def _classes(B):
    return [4, 1, 4][:B]                     # (B = 3: two clips share a class; classes 0, 2, 3 are absent)


def _is_new(k):
    return "gcond" in k or k.startswith("global_embedding")


def _grads_close(label, got, want):
    """every tensor within GRAD_RTOL of its max-abs (one whose reference is all but zero against 1e-3 of the largest tensor's, the
    rule of tests/test_gpu_cond_learned.py); the global block's tensors also against their OWN max-abs"""
    assert list(got) == list(want)
    gmax = max(float(r.abs().max()) for r in want.values())
    worst = ("", 0.0)
    for k, r in want.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((got[k].detach().cpu().double() - r).abs().max()) / scale
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= GRAD_RTOL, (label, k, e)
    own = {k: float((got[k].detach().cpu().double() - want[k]).abs().max()) / float(want[k].abs().max()) for k in want if _is_new(k)}
    print("  %s: worst gradient %.2e of its max-abs (%s), worst of the global block's %.2e (bar %.0e)"
          % (label, worst[1], worst[0], max(own.values()), GRAD_RTOL))
    assert max(own.values()) <= GRAD_RTOL, (label, own)


def _flat_grads(eng, like):
    g = eng.flat_grad.clone()
    return OrderedDict((n, g[eng.spec.off[n]:eng.spec.off[n] + t.numel()].view(t.shape)) for n, t in like.items())


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, the module surface's results under both objectives and the float64 reference (computed once, never modified)"""
    from music_amd.objective import nll_loss
    cfg, B, plan, _ = CASES[name]
    net = ref.build(cfg, 60 + list(CASES).index(name), scale=2.0)
    with torch.no_grad():
        net.post_process_2.weight.mul_(4.0)
    net = net.cuda()
    Q, k = cfg["quantization_channels"], cfg["filter_width"]
    T = net.receptive_field + 70
    W = T - net.receptive_field + 1
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, Q, (B, T), generator=g)
    x = torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()
    target = torch.randint(0, Q, (B * W,), generator=g).cuda()
    classes = _classes(B)
    params = OrderedDict((n, v.detach().cpu().clone()) for n, v in net.state_dict().items())
    out = dict(net=net, cfg=cfg, B=B, W=W, T=T, x=x, target=target, classes=classes, params=params, grads={}, losses={}, ref={})
    net.zero_grad()
    probs = net(x, classes)
    loss = torch.nn.CrossEntropyLoss()(probs, target)
    loss.backward()
    out["probs"] = probs.detach().clone()
    out["grads"]["reference"] = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    out["losses"]["reference"] = float(loss.detach())
    net.zero_grad()
    loss = nll_loss(net, x, target, classes=classes)
    loss.backward()
    out["grads"]["nll"] = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    out["losses"]["nll"] = float(loss.detach())
    out["eng"] = net._engine_for(x.device)
    out["pair"] = out["eng"].workspace(B, T).get("pair")
    for objective in ("reference", "nll"):
        l64, lg, g64 = ref.loss_and_grads(params, DIL, x.cpu(), target.cpu(), torch.tensor(classes), objective=objective, filter_width=k)
        out["ref"][objective] = dict(l64=float(l64), g64=g64)
        out["logits64"] = lg
    return out


@pytest.mark.parametrize("objective", ["reference", "nll"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_every_gradient_against_float64(name, objective):
    from music_amd.engine import WaveNetEngine
    from music_amd.engine_generic import GenericWaveNetEngine
    c = _case(name)
    cfg, B, plan, pair = CASES[name]
    eng, Q, r = c["eng"], cfg["quantization_channels"], c["ref"][objective]
    assert type(eng) is (WaveNetEngine if plan == "fast" else GenericWaveNetEngine) and eng.gcond
    assert eng.param_names[-5:] == ["gcond_layer_stack.%d.weight" % i for i in range(3)] + ["connection_gcond.weight", "global_embedding.weight"]
    assert eng.spec.off["gcond_layer_stack.0.weight"] == eng.n_gather == eng.spec.total - eng.n_gcond
    if pair is not None:
        assert bool(c["pair"]) == pair
    if objective == "reference":
        p64 = ref.chunk_probs(c["logits64"])
        e_p = float((c["probs"].cpu().double() - p64).abs().max())
        print("  %s: probabilities err %.2e (bar %.0e)" % (name, e_p, PROB_TOL))
        assert c["probs"].shape == (B * c["W"], Q) and e_p <= PROB_TOL
        nonvacuous(p64, "class-conditional, " + name, 6.0 / Q)
    print("  %s %s: loss %.6f (float64 %.6f)" % (name, objective, c["losses"][objective], r["l64"]))
    assert abs(c["losses"][objective] - r["l64"]) < 1e-4 * max(1.0, abs(r["l64"]))
    _grads_close("%s %s" % (name, objective), c["grads"][objective], r["g64"])
    for k, g in c["grads"][objective].items():
        if _is_new(k):
            assert float(g.abs().max()) > 0, k
    # classes nobody has: their embedding rows get exactly nothing
    demb = c["grads"][objective]["global_embedding.weight"]
    assert not demb[[0, 2, 3]].any() and not torch.signbit(demb[[0, 2, 3]]).any()


@pytest.mark.parametrize("name", list(CASES))
def test_the_fused_step_against_float64_twice_the_same_bits(name):
    c = _case(name)
    eng, x, target, classes = c["eng"], c["x"], c["target"], c["classes"]
    for objective in ("reference", "nll"):
        r = c["ref"][objective]
        loss = eng.loss_and_grad(x, target, objective=objective, classes=classes)
        g1 = eng.flat_grad.clone()
        assert abs(float(loss) - r["l64"]) < 1e-4 * max(1.0, abs(r["l64"]))
        _grads_close("%s %s fused" % (name, objective), _flat_grads(eng, c["grads"][objective]), r["g64"])
        # the global tail of flat_grad on its own: against float64, and against what autograd handed out
        tail = g1[eng.n_gather:]
        want = torch.cat([r["g64"][n].reshape(-1) for n in eng.param_names[-5:]])
        assert tail.numel() == want.numel() == eng.n_gcond
        assert float((tail.cpu().double() - want).abs().max()) <= GRAD_RTOL * float(want.abs().max())
        eng.loss_and_grad(x, target, objective=objective, classes=torch.tensor(classes))
        assert torch.equal(g1.view(torch.int32), eng.flat_grad.view(torch.int32)), "two fused steps differ"
    with torch.no_grad():
        a = c["net"](x, classes).clone()
        b = c["net"](x, torch.tensor(classes, device=x.device)).clone()
    assert torch.equal(a, b) and torch.equal(a, c["probs"])
    with pytest.raises(ValueError, match="classes"):
        eng.loss_and_grad(x, target)
    with pytest.raises(ValueError, match="class"):
        eng.loss_and_grad(x, target, classes=[NC] * c["B"])
    with pytest.raises(ValueError, match="class"):
        eng.loss_and_grad(x, target, classes=classes[:1])


@pytest.mark.parametrize("name", ["fast_a_b3", "fast_b_b3", "general_a_b3"])
def test_swapping_two_clips_classes_changes_them_and_nobody_else(name):
    c = _case(name)
    net, x, W = c["net"], c["x"], c["W"]
    with torch.no_grad():
        a = net(x, [4, 1, 4]).clone()
        b = net(x, [1, 4, 4]).clone()
    assert torch.equal(a[2 * W:], b[2 * W:])
    assert not torch.equal(a[:W], b[:W]) and not torch.equal(a[W:2 * W], b[W:2 * W])
    # clip 0 as class 1 is what any clip with that input and class gives: the batch's other clips do not matter
    with torch.no_grad():
        solo = net(x[:1].contiguous(), [1]).clone()
    assert float((solo - b[:W]).abs().max()) <= PROB_TOL


def test_windows_compose_with_the_classes():
    """objective "nll" under position windows, per-clip positions: loss, gradients and the sampled distribution"""
    from music_amd import objective
    c = _case(WINDOWED)
    net, x, B, W, Q = c["net"], c["x"], c["B"], c["W"], c["cfg"]["quantization_channels"]
    pos = [0, 1, 5]
    g = torch.Generator().manual_seed(9)
    target = torch.empty(B, W, dtype=torch.int64)
    for b in range(B):
        for w in range(W):
            lo, hi = WINDOWS[(pos[b] + w) % 2]
            target[b, w] = lo + int(torch.randint(0, hi - lo, (1,), generator=g))
    l64, lg, g64 = ref.loss_and_grads(c["params"], DIL, x.cpu(), target, torch.tensor(c["classes"]), objective="nll",
                                      filter_width=c["cfg"]["filter_width"], windows=WINDOWS, window_pos=pos)
    net.zero_grad()
    loss = objective.nll_loss(net, x, target.cuda(), classes=c["classes"], windows=WINDOWS, window_pos=pos)
    loss.backward()
    assert abs(float(loss.detach()) - float(l64)) < 1e-4 * max(1.0, abs(float(l64)))
    _grads_close("windowed nll", OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters()), g64)
    eng = c["eng"]
    fused = eng.loss_and_grad(x, target.cuda().view(-1), objective="nll", windows=WINDOWS, window_pos=pos, classes=c["classes"])
    assert abs(float(fused) - float(l64)) < 1e-4 * max(1.0, abs(float(l64)))
    _grads_close("windowed nll fused", _flat_grads(eng, g64), g64)
    p = objective.step_probs(net, x, classes=c["classes"], windows=WINDOWS, window_pos=pos)
    p64 = ref.step_probs(lg, WINDOWS, pos)
    assert float((p.cpu().double() - p64).abs().max()) <= PROB_TOL and torch.equal(p.cpu() == 0, p64 == 0)
    s = objective.score(net, x, target.cuda(), classes=c["classes"], windows=WINDOWS, window_pos=pos)
    want = -torch.log(p64.gather(1, target.view(-1, 1))).view(B, W).mean(1)
    assert float(((s["nll"].cpu() - want).abs() / want.abs().clamp(min=1.0)).max()) < 1e-4


def test_one_class_launch_per_pass_and_the_guard_and_ema_cover_the_tail(monkeypatch):
    """wn_gclass_fwd once per forward in front of the stack, wn_gclass_bwd once behind the last table gradient and in front of the
    optimizer; the guarded Adam step with EMA moves the global block and its shadow"""
    import sys
    from music_amd import _lib
    for name in ("fast_a_b2", "fast_b_b2", "general_b_b2"):
        c = _case(name)
        eng = c["eng"]
        seen = []
        real = _lib.call

        def spy(fn, *a):
            seen.append(fn)
            return real(fn, *a)
        for mod in [m for n, m in list(sys.modules.items()) if n.startswith("music_amd") and getattr(m, "call", None) is real]:
            monkeypatch.setattr(mod, "call", spy)
        eng.adam_init(lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
        before = eng.flat.clone()
        eng.loss_and_grad(c["x"], c["target"], classes=c["classes"])
        eng.adam_step()
        assert seen.count("wn_gclass_fwd") == 1 and seen.count("wn_gclass_bwd") == 1, name
        blocks = [i for i, f in enumerate(seen) if f in ("wn_resblock_fwd", "wn_gate_fwd")]
        grads = [i for i, f in enumerate(seen) if f in ("wn_cond_grad", "wn_resblock_bwd_pq_cond_reduce")]
        steps = [i for i, f in enumerate(seen) if f.startswith("wn_grad_guard") or f.startswith("wn_adam_flat")]
        assert seen.index("wn_gclass_fwd") < min(blocks) and max(grads) < seen.index("wn_gclass_bwd") < min(steps), name
        assert "wn_skip_epilogue_fwd" not in seen                       # (the fused forward epilogue takes no conditioning)
        tail = slice(eng.n_gather, eng.spec.total)
        assert not torch.equal(before[tail], eng.flat[tail]) and bool(torch.isfinite(eng.flat).all())
        assert eng.ema is not None
        monkeypatch.undo()
        with torch.no_grad():                                           # (give the cached case its parameters back)
            eng.flat.copy_(before)


def test_mode_off_is_the_parent_engine():
    """with the keys unset nothing of the feature exists in the engine: no tail, no table, the parent's parameter list"""
    from music_amd.model import wavenet
    cfg = {k: v for k, v in CASES["fast_a_b2"][0].items() if not k.startswith("global")}
    torch.manual_seed(1)
    net = wavenet(**cfg).cuda()
    x = c_x = _case("fast_a_b2")["x"]
    with torch.no_grad():
        net(x)
    eng = net._engine
    assert not eng.gcond and eng.n_gcond == 0 and eng.n_gather == eng.spec.total and "C1" not in eng.workspace(2, x.shape[2])
    assert eng.epilogue.fused_fwd_ok and not any("gcond" in n for n in eng.param_names)
    with pytest.raises(ValueError, match="classes must be None"):
        net(c_x, classes=[0, 1])
