"""The phase-conditioned WaveNet on the device (music_amd.model.wavenet with phase_period, wn_phase_tab_fwd / wn_phase_tab_bwd), both
plans against the float64 restatement tests/phase_ref.py: probabilities within 1e-3, every gradient tensor within 3e-4 of its max-abs
- the bars tests/test_gpu_class_cond_model.py applies to the class tables - with the phase tail of flat_grad checked on its own, under
both objectives.

    fast a        filter width 2, Q = 256, 64 / 64 / 256, dilations 1, 2, 4, 1, P = 4: batch 2 and 3 (the one-launch conditioned blocks,
                  the table on the matrix cores), batch 2 with classes
    fast b        32 / 32 / 256: batch 2 as clip pairs (tab_pair), batch 3 on the 32-channel kernels, batch 2 with classes
    general       filter width 3, Q = 40, 24 / 20 / 36, P = 3, batch 2, and the same with classes
T = 200 (fast), receptive field + 60 (general); positions 5, 10^10 + 3 (beyond int32) and 2.  Run with -m gpu."""
import functools
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import class_cond_ref as cref
from tests import phase_ref as ref
from tests.helpers import nonvacuous

PROB_TOL, GRAD_RTOL = 1e-3, 3e-4
NC = 5
DIL = [1, 2, 4, 1]
POS = [5, 10 ** 10 + 3, 2]


def _cfg(k, D, R, S, Q, P, E=0):
    cfg = dict(filter_width=k, dilations=DIL, dilation_channels=D, residual_channels=R, skip_channels=S, quantization_channels=Q,
               use_bias=False, phase_period=P)
    if E:
        cfg.update(global_classes=NC, global_channels=E)
    return cfg


# name -> (model, batch, plan, what the workspace must say about clip pairs)
CASES = OrderedDict([
    ("fast_a_b2", (_cfg(2, 64, 64, 256, 256, 4), 2, "fast", False)),
    ("fast_a_b3", (_cfg(2, 64, 64, 256, 256, 4), 3, "fast", False)),
    ("fast_b_b2", (_cfg(2, 32, 32, 256, 256, 4), 2, "fast", True)),
    ("fast_b_b3", (_cfg(2, 32, 32, 256, 256, 4), 3, "fast", False)),
    ("general_b2", (_cfg(3, 24, 20, 36, 40, 3), 2, "general", None)),
    ("fast_a_cls_b2", (_cfg(2, 64, 64, 256, 256, 4, 7), 2, "fast", False)),
    ("fast_b_cls_b2", (_cfg(2, 32, 32, 256, 256, 4, 7), 2, "fast", True)),
    ("general_cls_b2", (_cfg(3, 24, 20, 36, 40, 3, 7), 2, "general", None)),
])


def _is_new(k):
    return k.startswith("phase_layer_stack") or k == "connection_phase"


def _grads_close(label, got, want):
    """every tensor within GRAD_RTOL of its max-abs (one whose reference is all but zero against 1e-3 of the largest tensor's, the
    rule of tests/test_gpu_class_cond_model.py); the phase tables also against their OWN max-abs"""
    assert list(got) == list(want)
    gmax = max(float(r.abs().max()) for r in want.values())
    worst = ("", 0.0)
    for k, r in want.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((got[k].detach().cpu().double() - r).abs().max()) / scale
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= GRAD_RTOL, (label, k, e)
    own = {k: float((got[k].detach().cpu().double() - want[k]).abs().max()) / float(want[k].abs().max()) for k in want if _is_new(k)}
    print("  %s: worst gradient %.2e of its max-abs (%s), worst of the phase tables' %.2e (bar %.0e)"
          % (label, worst[1], worst[0], max(own.values()), GRAD_RTOL))
    assert max(own.values()) <= GRAD_RTOL, (label, own)


def _flat_grads(eng, like):
    g = eng.flat_grad.clone()
    return OrderedDict((n, g[eng.spec.off[n]:eng.spec.off[n] + t.numel()].view(t.shape)) for n, t in like.items())


def _kw(c, pos=None):
    kw = {"phase_pos": c["pos"] if pos is None else pos}
    if c["classes"] is not None:
        kw["classes"] = c["classes"]
    return kw


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, the module surface's results under both objectives and the float64 reference (computed once, never modified)"""
    from music_amd.objective import nll_loss
    cfg, B, plan, _ = CASES[name]
    net = cref.build(cfg, 80 + list(CASES).index(name), scale=2.0)
    with torch.no_grad():
        net.post_process_2.weight.mul_(4.0)
    net = net.cuda()
    Q, k = cfg["quantization_channels"], cfg["filter_width"]
    T = 200 if plan == "fast" else net.receptive_field + 60
    W = T - net.receptive_field + 1
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, Q, (B, T), generator=g)
    x = torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()
    target = torch.randint(0, Q, (B * W,), generator=g).cuda()
    named = OrderedDict(net.named_parameters())
    params = OrderedDict((n, v.detach().cpu().clone()) for n, v in named.items())
    out = dict(net=net, cfg=cfg, B=B, W=W, T=T, x=x, target=target, pos=POS[:B], params=params, grads={}, losses={}, ref={},
               classes=[4, 1, 4][:B] if cfg.get("global_classes") else None)
    kw = _kw(out)
    net.zero_grad()
    probs = net(x, **kw)
    loss = torch.nn.CrossEntropyLoss()(probs, target)
    loss.backward()
    out["probs"] = probs.detach().clone()
    out["grads"]["reference"] = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    out["losses"]["reference"] = float(loss.detach())
    net.zero_grad()
    loss = nll_loss(net, x, target, **kw)
    loss.backward()
    out["grads"]["nll"] = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    out["losses"]["nll"] = float(loss.detach())
    out["eng"] = net._engine_for(x.device)
    out["pair"] = out["eng"].workspace(B, T).get("pair")
    cls64 = torch.tensor(out["classes"]) if out["classes"] is not None else None
    for objective in ("reference", "nll"):
        l64, lg, g64 = ref.loss_and_grads(params, DIL, x.cpu(), target.cpu(), out["pos"], cls64, objective=objective, filter_width=k)
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
    eng, Q, r, N = c["eng"], cfg["quantization_channels"], c["ref"][objective], len(DIL)
    assert type(eng) is (WaveNetEngine if plan == "fast" else GenericWaveNetEngine) and eng.phase == cfg["phase_period"]
    assert eng.param_names[-N - 1:] == ["phase_layer_stack.%d" % i for i in range(N)] + ["connection_phase"]
    assert eng.spec.off["phase_layer_stack.0"] == eng.spec.total - eng.n_phase == eng.n_gather + eng.n_gcond
    assert eng.spec.shape["phase_layer_stack.0"] == (2 * cfg["dilation_channels"], cfg["phase_period"])
    assert eng.spec.shape["connection_phase"] == (cfg["skip_channels"], cfg["phase_period"])
    if pair is not None:
        assert bool(c["pair"]) == pair
    if objective == "reference":
        p64 = cref.chunk_probs(c["logits64"])
        e_p = float((c["probs"].cpu().double() - p64).abs().max())
        print("  %s: probabilities err %.2e (bar %.0e)" % (name, e_p, PROB_TOL))
        assert c["probs"].shape == (B * c["W"], Q) and e_p <= PROB_TOL
        nonvacuous(p64, "phase-conditioned, " + name, 6.0 / Q)
    print("  %s %s: loss %.6f (float64 %.6f)" % (name, objective, c["losses"][objective], r["l64"]))
    assert abs(c["losses"][objective] - r["l64"]) < 1e-4 * max(1.0, abs(r["l64"]))
    _grads_close("%s %s" % (name, objective), c["grads"][objective], r["g64"])
    for k, g in c["grads"][objective].items():
        if _is_new(k) or "gcond" in k:
            assert float(g.abs().max()) > 0, k


@pytest.mark.parametrize("name", list(CASES))
def test_the_fused_step_and_the_per_timestep_probabilities_against_float64(name):
    from music_amd import objective as wobj
    c = _case(name)
    eng, x, target, N = c["eng"], c["x"], c["target"], len(DIL)
    for objective in ("reference", "nll"):
        r = c["ref"][objective]
        loss = eng.loss_and_grad(x, target, objective=objective, **_kw(c))
        g1 = eng.flat_grad.clone()
        assert abs(float(loss) - r["l64"]) < 1e-4 * max(1.0, abs(r["l64"]))
        _grads_close("%s %s fused" % (name, objective), _flat_grads(eng, c["grads"][objective]), r["g64"])
        # the phase tail of flat_grad on its own: against float64
        tail = g1[eng.spec.total - eng.n_phase:]
        want = torch.cat([r["g64"][n].reshape(-1) for n in eng.param_names[-N - 1:]])
        assert tail.numel() == want.numel() == eng.n_phase
        assert float((tail.cpu().double() - want).abs().max()) <= GRAD_RTOL * float(want.abs().max())
        eng.loss_and_grad(x, target, objective=objective, **_kw(c, torch.tensor(c["pos"], device=x.device)))
        assert torch.equal(g1.view(torch.int32), eng.flat_grad.view(torch.int32)), "two fused steps differ"
    p = wobj.step_probs(c["net"], x, **_kw(c))
    p64 = cref.step_probs(c["logits64"])
    assert float((p.cpu().double() - p64).abs().max()) <= PROB_TOL
    s = wobj.score(c["net"], x, target, **_kw(c))
    want = -torch.log(p64.gather(1, target.cpu().view(-1, 1))).view(c["B"], c["W"]).mean(1)
    assert float(((s["nll"].cpu() - want).abs() / want.abs().clamp(min=1.0)).max()) < 1e-4


@pytest.mark.parametrize("name", ["fast_a_b2", "fast_b_b2", "fast_b_b3", "general_b2", "fast_a_cls_b2"])
def test_a_shift_by_the_period_is_the_same_bits_a_shift_by_one_is_not(name):
    c = _case(name)
    net, x, P, W = c["net"], c["x"], c["cfg"]["phase_period"], c["W"]
    with torch.no_grad():
        a = net(x, **_kw(c)).clone()
        b = net(x, **_kw(c, [p + P for p in c["pos"]])).clone()
        d = net(x, **_kw(c, torch.tensor([p + 7 * P for p in c["pos"]], device=x.device))).clone()
        one = net(x, **_kw(c, [c["pos"][0] + 1] + c["pos"][1:])).clone()
    assert torch.equal(a, c["probs"]) and torch.equal(a, b) and torch.equal(a, d)
    assert not torch.equal(a[:W], one[:W])
    # the per-timestep probabilities: the other clips are untouched
    from music_amd.objective import step_probs
    sa, so = step_probs(net, x, **_kw(c)), step_probs(net, x, **_kw(c, [c["pos"][0] + 1] + c["pos"][1:]))
    assert torch.equal(sa[W:], so[W:]) and not torch.equal(sa[:W], so[:W])
    # one int serves every clip
    with torch.no_grad():
        e = net(x, **_kw(c, 6)).clone()
        f = net(x, **_kw(c, [6] * c["B"])).clone()
    assert torch.equal(e, f)


def test_phase_pos_is_required_with_the_mode_on_and_refused_negative_or_with_the_mode_off():
    from music_amd.model import wavenet
    from music_amd import objective as wobj
    c = _case("fast_a_b2")
    net, x, target, eng = c["net"], c["x"], c["target"], c["eng"]
    with pytest.raises(ValueError, match="phase_pos"):
        net(x)
    with pytest.raises(ValueError, match="negative"):
        net(x, phase_pos=[3, -1])
    with pytest.raises(ValueError, match="phase_pos"):
        eng.loss_and_grad(x, target)
    with pytest.raises(ValueError, match="negative"):
        eng.loss_and_grad(x, target, phase_pos=[-2, 0])
    with pytest.raises(ValueError, match="one per clip"):
        eng.loss_and_grad(x, target, phase_pos=[1, 2, 3])
    with pytest.raises(ValueError, match="phase_pos"):
        wobj.nll_loss(net, x, target)
    with pytest.raises(ValueError, match="negative"):
        wobj.step_probs(net, x, phase_pos=-4)
    cfg = {k: v for k, v in c["cfg"].items() if k != "phase_period"}
    torch.manual_seed(1)
    plain = wavenet(**cfg).cuda()
    with pytest.raises(ValueError, match="phase_pos must be None"):
        plain(x, phase_pos=[0, 1])
    with torch.no_grad():
        plain(x)
    with pytest.raises(ValueError, match="takes no phase_pos"):
        plain._engine.loss_and_grad(x, target, phase_pos=[0, 1])


def test_one_table_launch_per_pass_and_the_guard_and_ema_cover_the_tail(monkeypatch):
    """wn_phase_tab_fwd once per forward in front of the stack (behind wn_gclass_fwd where there are classes), wn_phase_tab_bwd once
    behind the last table gradient and in front of wn_gclass_bwd and the optimizer; the guarded Adam step with EMA moves the tables"""
    import sys
    from music_amd import _lib
    for name in ("fast_a_b2", "fast_b_cls_b2", "general_cls_b2"):
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
        eng.loss_and_grad(c["x"], c["target"], **_kw(c))
        eng.adam_step()
        cls = int(c["classes"] is not None)
        assert seen.count("wn_phase_tab_fwd") == 1 and seen.count("wn_phase_tab_bwd") == 1, name
        assert seen.count("wn_gclass_fwd") == cls and seen.count("wn_gclass_bwd") == cls, name
        blocks = [i for i, f in enumerate(seen) if f in ("wn_resblock_fwd", "wn_gate_fwd")]
        grads = [i for i, f in enumerate(seen) if f in ("wn_cond_grad", "wn_resblock_bwd_pq_cond_reduce")]
        steps = [i for i, f in enumerate(seen) if f.startswith("wn_grad_guard") or f.startswith("wn_adam_flat")]
        assert seen.index("wn_phase_tab_fwd") < min(blocks) and max(grads) < seen.index("wn_phase_tab_bwd") < min(steps), name
        if cls:
            assert seen.index("wn_gclass_fwd") < seen.index("wn_phase_tab_fwd")
            assert seen.index("wn_phase_tab_bwd") < seen.index("wn_gclass_bwd") < min(steps)
        tail = slice(eng.spec.total - eng.n_phase, eng.spec.total)
        assert not torch.equal(before[tail], eng.flat[tail]) and bool(torch.isfinite(eng.flat).all())
        assert eng.ema is not None
        monkeypatch.undo()
        with torch.no_grad():                                           # (give the cached case its parameters back)
            eng.flat.copy_(before)
