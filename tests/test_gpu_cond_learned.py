"""`conditioning="learned"` on the device (music_amd/model1.py, music_amd/ae_generic.py, wn_cond_proj_fwd / wn_cond_proj_bwd): the whole
model against oracle.autoencoder_forward in float64, whose `cond` argument is the model's learned parameters with requires_grad -
autograd yields their gradients too.  Bars are the project's: probabilities within 1e-3, every gradient (the new tensors included)
within 3e-4 of its tensor's max-abs, the float64 pass taking the device's sign at ReLU pre-activations within the tolerance band
(tests/test_gpu_fullsize._device_relu).  Then the surfaces on top: autograd against the fused step, the NLL objective, determinism,
the guarded Adam step with EMA and its checkpoints, resynthesis.  Run with -m gpu."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo
from tests.ema_ref import Ref64, kernel_w
from tests.helpers import nonvacuous
from tests.test_gpu_fullsize import _device_relu

PROB_TOL = 1e-3
GRAD_RTOL = 3e-4
DIL = [1, 2, 4, 8]
W = 320          # output samples: with pool 40 (8 frames) blocks 0, 1 tile and blocks 2, 3 and the epilogue stretch (_conditon)

# name -> (constructor arguments, batch)
CASES = {
    "fast64": (dict(en=(64, 64), de=(64, 64, 256), bw=16, pool=40, bias=False), 2),
    "fast64_bias": (dict(en=(60, 52), de=(64, 60, 72), bw=10, pool=40, bias=True), 2),
    "pair32": (dict(en=(32, 32), de=(32, 32, 256), bw=16, pool=40, bias=False), 2),
    "odd32": (dict(en=(32, 32), de=(32, 32, 64), bw=16, pool=40, bias=False), 3),
    "long_encoding": (dict(en=(64, 64), de=(64, 64, 256), bw=16, pool=8, bias=False), 2),        # 40 frames: the gathered form
    "general": (dict(en=(72, 96), de=(96, 80, 112), bw=48, pool=40, bias=True, fw=3, q=64), 2),
}


def _cfg(en, de, bw, pool, bias, fw=2, q=256, conditioning="learned"):
    return dict(filter_width=fw, quantization_channel=q, dilations=DIL, en_residual_channel=en[0], en_dilation_channel=en[1],
                en_bottleneck_width=bw, en_pool_kernel_size=pool, de_residual_channel=de[0], de_dilation_channel=de[1],
                de_skip_channel=de[2], use_bias=bias, conditioning=conditioning)


def _build(name, conditioning="learned", seed=40):
    from music_amd.model1 import wavenet_autoencoder
    kw, B = CASES[name]
    cfg = _cfg(conditioning=conditioning, **kw)
    torch.manual_seed(seed + sorted(CASES).index(name))
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
    return net.cuda(), cfg, B


def _batch(net, cfg, B, seed=9):
    rng = np.random.default_rng(seed)
    Q, T = cfg["quantization_channel"], net.receptive_field + W - 1
    codes = torch.from_numpy(rng.integers(0, Q, size=(B, T)))
    x = F.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()
    target = torch.from_numpy(rng.integers(0, Q, size=(B * W,)).astype(np.int64)).cuda()
    return x, target


def _dev_pre(eng, B, T):
    """the device's pre-ReLU tensors in the oracle's shapes and names (autoencoder_encode / _decode), of either engine"""
    from music_amd.engine_base import SLACK
    ws = eng.workspace(B, T)
    pitch, lo, N = ws["pitch"], eng.rf - 1, eng.N
    cx, ch = (eng.CHe, eng.CHe) if hasattr(eng, "CHe") else (eng.ReP, eng.DeP)
    xe = ws["Xe"][SLACK:SLACK + (N + 1) * B * cx * pitch].view(N + 1, B, cx, pitch)
    he = ws["He"][SLACK:SLACK + N * B * ch * pitch].view(N, B, ch, pitch)
    pre = {}
    for i in range(N):
        pre["en_x%d" % i] = xe[i][:, :eng.Re, eng.off[i]:T].cpu().double()
        pre["en_h%d" % i] = he[i][:, :eng.De, eng.off[i + 1]:T].cpu().double()
    v = lambda buf: buf[SLACK:SLACK + B * eng.SP * pitch].view(B, eng.SP, pitch)[:, :eng.Sd, lo:T].cpu().double()
    pre["de_skip"], pre["de_conn"] = v(ws["U"]), v(ws["R1"])
    return pre


def _oracle64(net, cfg, x, relu, logits=False):
    """float64 forward of the oracle on the model's parameters as leaves; cond = the learned projections AMONG those leaves"""
    leaf = OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())
    N = len(DIL)
    cond = [(leaf["de_cond_layer_stack.%d.weight" % i], leaf["de_cond_layer_stack.%d.bias" % i]) for i in range(N)]
    cond.append((leaf["connection_cond.weight"], leaf["connection_cond.bias"]))
    keep = wo.chunk_softmax
    if logits:                      # with that one function as the identity the oracle's decoder returns the pre-softmax logits
        wo.chunk_softmax = lambda total, q: total
    try:
        out, enc = wo.autoencoder_forward(leaf, DIL, x.double().cpu(), cfg["en_pool_kernel_size"], cond, filter_width=cfg["filter_width"],
                                          q=cfg["quantization_channel"], relu=relu)
    finally:
        wo.chunk_softmax = keep
    return leaf, out, enc


def _grads_close(label, got, ref):
    """every tensor within GRAD_RTOL of its max-abs; a tensor whose reference is (all but) zero - a bias under the chunk softmax,
    which a constant per channel leaves unchanged - is measured against 1e-3 of the largest tensor's max-abs instead, the rule of
    tests/test_gpu_generic.py"""
    worst = ("", 0.0)
    assert list(got) == list(ref)
    gmax = max(float(r.abs().max()) for r in ref.values())
    for k, r in ref.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((got[k].detach().cpu().double() - r).abs().max()) / scale
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= GRAD_RTOL, (label, k, e)
    # ... and the projections' own gradients against their OWN max-abs, whatever the other tensors' sizes
    new = max(float((got[k].detach().cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if "cond" in k)
    assert new <= GRAD_RTOL, (label, new)
    print("  %s: worst gradient %.2e of its max-abs (%s), worst of the projections' %.2e (bar %.0e)" % (label, worst[1], worst[0], new, GRAD_RTOL))


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, module-surface results and the float64 reference of one case (computed once, never modified)"""
    net, cfg, B = _build(name)
    x, target = _batch(net, cfg, B)
    T = x.shape[2]
    net.zero_grad()
    probs = net(x)
    loss = torch.nn.CrossEntropyLoss()(probs, target)
    loss.backward()
    eng = net._engine_for(x.device)
    relu, stats = _device_relu(_dev_pre(eng, B, T))
    leaf, p64, enc64 = _oracle64(net, cfg, x, relu)
    l64 = F.cross_entropy(p64, target.cpu())
    g64 = OrderedDict((k, torch.zeros_like(v) if g is None else g)
                      for (k, v), g in zip(leaf.items(), torch.autograd.grad(l64, list(leaf.values()), allow_unused=True)))
    print("  %s: ReLU pre-activations inside the tolerance band: %d, of which the device's sign differs: %d" % (name, stats["near"], stats["flips"]))
    grads = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    return dict(net=net, cfg=cfg, B=B, x=x, target=target, probs=probs.detach().clone(), loss=float(loss.detach()), grads=grads, eng=eng,
                p64=p64.detach(), l64=float(l64), g64=g64, enc64=enc64.detach())


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_every_gradient_against_float64(name):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    c = _case(name)
    eng, B, T, Q = c["eng"], c["B"], c["x"].shape[2], c["cfg"]["quantization_channel"]
    assert type(eng) is (GenericAutoencoderEngine if name == "general" else _AutoencoderEngine) and eng.learned
    ws = eng.workspace(B, T)
    Le = W // c["cfg"]["en_pool_kernel_size"]
    stretch = [(T - eng.off[i + 1]) % Le == 0 for i in range(eng.N)]
    assert any(stretch) and not all(stretch)                                      # both branches of _conditon
    if name != "general":
        assert bool(ws["pair"]) == (name == "pair32") and ("cidx" in ws) == (name != "long_encoding" and name != "odd32")
        bw = ws["bwd"]
        assert bw["pq"] == (name in ("fast64", "pair32")) and (name != "fast64_bias" or bw["ms"]) and (name != "odd32" or not bw["ms"])
    e_enc = float((c["net"].last_encoding.cpu().double() - c["enc64"]).abs().max())
    e_p = float((c["probs"].cpu().double() - c["p64"]).abs().max())
    print("  %s: encoding err %.2e, probabilities err %.2e (bar %.0e), loss %.6f (float64 %.6f)" % (name, e_enc, e_p, PROB_TOL, c["loss"], c["l64"]))
    assert c["probs"].shape == (B * W, Q) and e_enc < 1e-4 and e_p <= PROB_TOL
    nonvacuous(c["p64"], "learned conditioning, " + name, 6.0 / Q)
    assert abs(c["loss"] - c["l64"]) < 1e-4
    _grads_close(name, c["grads"], c["g64"])
    for k, g in c["grads"].items():
        if "cond" in k:
            assert float(g.abs().max()) > 0, k                                    # the projections do get a gradient


@pytest.mark.parametrize("name", ["fast64", "pair32", "general"])
def test_autograd_gives_the_fused_steps_gradients(name):
    """engine.loss_and_grad on the input of the module-surface pass: float64's loss and gradients within the bars, bit-reproducible,
    and on the fast engine - where loss.backward() runs the same forward, fused softmax + CrossEntropyLoss kernel and backward - the
    same BITS in the new tensors as autograd's .grad (the general plan's module surface takes torch's loss kernels)."""
    c = _case(name)
    eng = c["eng"]
    loss = eng.loss_and_grad(c["x"], c["target"])
    g1 = eng.flat_grad.clone()
    assert abs(float(loss) - c["l64"]) < 1e-4
    fused = OrderedDict((n, g1[eng.spec.off[n]:eng.spec.off[n] + g.numel()].view(g.shape)) for n, g in c["grads"].items())
    _grads_close(name + " fused", fused, c["g64"])
    for n, g in c["grads"].items():
        if "cond" in n:
            d = float((fused[n] - g).abs().max())
            print("  %s: fused against autograd, %s: largest difference %.2e" % (name, n, d))
            if name == "general":               # two loss kernels: each side is within GRAD_RTOL of float64, so of each other within twice that
                assert d <= 2 * GRAD_RTOL * float(c["g64"][n].abs().max()), (n, d)
            else:
                assert torch.equal(fused[n], g), (n, d)
    eng.loss_and_grad(c["x"], c["target"], None)
    assert torch.equal(g1, eng.flat_grad)
    with pytest.raises(ValueError, match="learned"):
        eng.loss_and_grad(c["x"], c["target"], c["net"].conditioning_projections())


def test_nll_objective_against_float64():
    c = _case("fast64")
    net, eng, x, target, B = c["net"], c["eng"], c["x"], c["target"], c["B"]
    loss = eng.loss_and_grad(x, target, objective="nll")
    grads = OrderedDict()
    for n in eng.param_names:
        o, shp = eng.spec.off[n], eng.spec.shape[n]
        grads[n] = eng.flat_grad[o:o + int(np.prod(shp))].view(shp).clone()
    relu, _ = _device_relu(_dev_pre(eng, B, x.shape[2]))
    leaf, logits, _ = _oracle64(net, c["cfg"], x, relu, logits=True)
    assert tuple(logits.shape) == (B, 256, W)
    l64 = F.cross_entropy(logits.permute(0, 2, 1).reshape(-1, 256), target.cpu())
    g64 = OrderedDict((k, torch.zeros_like(v) if g is None else g)
                      for (k, v), g in zip(leaf.items(), torch.autograd.grad(l64, list(leaf.values()), allow_unused=True)))
    print("  nll: loss %.6f, float64 %.6f" % (float(loss), float(l64)))
    assert abs(float(loss) - float(l64)) < 1e-4
    _grads_close("nll", grads, g64)


def test_learned_forwards_are_deterministic_and_random_ones_are_not():
    c = _case("fast64")
    net, x = c["net"], c["x"]
    with torch.no_grad():
        a = net(x).clone()
        b = net(x).clone()
    assert torch.equal(a, b) and torch.equal(a, c["probs"])
    rnd, _, _ = _build("fast64", conditioning="random")
    with torch.no_grad():
        a = rnd(x).clone()
        b = rnd(x).clone()
    assert not torch.equal(a, b)
    with pytest.raises(ValueError, match="random"):
        rnd._engine_for(x.device).forward(x)


def test_three_guarded_adam_steps_with_ema_and_their_checkpoints(tmp_path):
    from music_amd import ema
    from music_amd.ae_train import load_model, save_model
    from music_amd.model1 import wavenet_autoencoder
    net, cfg, B = _build("fast64_bias", seed=60)
    x, target = _batch(net, cfg, B, seed=61)
    eng = net._engine_for(x.device)
    decay = 0.9
    eng.adam_init(lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=decay, ema_warmup=True)
    cond_names = [n for n in eng.param_names if "cond" in n]
    assert len(cond_names) == 2 * (len(DIL) + 1)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    ref = Ref64(eng.flat.cpu().numpy())
    for step in range(1, 4):
        eng.loss_and_grad(x, target)
        eng.adam_step()
        ref.step(eng.flat.cpu().numpy(), kernel_w(decay, True, step))
    rep = eng.guard_report()
    assert rep["taken"] == 3 and rep["skipped"] == 0
    for n, p in net.named_parameters():
        if n in cond_names:
            # every projection parameter has moved: the tensor, and each element the last step had a gradient for (a channel whose
            # ReLU behind connection_1 never opens gets exactly none)
            o = eng.spec.off[n]
            had_grad = eng.flat_grad[o:o + p.numel()].view(p.shape) != 0
            moved = p != start[n]
            assert bool(torch.isfinite(p).all()) and bool(moved.any()) and bool(moved[had_grad].all()), n
            print("  %s: %d of %d elements moved" % (n, int(moved.sum()), p.numel()))
    ratio = ref.check(eng.ema.flat.cpu().numpy(), "shadow after three steps")
    print("  shadow against the float64 lerp: largest error / bound %.3f" % ratio)
    # .model / .ema round trip: a fresh learned model restored from either file reproduces the probabilities bit for bit
    path = str(tmp_path) + "/"
    save_model(net, 3, path)
    ema.save_shadow(eng.ema, path + "wavenet_autoencoder3.ema")
    with torch.no_grad():
        p_model = net(x).clone()
        with eng.ema.swapped(net):
            p_ema = net(x).clone()
        assert torch.equal(net(x), p_model)
    assert not torch.equal(p_model, p_ema)
    for name, want in (("wavenet_autoencoder3.model", p_model), ("wavenet_autoencoder3.ema", p_ema)):
        twin = load_model(wavenet_autoencoder(**cfg), path, name).cuda()
        with torch.no_grad():
            assert torch.equal(twin(x), want), name
    with pytest.raises(RuntimeError, match="conditioning"):
        load_model(wavenet_autoencoder(**dict(cfg, conditioning="random")), path, "wavenet_autoencoder3.ema")


def test_resynthesis_of_a_learned_model_is_a_function_of_the_checkpoint():
    from music_amd.ae_generate import resynthesize
    c = _case("fast64")
    net, x, B = c["net"], c["x"], c["B"]
    codes, probs, enc = resynthesize(net, x, teacher_forced=True, want_probs=True)
    # a decode step's probabilities are the softmax over the Q channels of ONE output column: the forward's logits under that
    # softmax, on the device (step_probs) and in float64 (the oracle's pre-softmax, the device's near-zero ReLU signs)
    eng = c["eng"]
    with torch.no_grad():
        _, _, ws = eng.forward(x, want_probs=False)
        p_dev = eng.step_probs(ws).view(B, W, 256)
    relu, _ = _device_relu(_dev_pre(eng, B, x.shape[2]))
    _, logits, _ = _oracle64(net, c["cfg"], x, relu, logits=True)
    p64 = torch.softmax(logits.detach(), 1).transpose(1, 2)
    e_dev, e64 = float((probs - p_dev).abs().max()), float((probs.cpu().double() - p64).abs().max())
    print("  resynthesis against the forward: probabilities err %.2e (device), %.2e (float64; bar %.0e), largest probability %.3f"
          % (e_dev, e64, PROB_TOL, float(p64.max())))
    assert tuple(probs.shape) == (B, W, 256) and e_dev <= PROB_TOL and e64 <= PROB_TOL
    again, _, _ = resynthesize(net, x, teacher_forced=True)
    assert torch.equal(codes, again)
    free_a, _, _ = resynthesize(net, x)
    free_b, _, _ = resynthesize(net, x)
    assert torch.equal(free_a, free_b)
    with pytest.raises(ValueError, match="learned"):
        resynthesize(net, x, cond=net.conditioning_projections())
