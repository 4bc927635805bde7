"""Global class conditioning on the device (global_classes / global_channels of music_amd.wavenet_autoencoder, both engines,
wn_gcond_proj_fwd / wn_gcond_proj_bwd): the whole model against the UNCHANGED float64 oracle, the cases and bars of
tests/test_gpu_cond_learned.py (probabilities within 1e-3, every gradient within 3e-4 of its tensor's max-abs) with E = 12 channels
and n = 3 classes.

The oracle knows no classes.  It is called once per clip, in logits mode, with that clip's EFFECTIVE biases
b_i + G_i emb[cls[b]] built from float64 leaves (so autograd reaches G and the embedding), the device's ReLU signs sliced per
clip; the clips' logits are concatenated in batch order and the objective - the reference's chunk softmax + CrossEntropyLoss, or the
true NLL - is put on top in float64.  Then the surfaces: the fused step against autograd, determinism, one class for all clips
against a learned model with the term folded into its biases, the guarded Adam step with EMA and its checkpoints, class-aware
resynthesis and decode_codes.  Run with -m gpu."""
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
from tests.test_gpu_cond_learned import CASES, DIL, GRAD_RTOL, PROB_TOL, W, _batch, _cfg, _dev_pre
from tests.test_gpu_fullsize import _device_relu

E, NC = 12, 3
N = len(DIL)


def _classes(B):
    return [2, 0, 2][:B]                     # (B = 3: two clips share a class; class 1 is absent everywhere)


def _is_new(k):
    return "gcond" in k or k.startswith("global_embedding")


def _build(name, seed=40, **extra):
    from music_amd.model1 import wavenet_autoencoder
    kw, B = CASES[name]
    cfg = dict(_cfg(**kw), global_classes=NC, global_channels=E, **extra)
    torch.manual_seed(seed + sorted(CASES).index(name))
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
    return net.cuda(), cfg, B


def _logits64(net, cfg, x, classes, dev_pre):
    """(leaves, float64 logits (B, Q, W), encodings): one oracle call per clip with the clip's effective biases"""
    leaf = OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())
    G = [leaf["de_gcond_layer_stack.%d.weight" % i][:, :, 0] for i in range(N)] + [leaf["connection_gcond.weight"][:, :, 0]]
    Wc = [leaf["de_cond_layer_stack.%d.weight" % i] for i in range(N)] + [leaf["connection_cond.weight"]]
    bc = [leaf["de_cond_layer_stack.%d.bias" % i] for i in range(N)] + [leaf["connection_cond.bias"]]
    keep = wo.chunk_softmax
    wo.chunk_softmax = lambda total, q: total              # the oracle's decoder then returns the pre-softmax logits
    stats = dict(near=0, flips=0)
    outs, encs = [], []
    try:
        for b, c in enumerate(classes):
            v = leaf["global_embedding.weight"][c]
            cond = [(Wc[i], bc[i] + G[i] @ v) for i in range(N + 1)]
            relu, st = _device_relu({k: t[b:b + 1] for k, t in dev_pre.items()})
            out, enc = wo.autoencoder_forward(leaf, DIL, x[b:b + 1].double().cpu(), cfg["en_pool_kernel_size"], cond,
                                              filter_width=cfg["filter_width"], q=cfg["quantization_channel"], relu=relu)
            outs.append(out)
            encs.append(enc)
            stats = {k: stats[k] + st[k] for k in stats}
    finally:
        wo.chunk_softmax = keep
    return leaf, torch.cat(outs), torch.cat(encs).detach(), stats


def _objective64(logits, target, objective, Q):
    if objective == "nll":
        return None, F.cross_entropy(logits.permute(0, 2, 1).reshape(-1, Q), target.cpu())
    p64 = wo.chunk_softmax(logits.contiguous(), Q)
    return p64, F.cross_entropy(p64, target.cpu())


def _grads64(leaf, l64):
    return OrderedDict((k, torch.zeros_like(v) if g is None else g)
                       for (k, v), g in zip(leaf.items(), torch.autograd.grad(l64, list(leaf.values()), allow_unused=True, retain_graph=True)))


def _grads_close(label, got, ref):
    """every tensor within GRAD_RTOL of its max-abs (one whose reference is all but zero against 1e-3 of the largest tensor's, the
    rule of tests/test_gpu_cond_learned.py); the projections' and the new tensors' also against their OWN max-abs"""
    worst = ("", 0.0)
    assert list(got) == list(ref)
    gmax = max(float(r.abs().max()) for r in ref.values())
    for k, r in ref.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((got[k].detach().cpu().double() - r).abs().max()) / scale
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= GRAD_RTOL, (label, k, e)
    own = {k: float((got[k].detach().cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if "cond" in k or _is_new(k)}
    new = max(v for k, v in own.items() if _is_new(k))
    assert max(own.values()) <= GRAD_RTOL, (label, own)
    print("  %s: worst gradient %.2e of its max-abs (%s), worst of the new tensors' %.2e (bar %.0e)" % (label, worst[1], worst[0], new, GRAD_RTOL))


def _flat_grads(eng, like):
    g = eng.flat_grad.clone()
    return OrderedDict((n, g[eng.spec.off[n]:eng.spec.off[n] + t.numel()].view(t.shape)) for n, t in like.items())


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, the module surface's results under both objectives and the float64 reference (computed once, never modified)"""
    from music_amd.objective import nll_loss
    net, cfg, B = _build(name)
    x, target = _batch(net, cfg, B)
    classes, Q, T = _classes(B), cfg["quantization_channel"], x.shape[2]
    net.zero_grad()
    probs = net(x, classes)
    loss = torch.nn.CrossEntropyLoss()(probs, target)
    loss.backward()
    grads = {"ce": OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())}
    losses = {"ce": float(loss.detach())}
    enc = net.last_encoding.clone()
    eng = net._engine_for(x.device)
    ws_flags = {k: eng.workspace(B, T).get(k) for k in ("pair",)}
    dev_pre = _dev_pre(eng, B, T)
    net.zero_grad()
    loss = nll_loss(net, x, target, classes)
    loss.backward()
    grads["nll"] = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    losses["nll"] = float(loss.detach())
    leaf, logits, enc64, stats = _logits64(net, cfg, x, classes, dev_pre)
    print("  %s: ReLU pre-activations inside the tolerance band: %d, of which the device's sign differs: %d" % (name, stats["near"], stats["flips"]))
    ref = {}
    for objective in ("ce", "nll"):
        p64, l64 = _objective64(logits, target, objective, Q)
        ref[objective] = dict(p64=None if p64 is None else p64.detach(), l64=float(l64.detach()), g64=_grads64(leaf, l64))
    return dict(net=net, cfg=cfg, B=B, x=x, target=target, classes=classes, probs=probs.detach().clone(), losses=losses, grads=grads,
                eng=eng, enc=enc, enc64=enc64, ref=ref, logits64=logits.detach(), dev_pre=dev_pre, pair=ws_flags["pair"])


@pytest.mark.parametrize("objective", ["ce", "nll"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_every_gradient_against_float64(name, objective):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    c = _case(name)
    eng, B, Q, r = c["eng"], c["B"], c["cfg"]["quantization_channel"], c["ref"][objective]
    assert type(eng) is (GenericAutoencoderEngine if name == "general" else _AutoencoderEngine) and eng.learned and eng.gcond
    if name != "general":
        assert bool(c["pair"]) == (name == "pair32")
    e_enc = float((c["enc"].cpu().double() - c["enc64"]).abs().max())
    assert e_enc < 1e-4
    if objective == "ce":
        e_p = float((c["probs"].cpu().double() - r["p64"]).abs().max())
        print("  %s: encoding err %.2e, probabilities err %.2e (bar %.0e)" % (name, e_enc, e_p, PROB_TOL))
        assert c["probs"].shape == (B * W, Q) and e_p <= PROB_TOL
        nonvacuous(r["p64"], "global conditioning, " + name, 6.0 / Q)
    print("  %s %s: loss %.6f (float64 %.6f)" % (name, objective, c["losses"][objective], r["l64"]))
    assert abs(c["losses"][objective] - r["l64"]) < 1e-4
    _grads_close("%s %s" % (name, objective), c["grads"][objective], r["g64"])
    for k, g in c["grads"][objective].items():
        if _is_new(k):
            assert float(g.abs().max()) > 0, k                                    # the new tensors do get a gradient
    # a class no clip has: its embedding row gets exactly nothing
    assert not c["grads"][objective]["global_embedding.weight"][1].any() and not r["g64"]["global_embedding.weight"][1].any()


@pytest.mark.parametrize("name", ["fast64", "pair32", "odd32", "general"])
def test_the_fused_step_equals_the_module_path_and_is_reproducible(name):
    c = _case(name)
    eng, x, target, classes = c["eng"], c["x"], c["target"], c["classes"]
    for objective in ("ce", "nll"):
        r = c["ref"][objective]
        loss = eng.loss_and_grad(x, target, objective=None if objective == "ce" else "nll", classes=classes)
        g1 = eng.flat_grad.clone()
        assert abs(float(loss) - r["l64"]) < 1e-4
        fused = _flat_grads(eng, c["grads"][objective])
        _grads_close("%s %s fused" % (name, objective), fused, r["g64"])
        for n, g in c["grads"][objective].items():
            if _is_new(n):
                d = float((fused[n] - g).abs().max())
                print("  %s %s: fused against autograd, %s: largest difference %.2e" % (name, objective, n, d))
                if name == "general" and objective == "ce":      # two loss kernels (tests/test_gpu_cond_learned.py): twice the bar apart at most
                    assert d <= 2 * GRAD_RTOL * float(r["g64"][n].abs().max()), (n, d)
                else:
                    assert torch.equal(fused[n], g), (n, d)
        eng.loss_and_grad(x, target, None, objective=None if objective == "ce" else "nll", classes=torch.tensor(classes))
        assert torch.equal(g1, eng.flat_grad), "two fused steps differ"
    with torch.no_grad():
        a = c["net"](x, classes).clone()
        b = c["net"](x, torch.tensor(classes, device=x.device)).clone()
    assert torch.equal(a, b) and torch.equal(a, c["probs"])
    with pytest.raises(ValueError, match="classes"):
        eng.loss_and_grad(x, target)
    with pytest.raises(ValueError, match="class"):
        eng.loss_and_grad(x, target, classes=[NC] * c["B"])


@pytest.mark.parametrize("name", ["fast64_bias", "pair32"])
def test_one_class_for_all_clips_is_a_learned_model_with_the_term_in_its_biases(name):
    """cls[b] = c for every clip: the tables are those of a learned model whose biases are b_i + G_i emb[c]; the probabilities and
    the gradients of every parameter the two models share agree within the bars (both sides are the device's float32)."""
    from music_amd.model1 import wavenet_autoencoder
    net, cfg, B = _build(name, seed=70)
    x, target = _batch(net, cfg, B, seed=71)
    cls = 1
    plain = wavenet_autoencoder(**{k: v for k, v in cfg.items() if not k.startswith("global_")}).cuda()
    sd = net.state_dict()
    v = sd["global_embedding.weight"][cls].double()
    with torch.no_grad():
        for k, p in plain.named_parameters():
            p.copy_(sd[k])
        for i, m in enumerate(list(plain.de_cond_layer_stack) + [plain.connection_cond]):
            g = (net.de_gcond_layer_stack[i] if i < N else net.connection_gcond).weight[:, :, 0].double()
            m.bias.copy_((m.bias.double() + g @ v).float())
    out = {}
    for key, model, args in (("global", net, ([cls] * B,)), ("plain", plain, ())):
        model.zero_grad()
        probs = model(x, *args)
        torch.nn.CrossEntropyLoss()(probs, target).backward()
        out[key] = (probs.detach().clone(), OrderedDict((n, p.grad.clone()) for n, p in model.named_parameters()))
    e_p = float((out["global"][0] - out["plain"][0]).abs().max())
    assert e_p <= PROB_TOL
    worst, gmax = 0.0, max(float(g.abs().max()) for g in out["plain"][1].values())
    for k, g in out["plain"][1].items():
        e = float((out["global"][1][k] - g).abs().max()) / max(float(g.abs().max()), 1e-3 * gmax)      # (the rule of _grads_close)
        worst = max(worst, e)
        assert e <= GRAD_RTOL, (k, e)
    print("  %s: one class against the folded learned model: probabilities %.2e, worst shared gradient %.2e of its max-abs" % (name, e_p, worst))
    # ... and the embedding's gradient sits in row `cls` alone
    ge = out["global"][1]["global_embedding.weight"]
    assert float(ge[cls].abs().max()) > 0 and not ge[[0, 2]].any()


def test_three_guarded_adam_steps_with_ema_and_their_checkpoints(tmp_path):
    from music_amd import ema
    from music_amd.ae_train import load_model, save_model
    from music_amd.model1 import wavenet_autoencoder
    net, cfg, B = _build("fast64_bias", seed=60)
    x, target = _batch(net, cfg, B, seed=61)
    classes = _classes(B)
    eng = net._engine_for(x.device)
    decay = 0.9
    eng.adam_init(lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=decay, ema_warmup=True)
    new_names = [n for n in eng.param_names if _is_new(n)]
    assert len(new_names) == N + 2 and eng.param_names[-len(new_names):] == new_names
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    ref = Ref64(eng.flat.cpu().numpy())
    for step in range(1, 4):
        eng.loss_and_grad(x, target, classes=classes)
        eng.adam_step()
        ref.step(eng.flat.cpu().numpy(), kernel_w(decay, True, step))
    rep = eng.guard_report()
    assert rep["taken"] == 3 and rep["skipped"] == 0
    for n, p in net.named_parameters():
        if n in new_names:
            o = eng.spec.off[n]
            had_grad = eng.flat_grad[o:o + p.numel()].view(p.shape) != 0
            moved = p != start[n]
            assert bool(torch.isfinite(p).all()) and bool(moved.any()) and bool(moved[had_grad].all()), n
    assert torch.equal(net.global_embedding.weight[1], start["global_embedding.weight"][1])      # the absent class stays where it was
    ratio = ref.check(eng.ema.flat.cpu().numpy(), "shadow after three steps")
    print("  shadow against the float64 lerp: largest error / bound %.3f" % ratio)
    # .model / .ema round trip: a fresh model restored from either file continues bit for bit
    path = str(tmp_path) + "/"
    save_model(net, 3, path)
    ema.save_shadow(eng.ema, path + "wavenet_autoencoder3.ema")
    with torch.no_grad():
        p_model = net(x, classes).clone()
        with eng.ema.swapped(net):
            p_ema = net(x, classes).clone()
        assert torch.equal(net(x, classes), p_model)
    assert not torch.equal(p_model, p_ema)
    for name, want in (("wavenet_autoencoder3.model", p_model), ("wavenet_autoencoder3.ema", p_ema)):
        twin = load_model(wavenet_autoencoder(**cfg), path, name).cuda()
        with torch.no_grad():
            assert torch.equal(twin(x, classes), want), name
    loss = eng.loss_and_grad(x, target, classes=classes)
    twin = load_model(wavenet_autoencoder(**cfg), path, "wavenet_autoencoder3.model").cuda()
    teng = twin._engine_for(x.device)
    assert torch.equal(teng.loss_and_grad(x, target, classes=classes), loss) and torch.equal(teng.flat_grad, eng.flat_grad)
    with pytest.raises(RuntimeError, match="global_classes"):
        load_model(wavenet_autoencoder(**dict(cfg, global_classes=0, global_channels=0)), path, "wavenet_autoencoder3.ema")


def test_resynthesis_follows_the_class_it_is_given():
    from music_amd.ae_generate import resynthesize
    c = _case("fast64")
    net, x, B, eng, cfg = c["net"], c["x"], c["B"], c["eng"], c["cfg"]
    classes, other = c["classes"], [(k + 1) % NC for k in c["classes"]]
    p64 = {}
    for key, cls in (("own", classes), ("other", other)):
        with torch.no_grad():
            _, _, ws = eng.forward(x, want_probs=False, classes=cls)
            p_dev = eng.step_probs(ws).view(B, W, 256).clone()
            dev_pre = _dev_pre(eng, B, x.shape[2])
        _, logits, _, _ = _logits64(net, cfg, x, cls, dev_pre)
        p64[key] = torch.softmax(logits.detach(), 1).transpose(1, 2)
        codes, probs, enc = resynthesize(net, x, teacher_forced=True, want_probs=True, classes=cls)
        e_dev, e64 = float((probs - p_dev).abs().max()), float((probs.cpu().double() - p64[key]).abs().max())
        print("  resynthesis as %s class: probabilities err %.2e (device forward), %.2e (float64; bar %.0e)" % (key, e_dev, e64, PROB_TOL))
        assert tuple(probs.shape) == (B, W, 256) and e_dev <= PROB_TOL and e64 <= PROB_TOL
        if key == "own":
            own = probs.clone()
            again, _, _ = resynthesize(net, x, teacher_forced=True, global_vectors=net.global_vectors(cls))
            assert torch.equal(codes, again)
    # the feature has an effect: the reference alone shows the gap, and the device follows it
    gap64, gap = float((p64["own"] - p64["other"]).abs().max()), float((probs - own).abs().max())
    print("  swapped classes: largest change of a probability %.3f (float64), %.3f (device)" % (gap64, gap))
    assert gap64 > 1e-2 + 2 * PROB_TOL and gap > 1e-2
    # a mix of two embedding rows decodes; both arguments, or none, are refused
    mix = 0.5 * (net.global_vectors(classes) + net.global_vectors(other))
    free_a, _, _ = resynthesize(net, x, global_vectors=mix)
    free_b, _, _ = resynthesize(net, x, global_vectors=mix)
    assert torch.equal(free_a, free_b)
    for kw in ({}, dict(classes=classes, global_vectors=mix), dict(classes=[NC] * B), dict(global_vectors=mix[:, :-1])):
        with pytest.raises(ValueError, match="class|global_vectors"):
            resynthesize(net, x, **kw)


def test_decode_codes_takes_classes_or_their_vectors():
    from music_amd.ae_generate import decode_codes, encode_codes, resynthesize
    net, cfg, B = _build("fast64", seed=80, bottleneck="vq", vq_codes=16)
    x, _ = _batch(net, cfg, B, seed=81)
    classes = _classes(B)
    codes = encode_codes(net, x)                                                   # (the encoder takes no class)
    assert tuple(codes.shape) == (B, W // cfg["en_pool_kernel_size"])
    tf = x.argmax(1)
    a, pa = decode_codes(net, codes, W, teacher_forced=tf, want_probs=True, classes=classes)
    b, pb = decode_codes(net, codes, W, teacher_forced=tf, want_probs=True, global_vectors=net.global_vectors(classes))
    assert torch.equal(a, b) and torch.equal(pa, pb)
    # ... which is the resynthesis of those clips as those classes, and another class gives other probabilities
    _, pr, _ = resynthesize(net, x, teacher_forced=True, want_probs=True, classes=classes)
    assert torch.equal(pa, pr)
    _, po = decode_codes(net, codes, W, teacher_forced=tf, want_probs=True, classes=[(k + 1) % NC for k in classes])
    assert float((po - pa).abs().max()) > 1e-2
    free_a, _ = decode_codes(net, codes, W, classes=classes, temperature=0.8, seed=3)
    free_b, _ = decode_codes(net, codes, W, global_vectors=net.global_vectors(classes), temperature=0.8, seed=3)
    assert torch.equal(free_a, free_b)
    with pytest.raises(ValueError, match="class|global_vectors"):
        decode_codes(net, codes, W)
