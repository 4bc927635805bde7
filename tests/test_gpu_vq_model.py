"""`bottleneck="vq"` on the device (music_amd/model1.py, music_amd/ae_generic.py, wn_vq_fwd / wn_vq_bwd): the whole model against
float64 - oracle.autoencoder_encode -> tests/vq_ref.py -> oracle.autoencoder_decode, the model's parameters as leaves, the
codebook among them - on the case table of tests/test_gpu_cond_learned.py, K = 32 codes taken from the encodings of other clips.

The assignment cannot hide behind the device: every case first asserts, on the float64 side alone, that every frame's relative
margin (second-best - best) / best is at least MARGIN = 1e-3 (the seeds below were chosen on the CPU so that it is; the fp32
encoding is within 1e-4 of the float64 one, two orders below that), and then that the device's codes EQUAL the float64 argmin in
every frame.  Bars: probabilities within 1e-3, every gradient within 3e-4 of its tensor's max-abs (the codebook's and every
encoder tensor's against their OWN max-abs), vq_loss within 1e-5 relative; the float64 pass takes the device's sign at ReLU
pre-activations inside the tolerance band (tests/test_gpu_fullsize._device_relu).  Then the surfaces: autograd against the fused
step, vq_loss left out, torch's own loss kernels, the NLL objective, determinism, a guarded Adam + EMA step with its checkpoints,
and that a continuous model never calls wn_vq_*.  Run with -m gpu."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo
from tests import vq_ref
from tests.test_gpu_cond_learned import CASES, DIL, W, _cfg, _dev_pre
from tests.test_gpu_fullsize import _device_relu

PROB_TOL = 1e-3
GRAD_RTOL = 3e-4
VQ_LOSS_RTOL = 1e-5
MARGIN = 1e-3
K = 32
BETA = 0.25
B_INIT = 8                  # clips whose (float64) encodings the codebook is drawn from: at least 64 frames for 32 codes
# the batch seed of every case, verified on the CPU against MARGIN (model seed 70 + the case's rank, init batch seed 5)
# (the smallest seed from 9 on whose smallest margin is at least 2e-3: 1.4e-2, 5.1e-3, 1.1e-2, 1.1e-2, 2.9e-2, 2.8e-3)
SEEDS = {"fast64": 9, "fast64_bias": 9, "pair32": 9, "odd32": 10, "long_encoding": 11, "general": 9}


def _codes_batch(cfg, rf, B, seed):
    rng = np.random.default_rng(seed)
    Q, T = cfg["quantization_channel"], rf + W - 1
    codes = torch.from_numpy(rng.integers(0, Q, size=(B, T)))
    x = F.one_hot(codes, Q).permute(0, 2, 1).float().contiguous()
    target = torch.from_numpy(rng.integers(0, Q, size=(B * W,)).astype(np.int64))
    return x, target


def build_cpu(name, seed=70):
    """The case's vq model on the CPU, its codebook drawn from the float64 encodings of B_INIT other clips, and its batch.
    Everything here is a function of seeds and the oracle: the margins can be (and were) checked without a device."""
    from music_amd.model1 import wavenet_autoencoder
    kw, B = CASES[name]
    cfg = dict(_cfg(**kw), bottleneck="vq", vq_codes=K, vq_beta=BETA)
    torch.manual_seed(seed + sorted(CASES).index(name))
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
    leaf = {k: v.detach().double() for k, v in net.state_dict().items()}
    x_init, _ = _codes_batch(cfg, net.receptive_field, B_INIT, 5)
    with torch.no_grad():
        enc_init = wo.autoencoder_encode(leaf, DIL, x_init.double(), cfg["en_pool_kernel_size"])
    net.init_codebook(enc_init.float(), seed=3)
    x, target = _codes_batch(cfg, net.receptive_field, B, SEEDS[name])
    return net, cfg, B, x, target


def float64_margins(net, cfg, x):
    leaf = {k: v.detach().double() for k, v in net.state_dict().items()}
    with torch.no_grad():
        enc = wo.autoencoder_encode(leaf, DIL, x.double(), cfg["en_pool_kernel_size"])
    f = vq_ref.forward(enc.numpy(), leaf["vq_codebook.weight"].numpy(), BETA)
    return vq_ref.margins(f["dist"]), f


class _VQ64(torch.autograd.Function):
    """tests/vq_ref.py as a float64 autograd node: (e, codebook) -> (q, vq_loss); straight-through, as vq_ref.backward states it"""

    @staticmethod
    def forward(ctx, e, cb):
        f = vq_ref.forward(e.detach().numpy(), cb.detach().numpy(), BETA)
        ctx.save_for_backward(e, cb)
        ctx.idx = f["idx"]
        ctx.set_materialize_grads(False)
        return torch.from_numpy(np.ascontiguousarray(f["q"])), torch.tensor(f["vq_loss"], dtype=torch.float64)

    @staticmethod
    def backward(ctx, d_q, g):
        e, cb = ctx.saved_tensors
        d_e, d_c = vq_ref.backward(e.numpy(), cb.numpy(), ctx.idx, None if d_q is None else d_q.numpy(), BETA, 0.0 if g is None else float(g))
        return torch.from_numpy(np.ascontiguousarray(d_e)), torch.from_numpy(np.ascontiguousarray(d_c))


def _oracle64(net, cfg, x, relu, logits=False):
    """float64: encode -> vq_ref -> decode on the model's parameters as leaves -> (leaves, output, e, q, vq_loss, idx)"""
    leaf = OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())
    N = len(DIL)
    cond = [(leaf["de_cond_layer_stack.%d.weight" % i], leaf["de_cond_layer_stack.%d.bias" % i]) for i in range(N)]
    cond.append((leaf["connection_cond.weight"], leaf["connection_cond.bias"]))
    x64 = x.double().cpu()
    e = wo.autoencoder_encode(leaf, DIL, x64, cfg["en_pool_kernel_size"], relu)
    q, vq_loss = _VQ64.apply(e, leaf["vq_codebook.weight"])
    idx = vq_ref.forward(e.detach().numpy(), leaf["vq_codebook.weight"].detach().numpy(), BETA)["idx"]
    keep = wo.chunk_softmax
    if logits:
        wo.chunk_softmax = lambda total, q_: total
    try:
        out = wo.autoencoder_decode(leaf, DIL, x64, q, W, cond, cfg["quantization_channel"], relu)
    finally:
        wo.chunk_softmax = keep
    return leaf, out, e, q, vq_loss, idx


def _grads64(loss, leaf):
    return OrderedDict((k, torch.zeros_like(v) if g is None else g)
                       for (k, v), g in zip(leaf.items(), torch.autograd.grad(loss, list(leaf.values()), allow_unused=True)))


def _own_scale(k):
    """the codebook and every encoder tensor are measured against their own max-abs"""
    return k.startswith(("vq_codebook", "en_", "bottleneck_layer"))


def _grads_close(label, got, ref):
    assert list(got) == list(ref)
    gmax = max(float(r.abs().max()) for r in ref.values())
    worst, worst_own = ("", 0.0), ("", 0.0)
    for k, r in ref.items():
        own = float(r.abs().max())
        err = float((got[k].detach().cpu().double() - r).abs().max())
        if _own_scale(k):
            if own == 0.0:                          # (a bias under a constant shift: nothing to measure against)
                assert err <= GRAD_RTOL * 1e-3 * gmax, (label, k, err)
                continue
            worst_own = max(worst_own, (k, err / own), key=lambda t: t[1])
            assert err / own <= GRAD_RTOL, (label, k, err / own)
        else:
            e = err / max(own, 1e-3 * gmax)         # the rule of tests/test_gpu_cond_learned.py
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e <= GRAD_RTOL, (label, k, e)
    print("  %s: worst gradient %.2e of its max-abs (%s); codebook / encoder against their own: %.2e (%s) (bar %.0e)"
          % (label, worst[1], worst[0], worst_own[1], worst_own[0], GRAD_RTOL))


def _named(eng, flat_grad):
    return OrderedDict((n, flat_grad[eng.spec.off[n]:eng.spec.off[n] + int(np.prod(eng.spec.shape[n]))].view(eng.spec.shape[n]).clone())
                       for n in eng.param_names)


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, module-surface results and the float64 reference of one case (computed once, never modified)"""
    net, cfg, B, x, target = build_cpu(name)
    margins, f_cpu = float64_margins(net, cfg, x)
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    T = x.shape[2]
    net.zero_grad()
    probs = net(x)
    vq_loss = net.vq_loss
    loss = torch.nn.CrossEntropyLoss()(probs, target) + vq_loss
    loss.backward()
    eng = net._engine_for(x.device)
    relu, stats = _device_relu(_dev_pre(eng, B, T))
    leaf, p64, e64, q64, vq64, idx64 = _oracle64(net, cfg, x, relu)
    l64 = F.cross_entropy(p64, target.cpu()) + vq64
    g64 = _grads64(l64, leaf)
    print("  %s: ReLU pre-activations inside the tolerance band: %d, of which the device's sign differs: %d" % (name, stats["near"], stats["flips"]))
    grads = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    return dict(net=net, cfg=cfg, B=B, x=x, target=target, probs=probs.detach().clone(), loss=float(loss.detach()), grads=grads, eng=eng,
                vq_loss=float(vq_loss.detach()), codes=net.vq_codes.clone(), q=net.last_encoding.clone(), e=net.last_encoding_pre.clone(),
                stats=net.last_vq, margins=margins, f_cpu=f_cpu, p64=p64.detach(), l64=float(l64.detach()), g64=g64, e64=e64.detach(),
                q64=q64.detach(), vq64=float(vq64.detach()), idx64=idx64)


@pytest.mark.parametrize("name", list(CASES))
def test_codes_forward_and_every_gradient_against_float64(name):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    c = _case(name)
    eng, B, Q = c["eng"], c["B"], c["cfg"]["quantization_channel"]
    Le = W // c["cfg"]["en_pool_kernel_size"]
    assert type(eng) is (GenericAutoencoderEngine if name == "general" else _AutoencoderEngine) and eng.vq and eng.learned
    # ---- the float64 side alone: no frame is a near-tie, several codes are in use
    m = c["margins"]
    print("  %s: smallest relative margin %.3e over %d frames (bar %.0e), %d codes used" % (name, m.min(), m.size, MARGIN, (c["f_cpu"]["counts"] > 0).sum()))
    assert m.shape == (B, Le) and (m >= MARGIN).all()
    assert (c["f_cpu"]["counts"] > 0).sum() >= 3
    assert np.array_equal(c["idx64"], c["f_cpu"]["idx"])                           # (the device's ReLU signs do not move a frame)
    # ---- the device's codes EQUAL the float64 argmin: every frame, none left out
    codes = c["codes"].cpu().numpy()
    assert codes.shape == (B, Le) and c["codes"].dtype == torch.int64
    assert np.array_equal(codes, c["idx64"]), "codes differ in %d of %d frames" % ((codes != c["idx64"]).sum(), codes.size)
    cb = c["net"].vq_codebook.weight.detach()
    assert torch.equal(c["q"], cb[c["codes"]].permute(0, 2, 1))                    # last_encoding is q, rows of the codebook
    e_e = float((c["e"].cpu().double() - c["e64"]).abs().max())
    e_p = float((c["probs"].cpu().double() - c["p64"]).abs().max())
    rel = abs(c["vq_loss"] - c["vq64"]) / c["vq64"]
    print("  %s: pre-quantisation encoding err %.2e, probabilities err %.2e (bar %.0e), vq_loss %.8g (float64 %.8g, relative %.1e, bar %.0e)"
          % (name, e_e, e_p, PROB_TOL, c["vq_loss"], c["vq64"], rel, VQ_LOSS_RTOL))
    assert c["probs"].shape == (B * W, Q) and e_e < 1e-4 and e_p <= PROB_TOL and rel <= VQ_LOSS_RTOL
    assert abs(c["loss"] - c["l64"]) < 1e-4
    # ---- usage statistics
    s = c["stats"]
    assert np.array_equal(s.counts.cpu().numpy(), c["f_cpu"]["counts"]) and int(s.codes_used) == (c["f_cpu"]["counts"] > 0).sum()
    assert abs(float(s.perplexity) - c["f_cpu"]["perplexity"]) <= 1e-5 * c["f_cpu"]["perplexity"]
    assert abs(float(s.mse) * (1 + BETA) - c["vq_loss"]) <= 1e-6 * c["vq_loss"]
    # ---- gradients
    _grads_close(name, c["grads"], c["g64"])
    g_cb = c["grads"]["vq_codebook.weight"]
    unused = torch.from_numpy(c["f_cpu"]["counts"] == 0).to(g_cb.device)
    assert bool((g_cb[unused] == 0).all()) and bool((g_cb[~unused].abs().amax(1) > 0).all())


@pytest.mark.parametrize("name", ["fast64", "pair32", "general"])
def test_autograd_gives_the_fused_steps_gradients(name):
    """engine.loss_and_grad returns reconstruction loss + vq_loss and leaves float64's gradients; on the fast engine - where
    loss.backward() runs the same forward, the same fused softmax + CrossEntropyLoss kernel and the same backward - autograd's
    .grad holds the same BITS (the general plan's module surface takes torch's loss kernels: within the bar)."""
    c = _case(name)
    eng, net, x, target = c["eng"], c["net"], c["x"], c["target"]
    loss = eng.loss_and_grad(x, target)
    g1 = eng.flat_grad.clone()
    assert abs(float(loss) - c["l64"]) < 1e-4
    fused = _named(eng, g1)
    _grads_close(name + " fused", fused, c["g64"])
    gmax = max(float(r.abs().max()) for r in c["g64"].values())
    for n, g in c["grads"].items():
        if name == "general":
            # two loss kernels: each side is within GRAD_RTOL of float64 (a tensor whose reference is all but zero - a bias under the
            # chunk softmax - against 1e-3 of the largest tensor's max-abs, the rule of _grads_close), so of each other within twice that
            assert float((fused[n] - g).abs().max()) <= 2 * GRAD_RTOL * max(float(c["g64"][n].abs().max()), 1e-3 * gmax), n
        else:
            assert torch.equal(fused[n], g), n
    assert abs(float(eng.last_vq.vq_loss) - c["vq_loss"]) == 0.0
    eng.loss_and_grad(x, target, None)                                             # determinism: the same bits again
    assert torch.equal(g1, eng.flat_grad)


def test_leaving_vq_loss_out_and_torchs_own_loss_kernels():
    c = _case("fast64")
    net, x, target = c["net"], c["x"], c["target"]
    crit = torch.nn.CrossEntropyLoss()
    # ---- without net.vq_loss: the codebook's gradient is identically 0 and no commitment term reaches the encoder
    net.zero_grad()
    crit(net(x), target).backward()
    assert bool((net.vq_codebook.weight.grad == 0).all())
    relu, _ = _device_relu(_dev_pre(c["eng"], c["B"], x.shape[2]))
    leaf, p64, _, _, _, _ = _oracle64(net, c["cfg"], x, relu)
    g64 = _grads64(F.cross_entropy(p64, target.cpu()), leaf)
    assert float(g64["vq_codebook.weight"].abs().max()) == 0.0
    _grads_close("without vq_loss", OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters()), g64)
    assert not torch.equal(net.bottleneck_layer.weight.grad, c["grads"]["bottleneck_layer.weight"])
    # ---- fuse_loss = False: torch's criterion on the probabilities, the dense backward
    net.fuse_loss = False
    try:
        net.zero_grad()
        (crit(net(x), target) + net.vq_loss).backward()
        _grads_close("fuse_loss off", OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters()), c["g64"])
        # ---- an upstream factor on vq_loss alone reaches the codebook's gradient alone (exactly: a power of two)
        net.zero_grad()
        (crit(net(x), target) + 4.0 * net.vq_loss).backward()
        assert torch.equal(net.vq_codebook.weight.grad, 4.0 * c["grads"]["vq_codebook.weight"])
    finally:
        net.fuse_loss = True
    net.zero_grad()
    (crit(net(x), target) + 4.0 * net.vq_loss).backward()
    assert torch.equal(net.vq_codebook.weight.grad, 4.0 * c["grads"]["vq_codebook.weight"])
    assert torch.equal(net.connection_2.weight.grad, c["grads"]["connection_2.weight"])


def test_nll_objective_against_float64():
    from music_amd import objective
    c = _case("fast64")
    net, eng, x, target, B = c["net"], c["eng"], c["x"], c["target"], c["B"]
    loss = eng.loss_and_grad(x, target, objective="nll")
    grads = _named(eng, eng.flat_grad)
    relu, _ = _device_relu(_dev_pre(eng, B, x.shape[2]))
    leaf, logits, _, _, vq64, _ = _oracle64(net, c["cfg"], x, relu, logits=True)
    assert tuple(logits.shape) == (B, 256, W)
    l64 = F.cross_entropy(logits.permute(0, 2, 1).reshape(-1, 256), target.cpu()) + vq64
    print("  nll: loss %.6f, float64 %.6f" % (float(loss), float(l64.detach())))
    assert abs(float(loss) - float(l64.detach())) < 1e-4
    _grads_close("nll", grads, _grads64(l64, leaf))
    # objective.nll_loss adds nothing by itself: the caller adds net.vq_loss, and gets the fused step's bits
    net.zero_grad()
    net.vq_loss = None
    nll = objective.nll_loss(net, x, target)
    assert net.vq_loss is not None and abs(float(net.vq_loss) - c["vq_loss"]) == 0.0
    assert abs(float(nll) + float(net.vq_loss) - float(loss)) < 1e-6
    (nll + net.vq_loss).backward()
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, grads[n]), n
    # score runs on q
    s = objective.score(net, x, target.view(B, W))
    assert abs(float(s["nll"].mean()) - float(nll)) < 1e-5


def test_one_guarded_adam_and_ema_step_and_its_checkpoints_resume_bit_for_bit(tmp_path):
    from music_amd import ema, train as wtrain
    from music_amd.ae_train import load_model, save_model
    from music_amd.model1 import wavenet_autoencoder
    net, cfg, B, x, target = build_cpu("fast64_bias")
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    eng = net._engine_for(x.device)
    init = dict(lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=0.9, ema_warmup=True)
    eng.adam_init(**init)
    cb0 = net.vq_codebook.weight.detach().clone()
    eng.loss_and_grad(x, target)
    eng.adam_step()
    rep = eng.guard_report()
    assert rep["taken"] == 1 and rep["skipped"] == 0
    used = eng.last_vq.counts > 0
    moved = (net.vq_codebook.weight.detach() != cb0).any(1)
    assert bool(moved[used].all()) and int(used.sum()) >= 3                       # Adam, the guard and the EMA cover the codebook
    assert not torch.equal(eng.ema.tensors["vq_codebook.weight"], net.vq_codebook.weight.detach())
    path = str(tmp_path) + "/"
    save_model(net, 1, path)
    ema.save_shadow(eng.ema, path + "wavenet_autoencoder1.ema")
    blob = wtrain._optimizer_state(None, eng)
    blob["ema_updates"] = eng.ema.updates(eng.adam_state.get("guard"))
    torch.save(blob, path + "wavenet_autoencoder1.opt")
    with torch.no_grad():
        p_model = net(x).clone()
        with eng.ema.swapped(net):
            p_ema = net(x).clone()
    assert not torch.equal(p_model, p_ema)
    for name, want in (("wavenet_autoencoder1.model", p_model), ("wavenet_autoencoder1.ema", p_ema)):
        twin = load_model(wavenet_autoencoder(**cfg), path, name).cuda()
        with torch.no_grad():
            assert torch.equal(twin(x), want), name
    with pytest.raises(RuntimeError, match="bottleneck"):
        load_model(wavenet_autoencoder(**dict(cfg, bottleneck="continuous")), path, "wavenet_autoencoder1.model")
    # ---- resume: .model + .opt + .ema into a fresh model, one more step on both: the same bits everywhere
    twin = load_model(wavenet_autoencoder(**cfg), path, "wavenet_autoencoder1.model").cuda()
    teng = twin._engine_for(x.device)
    teng.adam_init(**init)
    assert wtrain._restore_optimizer_state(path + "wavenet_autoencoder1.opt", None, lambda: teng) is teng
    ema.restore_shadow(teng.ema, path + "wavenet_autoencoder1.ema", wtrain._saved_ema_updates(path + "wavenet_autoencoder1.opt"),
                       teng.adam_state.get("guard"))
    for e in (eng, teng):
        e.loss_and_grad(x, target)
        e.adam_step()
    assert torch.equal(eng.flat_grad, teng.flat_grad) and torch.equal(eng.flat, teng.flat)
    assert torch.equal(eng.ema.flat, teng.ema.flat)
    assert torch.equal(eng.adam_state["m"], teng.adam_state["m"]) and torch.equal(eng.adam_state["v"], teng.adam_state["v"])


def test_a_continuous_model_never_calls_the_vq_entries(monkeypatch):
    """With the key unset the step is the parent's: every entry the engines call is recorded ON the device run (and called through) -
    no wn_vq_* entry appears, on the vq model exactly the two per pass.  (tests/test_vq_model_cpu.py holds the whole launch list
    of both plans against the continuous step's with the recorder of tests/launch_trace.py, which replaces the device.)"""
    from music_amd import engine_base, model1
    from music_amd._lib import call as real_call
    from music_amd.model1 import wavenet_autoencoder
    names = []

    def recording(name, *args):
        names.append(name)
        return real_call(name, *args)
    for mod in (engine_base, model1):
        monkeypatch.setattr(mod, "call", recording)
    kw, B = CASES["fast64"]
    for mode in ("continuous", "vq"):
        torch.manual_seed(1)
        net = wavenet_autoencoder(**dict(_cfg(**kw), bottleneck=mode, vq_codes=K)).cuda()
        x, target = _codes_batch(_cfg(**kw), net.receptive_field, B, 2)
        del names[:]
        eng = net._engine_for(next(net.parameters()).device)
        eng.loss_and_grad(x.cuda(), target.cuda())
        (torch.nn.CrossEntropyLoss()(net(x.cuda()), target.cuda()) + (net.vq_loss if mode == "vq" else 0.0)).backward()
        torch.cuda.synchronize()
        vq_calls = [n for n in names if n.startswith("wn_vq")]
        assert "wn_avgpool" in names and "wn_cond_proj_bwd" in names
        assert vq_calls == ([] if mode == "continuous" else ["wn_vq_fwd", "wn_vq_bwd"] * 2), vq_calls
        assert (net.vq_loss is None) == (mode == "continuous")
