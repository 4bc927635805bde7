"""`vq_stages` = 3 on the device (music_amd/engine_base.py: wn_rvq_fwd / wn_rvq_bwd / wn_rvq_bwd_stats / wn_rvq_ema_update behind
both plans): the whole model against float64 - oracle.autoencoder_encode -> tests/rvq_ref.py -> oracle.autoencoder_decode, the model's
parameters as leaves - on the case table of tests/test_gpu_vq_model.py, whose helpers, seeds' rule and bars are used as they are:
K = 32 codes per stage, the stages filled in order by init_codebook from the float64 encodings of other clips.

Every case first asserts, on the float64 side alone, that every (frame, stage) pair's relative margin is at least MARGIN = 1e-3 (the
batch seeds below were chosen on the CPU so that it is: the smallest seed from 9 on whose smallest margin is at least 2e-3), then
that the device's codes EQUAL the float64 argmin in every frame and stage.  Bars: probabilities within 1e-3, every gradient within 3e-4
of its tensor's max-abs, vq_loss within 1e-5 relative.  Then the module surface against the fused step, EMA mode step by step against
the float64 rule per stage, and a checkpoint's resume.  Run with -m gpu."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo
from tests import rvq_ref, vq_ref
from tests import vq_ema_ref as er
from tests.test_gpu_cond_learned import CASES, DIL, W, _cfg, _dev_pre
from tests.test_gpu_fullsize import _device_relu
from tests.test_gpu_vq_ema_kernels import U, check_update
from tests.test_gpu_vq_model import (B_INIT, BETA, GRAD_RTOL, K, MARGIN, PROB_TOL, VQ_LOSS_RTOL, _codes_batch, _grads64, _grads_close,
                                     _named)

S = 3
# (smallest margins 5.4e-3, 3.7e-3, 4.3e-3, 4.3e-3, 2.3e-3, 3.1e-3; model seed 70 + the case's rank, init batch seed 5)
SEEDS = {"fast64": 10, "fast64_bias": 9, "pair32": 9, "odd32": 10, "long_encoding": 26, "general": 10}
DECAY, EPS, RESTART = 0.9, 1e-5, 0.95


def build_cpu(name, seed=70, **kw):
    """tests/test_gpu_vq_model.build_cpu with S stages: model, codebook from the float64 encodings of S B_INIT other clips, batch."""
    from music_amd.model1 import wavenet_autoencoder
    ckw, B = CASES[name]
    cfg = dict(_cfg(**ckw), bottleneck="vq", vq_codes=K, vq_beta=BETA, vq_stages=S, **kw)
    torch.manual_seed(seed + sorted(CASES).index(name))
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
    leaf = {k: v.detach().double() for k, v in net.state_dict().items()}
    x_init, _ = _codes_batch(cfg, net.receptive_field, S * B_INIT, 5)             # (frames for S stages: a frame that became a row is spent)
    with torch.no_grad():
        enc_init = wo.autoencoder_encode(leaf, DIL, x_init.double(), cfg["en_pool_kernel_size"])
    net.init_codebook(enc_init.float(), seed=3)
    x, target = _codes_batch(cfg, net.receptive_field, B, SEEDS[name])
    return net, cfg, B, x, target


def float64_margins(net, cfg, x):
    """(S, B, Le) relative margins of the float64 chain, and the chain"""
    leaf = {k: v.detach().double() for k, v in net.state_dict().items()}
    with torch.no_grad():
        enc = wo.autoencoder_encode(leaf, DIL, x.double(), cfg["en_pool_kernel_size"])
    f = rvq_ref.forward(enc.numpy(), leaf["vq_codebook.weight"].numpy(), S, BETA)
    return np.stack([vq_ref.margins(d) for d in f["dist"]]), f


class _RVQ64(torch.autograd.Function):
    """tests/rvq_ref.py as a float64 autograd node: (e, codebook) -> (q, vq_loss)"""

    @staticmethod
    def forward(ctx, e, cb):
        f = rvq_ref.forward(e.detach().numpy(), cb.detach().numpy(), S, BETA)
        ctx.save_for_backward(e, cb)
        ctx.idx = f["idx"]
        ctx.set_materialize_grads(False)
        return torch.from_numpy(np.ascontiguousarray(f["q"])), torch.tensor(f["vq_loss"], dtype=torch.float64)

    @staticmethod
    def backward(ctx, d_q, g):
        e, cb = ctx.saved_tensors
        d_e, d_c = rvq_ref.backward(e.numpy(), cb.numpy(), S, ctx.idx, None if d_q is None else d_q.numpy(), BETA, 0.0 if g is None else float(g))
        return torch.from_numpy(np.ascontiguousarray(d_e)), torch.from_numpy(np.ascontiguousarray(d_c))


def _oracle64(net, cfg, x, relu):
    leaf = OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())
    N = len(DIL)
    cond = [(leaf["de_cond_layer_stack.%d.weight" % i], leaf["de_cond_layer_stack.%d.bias" % i]) for i in range(N)]
    cond.append((leaf["connection_cond.weight"], leaf["connection_cond.bias"]))
    x64 = x.double().cpu()
    e = wo.autoencoder_encode(leaf, DIL, x64, cfg["en_pool_kernel_size"], relu)
    q, vq_loss = _RVQ64.apply(e, leaf["vq_codebook.weight"])
    f = rvq_ref.forward(e.detach().numpy(), leaf["vq_codebook.weight"].detach().numpy(), S, BETA)
    out = wo.autoencoder_decode(leaf, DIL, x64, q, W, cond, cfg["quantization_channel"], relu)
    return leaf, out, e, q, vq_loss, f


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, batch, module-surface results and the float64 reference of one case (computed once, never modified)"""
    net, cfg, B, x, target = build_cpu(name)
    margins, f_cpu = float64_margins(net, cfg, x)
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    net.zero_grad()
    probs = net(x)
    vq_loss = net.vq_loss
    loss = torch.nn.CrossEntropyLoss()(probs, target) + vq_loss
    loss.backward()
    eng = net._engine_for(x.device)
    relu, stats = _device_relu(_dev_pre(eng, B, x.shape[2]))
    leaf, p64, e64, q64, vq64, f64 = _oracle64(net, cfg, x, relu)
    l64 = F.cross_entropy(p64, target.cpu()) + vq64
    g64 = _grads64(l64, leaf)
    grads = OrderedDict((n, p.grad.clone()) for n, p in net.named_parameters())
    return dict(net=net, cfg=cfg, B=B, x=x, target=target, probs=probs.detach().clone(), loss=float(loss.detach()), grads=grads, eng=eng,
                vq_loss=float(vq_loss.detach()), codes=net.vq_codes.clone(), q=net.last_encoding.clone(), e=net.last_encoding_pre.clone(),
                stats=net.last_vq, margins=margins, f_cpu=f_cpu, p64=p64.detach(), l64=float(l64.detach()), g64=g64, e64=e64.detach(),
                vq64=float(vq64.detach()), f64=f64)


@pytest.mark.parametrize("name", list(CASES))
def test_codes_forward_and_every_gradient_against_float64(name):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    c = _case(name)
    eng, B, Q = c["eng"], c["B"], c["cfg"]["quantization_channel"]
    Le = W // c["cfg"]["en_pool_kernel_size"]
    assert type(eng) is (GenericAutoencoderEngine if name == "general" else _AutoencoderEngine) and eng.vq and eng.vq_S == S
    # ---- the float64 side alone: no (frame, stage) pair is a near-tie, several codes are in use in every stage
    m, f = c["margins"], c["f_cpu"]
    print("  %s: smallest relative margin per stage %s over %d frames (bar %.0e), codes used %s"
          % (name, ["%.2e" % v for v in m.reshape(S, -1).min(1)], B * Le, MARGIN, (f["counts"] > 0).sum(1).tolist()))
    assert m.shape == (S, B, Le) and (m >= MARGIN).all()
    assert ((f["counts"] > 0).sum(1) >= 3).all()
    assert np.array_equal(c["f64"]["idx"], f["idx"])                               # (the device's ReLU signs do not move a frame)
    # ---- the device's codes EQUAL the float64 argmin: every frame and stage
    codes = c["codes"].cpu().numpy()
    assert codes.shape == (B, S, Le) and c["codes"].dtype == torch.int64
    want = f["idx"].transpose(1, 0, 2)
    assert np.array_equal(codes, want), "codes differ in %d of %d (frame, stage) pairs" % ((codes != want).sum(), codes.size)
    cb = c["net"].vq_codebook.weight.detach()
    q = None
    for s in range(S):                                                             # last_encoding is q: the rows' fp32 sum in stage order
        row = cb[s * K:(s + 1) * K][c["codes"][:, s]].permute(0, 2, 1)
        q = row if q is None else q + row
    assert torch.equal(c["q"], q)
    e_e = float((c["e"].cpu().double() - c["e64"]).abs().max())
    e_p = float((c["probs"].cpu().double() - c["p64"]).abs().max())
    rel = abs(c["vq_loss"] - c["vq64"]) / c["vq64"]
    print("  %s: pre-quantisation encoding err %.2e, probabilities err %.2e (bar %.0e), vq_loss %.8g (float64 %.8g, relative %.1e, bar %.0e)"
          % (name, e_e, e_p, PROB_TOL, c["vq_loss"], c["vq64"], rel, VQ_LOSS_RTOL))
    assert c["probs"].shape == (B * W, Q) and e_e < 1e-4 and e_p <= PROB_TOL and rel <= VQ_LOSS_RTOL
    assert abs(c["loss"] - c["l64"]) < 1e-4
    # ---- usage statistics: per stage; mse is the LAST stage's, the error of q against e
    st = c["stats"]
    assert np.array_equal(st.counts.cpu().numpy(), f["counts"])
    assert np.array_equal(st.stage_codes_used.cpu().numpy(), (f["counts"] > 0).sum(1)) and int(st.codes_used) == (f["counts"][0] > 0).sum()
    mse = st.stage_mse.cpu().numpy().astype(np.float64)
    assert mse.shape == (S,) and (np.abs(mse - f["mse"]) <= 1e-5 * f["mse"]).all() and float(st.mse) == float(st.stage_mse[-1])
    err_q = float(((c["q"] - c["e"]).double() ** 2).mean())
    assert abs(float(st.mse) - err_q) <= 1e-5 * err_q
    ppl = st.stage_perplexity.cpu().numpy()
    assert all(abs(ppl[s] - vq_ref.perplexity(f["counts"][s])) <= 1e-5 * ppl[s] for s in range(S)) and float(st.perplexity) == float(ppl[0])
    assert abs(float(mse.sum()) * (1 + BETA) - c["vq_loss"]) <= 1e-6 * c["vq_loss"]
    # ---- gradients
    _grads_close(name, c["grads"], c["g64"])
    g_cb = c["grads"]["vq_codebook.weight"]
    unused = torch.from_numpy((f["counts"] == 0).reshape(-1)).to(g_cb.device)
    assert bool((g_cb[unused] == 0).all()) and bool((g_cb[~unused].abs().amax(1) > 0).all())


@pytest.mark.parametrize("name", ["fast64", "pair32", "general"])
def test_autograd_gives_the_fused_steps_gradients(name):
    """criterion(net(x), t) + net.vq_loss against engine.loss_and_grad: on the fast engine the same BITS (the general plan's module
    surface takes torch's loss kernels: within the bar, the rule of tests/test_gpu_vq_model.py)."""
    c = _case(name)
    eng, x, target = c["eng"], c["x"], c["target"]
    loss = eng.loss_and_grad(x, target)
    g1 = eng.flat_grad.clone()
    assert abs(float(loss) - c["l64"]) < 1e-4
    fused = _named(eng, g1)
    _grads_close(name + " fused", fused, c["g64"])
    gmax = max(float(r.abs().max()) for r in c["g64"].values())
    for n, g in c["grads"].items():
        if name == "general":
            assert float((fused[n] - g).abs().max()) <= 2 * GRAD_RTOL * max(float(c["g64"][n].abs().max()), 1e-3 * gmax), n
        else:
            assert torch.equal(fused[n], g), n
    assert abs(float(eng.last_vq.vq_loss) - c["vq_loss"]) == 0.0
    eng.loss_and_grad(x, target, None)                                             # determinism: the same bits again
    assert torch.equal(g1, eng.flat_grad)


def _snapshot(net):
    return dict(cb=net.vq_codebook.weight.detach().cpu().numpy().copy(), state=net.vq_ema_state.cpu().numpy().reshape(S, -1).copy())


def _stage(snap, s):
    return dict(cb=snap["cb"][s * K:(s + 1) * K], state=snap["state"][s])


@pytest.mark.parametrize("name", ["fast64", "general"])
def test_ema_mode_three_training_steps_follow_the_float64_rule_per_stage(name):
    net, cfg, B, x, target = build_cpu(name, vq_update="ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    net.reset_vq_ema_state()
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    eng = net._engine_for(x.device)
    assert eng.vq_ema and eng.vq_S == S
    eng.adam_init(lr=1e-3, skip_nonfinite=True)
    keep = torch.ones(eng.spec.total, dtype=torch.bool, device=x.device)
    keep[eng.vq_off:eng.vq_off + eng.n_vq] = False
    restarted = 0
    for step in range(3):
        eng.loss_and_grad(x, target)
        ws = eng.workspace(B, x.shape[2])
        assert bool((eng.flat_grad[~keep] == 0).all()) and bool((eng.flat_grad[keep] != 0).any())
        # the stat the backward left: per stage the counts of the forward and the sums of ITS input's frames
        stat = eng.vq_stat.cpu().numpy().reshape(S, -1)
        r_in = torch.cat([ws["enc_pre"][None], ws["vq_res"][:-1]]).cpu().numpy()
        idx = ws["vq_idx"].cpu().numpy()
        for s in range(S):
            n, sums = er.split(stat[s], K)
            assert np.array_equal(n, eng.last_vq.counts[s].cpu().numpy()) and n.sum() == B * ws["Le"]
            _, s64 = er.split(er.stats(r_in[s], idx[s], K), K)
            mag = np.zeros_like(s64)
            np.add.at(mag, idx[s].reshape(-1), np.abs(r_in[s].astype(np.float64)).transpose(0, 2, 1).reshape(-1, r_in[s].shape[1]))
            assert (np.abs(sums - s64) <= (n.max() + 1) * U * mag).all()
        before = _snapshot(net)
        eng.adam_step()
        after = _snapshot(net)
        for s in range(S):
            ref = check_update(_stage(before, s), _stage(after, s), stat[s], K, DECAY, EPS, RESTART, "%s step %d stage %d" % (name, step, s), False)
            restarted += ref["restarted"]
        assert bool((eng.adam_state["m"][~keep] == 0).all())
    assert restarted > 0 and eng.vq_restarted() == restarted and eng.vq_restarted() == 0


def test_a_checkpoint_resumes_bit_for_bit_and_another_stage_count_is_refused(tmp_path):
    from music_amd import train as wtrain
    from music_amd.ae_train import load_model, save_model
    from music_amd.model1 import wavenet_autoencoder
    kw = dict(vq_update="ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    net, cfg, B, x, target = build_cpu("fast64_bias", **kw)
    net.reset_vq_ema_state()
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    eng = net._engine_for(x.device)
    init = dict(lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    eng.adam_init(**init)
    eng.loss_and_grad(x, target)
    eng.adam_step()
    path = str(tmp_path) + "/"
    save_model(net, 1, path)
    torch.save(wtrain._optimizer_state(None, eng), path + "wavenet_autoencoder1.opt")
    assert list(net.state_dict())[-2:] == ["vq_codebook.weight", "vq_ema_state"]
    twin = load_model(wavenet_autoencoder(**cfg), path, "wavenet_autoencoder1.model").cuda()
    assert torch.equal(twin.vq_ema_state, net.vq_ema_state)
    with torch.no_grad():
        assert torch.equal(twin(x), net(x)) and torch.equal(twin.vq_codes, net.vq_codes) and twin.vq_codes.shape[1] == S
    with pytest.raises(RuntimeError, match="vq_stages"):
        load_model(wavenet_autoencoder(**dict(cfg, vq_stages=2)), path, "wavenet_autoencoder1.model")
    teng = twin._engine_for(x.device)
    teng.adam_init(**init)
    assert wtrain._restore_optimizer_state(path + "wavenet_autoencoder1.opt", None, lambda: teng) is teng
    for e in (eng, teng):
        e.loss_and_grad(x, target)
        e.adam_step()
    assert torch.equal(eng.flat_grad, teng.flat_grad) and torch.equal(eng.flat, teng.flat) and torch.equal(eng.vq_stat, teng.vq_stat)
    assert torch.equal(net.vq_ema_state, twin.vq_ema_state)
    assert torch.equal(eng.adam_state["m"], teng.adam_state["m"]) and torch.equal(eng.adam_state["v"], teng.adam_state["v"])
