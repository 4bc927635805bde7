"""`vq_update="ema"` on the device (music_amd/model1.py, music_amd/engine_base.py, wn_vq_bwd_stats / wn_vq_ema_update), on the case
table and sizes of tests/test_gpu_vq_model.py with K = 32: an ema-mode and a gradient-mode model from one seed give the same
gradients outside the codebook's rows, bit for bit, and exactly 0 in them; the loss is reconstruction + beta mse; the step leaves
codebook and running state where tests/vq_ema_ref.py puts them from the device's own stat (the bounds of
tests/test_gpu_vq_ema_kernels.py) and Adam's moments of the codebook at 0; the module surface with a flat optimizer gives the fused
step's bits; a skipped step changes nothing; the EMA shadow follows the UPDATED codebook; a collapsed codebook comes back with
vq_restart and does not without; a checkpoint resumes bit for bit.  Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import vq_ema_ref as er
from tests.test_gpu_cond_learned import CASES, DIL, W, _cfg
from tests.test_gpu_vq_ema_kernels import U, check_update
from tests.test_gpu_vq_model import B_INIT, BETA, K, SEEDS, _codes_batch

DECAY, EPS, RESTART = 0.9, 1e-5, 0.95          # an unused code's usage after one step is 0.9: dead at once, restarts in every step


def build(name, update, init="data", seed=70, **kw):
    """The case's vq model (tests/test_gpu_vq_model.build_cpu: the same seeds, so the same parameters in both update modes) on the
    device with its batch; init "data": the codebook drawn from the encodings of B_INIT other clips, "uniform": the constructor's."""
    from music_amd.model1 import wavenet_autoencoder
    ckw, B = CASES[name]
    cfg = dict(_cfg(**ckw), bottleneck="vq", vq_codes=K, vq_beta=BETA, vq_update=update, **kw)
    torch.manual_seed(seed + sorted(CASES).index(name))
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.connection_2.weight.mul_(6.0)
    net.reset_vq_ema_state()
    net = net.cuda()
    x, target = _codes_batch(cfg, net.receptive_field, B, SEEDS[name])
    x, target = x.cuda(), target.cuda()
    if init == "data":
        x_init, _ = _codes_batch(cfg, net.receptive_field, B_INIT, 5)
        with torch.no_grad():
            _, _, ws = net._engine_for(x.device).forward(x_init.cuda(), None, want_probs=False, encode_only=True)
        net.init_codebook(ws["enc_pre"], seed=3)
    return net, cfg, B, x, target


def _rows(eng, t):
    return t[eng.vq_off:eng.vq_off + eng.n_vq]


def _snapshot(net, eng):
    return dict(cb=net.vq_codebook.weight.detach().cpu().numpy().copy(), state=net.vq_ema_state.cpu().numpy().copy())


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_loss_and_one_adam_step_against_the_gradient_model_and_float64(name):
    ema_kw = dict(vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    gnet, _, B, x, target = build(name, "gradient")
    net, cfg, _, _, _ = build(name, "ema", **ema_kw)
    assert torch.equal(gnet.vq_codebook.weight, net.vq_codebook.weight)
    geng, eng = gnet._engine_for(x.device), net._engine_for(x.device)
    assert eng.vq_ema and not geng.vq_ema
    gloss, loss = geng.loss_and_grad(x, target), eng.loss_and_grad(x, target)
    T = x.shape[2]
    gws, ws = geng.workspace(B, T), eng.workspace(B, T)
    # ---- gradients: the gradient model's bits outside the codebook's rows, exactly 0 in them
    keep = torch.ones(eng.spec.total, dtype=torch.bool, device=x.device)
    _rows(eng, keep).fill_(False)
    assert torch.equal(eng.flat_grad[keep], geng.flat_grad[keep])
    assert bool((_rows(eng, eng.flat_grad) == 0).all()) and bool((_rows(geng, geng.flat_grad) != 0).any())
    # ---- loss = reconstruction + beta mse (the gradient model's: reconstruction + (1 + beta) mse, from the same partial sums)
    assert torch.equal(ws["loss_part"], gws["loss_part"]) and torch.equal(ws["vq_part"], gws["vq_part"])
    recon, mse = float(ws["loss_part"].double().sum()), float(ws["vq_part"].double().sum())
    print("  %s: reconstruction %.6f, mse %.6f, loss %.6f (gradient mode %.6f)" % (name, recon, mse, float(loss), float(gloss)))
    # (fp32 tree sums over 1024 and 256 positive partials round at most 10 times each, then one product and one sum: 16 u)
    assert abs(float(loss) - (recon + BETA * mse)) <= 16 * U * (recon + mse)
    assert abs(float(gloss) - (recon + (1 + BETA) * mse)) <= 16 * U * (recon + 2 * mse)
    assert abs(float(eng.last_vq.vq_loss) - BETA * mse) <= 16 * U * mse
    # ---- the stat the backward left: the counts of the forward, the sums of ITS frames
    stat = eng.vq_stat.cpu().numpy()
    n, s = er.split(stat, K)
    enc, idx = ws["enc_pre"].cpu().numpy(), ws["vq_idx"].cpu().numpy()
    assert np.array_equal(n, eng.last_vq.counts.cpu().numpy()) and n.sum() == idx.size
    _, s64 = er.split(er.stats(enc, idx, K), K)
    mag = np.zeros_like(s64)
    np.add.at(mag, idx.reshape(-1), np.abs(enc.astype(np.float64)).transpose(0, 2, 1).reshape(-1, enc.shape[1]))
    assert (np.abs(s - s64) <= (n.max() + 1) * U * mag).all()
    # ---- one Adam step: codebook and state where the rule puts them from that stat, Adam's moments of the codebook untouched
    eng.adam_init(lr=1e-3)
    before = _snapshot(net, eng)
    eng.adam_step()
    after = _snapshot(net, eng)
    ref = check_update(before, after, stat, K, DECAY, EPS, RESTART, name, False)
    assert ref["restarted"] + ref["left"] == int((n == 0).sum()) and (n > 0).sum() >= 3
    assert bool((_rows(eng, eng.adam_state["m"]) == 0).all()) and bool((_rows(eng, eng.adam_state["v"]) == 0).all())
    assert bool((eng.adam_state["m"][keep] != 0).any())
    assert int(eng.vq_ema_info[0]) == ref["restarted"] and eng.vq_restarted() == ref["restarted"] and eng.vq_restarted() == 0


@pytest.mark.parametrize("name", ["fast64", "pair32"])
@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_the_module_surface_gives_the_fused_steps_bits(name, kind):
    """criterion(net(x), t) + net.vq_loss, backward, get_optimizer(...).step(), twice.  Adam: parameters and running state have the
    bits of loss_and_grad + adam_step on a twin.  Every flat optimizer: its step ends with the update - codebook and state are
    where the rule puts them from the state in front of the step and the stat of this backward - and its own state of the
    codebook's rows stays 0."""
    from music_amd import train
    ema_kw = dict(vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    net, _, B, x, target = build(name, "ema", **ema_kw)
    opt = train.get_optimizer(net, kind, 1e-3, 0.9)
    crit = torch.nn.CrossEntropyLoss()
    if kind == "adam":
        twin, _, _, _, _ = build(name, "ema", **ema_kw)
        teng = twin._engine_for(x.device)
        teng.adam_init(lr=1e-3)
    for step in range(2):
        opt.zero_grad()
        (crit(net(x), target) + net.vq_loss).backward()
        eng = net._engine
        before = _snapshot(net, eng)
        opt.step()
        check_update(before, _snapshot(net, eng), eng.vq_stat.cpu().numpy(), K, DECAY, EPS, RESTART, "%s %s step %d" % (name, kind, step), False)
        if kind == "adam":
            teng.loss_and_grad(x, target)
            teng.adam_step()
            assert torch.equal(eng.vq_stat, teng.vq_stat)
            assert torch.equal(eng.flat, teng.flat) and torch.equal(net.vq_ema_state, twin.vq_ema_state), "step %d" % step
    st = opt.state[net.vq_codebook.weight]
    seen = [key for key in ("exp_avg", "exp_avg_sq", "momentum_buffer", "square_avg") if st.get(key) is not None]
    assert seen and all(bool((st[key] == 0).all()) for key in seen), seen


def test_a_skipped_step_leaves_codebook_state_and_counters_bit_for_bit():
    net, _, B, x, target = build("fast64", "ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    eng = net._engine_for(x.device)
    eng.adam_init(lr=1e-3, skip_nonfinite=True, ema_decay=0.9)
    eng.loss_and_grad(x, target)
    eng.adam_step()                                          # a taken step first: counters and state are no longer the initial ones
    assert eng.guard_report()["taken"] == 1 and int(eng.vq_ema_info[0]) > 0
    eng.loss_and_grad(x, target)
    eng.flat_grad[eng.spec.total // 3] = float("inf")
    keep = [t.clone() for t in (eng.flat, net.vq_ema_state, eng.vq_ema_info, eng.ema.flat, eng.adam_state["m"])]
    eng.adam_step()
    rep = eng.guard_report()
    assert rep["taken"] == 1 and rep["skipped"] == 1
    for a, b in zip(keep, (eng.flat, net.vq_ema_state, eng.vq_ema_info, eng.ema.flat, eng.adam_state["m"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    eng.loss_and_grad(x, target)                             # ... and the next finite step is taken again
    eng.adam_step()
    assert eng.guard_report()["taken"] == 2 and not torch.equal(keep[1], net.vq_ema_state)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_the_shadow_follows_the_updated_codebook(guarded):
    from music_amd import ema
    net, _, B, x, target = build("fast64", "ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    eng = net._engine_for(x.device)
    eng.adam_init(lr=1e-3, ema_decay=0.75, skip_nonfinite=guarded)
    old = _rows(eng, eng.flat).double().cpu()
    shadow0 = _rows(eng, eng.ema.flat).double().cpu()
    assert torch.equal(old, shadow0)
    eng.loss_and_grad(x, target)
    eng.adam_step()
    new = _rows(eng, eng.flat).double().cpu()
    got = _rows(eng, eng.ema.flat).double().cpu()
    w = ema.weight(0.75, False, 1)
    want = shadow0 + w * (new - shadow0)
    moved = (new - old).abs().max()
    err = (got - want).abs().max()
    print("  shadow: the codebook moved by %.3e, shadow against the lerp to the updated rows %.3e" % (moved, err))
    assert moved > 1e-3 * new.abs().max() and bool(((got - want).abs() <= 4 * U * (shadow0.abs() + new.abs())).all())
    assert (got - shadow0).abs().max() > 0.2 * moved         # (towards the OLD codebook the shadow would not have moved at all)


@pytest.mark.parametrize("name", ["fast64", "long_encoding"])
def test_a_collapsed_codebook_comes_back_with_restarts_and_not_without(name):
    """A batch of identical clips on the constructor's codebook (rows within 1 / K of the origin, the encodings far outside), three
    steps, then one more forward.  Without restarts the codes in use only ever shrink - fast64's 8 frames per clip sit on ONE code
    after the first step and stay there; with restarts dead codes take the batch means of the most used codes' frames in every
    step, the frames split, and more codes are in use than without: more than one.
    The rule in float64 on the oracle's encodings (encoder frozen) gives 3, 1, 1, 1 | 3, 3, 4, 4 codes in the four forwards of
    fast64 without | with restarts and 7, 7, 13, 19 with restarts for the 40 frames of long_encoding, every decision of the last
    forward with a relative margin above 1e-3.  (Where ALL frames sit on one code from the first forward on - the other four cases
    of the table - every restart lands on the same batch mean, the frames move over whole and the next restart duplicates that
    row: exact ties, which go to the smaller index, so one code stays in use.  That is the rule on a batch that never changes,
    not the device: DESIGN.md section 9.)"""
    used = {}
    for restart in (0.0, 0.995):
        net, cfg, B, x, target = build(name, "ema", init="uniform", vq_decay=0.99, vq_eps=1e-5, vq_restart=restart)
        x = x[:1].repeat(B, 1, 1).contiguous()
        eng = net._engine_for(x.device)
        eng.adam_init(lr=1e-4)
        per_step = []
        for _ in range(3):
            eng.loss_and_grad(x, target)
            eng.adam_step()
            per_step.append(int(eng.last_vq.codes_used))
        eng.loss_and_grad(x, target)                         # the codes the model uses AFTER three steps
        per_step.append(int(eng.last_vq.codes_used))
        used[restart] = per_step
        print("  %s, vq_restart %g: codes used in the four forwards %s, restarted %d" % (name, restart, per_step, eng.vq_restarted()))
    assert sorted(used[0.0], reverse=True) == used[0.0], "without restarts no code comes back"
    if name == "fast64":
        assert used[0.0][1:] == [1, 1, 1]                    # collapsed after the first step, and it stays 1
    assert used[0.995][-1] > max(1, used[0.0][-1])


def test_a_checkpoint_resumes_bit_for_bit(tmp_path):
    from music_amd import train as wtrain
    from music_amd.ae_train import load_model, save_model
    from music_amd.model1 import wavenet_autoencoder
    net, cfg, B, x, target = build("fast64_bias", "ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=RESTART)
    eng = net._engine_for(x.device)
    eng.adam_init(lr=1e-3)
    for _ in range(2):
        eng.loss_and_grad(x, target)
        eng.adam_step()
    path = str(tmp_path) + "/"
    save_model(net, 2, path)
    torch.save(wtrain._optimizer_state(None, eng), path + "wavenet_autoencoder2.opt")
    saved = torch.load(path + "wavenet_autoencoder2.model")
    assert list(saved)[-1] == "vq_ema_state" and torch.equal(saved["vq_ema_state"], net.vq_ema_state.cpu())
    assert not torch.equal(saved["vq_ema_state"][:K], torch.ones(K))
    with pytest.raises(RuntimeError, match="vq_update"):
        load_model(wavenet_autoencoder(**dict(cfg, vq_update="gradient")), path, "wavenet_autoencoder2.model")
    twin = load_model(wavenet_autoencoder(**cfg), path, "wavenet_autoencoder2.model").cuda()
    teng = twin._engine_for(x.device)
    teng.adam_init(lr=1e-3)
    assert wtrain._restore_optimizer_state(path + "wavenet_autoencoder2.opt", None, lambda: teng) is teng
    for e in (eng, teng):
        e.loss_and_grad(x, target)
        e.adam_step()
    assert torch.equal(eng.flat, teng.flat) and torch.equal(net.vq_ema_state, twin.vq_ema_state)
    assert torch.equal(eng.vq_stat, teng.vq_stat) and torch.equal(eng.adam_state["m"], teng.adam_state["m"])
