"""CPU checks of `vq_update="ema"` on the module surface of music_amd/model1.py, in the pattern of tests/test_vq_model_cpu.py: the
refusals, what the default mode leaves exactly as it was, the one buffer the ema mode adds and where, init_codebook, cross-mode
checkpoints, pickling, the JSON keys - and, through the recorder of tests/launch_trace.py, what an ema step LAUNCHES against the
gradient step of the same case.  No device is touched."""
import copy
import json
import pickle

import pytest
import torch

from tests import launch_trace as lt
from tests.test_engine_base import _ae_net

CFG = dict(filter_width=2, quantization_channel=256, dilations=[1, 2, 4], en_residual_channel=16, en_dilation_channel=24,
           en_bottleneck_width=12, en_pool_kernel_size=10, de_residual_channel=16, de_dilation_channel=20, de_skip_channel=40,
           use_bias=False)
BW, K = 12, 24
VQ = dict(conditioning="learned", bottleneck="vq", vq_codes=K)
EMA = dict(VQ, vq_update="ema")


def _net(seed=5, **kw):
    from music_amd.model1 import wavenet_autoencoder
    torch.manual_seed(seed)
    return wavenet_autoencoder(**dict(CFG, **kw))


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _initial(net):
    return torch.cat([torch.ones(K), net.vq_codebook.weight.detach().reshape(-1)])


def test_constructor_refusals():
    for bad in ("adam", None, "EMA"):
        with pytest.raises(ValueError, match="vq_update"):
            _net(**dict(VQ, vq_update=bad))
    for kw in ({}, {"conditioning": "learned"}, {"conditioning": "learned", "bottleneck": "continuous"}):
        with pytest.raises(ValueError, match='requires bottleneck="vq"'):
            _net(vq_update="ema", **kw)
    for decay in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="vq_decay"):
            _net(**dict(EMA, vq_decay=decay))
    for eps in (-1e-6, float("nan")):
        with pytest.raises(ValueError, match="vq_eps"):
            _net(**dict(EMA, vq_eps=eps))
    for r in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="vq_restart"):
            _net(**dict(EMA, vq_restart=r))
    net = _net(**EMA)
    assert (net.vq_update, net.vq_decay, net.vq_eps, net.vq_restart) == ("ema", 0.99, 1e-5, 0.0)
    net = _net(**dict(EMA, vq_decay=0.5, vq_eps=0.0, vq_restart=0.75))
    assert (net.vq_decay, net.vq_eps, net.vq_restart) == (0.5, 0.0, 0.75)


def test_the_default_mode_is_the_parents_vq_model_seed_for_seed():
    parent, net = _net(**VQ), _net(**dict(VQ, vq_update="gradient", vq_decay=0.5, vq_eps=3.0, vq_restart=2.0))
    a, b = parent.state_dict(), net.state_dict()
    assert list(a) == list(b) and list(b)[-1] == "vq_codebook.weight" and all(_equal(a[k], b[k]) for k in a)
    assert net.vq_update == parent.vq_update == "gradient" and not hasattr(net, "vq_ema_state") and list(net.buffers()) == []
    # ... and the ema mode consumes no RNG beyond it either: the same parameters, the same generator state behind the constructor
    torch.manual_seed(5)
    _net(**VQ)
    rng = torch.get_rng_state()
    ema = _net(**EMA)
    assert torch.equal(torch.get_rng_state(), rng)
    assert all(_equal(a[k], ema.state_dict()[k]) for k in a)


@pytest.mark.parametrize("use_bias", [False, True])
def test_ema_mode_adds_one_buffer_as_the_last_key(use_bias):
    parent, net = _net(use_bias=use_bias, **VQ), _net(use_bias=use_bias, **EMA)
    a, b = parent.state_dict(), net.state_dict()
    assert list(b)[:-1] == list(a) and list(b)[-1] == "vq_ema_state"
    assert [n for n, _ in net.named_parameters()] == list(a)                      # a buffer: no optimizer sees it
    assert [n for n, _ in net.named_buffers()] == ["vq_ema_state"]
    state = b["vq_ema_state"]
    assert state.dtype == torch.float32 and tuple(state.shape) == (K * (BW + 1),) and not state.requires_grad
    assert torch.equal(state, _initial(net))                                      # [1 | codebook]
    assert list(net.state_dict(prefix="m.")) == ["m." + k for k in b]


def test_init_codebook_and_the_reset_set_the_state_back():
    net = _net(**EMA)
    with torch.no_grad():
        net.vq_ema_state.add_(3.0)
    many = torch.randn(3, BW, 11, generator=torch.Generator().manual_seed(9))
    net.init_codebook(many, seed=4)
    assert torch.equal(net.vq_ema_state, _initial(net)) and float(net.vq_codebook.weight.detach().abs().max()) > 0.5
    with torch.no_grad():
        net.vq_codebook.weight.mul_(2.0)
    ptr = net.vq_ema_state.data_ptr()
    net.reset_vq_ema_state()
    assert torch.equal(net.vq_ema_state, _initial(net)) and net.vq_ema_state.data_ptr() == ptr      # in place
    _net(**VQ).reset_vq_ema_state()                                               # gradient mode: nothing to do


def test_a_checkpoint_of_the_other_update_mode_is_refused_whole(tmp_path):
    from music_amd.ae_train import load_model, save_model
    grad, ema = _net(seed=1, **VQ), _net(seed=2, **EMA)
    save_model(grad, 1, str(tmp_path) + "/")
    save_model(ema, 2, str(tmp_path) + "/")
    for model, name, saved in ((ema, "wavenet_autoencoder1.model", "gradient"), (grad, "wavenet_autoencoder2.model", "ema")):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError) as err:
            load_model(model, str(tmp_path) + "/", name)
        msg = str(err.value)
        assert "vq_update" in msg and '"%s"' % saved in msg and '"%s"' % model.vq_update in msg
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)              # nothing was loaded
    twin = _net(seed=3, **EMA)
    with torch.no_grad():
        ema.vq_ema_state.mul_(1.5)                                                # (a state that is not the initial one travels)
    save_model(ema, 2, str(tmp_path) + "/")
    assert load_model(twin, str(tmp_path) + "/", "wavenet_autoencoder2.model") is twin
    assert list(twin.state_dict()) == list(ema.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(ema.state_dict().values(), twin.state_dict().values()))
    # a continuous checkpoint into an ema model: refused by the bottleneck rule, which comes first
    with pytest.raises(RuntimeError, match="bottleneck"):
        ema.load_state_dict(_net(seed=4, conditioning="learned").state_dict())


def test_deepcopy_pickle_and_a_pickle_from_before_the_attribute():
    from music_amd.model1 import wavenet_autoencoder
    net = _net(**dict(EMA, vq_decay=0.9, vq_restart=0.5))
    with torch.no_grad():
        net.vq_ema_state.mul_(0.75)
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert (twin.vq_update, twin.vq_decay, twin.vq_eps, twin.vq_restart) == ("ema", 0.9, 1e-5, 0.5) and twin._engine is None
        a, b = net.state_dict(), twin.state_dict()
        assert list(a) == list(b) and list(b)[-1] == "vq_ema_state" and all(_equal(a[k], b[k]) for k in a)
        assert twin.vq_ema_state.data_ptr() != net.vq_ema_state.data_ptr()
    old = _net(**VQ)
    state = old.__getstate__()
    for k in ("vq_update", "vq_decay", "vq_eps", "vq_restart"):
        del state[k]
    bare = wavenet_autoencoder.__new__(wavenet_autoencoder)
    bare.__setstate__(state)
    assert bare.vq_update == "gradient" and bare.bottleneck == "vq"
    bare.load_state_dict(old.state_dict())                                        # ... and behaves as one


def test_the_json_keys_parse():
    from music_amd.model1 import wavenet_autoencoder
    params = json.loads(json.dumps(dict(CFG, **dict(EMA, vq_decay=0.95, vq_eps=1e-4, vq_restart=0.01))))
    net = wavenet_autoencoder(**params)
    assert (net.vq_update, net.vq_decay, net.vq_eps, net.vq_restart) == ("ema", 0.95, 1e-4, 0.01)
    assert wavenet_autoencoder(**json.loads(json.dumps(dict(CFG, **dict(VQ, vq_update="gradient"))))).vq_update == "gradient"


def _step_trace(trace, Engine, en, de, B, kw, update, guarded):
    from music_amd.ae_generic import GenericAutoencoderEngine
    T = 600 if Engine is GenericAutoencoderEngine else lt.AE_T
    net = _ae_net(en, de, conditioning="learned", bottleneck="vq", vq_codes=K, vq_update=update, vq_restart=0.5, **kw)
    eng = Engine(net, torch.device("cpu"))
    eng.adam_init(lr=1e-3, ema_decay=0.999, skip_nonfinite=guarded)
    x = lt.on_device(torch.zeros(B, 256, T))
    target = lt.on_device(torch.zeros(B * (T - eng.rf + 1), dtype=torch.int64))
    del trace[:]
    eng.loss_and_grad(x, target, None)
    eng.adam_step()
    return net, eng, eng._ws.peek(B, T), [item for item in trace if item[0] not in ("record", "wait", "mark")]


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (32, 32, 3, {}), (64, 64, 2, {"filter_width": 3})])
def test_an_ema_step_is_the_gradient_step_with_two_changes(en, de, B, kw, guarded, monkeypatch):
    """The fused step (loss_and_grad + adam_step with an EMA shadow) of an ema model against the gradient model of the same case, on
    both plans: wn_vq_bwd replaced by wn_vq_bwd_stats, wn_vq_ema_update added behind the optimizer's launch and in front of
    wn_ema_flat; every other launch is the gradient step's, in its order."""
    from music_amd import _lib
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    Engine = GenericAutoencoderEngine if kw.get("filter_width", 2) != 2 else _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)                           # (once: the recorder replaces every module's `call`)
    _, geng, _, grad = _step_trace(trace, Engine, en, de, B, kw, "gradient", guarded)
    net, eng, ws, ema = _step_trace(trace, Engine, en, de, B, kw, "ema", guarded)
    g, e = [c[0] for c in grad], [c[0] for c in ema]
    assert not geng.vq_ema and not any(n in g for n in ("wn_vq_bwd_stats", "wn_vq_ema_update")) and not hasattr(geng, "vq_stat")
    assert eng.vq_ema and "wn_vq_bwd" not in e and e.count("wn_vq_bwd_stats") == 1 and e.count("wn_vq_ema_update") == 1
    opt = "wn_adam_flat_guarded" if guarded else "wn_adam_flat"
    i = e.index("wn_vq_ema_update")
    assert e[i - 1] == opt and e[i + 1] == "wn_ema_flat" and i + 2 == len(e)
    want = ["wn_vq_bwd_stats" if n == "wn_vq_bwd" else n for n in g]
    assert e[:i] + e[i + 1:] == want, "an ema step differs from the gradient step beyond its two changes"
    # the arguments: the gradient call's, plus the stat vector; the update on the MODULE's buffer, the engine's scratch and counters
    gb = dict((c[0], c[1]) for c in grad)["wn_vq_bwd"]
    calls = dict((c[0], c[1]) for c in ema)
    sb, up = calls["wn_vq_bwd_stats"], calls["wn_vq_ema_update"]
    Bw, Le = eng.Bw, ws["Le"]
    assert sb[4:7] == gb[4:7] == (eng.vq_off, 0.25, 1.0) and tuple(sb[10:14]) == (K, Bw, Le, B) == tuple(gb[9:13])
    assert sb[0].t is ws["enc_pre"] and sb[1].t is ws["vq_idx"] and sb[2].addr == sb[7].addr and sb[8].t is eng.flat_grad
    assert sb[9].t is eng.vq_stat and eng.vq_stat.numel() == K * (Bw + 1) == net.vq_ema_state.numel()
    assert up[0].t is eng.flat and up[1] == eng.vq_off and up[2].t is eng.vq_stat and up[3].t is net.vq_ema_state
    assert up[4].t is eng.vq_ema_work and eng.vq_ema_work.numel() * 4 == _lib.VQ_EMA_WORK_BYTES and up[5].t is eng.vq_ema_info
    assert tuple(up[6:11]) == (K, Bw, 0.99, 1e-5, 0.5)
    gd = eng.adam_state["guard"]
    assert (up[11] is None) == (not guarded) and (not guarded or up[11] == gd.state_ptr() == calls["wn_ema_flat"][6])
    # the loss is the reconstruction loss + beta mse; the module's figure follows
    assert eng.vq_loss_coef == 0.25 and geng.vq_loss_coef == 1.25 and eng.last_vq.coef == 0.25 and geng.last_vq.coef == 1.25


def test_the_flat_optimizers_end_their_step_with_the_update(monkeypatch):
    """get_optimizer(...).step() on a model whose engine is in ema mode: wn_vq_ema_update behind the optimizer's launch, in front of
    wn_ema_flat - unguarded and guarded, for the three flat optimizers; a gradient-mode model's step launches what it did."""
    from music_amd import train
    from music_amd.model1 import _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    for update in ("gradient", "ema"):
        for kind, entry in (("adam", "wn_adam_flat"), ("sgd", "wn_sgd_flat"), ("rmsprop", "wn_rmsprop_flat")):
            for guarded in (False, True):
                net = _ae_net(64, 64, conditioning="learned", bottleneck="vq", vq_codes=K, vq_update=update)
                eng = net._engine = _AutoencoderEngine(net, torch.device("cpu"))
                named = list(net.named_parameters())
                for n, p in named:                                                # the parameters and gradients as views of the flat buffers
                    o = eng.spec.off[n]
                    p.data = eng.flat[o:o + p.numel()].view(p.shape)
                    p.grad = eng.flat_grad[o:o + p.numel()].view(p.shape)
                opt = train.get_optimizer(net, kind, 1e-3, 0.9, skip_nonfinite=guarded, ema_decay=0.99)
                monkeypatch.setattr(type(opt), "_guard_get", lambda self, device: _FakeGuard(), raising=False)
                del trace[:]
                opt.step()
                names = [item[0] for item in trace if item[0] not in ("record", "wait", "mark")]
                tail = [entry + "_guarded" if guarded else entry] + (["wn_vq_ema_update"] if update == "ema" else []) + ["wn_ema_flat"]
                assert names[-len(tail):] == tail and names.count("wn_vq_ema_update") == (update == "ema"), (update, kind, guarded, names)
                if update == "ema":
                    up = [item[1] for item in trace if item[0] == "wn_vq_ema_update"][0]
                    assert up[3].t is net.vq_ema_state and (up[11] == 4096 if guarded else up[11] is None)


class _FakeGuard:
    """A GradGuard without a device: the launches are recorded, the state block is an address."""
    offset = 0

    def run(self, gptr, n, gscale=1.0):
        pass

    def state_ptr(self):
        return 4096


def test_the_engine_finds_the_modules_buffer_or_says_so():
    from music_amd.model1 import _AutoencoderEngine
    net = _ae_net(64, 64, conditioning="learned", bottleneck="vq", vq_codes=K, vq_update="ema")
    eng = _AutoencoderEngine(net, torch.device("cpu"))
    assert eng.vq_ema_state() is net.vq_ema_state
    del net._buffers["vq_ema_state"]
    with pytest.raises(RuntimeError, match="vq_ema_state"):
        eng.vq_ema_state()
