"""CPU checks of `conditioning="learned"` on the module surface of music_amd/model1.py (the constructor needs no device): what is
registered and in which order, what a seed gives in both modes, pickling, the JSON key, conditioning_projections(), cross-mode
checkpoints - and, through the recorder of tests/launch_trace.py, what a learned step LAUNCHES against the random step of the
same case.  No device is touched."""
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
N, DD, SD, BW = 3, 20, 40, 12


def _net(seed=5, **kw):
    from music_amd.model1 import wavenet_autoencoder
    torch.manual_seed(seed)
    return wavenet_autoencoder(**dict(CFG, **kw))


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("kw", [{}, {"conditioning": "random"}])
def test_default_and_random_are_the_model_without_the_keyword(kw):
    from music_amd.model1 import wavenet_autoencoder
    torch.manual_seed(5)
    parent = wavenet_autoencoder(*[CFG[k] for k in ("filter_width", "quantization_channel", "dilations", "en_residual_channel",
                                                     "en_dilation_channel", "en_bottleneck_width", "en_pool_kernel_size",
                                                     "de_residual_channel", "de_dilation_channel", "de_skip_channel", "use_bias")])
    rng_parent = torch.get_rng_state()
    net = _net(**kw)
    assert torch.equal(torch.get_rng_state(), rng_parent)                       # the same RNG consumption
    a, b = parent.state_dict(), net.state_dict()
    assert list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    assert net.conditioning == "random" and not hasattr(net, "de_cond_layer_stack")


@pytest.mark.parametrize("use_bias", [False, True])
def test_learned_registers_the_projections_behind_everything_else(use_bias):
    rnd, net = _net(use_bias=use_bias), _net(use_bias=use_bias, conditioning="learned")
    a, b = rnd.state_dict(), net.state_dict()
    keys = list(b)
    assert keys[:len(a)] == list(a) and all(_equal(a[k], b[k]) for k in a)
    more = keys[len(a):]
    want = [("de_cond_layer_stack.%d.%s" % (i, p), (2 * DD, BW, 1) if p == "weight" else (2 * DD,)) for i in range(N)
            for p in ("weight", "bias")]
    want += [("connection_cond.weight", (SD, BW, 1)), ("connection_cond.bias", (SD,))]
    assert len(more) == 2 * (N + 1) and [(k, tuple(b[k].shape)) for k in more] == want
    assert [n for n, _ in net.named_parameters()] == keys                         # ... and they are parameters, in that order
    assert isinstance(net.de_cond_layer_stack, torch.nn.ModuleList) and isinstance(net.connection_cond, torch.nn.Conv1d)


def test_a_bad_value_is_refused():
    with pytest.raises(ValueError, match="conditioning"):
        _net(conditioning="trained")
    with pytest.raises(ValueError, match="conditioning"):
        _net(conditioning=None)


def test_deepcopy_pickle_and_the_json_key():
    from music_amd.model1 import wavenet_autoencoder
    net = _net(conditioning="learned")
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert twin.conditioning == "learned" and twin._engine is None
        a, b = net.state_dict(), twin.state_dict()
        assert list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(net.parameters(), twin.parameters()))
    # a module pickled before the attribute existed is a random-mode one
    old = _net()
    state = old.__getstate__()
    del state["conditioning"]
    bare = wavenet_autoencoder.__new__(wavenet_autoencoder)
    bare.__setstate__(state)
    assert bare.conditioning == "random" and len(bare.conditioning_projections()) == N + 1
    via_json = wavenet_autoencoder(**json.loads(json.dumps(dict(CFG, conditioning="learned"))))
    assert via_json.conditioning == "learned" and len(list(via_json.parameters())) == len(list(net.parameters()))


def test_conditioning_projections():
    net = _net(conditioning="learned")
    before = torch.get_rng_state()
    proj = net.conditioning_projections()
    assert torch.equal(torch.get_rng_state(), before)                             # nothing is drawn
    mods = list(net.de_cond_layer_stack) + [net.connection_cond]
    assert len(proj) == N + 1
    for (w, b), m in zip(proj, mods):
        assert _equal(w, m.weight.detach()) and _equal(b, m.bias.detach()) and not w.requires_grad and not b.requires_grad
    assert net.engine_cond() is None
    with pytest.raises(ValueError, match="learned"):
        net.engine_cond(proj)
    rnd = _net()
    torch.manual_seed(11)
    drawn = rnd._draw_conditioning()
    torch.manual_seed(11)
    again = rnd.conditioning_projections()
    assert all(_equal(w0, w1) and _equal(b0, b1) for (w0, b0), (w1, b1) in zip(drawn, again))
    torch.manual_seed(11)
    assert all(_equal(w0, w1) for (w0, _), (w1, _) in zip(drawn, rnd.engine_cond()))
    assert rnd.engine_cond(drawn) is drawn
    # the generation entry points refuse a list on a learned model before any work
    from music_amd.ae_generate import generate_cached, resynthesize
    piece = torch.zeros(1, 256, net.receptive_field + 10)
    with pytest.raises(ValueError, match="learned"):
        generate_cached(net, piece, 4, cond=proj)


def test_a_checkpoint_of_the_other_mode_is_refused_whole(tmp_path):
    from music_amd.ae_train import load_model, save_model
    rnd, net = _net(seed=1), _net(seed=2, conditioning="learned")
    save_model(rnd, 1, str(tmp_path) + "/")
    save_model(net, 2, str(tmp_path) + "/")
    for model, name, saved in ((net, "wavenet_autoencoder1.model", "random"), (rnd, "wavenet_autoencoder2.model", "learned")):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError) as err:
            load_model(model, str(tmp_path) + "/", name)
        msg = str(err.value)
        assert "conditioning" in msg and '"%s"' % saved in msg and '"%s"' % model.conditioning in msg
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)              # nothing was loaded
    # ... and its own mode loads, "module." prefix included
    twin = _net(seed=3, conditioning="learned")
    assert load_model(twin, str(tmp_path) + "/", "wavenet_autoencoder2.model") is twin
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    torch.save({"module." + k: v.clone() for k, v in net.state_dict().items()}, str(tmp_path) + "/wavenet_autoencoder3.model")
    third = _net(seed=4, conditioning="learned")
    assert load_model(third, str(tmp_path) + "/", "wavenet_autoencoder3.model") is third
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), third.state_dict().values()))


def test_the_engines_refuse_the_wrong_cond(monkeypatch):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    lt.install(monkeypatch)
    x = lt.on_device(torch.zeros(2, 256, lt.AE_T))
    learned = _AutoencoderEngine(_ae_net(64, 64, conditioning="learned"), torch.device("cpu"))
    random = _AutoencoderEngine(_ae_net(64, 64), torch.device("cpu"))
    assert learned.learned and learned.n_cond == sum(p.numel() for n, p in learned.net.named_parameters() if "cond" in n)
    assert not random.learned and random.n_cond == 0 and random.n_gather == random.spec.total
    with pytest.raises(ValueError, match="learned"):
        learned.forward(x, random.net._draw_conditioning())
    with pytest.raises(ValueError, match="random"):
        random.forward(x)
    with pytest.raises(ValueError, match="random"):
        random.loss_and_grad(x, None, None)
    gen = GenericAutoencoderEngine(_ae_net(64, 64, conditioning="learned", filter_width=3), torch.device("cpu"))
    assert gen.learned and gen.n_gather == gen.spec.total - gen.n_cond
    with pytest.raises(ValueError, match="learned"):
        gen.forward(lt.on_device(torch.zeros(2, 256, 600)), random.net._draw_conditioning())


NEW = ("wn_cond_proj_fwd", "wn_cond_proj_bwd")


@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (32, 32, 2, {}), (32, 32, 3, {}), (64, 64, 2, {"use_bias": True}),
                                        (64, 64, 2, {"en_pool_kernel_size": 8})])
def test_a_learned_step_launches_the_new_entries_and_nothing_else_new(en, de, B, kw, monkeypatch):
    """The fused step of a learned model against the random model of the same case: one wn_cond_proj_fwd and one wn_cond_proj_bwd,
    no staging of drawn projections, and otherwise a subset of the random step's launches, in its order."""
    from music_amd.model1 import _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    staged = []
    stub = _AutoencoderEngine._stage_cond
    monkeypatch.setattr(_AutoencoderEngine, "_stage_cond", lambda self, cond: staged.append(1) or stub(self, cond))
    x, W = lt.on_device(torch.zeros(B, 256, lt.AE_T)), None
    names = {}
    for mode in ("random", "learned"):
        net = _ae_net(en, de, conditioning=mode, **kw)
        eng = _AutoencoderEngine(net, torch.device("cpu"))
        target = lt.on_device(torch.zeros(B * (lt.AE_T - eng.rf + 1), dtype=torch.int64))
        del trace[:], staged[:]
        eng.loss_and_grad(x, target, net.engine_cond())
        names[mode] = [item[0] for item in trace if item[0] not in ("record", "wait", "mark")]
        assert len(staged) == (1 if mode == "random" else 0)
        calls = {item[0]: item[1] for item in trace if item[0] in NEW}
        if mode == "learned":
            ws = eng._ws.peek(B, lt.AE_T)
            fwd, bwd = calls["wn_cond_proj_fwd"], calls["wn_cond_proj_bwd"]
            # the offsets are the parameters', the tables are the ones the blocks read, the pair flag is the workspace's
            assert tuple(fwd[2:7]) == eng.cond_off == tuple(bwd[5:10])
            assert eng.cond_off[0] == eng.spec.off["de_cond_layer_stack.0.weight"] == eng.n_gather
            assert bwd[1] == (1 if ws["pair"] else 0) and (fwd[8] is not None) == bool(ws["pair"])
            assert fwd[10:17] == bwd[12:19] == (eng.N, eng.Dd, eng.CHd, eng.Sd, eng.Bw, ws["Le"], B)
            gathers = [item[1] for item in trace if item[0] in ("wn_gather_grads", "wn_gather_grads2") and item[1][-2] == eng.n_gather]
            assert len(gathers) == 1                       # the gradient gather stops in front of the projections' gradients
    assert names["learned"].count(NEW[0]) == 1 and names["learned"].count(NEW[1]) == 1
    assert not any(n in names["random"] for n in NEW)
    rest = [n for n in names["learned"] if n not in NEW]
    it = iter(names["random"])
    assert all(n in it for n in rest), "a learned step launches something the random step of the same case does not"
