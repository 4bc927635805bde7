"""CPU checks of `bottleneck="vq"` on the module surface of music_amd/model1.py (the constructor needs no device): the refusals,
what is registered and where, what a seed gives in both modes, cross-mode checkpoints, pickling, init_codebook, the JSON keys -
and, through the recorder of tests/launch_trace.py, what a vq step LAUNCHES against the continuous step of the same case.
No device is touched."""
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


def _net(seed=5, **kw):
    from music_amd.model1 import wavenet_autoencoder
    torch.manual_seed(seed)
    return wavenet_autoencoder(**dict(CFG, **kw))


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="bottleneck"):
        _net(conditioning="learned", bottleneck="quantised")
    with pytest.raises(ValueError, match="bottleneck"):
        _net(conditioning="learned", bottleneck=None)
    for kw in ({}, {"conditioning": "random"}):
        with pytest.raises(ValueError, match='requires conditioning="learned"'):
            _net(bottleneck="vq", **kw)
    for codes in (1, 0, 1025):
        with pytest.raises(ValueError, match="vq_codes"):
            _net(**dict(VQ, vq_codes=codes))
    with pytest.raises(ValueError, match="en_bottleneck_width"):
        _net(**dict(VQ, en_bottleneck_width=513))
    with pytest.raises(ValueError, match="vq_beta"):
        _net(**dict(VQ, vq_beta=-0.5))
    assert _net().bottleneck == "continuous" and _net(conditioning="learned", bottleneck="continuous").bottleneck == "continuous"
    # the limits themselves
    assert _net(**dict(VQ, vq_codes=2)).vq_codebook.weight.shape == (2, BW)
    assert _net(**dict(VQ, vq_codes=1024, en_bottleneck_width=512)).vq_codebook.weight.shape == (1024, 512)


@pytest.mark.parametrize("use_bias", [False, True])
def test_the_codebook_is_the_last_parameter_and_a_seed_gives_the_rest_unchanged(use_bias):
    cont, net = _net(use_bias=use_bias, conditioning="learned"), _net(use_bias=use_bias, **VQ)
    a, b = cont.state_dict(), net.state_dict()
    keys = list(b)
    assert keys[:-1] == list(a) and keys[-1] == "vq_codebook.weight"
    assert all(_equal(a[k], b[k]) for k in a)                                     # every earlier parameter: bit-equal
    assert [n for n, _ in net.named_parameters()] == keys
    assert isinstance(net.vq_codebook, torch.nn.Embedding) and net.vq_codebook.weight.requires_grad
    w = net.vq_codebook.weight.detach()
    assert tuple(w.shape) == (K, BW)
    assert float(w.abs().max()) <= 1.0 / K and float(w.abs().max()) > 0.5 / K and float(w.min()) < 0 < float(w.max())
    assert net.vq_beta == 0.25 and _net(**dict(VQ, vq_beta=1.5)).vq_beta == 1.5
    assert net.vq_loss is None and net.vq_codes is None and net.last_encoding_pre is None
    # "continuous" consumes no RNG beyond the parent's
    torch.manual_seed(5)
    _net(conditioning="learned")
    rng = torch.get_rng_state()
    _net(conditioning="learned", bottleneck="continuous", vq_codes=77, vq_beta=3.0)
    assert torch.equal(torch.get_rng_state(), rng)


def test_a_checkpoint_of_the_other_mode_is_refused_whole(tmp_path):
    from music_amd.ae_train import load_model, save_model
    cont, net = _net(seed=1, conditioning="learned"), _net(seed=2, **VQ)
    save_model(cont, 1, str(tmp_path) + "/")
    save_model(net, 2, str(tmp_path) + "/")
    for model, name, saved in ((net, "wavenet_autoencoder1.model", "continuous"), (cont, "wavenet_autoencoder2.model", "vq")):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError) as err:
            load_model(model, str(tmp_path) + "/", name)
        msg = str(err.value)
        assert "bottleneck" in msg and '"%s"' % saved in msg and '"%s"' % model.bottleneck in msg
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)              # nothing was loaded
    twin = _net(seed=3, **VQ)
    assert load_model(twin, str(tmp_path) + "/", "wavenet_autoencoder2.model") is twin
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    # a random-conditioning checkpoint into a vq model: refused by the conditioning rule, which comes first
    with pytest.raises(RuntimeError, match="conditioning"):
        net.load_state_dict(_net(seed=4).state_dict())


def test_deepcopy_pickle_and_a_pickle_from_before_the_attribute():
    from music_amd.model1 import wavenet_autoencoder
    net = _net(**VQ)
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert twin.bottleneck == "vq" and twin.vq_beta == net.vq_beta and twin._engine is None
        a, b = net.state_dict(), twin.state_dict()
        assert list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    # what a forward leaves on the module does not travel: vq_loss hangs on an autograd graph, last_vq on the engine's buffers
    net.vq_loss = (net.vq_codebook.weight * 2.0).sum()
    net.last_vq = object()
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert twin.vq_loss is None and twin.last_vq is None and twin.bottleneck == "vq"
    old = _net(conditioning="learned")
    state = old.__getstate__()
    for k in ("bottleneck", "vq_num_codes", "vq_beta", "vq_loss", "vq_codes", "last_encoding_pre", "last_vq"):
        del state[k]
    bare = wavenet_autoencoder.__new__(wavenet_autoencoder)
    bare.__setstate__(state)
    assert bare.bottleneck == "continuous" and bare.conditioning == "learned" and bare.vq_loss is None
    bare.load_state_dict(old.state_dict())                                        # ... and behaves as one


def test_init_codebook_is_seeded_cycles_and_draws_without_replacement():
    net = _net(**VQ)
    gen = torch.Generator().manual_seed(9)
    many = torch.randn(3, BW, 11, generator=gen)                                  # 33 frames >= K = 24
    net.init_codebook(many, seed=4)
    first = net.vq_codebook.weight.detach().clone()
    net.init_codebook(many, seed=4)
    assert torch.equal(net.vq_codebook.weight.detach(), first)                    # deterministic
    net.init_codebook(many, seed=5)
    assert not torch.equal(net.vq_codebook.weight.detach(), first)
    frames = many.permute(0, 2, 1).reshape(-1, BW)
    rows = [int((frames == r).all(1).nonzero()[0]) for r in first]                # every code IS a frame ...
    assert len(set(rows)) == K                                                    # ... and no frame twice
    few = torch.randn(1, BW, 5, generator=gen)                                    # 5 frames < K: cycled through
    net.init_codebook(few, seed=1)
    w = net.vq_codebook.weight.detach()
    f5 = few.permute(0, 2, 1).reshape(-1, BW)
    rows = [int((f5 == r).all(1).nonzero()[0]) for r in w]
    assert rows[:5] == rows[5:10] == rows[10:15] and sorted(rows[:5]) == [0, 1, 2, 3, 4]
    assert net.vq_codebook.weight.requires_grad and net.vq_codebook.weight.is_leaf
    with pytest.raises(ValueError, match="init_codebook"):
        net.init_codebook(torch.zeros(1, BW + 1, 4))
    with pytest.raises(ValueError, match="vq"):
        _net(conditioning="learned").init_codebook(many)


def test_the_json_keys_parse():
    from music_amd.model1 import wavenet_autoencoder
    params = json.loads(json.dumps(dict(CFG, conditioning="learned", bottleneck="vq", vq_codes=64, vq_beta=0.5)))
    net = wavenet_autoencoder(**params)
    assert net.bottleneck == "vq" and net.vq_codebook.num_embeddings == 64 and net.vq_beta == 0.5
    assert wavenet_autoencoder(**json.loads(json.dumps(dict(CFG, bottleneck="continuous")))).bottleneck == "continuous"


NEW = ("wn_vq_fwd", "wn_vq_bwd", "wn_vq_lookup")


@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (32, 32, 2, {}), (32, 32, 3, {}), (64, 64, 2, {"use_bias": True}),
                                        (64, 64, 2, {"en_pool_kernel_size": 8}), (64, 64, 2, {"filter_width": 3})])
def test_a_vq_step_launches_the_two_entries_and_nothing_else_new(en, de, B, kw, monkeypatch):
    """The fused step of a vq model against the continuous (learned) model of the same case, on both plans: one wn_vq_fwd between
    wn_avgpool and wn_cond_proj_fwd, one wn_vq_bwd between wn_cond_proj_bwd and wn_avgpool_bwd, everything else the continuous
    step's launches in its order; with the key unset no wn_vq_* entry is ever called."""
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    Engine = GenericAutoencoderEngine if kw.get("filter_width", 2) != 2 else _AutoencoderEngine
    T = 600 if Engine is GenericAutoencoderEngine else lt.AE_T
    x = lt.on_device(torch.zeros(B, 256, T))
    names, calls = {}, {}
    for mode in ("continuous", "vq"):
        net = _ae_net(en, de, conditioning="learned", bottleneck=mode, vq_codes=K, **kw)
        eng = Engine(net, torch.device("cpu"))
        target = lt.on_device(torch.zeros(B * (T - eng.rf + 1), dtype=torch.int64))
        del trace[:]
        eng.loss_and_grad(x, target, None)
        names[mode] = [item[0] for item in trace if item[0] not in ("record", "wait", "mark")]
        calls[mode] = {item[0]: item[1] for item in trace if item[0] in NEW}
        if mode == "vq":
            ws = eng._ws.peek(B, T)
            fwd, bwd = calls["vq"]["wn_vq_fwd"], calls["vq"]["wn_vq_bwd"]
            Le, Bw = ws["Le"], eng.Bw
            assert eng.vq and eng.vq_off == eng.spec.off["vq_codebook.weight"] == eng.spec.total - K * Bw
            assert eng.n_gather == eng.spec.off["de_cond_layer_stack.0.weight"] and eng.n_gather + eng.n_cond + eng.n_vq == eng.spec.total
            assert "vq_codebook.weight" not in eng.gathered_param_names and eng.param_names[-1] == "vq_codebook.weight"
            assert fwd[2] == eng.vq_off == bwd[4] and tuple(fwd[7:11]) == (K, Bw, Le, B) == tuple(bwd[9:13])
            assert (bwd[5], bwd[6]) == (0.25, 1.0)                                   # beta, and the fused step's upstream scalar
            assert fwd[0].t is ws["enc_pre"] is bwd[0].t and fwd[3].t is ws["enc"]   # e in, q out: the tables are built from q
            assert fwd[4].t is ws["vq_idx"] is bwd[1].t and fwd[5].t is ws["vq_counts"] and fwd[6].t is ws["vq_part"]
            assert bwd[2].addr == bwd[7].addr                                        # d_enc written over d_q
            gathers = [item[1] for item in trace if item[0] in ("wn_gather_grads", "wn_gather_grads2") and item[1][-2] == eng.n_gather]
            assert len(gathers) == 1                       # the gradient gather stops in front of projections and codebook
            assert isinstance(eng.last_vq.mse, torch.Tensor)
    assert calls["continuous"] == {} and not any(n.startswith("wn_vq") for n in names["continuous"])
    v = names["vq"]
    assert v.count("wn_vq_fwd") == 1 and v.count("wn_vq_bwd") == 1 and "wn_vq_lookup" not in v
    assert v[v.index("wn_vq_fwd") - 1] == "wn_avgpool" and v[v.index("wn_vq_fwd") + 1] == "wn_cond_proj_fwd"
    assert v[v.index("wn_vq_bwd") - 1] == "wn_cond_proj_bwd" and v[v.index("wn_vq_bwd") + 1] == "wn_avgpool_bwd"
    assert [n for n in v if n not in NEW] == names["continuous"], "a vq step differs from the continuous step beyond its two launches"


def test_the_engines_refuse_vq_without_learned_projections():
    """(the constructor refuses it first; a module whose attribute was set by hand reaches the engine's own check)"""
    from music_amd.model1 import _AutoencoderEngine
    net = _ae_net(64, 64)
    net.bottleneck = "vq"
    with pytest.raises(ValueError, match="learned"):
        _AutoencoderEngine(net, torch.device("cpu"))
