"""CPU checks of global class conditioning (global_classes / global_channels of music_amd.wavenet_autoencoder): with the keys unset
the model is the parent's - keys, values, RNG consumption; set, the new parameters sit behind everything else (the codebook
included, vq_ema_state still the last key); bad values, cross-mode checkpoints and wrong `classes` are refused; and, through the
recorder of tests/launch_trace.py, a global step launches the learned step's sequence with exactly the two entry points exchanged.
No device is touched."""
import copy
import json
import os
import pickle

import pytest
import torch

from tests import launch_trace as lt
from tests.test_cond_learned_cpu import BW, CFG, DD, N, SD, _equal, _net
from tests.test_engine_base import _ae_net

E, NC = 12, 3
LEARNED = dict(conditioning="learned")
VQ_EMA = dict(conditioning="learned", bottleneck="vq", vq_codes=16, vq_update="ema")
GLOBAL = dict(global_classes=NC, global_channels=E)
NEW_KEYS = [("de_gcond_layer_stack.%d.weight" % i, (2 * DD, E, 1)) for i in range(N)] + [("connection_gcond.weight", (SD, E, 1)),
                                                                                       ("global_embedding.weight", (NC, E))]


@pytest.mark.parametrize("base", [LEARNED, VQ_EMA], ids=["learned", "learned_vq_ema"])
def test_the_defaults_are_the_parent_model(base):
    from music_amd.model1 import wavenet_autoencoder
    parent = _net(**base)
    rng_parent = torch.get_rng_state()
    for kw in ({}, dict(global_classes=0, global_channels=0)):
        net = _net(**dict(base, **kw))
        assert torch.equal(torch.get_rng_state(), rng_parent)                   # the same RNG consumption
        a, b = parent.state_dict(), net.state_dict()
        assert list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
        assert net.global_classes == 0 == net.global_channels and not hasattr(net, "global_embedding")
        assert [n for n, _ in net.named_parameters()] == [n for n, _ in parent.named_parameters()]


@pytest.mark.parametrize("base", [LEARNED, VQ_EMA, dict(LEARNED, use_bias=True)], ids=["learned", "learned_vq_ema", "bias"])
def test_the_new_parameters_sit_behind_everything_else(base):
    parent, net = _net(**base), _net(**dict(base, **GLOBAL))
    a, b = parent.state_dict(), net.state_dict()
    pa, pb = [n for n, _ in parent.named_parameters()], [n for n, _ in net.named_parameters()]
    # every parameter the parent has keeps its value and its place; the new ones follow in the issue's order
    assert pb[:len(pa)] == pa and all(_equal(a[k], b[k]) for k in a)
    assert [(k, tuple(b[k].shape)) for k in pb[len(pa):]] == NEW_KEYS
    keys = list(b)
    if "vq_ema_state" in a:
        assert keys[-1] == "vq_ema_state" and keys[:-1] == pb and pb[len(pa) - 1] == "vq_codebook.weight"
    else:
        assert keys == pb
    assert isinstance(net.global_embedding, torch.nn.Embedding) and net.connection_gcond.bias is None
    assert all(m.bias is None for m in net.de_gcond_layer_stack)
    G = net.global_projections()
    assert [tuple(g.shape) for g in G] == [(2 * DD, E)] * N + [(SD, E)] and not any(g.requires_grad for g in G)
    assert all(torch.equal(g, m.weight.detach()[:, :, 0]) for g, m in zip(G, list(net.de_gcond_layer_stack) + [net.connection_gcond]))
    v = net.global_vectors([2, 0, 2])
    assert torch.equal(v, net.global_embedding.weight.detach()[[2, 0, 2]]) and not v.requires_grad
    with pytest.raises(ValueError, match="global_classes"):
        net.global_vectors([0, NC])
    with pytest.raises(ValueError, match="global_classes"):
        parent.global_projections()


def test_bad_values_are_refused_by_name():
    from music_amd import _lib
    for kw, key in ((dict(global_classes=3), "global_channels"), (dict(global_channels=4), "global_classes"),
                    (dict(global_classes=-1, global_channels=4), "global_classes"), (dict(global_classes=3, global_channels=-2), "global_channels"),
                    (dict(global_classes=3.0, global_channels=4), "global_classes"), (dict(global_classes=3, global_channels="4"), "global_channels"),
                    (dict(global_classes=3, global_channels=_lib.GCOND_MAX_CHANNELS + 1), "global_channels")):
        with pytest.raises(ValueError, match=key):
            _net(**dict(LEARNED, **kw))
    with pytest.raises(ValueError, match="learned"):
        _net(**GLOBAL)                                                          # conditioning="random"
    assert _net(**dict(LEARNED, global_classes=1, global_channels=_lib.GCOND_MAX_CHANNELS)).global_channels == 512


def test_deepcopy_pickle_and_the_json_keys():
    from music_amd.model1 import wavenet_autoencoder
    net = _net(**dict(VQ_EMA, **GLOBAL))
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert (twin.global_classes, twin.global_channels) == (NC, E) and twin._engine is None
        a, b = net.state_dict(), twin.state_dict()
        assert list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    # a module pickled before the attributes existed has the mode off
    old = _net(**LEARNED)
    state = old.__getstate__()
    del state["global_classes"], state["global_channels"]
    bare = wavenet_autoencoder.__new__(wavenet_autoencoder)
    bare.__setstate__(state)
    assert bare.global_classes == 0 == bare.global_channels
    via_json = wavenet_autoencoder(**json.loads(json.dumps(dict(CFG, **dict(LEARNED, **GLOBAL)))))
    assert (via_json.global_classes, via_json.global_channels) == (NC, E)


def test_checkpoints_of_another_mode_or_size_are_refused_whole(tmp_path):
    from music_amd.ae_train import load_model, save_model
    nets = {"off": _net(seed=1, **LEARNED), "on": _net(seed=2, **dict(LEARNED, **GLOBAL)),
            "classes": _net(seed=3, **dict(LEARNED, global_classes=NC + 1, global_channels=E)),
            "channels": _net(seed=4, **dict(LEARNED, global_classes=NC, global_channels=E + 1))}
    for i, net in enumerate(nets.values()):
        save_model(net, i, str(tmp_path) + "/")
    names = {k: "wavenet_autoencoder%d.model" % i for i, k in enumerate(nets)}
    for into, source in (("on", "off"), ("off", "on"), ("on", "classes"), ("on", "channels"), ("classes", "on")):
        model = nets[into]
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError) as err:
            load_model(model, str(tmp_path) + "/", names[source])
        msg = str(err.value)
        assert "global_classes=%d" % nets[source].global_classes in msg and "global_channels=%d" % nets[source].global_channels in msg
        assert "nothing was loaded" in msg
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)
    twin = _net(seed=9, **dict(LEARNED, **GLOBAL))
    assert load_model(twin, str(tmp_path) + "/", names["on"]) is twin
    assert all(torch.equal(a, b) for a, b in zip(nets["on"].state_dict().values(), twin.state_dict().values()))


def _engines():
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    return [(_AutoencoderEngine, {}, lt.AE_T), (GenericAutoencoderEngine, dict(filter_width=3), 600)]


def test_classes_missing_refused_and_out_of_range(monkeypatch):
    trace = lt.install(monkeypatch)
    for cls_, kw, T in _engines():
        x = lt.on_device(torch.zeros(2, 256, T))
        on = cls_(_ae_net(64, 64, **dict(LEARNED, **GLOBAL, **kw)), torch.device("cpu"))
        off = cls_(_ae_net(64, 64, **dict(LEARNED, **kw)), torch.device("cpu"))
        assert on.gcond and (on.g_E, on.g_n) == (E, NC) and not off.gcond and off.n_gcond == 0
        n_new = sum(p.numel() for n, p in on.net.named_parameters() if "gcond" in n or "global_embedding" in n)
        assert on.n_gcond == n_new and on.n_gather == on.spec.total - on.n_cond - n_new == off.n_gather
        assert on.gathered_param_names == off.gathered_param_names == off.param_names[:len(off.param_names) - 2 * (on.N + 1)]
        assert on.gcond_off[0] == on.spec.off["de_gcond_layer_stack.0.weight"] == on.spec.total - n_new
        del trace[:]
        with pytest.raises(ValueError, match="classes"):
            on.forward(x)
        with pytest.raises(ValueError, match="classes"):
            on.loss_and_grad(x, None)
        with pytest.raises(ValueError, match="classes"):
            off.forward(x, classes=[0, 1])
        with pytest.raises(ValueError, match="classes"):
            off.loss_and_grad(x, None, classes=torch.tensor([0, 1]))
        for bad in ([0, NC], [-1, 0], torch.tensor([0, NC]), [0], [0, 1, 2], torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
            with pytest.raises(ValueError, match="class"):
                on.forward(x, classes=bad)
        assert not [item for item in trace if item[0].startswith("wn_")], "something was launched before the refusal"
        on.forward(x, classes=[NC - 1, 0])                                       # the largest class passes
    # ... and the module says the same before it builds an engine
    net, plain = _ae_net(64, 64, **dict(LEARNED, **GLOBAL)), _ae_net(64, 64, **LEARNED)
    piece = torch.zeros(2, 256, lt.AE_T)
    with pytest.raises(ValueError, match="classes"):
        net(piece)
    with pytest.raises(ValueError, match="classes"):
        plain(piece, classes=[0, 1])
    assert net._engine is None and plain._engine is None


def test_vq_with_global_keeps_the_codebook_in_front_of_the_global_block(monkeypatch):
    from music_amd.model1 import _AutoencoderEngine
    lt.install(monkeypatch)
    eng = _AutoencoderEngine(_ae_net(64, 64, **dict(VQ_EMA, **GLOBAL)), torch.device("cpu"))
    assert eng.vq and eng.gcond
    assert eng.n_gather + eng.n_cond == eng.vq_off and eng.vq_off + eng.n_vq == eng.gcond_off[0] == eng.spec.total - eng.n_gcond
    assert eng.param_names[len(eng.gathered_param_names):][2 * (eng.N + 1)] == "vq_codebook.weight"


SWAP = {"wn_cond_proj_fwd": "wn_gcond_proj_fwd", "wn_cond_proj_bwd": "wn_gcond_proj_bwd"}


@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (32, 32, 2, {}), (32, 32, 3, {}), (64, 64, 2, {"use_bias": True}),
                                        (64, 64, 2, {"filter_width": 3})])
def test_a_global_step_launches_the_learned_step_with_the_two_entries_exchanged(en, de, B, kw, monkeypatch):
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    generic = "filter_width" in kw
    cls_, T = _engines()[1 if generic else 0][::2]
    x = lt.on_device(torch.zeros(B, 256, T))
    names, calls = {}, {}
    for mode, extra in (("learned", {}), ("global", GLOBAL)):
        net = _ae_net(en, de, **dict(LEARNED, **kw, **extra))
        eng = cls_(net, torch.device("cpu"))
        target = lt.on_device(torch.zeros(B * (T - eng.rf + 1), dtype=torch.int64))
        del trace[:]
        eng.loss_and_grad(x, target, None, classes=[B - 1 - b for b in range(B)] if extra else None)
        names[mode] = [item[0] for item in trace if item[0] not in ("record", "wait", "mark")]
        calls[mode] = {item[0]: item[1] for item in trace if item[0] in SWAP or item[0] in SWAP.values()}
    assert names["global"] == [SWAP.get(n, n) for n in names["learned"]]
    assert names["global"].count("wn_gcond_proj_fwd") == 1 == names["global"].count("wn_gcond_proj_bwd")
    # the shared arguments are the learned step's shapes, the new ones the global block's offsets and sizes
    fwd, bwd = calls["global"]["wn_gcond_proj_fwd"], calls["global"]["wn_gcond_proj_bwd"]
    lf, lb = calls["learned"]["wn_cond_proj_fwd"], calls["learned"]["wn_cond_proj_bwd"]
    assert tuple(fwd[2:7]) == eng.cond_off == tuple(bwd[5:10]) and fwd[10:17] == lf[10:17] and bwd[12:19] == lb[12:19]
    assert tuple(fwd[18:24]) == tuple(bwd[20:26]) == eng.gcond_off + (E, NC)
    assert fwd[17] is not None and bwd[19] is not None
    assert eng.gcond_off[0] + eng.n_gcond == eng.spec.total


def _train_run(tmp_path, extra_train=None, labels=True, model=True):
    from tests.test_ae_harness_cpu import g9, write_g9_run
    g = g9()
    if model:
        g = dict(g, model_params=dict(g["model_params"], conditioning="learned", global_classes=NC, global_channels=E))
    if labels:
        path = str(tmp_path / "labels.json")
        json.dump([k % NC for k in range(len(g["data_lens"]))], open(path, "w"))
        g = dict(g, dataset_params=dict(g["dataset_params"], labels_path=path))
    write_g9_run(tmp_path, g, extra_train)


def test_a_model_without_labels_and_labels_without_a_model_are_refused_at_start(tmp_path, monkeypatch):
    from music_amd import ae_train as A
    monkeypatch.chdir(tmp_path)
    _train_run(tmp_path, labels=False)
    with pytest.raises(ValueError, match="labels_path"):
        A.train()
    _train_run(tmp_path, model=False)
    with pytest.raises(ValueError, match="global_classes"):
        A.train()
    _train_run(tmp_path, {"valid_audio_path": str(tmp_path / "np_audio.pkl"), "validate_every": 1})
    with pytest.raises(ValueError, match="valid_labels_path"):
        A.train()
    assert not os.path.exists(tmp_path / "log")                                   # nothing was started
