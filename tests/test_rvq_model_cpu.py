"""CPU checks of `vq_stages` (residual vector quantisation) on the module surface of music_amd/model1.py, in the pattern of
tests/test_vq_model_cpu.py: the refusals, what is registered and where, what a seed gives, vq_stages = 1 against the parent,
checkpoints of another stage count, init_codebook over the stages, split_code_stream - and, through the recorder of
tests/launch_trace.py, what a step of S stages LAUNCHES.  No device is touched."""
import json

import pytest
import torch

from tests import launch_trace as lt
from tests.test_engine_base import _ae_net
from tests.test_vq_model_cpu import BW, CFG, K, VQ, _equal, _net

S = 3
EMA = dict(VQ, vq_update="ema")


def test_constructor_refusals():
    for s in (0, 9, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="vq_stages"):
            _net(**dict(VQ, vq_stages=s))
    for kw in ({}, {"conditioning": "learned"}, {"conditioning": "learned", "bottleneck": "continuous"}):
        with pytest.raises(ValueError, match='vq_stages > 1 requires bottleneck="vq"'):
            _net(vq_stages=2, **kw)
    assert _net(vq_stages=1).vq_stages == 1 and _net(**VQ).vq_stages == 1                # the default; 1 needs no vq
    assert _net(**dict(VQ, vq_stages=8)).vq_codebook.weight.shape == (8 * K, BW)          # the limit itself
    params = json.loads(json.dumps(dict(CFG, **dict(VQ, vq_stages=4))))
    from music_amd.model1 import wavenet_autoencoder
    assert wavenet_autoencoder(**params).vq_stages == 4


@pytest.mark.parametrize("update", ["gradient", "ema"])
def test_shapes_order_and_what_a_seed_gives(update):
    kw = dict(VQ, vq_update=update)
    one, net = _net(**kw), _net(vq_stages=S, **kw)
    a, b = one.state_dict(), net.state_dict()
    assert list(a) == list(b)                                                      # the same keys in the same order
    tail = ["vq_codebook.weight"] + (["vq_ema_state"] if update == "ema" else [])
    assert list(b)[-len(tail):] == tail
    assert all(_equal(a[k], b[k]) for k in a if k not in tail)                     # every earlier parameter: the parent's bits
    assert [n for n, _ in net.named_parameters()][-1] == "vq_codebook.weight"
    w = net.vq_codebook.weight.detach()
    assert tuple(w.shape) == (S * K, BW)
    # with a global block behind it the codebook stays in front: [projections | codebook | global block], and keeps its bits
    g = _net(vq_stages=S, global_classes=3, global_channels=4, **kw)
    names = [n for n, _ in g.named_parameters()]
    assert names.index("vq_codebook.weight") + 1 == names.index("de_gcond_layer_stack.0.weight")
    assert torch.equal(g.vq_codebook.weight.detach(), w)
    for s in range(S):                                                             # every stage uniform in +- 1 / K (not 1 / (S K))
        rows = w[s * K:(s + 1) * K]
        assert 0.5 / K < float(rows.abs().max()) <= 1.0 / K and float(rows.min()) < 0 < float(rows.max())
    if update == "ema":
        state = net.vq_ema_state.view(S, -1)
        assert net.vq_ema_state.shape == (S * K * (BW + 1),)
        assert bool((state[:, :K] == 1).all()) and torch.equal(state[:, K:].reshape(S * K, BW), w)
        with torch.no_grad():
            net.vq_codebook.weight.mul_(2.0)
            net.vq_ema_state.zero_()
        net.reset_vq_ema_state()                                                   # per stage: [1 | that stage's rows]
        state = net.vq_ema_state.view(S, -1)
        assert bool((state[:, :K] == 1).all()) and torch.equal(state[:, K:].reshape(S * K, BW), net.vq_codebook.weight.detach())


def test_one_stage_is_the_parent_in_state_dict_and_rng_state():
    for kw in (VQ, EMA, dict(VQ, global_classes=3, global_channels=4)):
        torch.manual_seed(5)
        a = _net(**kw)
        rng_a = torch.get_rng_state()
        b = _net(vq_stages=1, **kw)
        rng_b = torch.get_rng_state()
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(_equal(sa[k], sb[k]) for k in sa) and torch.equal(rng_a, rng_b)
        assert sb["vq_codebook.weight"].shape == (K, BW)


def test_a_checkpoint_of_another_stage_count_is_refused_whole(tmp_path):
    from music_amd.ae_train import load_model, save_model
    for kw in (VQ, EMA):
        one, three = _net(seed=1, **kw), _net(seed=2, vq_stages=S, **kw)
        save_model(one, 1, str(tmp_path) + "/")
        save_model(three, 3, str(tmp_path) + "/")
        for model, name, saved in ((three, "wavenet_autoencoder1.model", 1), (one, "wavenet_autoencoder3.model", S)):
            before = {k: v.clone() for k, v in model.state_dict().items()}
            with pytest.raises(RuntimeError) as err:
                load_model(model, str(tmp_path) + "/", name)
            msg = str(err.value)
            assert '"vq_stages"' in msg and "vq_stages=%d" % saved in msg and "vq_stages=%d" % model.vq_stages in msg
            assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())      # nothing was loaded
        twin = _net(seed=3, vq_stages=S, **kw)
        assert load_model(twin, str(tmp_path) + "/", "wavenet_autoencoder3.model") is twin
        assert all(torch.equal(a, b) for a, b in zip(three.state_dict().values(), twin.state_dict().values()))


def test_init_codebook_fills_the_stages_in_order_from_the_residuals():
    net, one = _net(vq_stages=S, **EMA), _net(**VQ)
    gen = torch.Generator().manual_seed(9)
    many = torch.randn(3, BW, 33, generator=gen)                                   # 99 frames >= S K = 72
    net.init_codebook(many, seed=4)
    one.init_codebook(many, seed=4)
    w = net.vq_codebook.weight.detach().clone()
    assert torch.equal(w[:K], one.vq_codebook.weight.detach())                     # stage 0: the one-stage draw of the same seed
    frames = many.permute(0, 2, 1).reshape(-1, BW)
    spent = set()
    for s in range(S):
        rows = w[s * K:(s + 1) * K]
        hit = [int((frames == r).all(1).nonzero()[0]) for r in rows]               # every row IS a frame of this stage's input ...
        assert len(set(hit)) == K and not set(hit) & spent                        # ... no frame twice, never one an earlier stage took
        spent |= set(hit)
        frames = frames - rows[torch.cdist(frames, rows).argmin(1)]
        if s == 0:
            assert float(frames.abs().sum(1).min()) == 0                           # a frame that became a row leaves nothing over
    state = net.vq_ema_state.view(S, -1)
    assert bool((state[:, :K] == 1).all()) and torch.equal(state[:, K:].reshape(S * K, BW), w)
    net.init_codebook(many, seed=4)
    assert torch.equal(net.vq_codebook.weight.detach(), w)                         # deterministic


def test_split_code_stream_and_its_refusals():
    from music_amd.ae_generate import split_code_stream
    codes = torch.tensor([[[3, 0, 23], [5, 7, 1], [1, 23, 0]], [[0, 1, 2], [3, 4, 5], [6, 7, 8]]])       # (B, S, Le)
    tokens = (codes + torch.arange(S).view(1, S, 1) * K).permute(0, 2, 1).reshape(2, -1)                 # l0s0, l0s1, l0s2, l1s0, ..
    assert tokens[0].tolist() == [3, K + 5, 2 * K + 1, 0, K + 7, 2 * K + 23, 23, K + 1, 2 * K]
    back = split_code_stream(tokens, S, K)
    assert back.dtype == torch.int64 and torch.equal(back, codes)
    assert torch.equal(split_code_stream(tokens[1].numpy(), S, K), codes[1:])      # one clip, 1-D: (1, S, Le)
    assert torch.equal(split_code_stream(codes[:, 0], 1, K), codes[:, :1])         # one stage: the codes themselves
    with pytest.raises(ValueError, match="multiple of 3"):
        split_code_stream(tokens[:, :-1], S, K)
    bad = tokens.clone()
    bad[1, 4] = 2 * K                                                              # frame 1, stage 1 holds a stage-2 token
    with pytest.raises(ValueError, match=r"clip 1 at frame 1, stage 1 .*\[24, 48\)"):
        split_code_stream(bad, S, K)
    bad[1, 4] = -1
    with pytest.raises(ValueError, match="stage 1"):
        split_code_stream(bad, S, K)
    with pytest.raises(ValueError, match="integers"):
        split_code_stream(tokens.float(), S, K)


def test_the_dataset_tool_refuses_an_alphabet_the_sampler_cannot_draw():
    import importlib.util
    import os
    from tests.helpers import ROOT
    spec = importlib.util.spec_from_file_location("vq_codes_dataset", os.path.join(ROOT, "tools", "vq_codes_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.check_alphabet(2, 512)
    tool.check_alphabet(1, 1024)
    with pytest.raises(ValueError, match="1536 tokens"):
        tool.check_alphabet(3, 512)


NEW = ("wn_rvq_fwd", "wn_rvq_bwd", "wn_rvq_bwd_stats", "wn_rvq_ema_update", "wn_rvq_lookup")
PLAIN = ("wn_vq_fwd", "wn_vq_bwd", "wn_vq_bwd_stats", "wn_vq_ema_update", "wn_vq_lookup")


def _step(trace, Engine, en, de, B, kw, optimizer=False, **model):
    from music_amd.ae_generic import GenericAutoencoderEngine
    T = 600 if Engine is GenericAutoencoderEngine else lt.AE_T
    net = _ae_net(en, de, conditioning="learned", **dict(kw, **model))
    eng = Engine(net, torch.device("cpu"))
    if optimizer:
        eng.adam_init(lr=1e-3, ema_decay=0.999, skip_nonfinite=True)
    x = lt.on_device(torch.zeros(B, 256, T))
    target = lt.on_device(torch.zeros(B * (T - eng.rf + 1), dtype=torch.int64))
    del trace[:]
    eng.loss_and_grad(x, target, None)
    if optimizer:
        eng.adam_step()
    return net, eng, eng._ws.peek(B, T), [item for item in trace if item[0] not in ("record", "wait", "mark")]


@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (32, 32, 3, {}), (64, 64, 2, {"use_bias": True}), (64, 64, 2, {"filter_width": 3})])
def test_a_step_of_three_stages_is_the_continuous_step_plus_two_launches(en, de, B, kw, monkeypatch):
    """Both plans: one wn_rvq_fwd between wn_avgpool and wn_cond_proj_fwd, one wn_rvq_bwd between wn_cond_proj_bwd and
    wn_avgpool_bwd, everything else the continuous step's launches in its order; vq_stages = 1 launches exactly the parent's list."""
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    Engine = GenericAutoencoderEngine if kw.get("filter_width", 2) != 2 else _AutoencoderEngine
    cont = [c[0] for c in _step(trace, Engine, en, de, B, kw, bottleneck="continuous")[3]]
    parent = _step(trace, Engine, en, de, B, kw, bottleneck="vq", vq_codes=K)[3]
    one = _step(trace, Engine, en, de, B, kw, bottleneck="vq", vq_codes=K, vq_stages=1)[3]
    assert [c[0] for c in one] == [c[0] for c in parent] and not any(c[0] in NEW for c in one)
    scalars = lambda calls: [[a for a in c[1] if isinstance(a, (int, float))] for c in calls if c[0] in PLAIN]
    assert scalars(one) == scalars(parent)                                        # ... with the parent's scalar arguments
    net, eng, ws, calls = _step(trace, Engine, en, de, B, kw, bottleneck="vq", vq_codes=K, vq_stages=S)
    v = [c[0] for c in calls]
    assert v.count("wn_rvq_fwd") == 1 and v.count("wn_rvq_bwd") == 1 and not any(n in PLAIN for n in v)
    assert v[v.index("wn_rvq_fwd") - 1] == "wn_avgpool" and v[v.index("wn_rvq_fwd") + 1] == "wn_cond_proj_fwd"
    assert v[v.index("wn_rvq_bwd") - 1] == "wn_cond_proj_bwd" and v[v.index("wn_rvq_bwd") + 1] == "wn_avgpool_bwd"
    assert [n for n in v if n not in NEW] == cont, "a step of three stages differs from the continuous step beyond its two launches"
    fwd, bwd = dict(calls)["wn_rvq_fwd"], dict(calls)["wn_rvq_bwd"]
    Le, Bw = ws["Le"], eng.Bw
    assert eng.vq_S == S and eng.vq_K == K and eng.n_vq == S * K * Bw and eng.vq_off == eng.spec.total - S * K * Bw
    assert eng.n_gather + eng.n_cond + eng.n_vq == eng.spec.total and eng.param_names[-1] == "vq_codebook.weight"
    assert fwd[2] == eng.vq_off == bwd[5] and tuple(fwd[8:13]) == (S, K, Bw, Le, B) == tuple(bwd[10:15])
    assert (bwd[6], bwd[7]) == (0.25, 1.0)
    assert fwd[0].t is ws["enc_pre"] is bwd[0].t and fwd[3].t is ws["enc"]         # e in, q out: the tables are built from q
    assert fwd[4].t is ws["vq_idx"] is bwd[1].t and fwd[5].t is ws["vq_counts"] and fwd[6].t is ws["vq_res"] is bwd[2].t
    assert fwd[7].t is ws["vq_part"] and bwd[3].addr == bwd[8].addr and bwd[9].t is eng.flat_grad
    assert ws["vq_idx"].shape == (S, B, Le) and ws["vq_counts"].shape == (S, K) and ws["vq_res"].shape == (S, B, Bw, Le)
    assert eng.vq_codes_of(ws).shape == (B, S, Le) and eng.last_vq.stage_mse.shape == (S,)


@pytest.mark.parametrize("en,de,B,kw", [(64, 64, 2, {}), (64, 64, 2, {"filter_width": 3})])
def test_an_ema_step_of_three_stages_launches_the_stats_and_one_update(en, de, B, kw, monkeypatch):
    from music_amd import _lib
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    for k in lt.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    trace = lt.install(monkeypatch)
    Engine = GenericAutoencoderEngine if kw.get("filter_width", 2) != 2 else _AutoencoderEngine
    model = dict(bottleneck="vq", vq_codes=K, vq_stages=S, vq_restart=0.5)
    grad = [c[0] for c in _step(trace, Engine, en, de, B, kw, optimizer=True, **model)[3]]
    net, eng, ws, calls = _step(trace, Engine, en, de, B, kw, optimizer=True, vq_update="ema", **model)
    e = [c[0] for c in calls]
    assert "wn_rvq_bwd" not in e and e.count("wn_rvq_bwd_stats") == 1 and e.count("wn_rvq_ema_update") == 1
    assert not any(n in PLAIN for n in e)
    i = e.index("wn_rvq_ema_update")
    assert e[i - 1] == "wn_adam_flat_guarded" and e[i + 1] == "wn_ema_flat" and i + 2 == len(e)
    assert e[:i] + e[i + 1:] == ["wn_rvq_bwd_stats" if n == "wn_rvq_bwd" else n for n in grad]
    sb, up = dict(calls)["wn_rvq_bwd_stats"], dict(calls)["wn_rvq_ema_update"]
    Bw, Le = eng.Bw, ws["Le"]
    assert sb[10].t is eng.vq_stat and tuple(sb[11:16]) == (S, K, Bw, Le, B) and sb[2].t is ws["vq_res"]
    assert eng.vq_stat.numel() == S * K * (Bw + 1) == net.vq_ema_state.numel()    # ONE tensor: one all-reduce in a data-parallel run
    assert up[0].t is eng.flat and up[1] == eng.vq_off and up[2].t is eng.vq_stat and up[3].t is net.vq_ema_state
    assert up[4].t is eng.vq_ema_work and eng.vq_ema_work.numel() * 4 == S * _lib.VQ_EMA_WORK_BYTES
    assert up[5].t is eng.vq_ema_info and eng.vq_ema_info.numel() == 2 * S
    assert tuple(up[6:12]) == (S, K, Bw, 0.99, 1e-5, 0.5) and up[12] == eng.adam_state["guard"].state_ptr()
    assert eng.vq_loss_coef == 0.25 and eng.last_vq.coef == 0.25
