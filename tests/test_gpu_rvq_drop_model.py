"""Quantiser dropout on the device behind both plans (music_amd/engine_base.py: wn_rvq_fwd_n / wn_rvq_bwd_n / wn_rvq_bwd_stats_n /
wn_rvq_lookup_n), at test size: the fast engine ("fast64") and the general plan ("general") of tests/test_gpu_rvq_model.py, whose
models, batches, float64 margins (every (frame, stage) pair at least MARGIN: an active pair of a forward with stage counts is a pair of
the full chain) and bars are used as they are - probabilities within 1e-3, every gradient within 3e-4 of its tensor's max-abs, vq_loss
within 1e-5 relative.  The float64 side is oracle.autoencoder_encode -> tests/rvq_drop_ref.py -> oracle.autoencoder_decode with the
model's parameters as leaves.  Run with -m gpu."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo
from tests import rvq_drop_ref as dr
from tests import vq_ref
from tests.test_gpu_cond_learned import DIL, W, _dev_pre
from tests.test_gpu_fullsize import _device_relu
from tests.test_gpu_rvq_model import DECAY, EPS, S, _case as rvq_case, build_cpu
from tests.test_gpu_vq_ema_kernels import check_update
from tests.test_gpu_vq_model import BETA, K, MARGIN, PROB_TOL, VQ_LOSS_RTOL, _grads64, _grads_close, _named

PLANS = ["fast64", "general"]
COUNTS = [1, S]                       # the two clips of either case: the coarsest code beside the full chain


def _drop64(n):
    class _Drop64(torch.autograd.Function):
        """tests/rvq_drop_ref.py as a float64 autograd node: (e, codebook) -> (q, vq_loss) under the stage counts n"""

        @staticmethod
        def forward(ctx, e, cb):
            f = dr.forward(e.detach().numpy(), cb.detach().numpy(), S, n, BETA)
            ctx.save_for_backward(e, cb)
            ctx.idx = f["idx"]
            ctx.set_materialize_grads(False)
            return torch.from_numpy(np.ascontiguousarray(f["q"])), torch.tensor(f["vq_loss"], dtype=torch.float64)

        @staticmethod
        def backward(ctx, d_q, g):
            e, cb = ctx.saved_tensors
            d_e, d_c = dr.backward(e.numpy(), cb.numpy(), S, n, ctx.idx, None if d_q is None else d_q.numpy(), BETA, 0.0 if g is None else float(g))
            return torch.from_numpy(np.ascontiguousarray(d_e)), torch.from_numpy(np.ascontiguousarray(d_c))
    return _Drop64


@functools.lru_cache(maxsize=None)
def _case(name):
    """the fused step with stage counts on the shared model of tests/test_gpu_rvq_model.py, and its float64 reference (computed once)"""
    c = rvq_case(name)
    net, cfg, B, x, target, eng = c["net"], c["cfg"], c["B"], c["x"], c["target"], c["eng"]
    assert B == len(COUNTS)
    n = np.asarray(COUNTS)
    loss = eng.loss_and_grad(x, target, stages=COUNTS)
    grads = _named(eng, eng.flat_grad.clone())
    ws = eng.workspace(B, x.shape[2])
    stats, codes, q, e = eng.last_vq, eng.vq_codes_of(ws).clone(), None, ws["enc_pre"].clone()
    with torch.no_grad():
        probs, q, _ = eng.forward(x, None, stages=torch.tensor(COUNTS))
        probs, q = probs.clone(), q.clone()
    relu, _ = _device_relu(_dev_pre(eng, B, x.shape[2]))
    leaf = OrderedDict((k, v.detach().double().cpu().clone().requires_grad_(True)) for k, v in net.state_dict().items())
    cond = [(leaf["de_cond_layer_stack.%d.weight" % i], leaf["de_cond_layer_stack.%d.bias" % i]) for i in range(len(DIL))]
    cond.append((leaf["connection_cond.weight"], leaf["connection_cond.bias"]))
    x64 = x.double().cpu()
    e64 = wo.autoencoder_encode(leaf, DIL, x64, cfg["en_pool_kernel_size"], relu)
    q64, vq64 = _drop64(n).apply(e64, leaf["vq_codebook.weight"])
    f64 = dr.forward(e64.detach().numpy(), leaf["vq_codebook.weight"].detach().numpy(), S, n, BETA)
    p64 = wo.autoencoder_decode(leaf, DIL, x64, q64, W, cond, cfg["quantization_channel"], relu)
    l64 = F.cross_entropy(p64, target.cpu()) + vq64
    return dict(c, n=n, loss=float(loss), grads=grads, stats=stats, codes=codes, q=q, e=e, probs=probs, f64=f64, p64=p64.detach(),
                l64=float(l64.detach()), vq64=float(vq64.detach()), g64=_grads64(l64, leaf), full=c)


@pytest.mark.parametrize("name", PLANS)
def test_the_fused_step_with_stage_counts_against_float64(name):
    from music_amd.ae_generic import GenericAutoencoderEngine
    from music_amd.model1 import _AutoencoderEngine
    c = _case(name)
    eng, B, n, f = c["eng"], c["B"], c["n"], c["f64"]
    Le = W // c["cfg"]["en_pool_kernel_size"]
    C = B * Le
    assert type(eng) is (GenericAutoencoderEngine if name == "general" else _AutoencoderEngine) and eng.vq_S == S
    assert (c["full"]["margins"] >= MARGIN).all()                                  # the full chain's margins cover every active pair
    # ---- codes: the float64 argmin in every active (frame, stage) pair, -1 in every inactive one
    codes = c["codes"].cpu().numpy()
    want = f["idx"].transpose(1, 0, 2)
    assert codes.shape == (B, S, Le) and c["codes"].dtype == torch.int64
    assert np.array_equal(codes, want), "codes differ in %d of %d (frame, stage) pairs" % ((codes != want).sum(), codes.size)
    assert (codes[0, 1:] == -1).all() and (codes[1] >= 0).all() and np.array_equal(codes[0, 0], c["full"]["codes"].cpu().numpy()[0, 0])
    cb = c["net"].vq_codebook.weight.detach()
    q = torch.zeros_like(c["q"])
    for b in range(B):                                                             # q: every clip the fp32 sum of ITS stages' rows
        for s in range(int(n[b])):
            row = cb[s * K:(s + 1) * K][c["codes"][b, s]].t()
            q[b] = row if s == 0 else q[b] + row
    assert torch.equal(c["q"], q)
    # ---- loss, vq_loss, probabilities
    st = c["stats"]
    vq_loss = float(st.vq_loss)
    rel = abs(vq_loss - c["vq64"]) / c["vq64"]
    e_p = float((c["probs"].cpu().double() - c["p64"]).abs().max())
    print("  %s: loss %.8g (float64 %.8g), vq_loss %.8g (float64 %.8g, relative %.1e, bar %.0e), probabilities err %.2e (bar %.0e)"
          % (name, c["loss"], c["l64"], vq_loss, c["vq64"], rel, VQ_LOSS_RTOL, e_p, PROB_TOL))
    assert abs(c["loss"] - c["l64"]) < 1e-4 and rel <= VQ_LOSS_RTOL and e_p <= PROB_TOL
    # ---- the statistics: per stage over the frames it saw
    assert np.array_equal(st.counts.cpu().numpy(), f["counts"])
    assert st.stage_frames.tolist() == f["stage_frames"].tolist() == [C, Le, Le] == st.counts.sum(1).tolist()
    mse = st.stage_mse.cpu().numpy().astype(np.float64)
    assert (np.abs(mse - f["mse"]) <= 1e-5 * f["mse"]).all()                        # the fixed denominator: vq_loss = coef x their sum
    assert abs(float(mse.sum()) * (1 + BETA) - vq_loss) <= 1e-6 * vq_loss
    act = st.stage_mse_active.cpu().numpy().astype(np.float64)
    assert (np.abs(act - f["mse"] * C / f["stage_frames"]) <= 1e-5 * act).all()
    err_q = float(((c["q"] - c["e"]).double() ** 2).mean())
    assert abs(float(st.mse) - err_q) <= 1e-5 * err_q                               # q against e, whatever stage a frame stopped at
    ppl = st.stage_perplexity.cpu().numpy()
    assert all(abs(ppl[s] - vq_ref.perplexity(f["counts"][s])) <= 1e-5 * ppl[s] for s in range(S)) and float(st.perplexity) == float(ppl[0])
    # ---- gradients
    _grads_close(name + " stages", c["grads"], c["g64"])
    g_cb = c["grads"]["vq_codebook.weight"]
    unused = torch.from_numpy((f["counts"] == 0).reshape(-1)).to(g_cb.device)
    assert bool((g_cb[unused] == 0).all()) and bool((g_cb[~unused].abs().amax(1) > 0).all())
    # a code of a later stage that only the dropped clip would have chosen gets nothing
    full = c["full"]["codes"].cpu().numpy()
    only_dropped = sorted(set(full[0, S - 1].tolist()) - set(full[1, S - 1].tolist()))
    assert only_dropped and bool((g_cb[(S - 1) * K + torch.tensor(only_dropped)] == 0).all())


@pytest.mark.parametrize("name", PLANS)
def test_all_stages_given_has_the_bits_of_no_stages_given(name):
    c = rvq_case(name)
    eng, net, x, target, B = c["eng"], c["net"], c["x"], c["target"], c["B"]
    outs = []
    for stages in (None, S, [S] * B, torch.full((B,), S)):
        loss = eng.loss_and_grad(x, target, stages=stages)
        ws = eng.workspace(B, x.shape[2])
        assert (ws["vq_nstage"] is None) == (stages is None)                        # a non-None value runs the _n entries
        outs.append((loss.clone(), eng.flat_grad.clone(), eng.vq_codes_of(ws).clone(), ws["vq_part"].clone(), ws["vq_res"].clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
    with torch.no_grad():
        net.eval()
        assert torch.equal(net(x, stages=S), net(x)) and torch.equal(net(x), c["probs"])
        net.train()
    for bad in (0, S + 1, [1, 2, 3], 1.0, True, [1.0, 2.0]):                        # refused before a launch
        with pytest.raises(ValueError, match="stages"):
            eng.loss_and_grad(x, target, stages=bad)


def test_the_module_draws_in_training_mode_and_uses_all_stages_in_eval_mode():
    from music_amd import objective
    from music_amd.vq_dropout import draw_stages
    net, cfg, B, x, target = build_cpu("fast64", vq_stage_dropout=1.0)
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    net.vq_dropout_seed = 4
    want = [draw_stages(4, t, 0, B, S, 1.0) for t in range(3)]
    assert any((w < S).any() for w in want)
    net.train()
    for t in range(2):                                                             # the module's own counter: steps 0, 1
        net.zero_grad()
        probs = net(x)
        codes = net.vq_codes.cpu().numpy()
        for b in range(B):
            assert (codes[b, :want[t][b]] >= 0).all() and (codes[b, want[t][b]:] == -1).all()
        assert net.last_vq.stage_frames.tolist() == [int((want[t] > s).sum()) * codes.shape[2] for s in range(S)]
        (torch.nn.CrossEntropyLoss()(probs, target) + net.vq_loss).backward()
        ref = net.vq_codebook.weight.grad.clone()
        # the fused step with the same counts gives the same codebook gradient bits (the fast engine runs the same launches)
        eng = net._engine_for(x.device)
        eng.loss_and_grad(x, target, stages=want[t])
        assert torch.equal(_named(eng, eng.flat_grad)["vq_codebook.weight"], ref)
    assert net.vq_dropout_calls == 2 and "vq_dropout_calls" not in net.state_dict()
    with torch.no_grad():
        explicit = net(x, stages=[S, 1]).clone()                                   # explicit counts: nothing is drawn
        assert net.vq_dropout_calls == 2 and bool((net.vq_codes[1, 1:] == -1).all()) and bool((net.vq_codes[0] >= 0).all())
        net.eval()
        full = net(x).clone()
        assert bool((net.vq_codes >= 0).all()) and net.vq_dropout_calls == 2 and not torch.equal(full, explicit)
        net.train()
    loss = objective.nll_loss(net, x, target.view(B, -1), stages=want[2])          # the nll objective takes the counts too, and draws nothing
    assert bool(torch.isfinite(loss)) and net.vq_dropout_calls == 2
    codes = net.vq_codes.cpu().numpy()
    assert all((codes[b, want[2][b]:] == -1).all() and (codes[b, :want[2][b]] >= 0).all() for b in range(B))
    (loss + net.vq_loss).backward()


def _snapshot(net):
    return dict(cb=net.vq_codebook.weight.detach().cpu().numpy().copy(), state=net.vq_ema_state.cpu().numpy().reshape(S, -1).copy())


@pytest.mark.parametrize("name", PLANS)
def test_an_ema_training_step_leaves_a_code_no_active_frame_chose_to_its_decay(name):
    net, cfg, B, x, target = build_cpu(name, vq_update="ema", vq_decay=DECAY, vq_eps=EPS, vq_restart=0.0, vq_stage_dropout=0.5)
    net.reset_vq_ema_state()
    net, x, target = net.cuda(), x.cuda(), target.cuda()
    eng = net._engine_for(x.device)
    eng.adam_init(lr=1e-3)
    # the first step of the module's own draws (p = 0.5) that drops exactly one clip out of the last stage
    step = next(t for t in range(64) if sorted(net.draw_stages(B, step=t) == S) == [False, True])
    n = net.draw_stages(B, step=step)
    dropped = int(np.argmin(n))
    eng.loss_and_grad(x, target)                                                   # all stages first: the codes and sums dropout takes away
    full = eng.vq_codes_of(eng.workspace(B, x.shape[2])).cpu().numpy()
    stat_full = eng.vq_stat.cpu().numpy().reshape(S, -1).copy()
    eng.loss_and_grad(x, target, stages=n)
    ws = eng.workspace(B, x.shape[2])
    codes = eng.vq_codes_of(ws).cpu().numpy()
    assert (codes[dropped, n[dropped]:] == -1).all() and np.array_equal(codes[1 - dropped], full[1 - dropped])
    stat = eng.vq_stat.cpu().numpy().reshape(S, -1)
    assert np.array_equal(stat[:, :K], eng.last_vq.counts.cpu().numpy()) and stat[S - 1, :K].sum() == ws["Le"]
    lost = sorted(set(full[dropped, S - 1].tolist()) - set(full[1 - dropped, S - 1].tolist()))
    assert lost, "no code of the last stage is the dropped clip's alone: the case decides nothing"
    before = _snapshot(net)
    eng.adam_step()
    after = _snapshot(net)
    for s in range(S):                                                             # the float64 rule per stage, on the stats of the ACTIVE frames
        check_update(dict(cb=before["cb"][s * K:(s + 1) * K], state=before["state"][s]),
                     dict(cb=after["cb"][s * K:(s + 1) * K], state=after["state"][s]), stat[s], K, DECAY, EPS, 0.0,
                     "%s stage %d" % (name, s), False)
    g = np.float32(DECAY)
    for k in lost:                                                                 # no frame: N' = g N and m' = g m, one fp32 product each
        assert stat[S - 1, k] == 0
        assert after["state"][S - 1][k] == g * before["state"][S - 1][k]
        m0 = before["state"][S - 1][K:].reshape(K, -1)[k]
        assert np.array_equal(after["state"][S - 1][K:].reshape(K, -1)[k], g * m0)
    assert (stat_full[S - 1, lost] > 0).all()                                     # without dropout the same batch DOES feed those rows


@pytest.mark.parametrize("name", PLANS)
def test_codes_with_absent_stages_decode_as_the_resynthesis_does(name):
    from music_amd.ae_generate import decode_codes, encode_codes, resynthesize
    c = rvq_case(name)
    net, x, B = c["net"], c["x"], c["B"]
    rf, Le = net.receptive_field, W // c["cfg"]["en_pool_kernel_size"]
    eng = c["eng"]
    full = encode_codes(net, x)
    codes = encode_codes(net, x, stages=COUNTS)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (B, S, Le)
    assert bool((codes[0, 1:] == -1).all()) and torch.equal(codes[0, 0], full[0, 0]) and torch.equal(codes[1], full[1])
    assert torch.equal(encode_codes(net, x, stages=S), full) and bool((encode_codes(net, x, stages=2)[:, 2] == -1).all())
    r_codes, r_probs, r_enc = resynthesize(net, x, teacher_forced=True, want_probs=True, stages=COUNTS)
    assert torch.equal(net.vq_codes, codes)
    clip = x.argmax(1)
    out, probs = decode_codes(net, codes, W, start=clip[:, :rf - 1], teacher_forced=clip, want_probs=True)
    assert torch.equal(out, r_codes) and torch.equal(probs, r_probs) and torch.equal(eng.vq_lookup(codes), r_enc)
    # a uniform prefix: the path and bits of prefix codes without -1
    two = encode_codes(net, x, stages=2)
    assert torch.equal(eng.vq_lookup(two), eng.vq_lookup(full[:, :2])) and torch.equal(eng.vq_lookup(two[:, :2]), eng.vq_lookup(full[:, :2]))
    # refused on the host: a hole, stage 0 absent, one frame alone; on the device: an active code out of range
    for change in (lambda w: w[1, 1].fill_(-1), lambda w: w[0, 0].fill_(-1), lambda w: w[1, 2, 3].fill_(-1)):
        w = codes.clone()
        change(w)
        with pytest.raises(ValueError):
            decode_codes(net, w, W)
    w = codes.clone()
    w[1, 2, 3] = K
    with pytest.raises(ValueError, match="outside"):
        decode_codes(net, w, W)


@pytest.mark.parametrize("name", PLANS)
def test_rate_distortion_has_a_row_per_prefix_and_the_error_does_not_grow(name):
    """A stage refines only where one of its rows is nearer to the residual than 0 is - rows drawn from other clips' residuals need not
    be (Bw = 48 of the general case: they are not) -, so the error of an unfitted chain may GROW with the stages.  With the zero row in
    every stage's codebook it cannot: the nearest row is at most as far as 0, and at these cases' margins (>= MARGIN) fp32 decides
    as float64 does.  The case's model is copied and row 0 of every stage zeroed."""
    import copy
    from music_amd.ae_generate import rate_distortion
    c = rvq_case(name)
    net, x = copy.deepcopy(c["net"]), c["x"]
    with torch.no_grad():
        for s in range(S):
            net.vq_codebook.weight[s * K].zero_()
    net.train()
    rows = rate_distortion(net, x)
    assert net.training
    assert [r["stages"] for r in rows] == list(range(1, S + 1)) and [r["bits_per_frame"] for r in rows] == [5.0 * n for n in range(1, S + 1)]
    mse = [r["mse"] for r in rows]
    print("  %s: %s" % (name, rows))
    assert all(np.isfinite(r["nll"]) and r["nll"] > 0 for r in rows) and all(a >= b for a, b in zip(mse, mse[1:])) and mse[-1] > 0
