"""Cached-queue generation for any filter width and quantisation width (ABI 6, wn_decode_batch_fw): block i keeps a ring of
(k-1) d_i input columns, the causal layer k-1 previous input columns, the sampler takes any Q.  Teacher-forced probabilities
against the float64 oracle's forward over the whole window, free-running greedy generation against the oracle's naive loop,
batched rows against single launches, the reference-style queue surface and the autoencoder's cached generation.
Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo

PROB_TOL = 1e-3
MARGIN = 1e-4


def _abi():
    # checked before anything is launched: an older library's decoder assumes filter_width 2 and Q = 256
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 6
    assert _lib.load().wn_version() >= 6


def _net(fw, dil, D, R, S, Q, bias, seed, gain=2.0):
    from music_amd.model import wavenet
    cfg = dict(filter_width=fw, dilations=dil, dilation_channels=D, residual_channels=R, skip_channels=S,
               quantization_channels=Q, use_bias=bias)
    torch.manual_seed(seed)
    net = wavenet(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gain)
    params = {k: v.detach().clone().double() for k, v in net.state_dict().items()}
    return net.cuda(), cfg, params


def _onehot(codes, Q):
    codes = np.asarray(codes)
    x = torch.zeros(1, Q, len(codes))
    x[0, torch.from_numpy(codes.astype(np.int64)), torch.arange(len(codes))] = 1.0
    return x


def _oracle_probs(params, cfg, x):
    """softmax over Q of the float64 oracle's pre-softmax at every output position of the window: (W, Q)."""
    inter = {}
    wo.wavenet_forward(params, cfg["dilations"], x.double(), filter_width=cfg["filter_width"],
                       quantization_channels=cfg["quantization_channels"], intermediates=inter)
    return torch.softmax(inter["pre_softmax"][0], 0).t()


def _margin(p):
    top = torch.topk(p, 2).values
    return float(top[0] - top[1])


def _forced(net, codes, Q, n):
    """predict_next on the first receptive field of `codes`, then n teacher-forced steps: (first code, codes, probabilities)."""
    from music_amd import fast_generate as fg
    rf = net.receptive_field
    x = _onehot(codes[:rf + n], Q)
    pred, st = fg.predict_next(net, x[:, :, :rf].cuda(), None)
    nxt = torch.from_numpy(np.concatenate([codes[rf + 1:rf + n], [0]]).astype(np.int32))
    got, probs, _ = fg._decode(net, st, x[0, :, rf].contiguous().cuda(), n, forced=nxt, want_probs=True, correct_queue=True)
    return pred, got, probs


CASES = [
    # (name, filter_width, dilations, D, R, S, Q, bias, teacher-forced steps, matrix-core kernel)
    ("k3_64_256", 3, [1, 2, 4, 8, 16, 32, 64, 128], 64, 64, 256, 256, False, 600, True),      # tap-0 table in LDS
    ("k4_32_512", 4, [1, 2, 4, 8, 16, 32, 64], 32, 32, 512, 256, False, 450, True),          # split skip workgroups
    ("k3_40_blocks", 3, [1, 2, 4, 8] * 10, 64, 64, 256, 256, False, 120, True),              # table in the hand-off area
    ("k3_bias", 3, [1, 2, 4, 8, 16, 32], 64, 64, 256, 256, True, 200, True),
    ("k1", 1, [1, 2, 4, 8], 32, 32, 64, 256, True, 40, False),
    ("k3_96_128_160", 3, [1, 2, 4, 8, 16], 96, 128, 160, 256, False, 100, False),
    ("k2_q512", 2, [1, 2, 4, 8, 16], 32, 32, 96, 512, False, 80, False),
    ("k2_q100", 2, [1, 2, 4, 8, 16], 32, 32, 64, 100, True, 80, False),
    ("k4_q64", 4, [1, 2, 4, 8], 32, 32, 64, 64, False, 90, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_teacher_forced_probabilities_match_the_float64_oracle(case):
    """A random clip forced through the decoder (every ring wraps at least once): each step's probabilities equal the softmax
    of the oracle's pre-softmax at that position within 1e-3, and wherever the oracle's top two are further apart than 1e-4
    the decoder's code is the oracle's argmax."""
    _abi()
    from music_amd import fast_generate as fg
    name, fw, dil, D, R, S, Q, bias, n, mfma = case
    # (512 quantisation channels spread the same logits thinner: a larger gain keeps the distributions peaked)
    net, cfg, params = _net(fw, dil, D, R, S, Q, bias, seed=300 + CASES.index(case), gain=3.0 if Q > 256 else 2.0)
    rf = net.receptive_field
    assert n > (fw - 1) * max(dil)                          # every ring wraps
    rng = np.random.default_rng(11 + CASES.index(case))
    codes = rng.integers(0, Q, size=rf + n)
    x = _onehot(codes, Q)
    pred, got, probs = _forced(net, codes, Q, n)
    assert fg._mfma_decode(net._engine) == mfma
    p_ref = _oracle_probs(params, cfg, x)                   # (n + 1, Q)
    assert probs.shape == (n, Q)
    err = (probs.double().cpu() - p_ref[1:]).abs().max().item()
    print("%s: teacher-forced probability error %.2e over %d steps, largest oracle probability %.3f"
          % (name, err, n, float(p_ref.max())))
    assert err < PROB_TOL, err
    assert abs(probs.sum(1).cpu().double() - 1).max().item() < 1e-4
    if _margin(p_ref[0]) > MARGIN:
        assert int(pred[0]) == int(p_ref[0].argmax())
    got = got.cpu().tolist()
    checked = 0
    for s in range(n):
        if _margin(p_ref[s + 1]) > MARGIN:
            assert got[s] == int(p_ref[s + 1].argmax()), (s, got[s])
            checked += 1
    print("  codes checked against the oracle's argmax: %d of %d" % (checked, n))
    assert checked >= max(1, n // 8)
    assert 0 <= min(got) and max(got) < Q


def test_free_running_greedy_follows_the_oracle_naive_loop():
    """generate_codes (one launch) for filter_width 3 follows the oracle's naive greedy loop - one full forward over the
    growing window per sample - up to the first near-tie."""
    _abi()
    from music_amd import fast_generate as fg
    net, cfg, params = _net(3, [1, 2, 4, 8, 16, 1, 2], 48, 40, 96, 256, True, seed=41)
    rf = net.receptive_field
    rng = np.random.default_rng(4)
    seq = list(rng.integers(0, 256, size=rf))
    n = 60
    got = fg.generate_codes(net, _onehot(seq, 256).cuda(), n, correct_queue=True).cpu().tolist()
    agreed = 0
    for s in range(n):
        p = _oracle_probs(params, cfg, _onehot(seq[-rf:], 256))[-1]
        if _margin(p) <= MARGIN:
            break
        want = int(p.argmax())
        assert got[s] == want, (s, got[s], want)
        seq.append(want)
        agreed += 1
    print("free-running greedy: %d of %d codes equal the naive loop's before the first near-tie" % (agreed, n))
    assert agreed >= 20


MF_CASES = [
    # (name, filter_width, dilations, D, R, S, bias)
    ("k3_64_bias", 3, [1, 2, 4, 8, 16, 32] * 2, 64, 64, 256, True),
    ("k3_t0_hand_off", 3, [1, 2, 4, 8, 16] * 7, 48, 40, 256, False),
    ("k4_32_512", 4, [1, 2, 4, 8, 16] * 2, 32, 32, 512, True),
]


@pytest.mark.parametrize("case", MF_CASES, ids=[c[0] for c in MF_CASES])
def test_matrix_core_decode_equals_the_fp32_kernel(case, monkeypatch):
    """Filter widths 3 / 4 on the matrix-core kernels (history taps summed a sample ahead) against the fp32 kernel on a fresh
    net with the same weights (WN_DEC_MFMA=0): probabilities within 1e-4, and the same codes wherever the top two are
    further apart than that."""
    _abi()
    from music_amd import fast_generate as fg
    name, fw, dil, D, R, S, bias = case
    seed = 500 + MF_CASES.index(case)
    net, cfg, params = _net(fw, dil, D, R, S, 256, bias, seed=seed)
    n = 2 * (fw - 1) * max(dil) + 60
    codes = np.random.default_rng(seed).integers(0, 256, size=net.receptive_field + n)
    pm, cm, probs_m = _forced(net, codes, 256, n)
    assert fg._mfma_decode(net._engine)
    monkeypatch.setenv("WN_DEC_MFMA", "0")
    net2, _, _ = _net(fw, dil, D, R, S, 256, bias, seed=seed)
    pf, cf, probs_f = _forced(net2, codes, 256, n)
    assert not fg._mfma_decode(net2._engine)
    err = (probs_m - probs_f).abs().max().item()
    print("%s: matrix-core vs fp32 kernel, largest probability difference %.2e over %d steps" % (name, err, n))
    assert err < 1e-4, err
    pfc = probs_f.cpu()
    cm, cf = cm.cpu().tolist(), cf.cpu().tolist()
    for s in range(n):
        if _margin(pfc[s]) > 1e-4:
            assert cm[s] == cf[s], s


@pytest.mark.parametrize("shape", [(32, 32, 64), (32, 32, 256)], ids=["fp32", "matrix_core"])
def test_batched_rows_equal_single_launches(shape):
    """generate_codes_batch for filter_width 3 with 1, 3 and 9 utterances: greedy rows are bit-identical to single launches;
    sampled rows depend only on (seed, step, utterance index), so the 3-utterance launch's rows are the 9-utterance launch's
    first rows and row 0 is the single launch; a fixed seed repeats exactly, another seed does not."""
    _abi()
    from music_amd import fast_generate as fg
    D, R, S = shape
    net, cfg, params = _net(3, [1, 2, 4, 8, 1, 2, 4], D, R, S, 256, False, seed=77)
    rf = net.receptive_field
    rng = np.random.default_rng(8)
    starts = torch.cat([_onehot(rng.integers(0, 256, size=rf), 256) for _ in range(9)]).cuda()
    n = 50
    single = [fg.generate_codes(net, starts[u:u + 1], n, correct_queue=True).cpu() for u in range(9)]
    assert fg._mfma_decode(net._engine) == (S == 256)
    for U in (1, 3, 9):
        out = fg.generate_codes_batch(net, starts[:U], n, correct_queue=True).cpu()
        assert out.shape == (U, n)
        for u in range(U):
            assert torch.equal(out[u], single[u]), (U, u)
    t3 = fg.generate_codes_batch(net, starts[:3], n, correct_queue=True, temperature=0.8, seed=5).cpu()
    t9 = fg.generate_codes_batch(net, starts[:9], n, correct_queue=True, temperature=0.8, seed=5).cpu()
    assert torch.equal(t3, t9[:3])
    assert torch.equal(t9, fg.generate_codes_batch(net, starts[:9], n, correct_queue=True, temperature=0.8, seed=5).cpu())
    s0 = fg.generate_codes(net, starts[:1], n, correct_queue=True, temperature=0.8, seed=5).cpu()
    assert torch.equal(s0, t9[0])
    assert not torch.equal(t9, fg.generate_codes_batch(net, starts[:9], n, correct_queue=True, temperature=0.8, seed=6).cpu())
    assert not torch.equal(t9, torch.stack(single))


def test_reference_queue_surface_for_filter_width_3():
    """predict_next with filter_width 3: the queue dict has the reference's keys, 'block_i' -> (1, R, 2 d_i) and
    'causal_layer' -> (1, Q, 2), oldest column first - the last 2 d_i columns of the oracle's block inputs, after several
    steps too; a state rebuilt from those tensors (from_tensors) gives the same codes; correct_queue=False raises."""
    _abi()
    from music_amd import fast_generate as fg
    dil = [1, 2, 4, 3]
    net, cfg, params = _net(3, dil, 32, 24, 48, 256, True, seed=9)
    rf, R = net.receptive_field, 24
    rng = np.random.default_rng(10)
    codes = rng.integers(0, 256, size=rf + 30)
    x = _onehot(codes, 256)
    pred, st = fg.predict_next(net, x[:, :, :rf].cuda(), None)

    def check(state, t):
        inter = {}
        wo.wavenet_forward(params, dil, x[:, :, :t].double(), filter_width=3, intermediates=inter)
        assert list(state.keys()) == ["causal_layer"] + ["block_%d" % (i + 1) for i in range(len(dil))]
        c = state["causal_layer"]
        assert tuple(c.shape) == (1, 256, 2)
        assert torch.equal(c.cpu(), x[:, :, t - 2:t])
        for i, d in enumerate(dil):
            q = state["block_%d" % (i + 1)]
            assert tuple(q.shape) == (1, R, 2 * d)
            want = inter["x"][i][:, :, -2 * d:]
            assert (q.double().cpu() - want).abs().max().item() < 1e-3 * max(1.0, want.abs().max().item())
    check(st, rf)
    for t in range(rf, rf + 12):
        pred, st = fg.predict_next(net, x[:, :, t:t + 1].cuda(), st, correct_queue=True)
    check(st, rf + 12)
    plain = {k: v for k, v in st.items()}
    a, b = [], []
    st_a = st
    for t in range(rf + 12, rf + 30):
        pa, st_a = fg.predict_next(net, x[:, :, t:t + 1].cuda(), st_a, correct_queue=True)
        a.append(int(pa[0]))
    st_b = fg.DecodeState.from_tensors(st.eng, plain)
    for t in range(rf + 12, rf + 30):
        pb, st_b = fg.predict_next(net, x[:, :, t:t + 1].cuda(), st_b, correct_queue=True)
        b.append(int(pb[0]))
    assert a == b
    with pytest.raises(ValueError, match="correct_queue=True"):
        fg.predict_next(net, x[:, :, rf:rf + 1].cuda(), st_b)
    with pytest.raises(ValueError, match="correct_queue=True"):
        fg.generate_codes(net, x[:, :, :rf].cuda(), 8)
    with pytest.raises(ValueError, match="correct_queue=True"):
        fg.generate_codes_batch(net, x[:, :, :rf].cuda(), 8)


def test_autoencoder_cached_generation_with_filter_width_3():
    """ae_generate.generate_cached on a filter_width 3 autoencoder runs (its decoder net has filter_width 3) and its codes are
    generate_codes on the returned decoder net."""
    _abi()
    from music_amd.model1 import wavenet_autoencoder
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    cfg = dict(filter_width=3, quantization_channel=256, dilations=[1, 2, 4, 1, 2], en_residual_channel=24,
               en_dilation_channel=20, en_bottleneck_width=6, en_pool_kernel_size=32, de_residual_channel=40,
               de_dilation_channel=36, de_skip_channel=72, use_bias=False)
    torch.manual_seed(71)
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.5)
    net = net.cuda()
    rf = net.receptive_field
    rng = np.random.default_rng(72)
    x0 = _onehot(rng.integers(0, 256, size=rf + 32 + 5), 256)          # pools to exactly one frame
    torch.manual_seed(73)
    cond = net._draw_conditioning()
    got, wnet, enc = ag.generate_cached(net, x0, 40, cond=cond)
    assert wnet.filter_width == 3 and tuple(enc.shape) == (1, 6, 1)
    want = fg.generate_codes(wnet, x0[:, :, -wnet.receptive_field:].cuda(), 40, correct_queue=True)
    assert torch.equal(got.cpu(), want.cpu())
    assert got.numel() == 40 and int(got.max()) < 256
