"""Position-windowed sampling inside the persistent decode launch (wn_win_decode_batch; include/wavenet_hip.h) on small untrained
models: the matrix-core kernel (64 / 64 / 256 / Q 256, one-workgroup and split skip stage) and the fp32 kernel (Q = 96, 64, 1024).

The sharp numeric check of the rule is tests/test_gpu_window_sampler.py (the same device function on given logits); a decode launch
does not return its logits, so here the windowed run is held against the PLAIN run's probabilities p of the same teacher-forced
steps: with M = sum of p over the window (float64), |r_i - p_i / M| <= 1e-6 + (1 + width) 1e-6 / M follows from the 1e-6 bars on r
and on every p_i.  That catches plumbing - the right pair at the right step, in every kernel form, across launches and batches.
Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sampling_ref as sr
from tests.helpers import ROOT
from tests.test_gpu_decode_sample import _model, _run, _state

P_TOL = 1e-6
BAND = 1e-5
TINY = 1e-30

# name -> (model arguments, [(stages, K)]): the window tables are fast_generate.stage_windows(stages, K)
MODELS = {
    "mfma": (dict(), [(2, 128), (4, 64)]),
    "q96": (dict(S=48, Q=96, R=24, D=20, dil=(1, 2, 4, 1), bias=True), [(3, 32)]),
    "q64": (dict(S=32, Q=64, R=16, D=16, dil=(1, 2, 4)), [(4, 16)]),
    "q1024": (dict(S=64, Q=1024, R=32, D=32, dil=(1, 2, 4)), [(8, 128)]),
}


def _same(a, b):
    """two _run results: codes, probability bits, handed-back columns, queues"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and torch.equal(a[2], b[2])
            and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]))


def _whole_alphabet_is_the_sampling_entry(net, Q):
    """every pair (0, Q): wn_decode_batch_samp bit for bit, greedy and top-k 40 / top-p 0.9, forced and free-running"""
    n, U = 24, 3
    st = _state(net, U, n)
    for forced in (True, None):
        for kw in (dict(), dict(temperature=0.9, seed=23, top_k=40, top_p=0.9)):
            old = _run(net, st, n, forced=forced, **kw)
            new = _run(net, st, n, forced=forced, windows=[(0, Q)] * 3, window_pos=2, **kw)
            assert _same(old, new), (forced, kw)
    assert len(np.unique(old[0])) > 1


def _inverse_cdf(r, c, u, what):
    cdf = np.cumsum(r.astype(np.float64))
    below = cdf[c - 1] if c > 0 else 0.0
    assert r[c] > 0 and (below - BAND <= u < cdf[c] + BAND or (u >= cdf[-1] - BAND and c == np.nonzero(r > 0)[0][-1])), \
        (what, c, u, below, cdf[c])


def _teacher_forced(net, wins, Q, pos=1, step0=3, seed=17):
    period = len(wins)
    n = 3 * period + 1
    st = _state(net, 1, n)
    plain = _run(net, st, n, step0=step0, temperature=1.0, seed=seed)
    win = _run(net, st, n, step0=step0, temperature=1.0, seed=seed, windows=wins, window_pos=pos)
    trunc = _run(net, st, n, step0=step0, temperature=1.0, seed=seed, top_k=40, top_p=0.9, windows=wins, window_pos=pos)
    greedy = _run(net, st, n, step0=step0, windows=wins, window_pos=pos)
    m_min = 1.0
    for t in range(n):
        lo, hi = wins[(pos + t) % period]
        p = plain[1][0, t].astype(np.float64)
        M = p[lo:hi].sum()
        m_min = min(m_min, M)
        inside = np.zeros(Q, bool)
        inside[lo:hi] = True
        u = sr.uniform(seed, step0 + t, 0)
        for what, run in (("plain", win), ("top-k 40 / top-p 0.9", trunc), ("greedy", greedy)):
            r, c = run[1][0, t], int(run[0][0, t])
            assert (r[~inside].view(np.int32) == 0).all(), (what, t, "support outside the window")
            assert abs(r.astype(np.float64).sum() - 1) < 1e-5 and lo <= c < hi, (what, t, c, (lo, hi))
            if what != "greedy":
                _inverse_cdf(r, c, u, (what, t))
            if what != "top-k 40 / top-p 0.9":
                # the support is the whole window (short of fp32 underflow) and r is p renormalised over it
                assert not (inside & (r <= 0) & (p / M > TINY)).any(), (what, t)
                assert np.abs(r[lo:hi] - p[lo:hi] / M).max() <= P_TOL + (1 + hi - lo) * P_TOL / M, (what, t, M)
            else:
                assert (r > 0).sum() <= min(42, hi - lo) and ((r > 0) & inside).any()
        assert p[int(greedy[0][0, t])] >= p[lo:hi].max() - 2e-6, t
    print("  windows %s: %d teacher-forced steps, smallest window mass M = %.3g" % (wins, n, m_min))


def _two_launches(net, wins, n1=5, n2=6, pos=1, step0=3):
    """one launch of n1 + n2 steps = two launches on the carried state, step0 and window_pos both advanced by n1"""
    st = _state(net, 1, n1 + n2, seed=61)
    kw = dict(forced=None, temperature=1.0, top_p=0.9, seed=5, windows=wins)
    one = _run(net, st, n1 + n2, step0=step0, window_pos=pos, **kw)
    a = _run(net, st, n1, step0=step0, window_pos=pos, **kw)
    dev = st[1].device
    b = _run(net, (st[0], a[4].to(dev), a[3].to(dev), a[2].to(dev), None), n2, step0=step0 + n1, window_pos=pos + n1, **kw)
    assert np.array_equal(one[0], np.concatenate([a[0], b[0]], 1))
    assert np.array_equal(one[1].view(np.int32), np.concatenate([a[1], b[1]], 1).view(np.int32))
    assert torch.equal(one[2], b[2]) and torch.equal(one[3], b[3]) and torch.equal(one[4], b[4])
    # ... and the position matters: the same second launch at another position gives other codes or other supports
    c = _run(net, (st[0], a[4].to(dev), a[3].to(dev), a[2].to(dev), None), n2, step0=step0 + n1, window_pos=pos + n1 + 1, **kw)
    assert not np.array_equal((b[1] > 0), (c[1] > 0))


def _batch_rows(net, wins, n=9, pos=2):
    """row u of a batched launch with per-utterance settings = its single-utterance launch with streams=[u]; one table for all"""
    U = 3
    eng, rings, prev, note, _ = _state(net, U, n, seed=53)
    T, K, Pn, S = [1.0, 0.0, 0.7], [0, 0, 5], [0.9, 1.0, 1.0], [11, 12, 13]
    full = _run(net, (eng, rings, prev, note, None), n, forced=None, temperature=T, top_k=K, top_p=Pn, seed=S, windows=wins, window_pos=pos)
    for uu in range(U):
        one = (eng, rings[uu:uu + 1], prev[uu:uu + 1], note[uu:uu + 1], None)
        single = _run(net, one, n, forced=None, temperature=[T[uu]], top_k=[K[uu]], top_p=[Pn[uu]], seed=[S[uu]], streams=[uu],
                      windows=wins, window_pos=pos)
        assert np.array_equal(full[0][uu], single[0][0]), uu
        assert np.array_equal(full[1][uu].view(np.int32), single[1][0].view(np.int32)), uu
        assert torch.equal(full[4][uu], single[4][0]) and torch.equal(full[2][uu], single[2][0]), uu
        for t in range(n):
            lo, hi = wins[(pos + t) % len(wins)]
            assert lo <= full[0][uu, t] < hi and (full[1][uu, t, :lo] == 0).all() and (full[1][uu, t, hi:] == 0).all(), (uu, t)


def _free_running(net, stages, K, frames=4):
    """generate_codes_batch under stage windows: every code inside its position's window, the stream splits; row 0 is generate_codes"""
    from music_amd import fast_generate as fg
    from music_amd.ae_generate import split_code_stream
    Q, rf, U = net.quantization_channels, net.receptive_field, 2
    rng = np.random.default_rng(7)
    x = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, Q, size=(U, rf))), Q).transpose(1, 2).float().cuda()
    wins = fg.stage_windows(stages, K)
    kw = dict(correct_queue=True, temperature=1.0, top_p=0.9, seed=3, windows=wins)
    tokens = fg.generate_codes_batch(net, x, frames * stages, **kw)
    assert tuple(tokens.shape) == (U, frames * stages)
    t = tokens.cpu().numpy()
    for j in range(frames * stages):
        lo, hi = wins[j % stages]
        assert ((lo <= t[:, j]) & (t[:, j] < hi)).all(), (j, t[:, j], (lo, hi))
    codes = split_code_stream(tokens, stages, K)
    assert tuple(codes.shape) == (U, stages, frames) and int(codes.min()) >= 0 and int(codes.max()) < K
    assert len(np.unique(t)) > stages
    assert torch.equal(fg.generate_codes(net, x[:1], frames * stages, **kw), tokens[0])
    # a stream that starts inside a frame: window_pos is the position of the first code returned
    late = fg.generate_codes_batch(net, x, 6, window_pos=stages - 1, **kw).cpu().numpy()
    for j in range(6):
        lo, hi = wins[(stages - 1 + j) % stages]
        assert ((lo <= late[:, j]) & (late[:, j] < hi)).all(), j
    with pytest.raises(ValueError, match="correct_queue=True"):
        fg.generate_codes_batch(net, x, 6, windows=wins)


def _suite(name):
    from music_amd import fast_generate as fg
    kw, tables = MODELS[name]
    net = _model(**kw)
    assert fg._mfma_decode(net._engine_for(torch.device("cuda", 0))) == (name == "mfma")
    Q = net.quantization_channels
    _whole_alphabet_is_the_sampling_entry(net, Q)
    for stages, K in tables:
        wins = fg.stage_windows(stages, K)
        _teacher_forced(net, wins, Q)
        _two_launches(net, wins)
        _batch_rows(net, wins)
        _free_running(net, stages, K)


@pytest.mark.parametrize("ks", ["1", "4"], ids=["one-workgroup-skip-stage", "split-skip-stage"])
def test_matrix_core_decode_under_windows(ks):
    """64 / 64 / 256 / 256, dilations 1..16, windows stage_windows(2, 128) and (4, 64).  WN_DEC_KS (read once per process, hence the
    child process) holds the skip stage's form fixed, as tests/test_gpu_decode_sample.py does: a batch and a single launch are
    comparable bit for bit in the same form only."""
    e = dict(os.environ, WN_DEC_KS=ks, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from tests.test_gpu_window_decode import _suite; _suite('mfma')"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, check=True, timeout=600)


@pytest.mark.parametrize("name", ["q96", "q64", "q1024"])
def test_fp32_decode_under_windows(name):
    """decode_k: Q = 96 with windows (3, 32) (two entries per lane, the last lanes padding), Q = 64 with (4, 16) (one entry per
    lane), Q = 1024 with (8, 128) (sixteen per lane), three or four blocks"""
    _suite(name)


def test_code_prior_to_audio_end_to_end():
    """A tiny residual-vq autoencoder (2 stages of 16 codes, learned conditioning) and a prior over its 32 tokens: the codes of two
    clips become the token stream tools/vq_codes_dataset.py writes (frame-major, token = s K + code), sample_code_stream continues
    it by three frames under the stage windows, and decode_codes turns the new codes into audio codes."""
    from music_amd import ae_generate as ag
    from music_amd.model import wavenet
    from music_amd.model1 import wavenet_autoencoder
    from tests.test_gpu_cond_learned import _cfg
    S, K, pool, W = 2, 16, 8, 64
    torch.manual_seed(5)
    ae = wavenet_autoencoder(**dict(_cfg(en=(32, 32), de=(32, 32, 64), bw=16, pool=pool, bias=False), bottleneck="vq", vq_codes=K,
                                    vq_stages=S)).cuda()
    prior = wavenet(filter_width=2, dilations=[1, 2, 4], dilation_channels=16, residual_channels=16, skip_channels=32,
                    quantization_channels=S * K, use_bias=False)
    with torch.no_grad():
        for p in prior.parameters():
            p.mul_(2.0)
    prior = prior.cuda()
    rng = np.random.default_rng(9)
    clips = torch.from_numpy(rng.integers(0, 256, size=(2, ae.receptive_field - 1 + W)))
    x = torch.nn.functional.one_hot(clips, 256).permute(0, 2, 1).float().contiguous().cuda()
    codes = ag.encode_codes(ae, x)                                                 # (2, S, Le)
    Le = W // pool
    assert tuple(codes.shape) == (2, S, Le)
    stream = (codes.permute(0, 2, 1) + torch.arange(S, device=codes.device) * K).reshape(2, Le * S)
    assert torch.equal(ag.split_code_stream(stream, S, K).to(codes.device), codes) and Le * S >= prior.receptive_field
    new = ag.sample_code_stream(prior, S, K, frames=3, start_tokens=stream, temperature=1.0, top_p=0.9, seed=4)
    assert new.dtype == torch.int64 and tuple(new.shape) == (2, S, 3) and int(new.min()) >= 0 and int(new.max()) < K
    again = ag.sample_code_stream(prior, S, K, frames=3, start_tokens=stream, temperature=1.0, top_p=0.9, seed=4)
    assert torch.equal(new, again)
    audio, _ = ag.decode_codes(ae, new, 3 * pool)
    assert audio.dtype == torch.int64 and tuple(audio.shape) == (2, 3 * pool) and int(audio.min()) >= 0 and int(audio.max()) < 256
    # a prompt that ends inside a frame is refused; with the position that makes it a frame boundary it is taken
    with pytest.raises(ValueError, match="frame boundary"):
        ag.sample_code_stream(prior, S, K, 3, stream[:, 1:])
    assert tuple(ag.sample_code_stream(prior, S, K, 2, stream[:, 1:], start_pos=1).shape) == (2, S, 2)
