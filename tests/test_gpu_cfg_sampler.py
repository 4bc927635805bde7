"""The guided sampler at kernel level: wn_cfg_sample_logits (the decode kernels' combine-and-pick device function on two logits
matrices) against the float64 rule of include/wavenet_hip.h - g = l_c + (s - 1)(l_c - l_u) in float64 (tests/cfg_ref.combine), then
tests/window_ref.py's windowed rule on g.

Q = 64, 100, 256, 1024 (1, 2, 4 and 16 entries per lane); the rows' scales cycle through 0, 1, 1.5, 3 and -0.75; greedy, temperature,
top-k, top-p and both filters, each over the whole alphabet and under window_ref.window_table(Q).

Bars: those of tests/test_gpu_window_sampler.py on the guided reference - codes and kept sets EXACT (the only excuse a top-p boundary:
a candidate threshold whose float64 head mass lies within 1e-5 of top_p, at most 2 % of a case's rows), exact zeros outside the
window - and the probabilities within that test's 1e-6 times (|s| + |s - 1|), the factor by which the rule multiplies an error of its
two inputs.  The logits are unit normal: the kernel forms g in float32 (one rounding of the difference, one of the fused multiply-
add: under 1.5 ulp of |g| < 16, 1.5e-6, before the temperature), which the bar has to hold as well.
s = 1 is the plain windowed sampler on logits_c bit for bit with NaN all over logits_u; NaN outside a row's window, in either
matrix, changes no bit.  Run with -m gpu."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cfg_ref as cr
from tests import sampling_ref as sr
from tests import window_ref as wr

P_TOL = 1e-6                                              # tests/test_gpu_window_sampler.P_TOL, times amp(s) per row
BAND = 1e-5
TINY = 1e-30
QS = [64, 100, 256, 1024]
ROWS = 60
ROW_SCALES = [0.0, 1.0, 1.5, 3.0, -0.75]
SETTINGS = [("temperature", 0, 1.0), ("top-k", 5, 1.0), ("top-p", 0, 0.9), ("both", 40, 0.5)]


@functools.lru_cache(maxsize=None)
def _inputs(Q):
    """(logits_c, logits_u float32, scales, g float64, u, temperatures): computed once per Q, never modified"""
    rng = np.random.default_rng(4000 + Q)
    lc = rng.standard_normal((ROWS, Q)).astype(np.float32)
    lu = rng.standard_normal((ROWS, Q)).astype(np.float32)
    s = np.array([ROW_SCALES[i % len(ROW_SCALES)] for i in range(ROWS)], np.float32)
    u = np.array([sr.U_EDGE[i] if i < 3 else int(rng.integers(0, 1 << 24)) / 16777216.0 for i in range(ROWS)], np.float32)
    return lc, lu, s, cr.combine(lc, lu, s), u, sr.temperatures(ROWS)


def _wins(Q, table):
    return [table[i % len(table)] for i in range(ROWS)] if table else [(0, Q)] * ROWS


def _check_rows(g, s, wins, T, top_k, top_p, u, codes, probs):
    """every row of one launch against the windowed rule on g; returns (rows excused, worst share of the probability bar)"""
    excused, worst = 0, 0.0
    Q = g.shape[1]
    for i, (lo, hi) in enumerate(wins):
        c = int(codes[i])
        assert lo <= c < hi, ("code outside the window", i, (lo, hi), c)
        out = np.ones(Q, bool)
        out[lo:hi] = False
        assert (probs[i][out].view(np.int32) == 0).all(), ("not an exact zero outside the window", i, (lo, hi))
        ref = wr.windowed_row(g[i], lo, hi, T[i], top_k, top_p)
        sup = probs[i] > 0
        e = np.zeros(Q)
        e[lo:hi] = np.exp((g[i, lo:hi] - g[i, lo:hi].max()) / (T[i] if T[i] > 0 else 1.0))
        which = None
        for j, cand in enumerate(ref.alt):                  # the rule's set first, then what a boundary row may round to
            full = np.where(cand, e, 0.0)
            full = full / full.sum()
            if not (sup & ~cand).any() and (full[cand & ~sup] < TINY).all():
                which, r = j, full
                break
        assert which is not None, ("kept set", i, float(s[i]), (lo, hi), top_k, top_p, np.nonzero(sup)[0][:12], np.nonzero(ref.N)[0][:12])
        excused += which > 0
        bar = P_TOL * cr.amp([s[i]])
        err = float(np.abs(probs[i] - r).max())
        worst = max(worst, err / bar)
        assert err <= bar, (i, float(s[i]), (lo, hi), top_k, top_p, err, bar)
        kept = ref.alt[which]
        assert kept[c], ("code outside the kept set", i, (lo, hi), top_k, top_p, c, float(u[i]))
        if T[i] > 0:
            cdf = np.cumsum(probs[i].astype(np.float64))
            below = cdf[c - 1] if c > 0 else 0.0
            assert below - BAND <= u[i] < cdf[c] + BAND or (u[i] >= cdf[-1] - BAND and c == np.nonzero(kept)[0][-1]), \
                (i, c, float(u[i]), below, cdf[c])
        else:
            assert c == lo + int(np.argmax(g[i, lo:hi]))
    return excused, worst


@pytest.mark.parametrize("windowed", [False, True], ids=["whole-alphabet", "windows"])
@pytest.mark.parametrize("Q", QS)
def test_guided_sampler_follows_the_rule(Q, windowed):
    from music_amd import fast_generate as fg
    lc, lu, s, g, u, T = _inputs(Q)
    table = wr.window_table(Q) if windowed else None
    wins = _wins(Q, table)
    xc, xu = torch.from_numpy(lc).cuda(), torch.from_numpy(lu).cuda()
    kw = dict(u=u, want_probs=True, windows=table, guidance=s.tolist(), logits_u=xu)
    worst = 0.0
    # the greedy margins the exact argmax rests on: 1e-4 (|s| + |s - 1|) in float64, far over float32's rounding of g
    for i, (lo, hi) in enumerate(wins):
        assert cr.top2_margin(g[i], lo, hi) > 1e-4 * cr.amp([s[i]]), ("inputs", Q, i)
    codes, probs = fg.sample_logits(xc, temperature=None, **kw)
    n, w = _check_rows(g, s, wins, np.zeros(ROWS, np.float32), 0, 1.0, u, codes.cpu().numpy(), probs.cpu().numpy())
    worst = max(worst, w)
    for name, k, p in SETTINGS:
        codes, probs = fg.sample_logits(xc, temperature=T.tolist(), top_k=k, top_p=p, **kw)
        n, w = _check_rows(g, s, wins, T, k, p, u, codes.cpu().numpy(), probs.cpu().numpy())
        assert n <= max(1, sr.EXCUSED_CAP * ROWS), (name, n)
        worst = max(worst, w)
    print("Q = %d, %s: greedy + %d settings of %d rows, worst share of the probability bar %.3f" % (Q, "windows" if windowed else "plain", len(SETTINGS), ROWS, worst))
    # the guided rows are not the conditional ones: wherever s != 1 the distribution moved by far more than the bar
    _, pp = fg.sample_logits(xc, temperature=T.tolist(), u=u, want_probs=True, windows=table)
    _, p1 = fg.sample_logits(xc, temperature=T.tolist(), **kw)
    wide = np.array([hi - lo >= 16 for lo, hi in wins])       # (a window of one entry has one distribution, a few entries may agree)
    moved = (p1 - pp).abs().amax(1).cpu().numpy()
    assert (moved[(s != 1.0) & wide] > 100 * P_TOL * 5).all() and (moved[s == 1.0] == 0).all()


@pytest.mark.parametrize("Q", QS)
def test_scale_one_is_the_windowed_sampler_on_the_conditional_logits_bit_for_bit(Q):
    """s = 1 never reads logits_u: NaN all over it (and inf in places), every setting, with and without windows"""
    from music_amd import fast_generate as fg
    lc, lu, s, g, u, T = _inputs(Q)
    xc = torch.from_numpy(lc).cuda()
    bad = np.full_like(lu, np.nan)
    bad[::3, ::5] = np.inf
    bad[1::3, 1::7] = -np.inf
    xu = torch.from_numpy(bad).cuda()
    for table in (None, wr.window_table(Q)):
        for temp, k, p in [(None, 0, 1.0)] + [(T.tolist(), k, p) for _, k, p in SETTINGS]:
            kw = dict(temperature=temp, top_k=k, top_p=p, u=u, want_probs=True, windows=table, window_pos=3 if table else 0)
            c0, p0 = fg.sample_logits(xc, **kw)
            c1, p1 = fg.sample_logits(xc, guidance=1.0, logits_u=xu, **kw)
            assert torch.equal(c0, c1) and torch.equal(p0.view(torch.int32), p1.view(torch.int32)), (table is not None, k, p)
    # mixed scales: the rows at s = 1 keep the plain sampler's bits next to guided rows (their NaN rows of logits_u are never read)
    mixed = lu.copy()
    mixed[s == 1.0] = np.nan
    kw = dict(temperature=T.tolist(), top_k=40, top_p=0.9, u=u, want_probs=True)
    c0, p0 = fg.sample_logits(xc, **kw)
    c1, p1 = fg.sample_logits(xc, guidance=s.tolist(), logits_u=torch.from_numpy(mixed).cuda(), **kw)
    one = torch.from_numpy(s == 1.0).cuda()
    assert torch.equal(c0[one], c1[one]) and torch.equal(p0[one].view(torch.int32), p1[one].view(torch.int32))
    assert not bool(torch.isnan(p1).any())


@pytest.mark.parametrize("Q", QS)
def test_nan_outside_the_window_influences_nothing(Q):
    """NaN (even rows) or the in-window maximum + 300 (odd rows) everywhere outside each row's window, in both matrices: the bits of
    the launch on the clean matrices"""
    from music_amd import fast_generate as fg
    lc, lu, s, g, u, T = _inputs(Q)
    table = wr.window_table(Q)
    wins = _wins(Q, table)

    def hostile(a, fill):
        out = a.copy()
        for i, (lo, hi) in enumerate(wins):
            v = np.float32(np.nan) if (i % 2 == 0) == fill else np.float32(a[i, lo:hi].max() + 300.0)
            out[i, :lo] = v
            out[i, hi:] = v
        return out
    xc, xu = torch.from_numpy(lc).cuda(), torch.from_numpy(lu).cuda()
    hc, hu = torch.from_numpy(hostile(lc, True)).cuda(), torch.from_numpy(hostile(lu, False)).cuda()
    for temp, k, p in [(None, 0, 1.0)] + [(T.tolist(), k, p) for _, k, p in SETTINGS]:
        kw = dict(temperature=temp, top_k=k, top_p=p, u=u, want_probs=True, windows=table, guidance=s.tolist())
        c0, p0 = fg.sample_logits(xc, logits_u=xu, **kw)
        c1, p1 = fg.sample_logits(hc, logits_u=hu, **kw)
        assert torch.equal(c0, c1) and torch.equal(p0.view(torch.int32), p1.view(torch.int32)), (k, p)


def test_generated_uniforms_streams_and_refusals():
    """without u the uniform of row i is that of step step0 + i of the row's stream (its own settings: the guided sampler has no second
    row to take them from); the Python wrapper's refusals"""
    from music_amd import fast_generate as fg
    Q = 256
    lc, lu, s, g, _, T = _inputs(Q)
    xc, xu = torch.from_numpy(lc).cuda(), torch.from_numpy(lu).cuda()
    step0, seed = 2 ** 33 + 11, 9
    streams = [(7 * i) % 13 for i in range(ROWS)]
    codes, probs = fg.sample_logits(xc, temperature=T.tolist(), top_k=5, top_p=0.9, seed=seed, step0=step0, want_probs=True, streams=streams,
                                    guidance=s.tolist(), logits_u=xu)
    u = np.array([sr.uniform(seed, step0 + i, streams[i]) for i in range(ROWS)])
    n, _ = _check_rows(g, s, _wins(Q, None), T, 5, 0.9, u, codes.cpu().numpy(), probs.cpu().numpy())
    assert n <= max(1, sr.EXCUSED_CAP * ROWS)
    for bad in (dict(guidance=1.5), dict(logits_u=xu), dict(guidance=1.5, logits_u=xu[:, :100]), dict(guidance=[1.0, 2.0], logits_u=xu),
                dict(guidance=float("nan"), logits_u=xu), dict(guidance=1.5, logits_u=xu.cpu())):
        with pytest.raises(ValueError):
            fg.sample_logits(xc, **bad)
