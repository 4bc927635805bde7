"""Position-windowed sampling at kernel level: wn_win_sample_logits against tests/window_ref.py, the float64 rule of
include/wavenet_hip.h applied inside each row's window.

Bars: those of tests/test_gpu_decode_sample.py on the windowed reference - kept sets EXACT, the only excuse a top-p boundary (a
candidate threshold whose sliced float64 head mass lies within 1e-5 of top_p, at most 2 % of a case's rows; counted on the CPU in
tests/test_window_ref.py); probabilities within 1e-6; the code is the inverse CDF of the RETURNED row within +-1e-5 and lies inside
the kept set - plus exact zeros everywhere outside the window, whatever stands there.  A row whose logits inside its window are all
-inf has no distribution: its code must still lie inside the window (and outside it the zeros stay exact).
Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sampling_ref as sr
from tests import window_ref as wr

P_TOL = 1e-6
BAND = 1e-5
TINY = 1e-30
CASES = [(k, p) for k in (0, 1, 5, 40) for p in sr.TOP_P]

_INPUTS = {}


def _inputs(Q):
    """(rows, hostile rows, u, temperatures, windows of the rows, dead mask, table): computed once per Q, never modified"""
    if Q not in _INPUTS:
        rows, u = sr.make_rows(Q)
        wins = wr.row_windows(Q)
        _INPUTS[Q] = (rows, wr.hostile(rows, wins), u, sr.temperatures(sr.ROWS), wins, wr.dead(rows, wins), wr.window_table(Q))
    return _INPUTS[Q]


def _check_rows(rows, wins, dead, T, top_k, top_p, u, codes, probs):
    """every row of one wn_win_sample_logits launch against the windowed rule; returns the number of excused rows"""
    excused = 0
    Q = rows.shape[1]
    for i, (lo, hi) in enumerate(wins):
        c = int(codes[i])
        assert lo <= c < hi, ("code outside the window", i, (lo, hi), c)
        out = np.ones(Q, bool)
        out[lo:hi] = False
        assert (probs[i][out].view(np.int32) == 0).all(), ("not an exact zero outside the window", i, (lo, hi))
        if dead[i]:
            continue
        ref = wr.windowed_row(rows[i], lo, hi, T[i], top_k, top_p)
        sup = probs[i] > 0
        l64 = rows[i].astype(np.float64)
        e = np.zeros(Q)
        e[lo:hi] = np.exp((l64[lo:hi] - l64[lo:hi].max()) / (T[i] if T[i] > 0 else 1.0))
        which = None
        for j, cand in enumerate(ref.alt):                  # the rule's set first, then what a boundary row may round to
            full = np.where(cand, e, 0.0)
            full = full / full.sum()
            if not (sup & ~cand).any() and (full[cand & ~sup] < TINY).all():
                which, r = j, full
                break
        assert which is not None, ("kept set", i, (lo, hi), top_k, top_p, np.nonzero(sup)[0][:12], np.nonzero(ref.N)[0][:12])
        excused += which > 0
        assert np.abs(probs[i] - r).max() < P_TOL, (i, (lo, hi), top_k, top_p, np.abs(probs[i] - r).max())
        kept = ref.alt[which]
        assert kept[c], ("code outside the kept set", i, (lo, hi), top_k, top_p, c, float(u[i]))
        if T[i] > 0:
            cdf = np.cumsum(probs[i].astype(np.float64))
            below = cdf[c - 1] if c > 0 else 0.0
            assert below - BAND <= u[i] < cdf[c] + BAND or (u[i] >= cdf[-1] - BAND and c == np.nonzero(kept)[0][-1]), \
                (i, c, float(u[i]), below, cdf[c])
        else:
            assert c == lo + int(np.argmax(rows[i, lo:hi]))
    return excused


@pytest.mark.parametrize("variant", ["as-they-are", "hostile-outside"])
@pytest.mark.parametrize("Q", sr.QS)
def test_windowed_sampler_follows_the_rule(Q, variant):
    """200 seeded rows, row i under window i mod period of window_table(Q); top_k in {0, 1, 5, 40} x TOP_P and greedy; with everything
    outside each row's window left as it is, or set to the in-window maximum + 300 (even rows) / NaN (odd rows): the reference never
    sees the outside, so both variants face the same expectations."""
    from music_amd import fast_generate as fg
    rows, bad, u, T, wins, dead, table = _inputs(Q)
    x = torch.from_numpy(rows if variant == "as-they-are" else bad).cuda()
    worst = 0
    for k, p in CASES:
        codes, probs = fg.sample_logits(x, temperature=T.tolist(), top_k=k, top_p=p, u=u, want_probs=True, windows=table)
        n = _check_rows(rows, wins, dead, T, k, p, u, codes.cpu().numpy(), probs.cpu().numpy())
        assert n <= sr.EXCUSED_CAP * sr.ROWS, (k, p, n)
        worst = max(worst, n)
    codes, probs = fg.sample_logits(x, temperature=None, u=u, want_probs=True, windows=table)
    _check_rows(rows, wins, dead, np.zeros(sr.ROWS, np.float32), 0, 1.0, u, codes.cpu().numpy(), probs.cpu().numpy())
    print("Q = %d, %s: %d windows, %d cases + greedy of %d rows (%d dead), at most %d rows excused per case"
          % (Q, variant, len(table), len(CASES), sr.ROWS, dead.sum(), worst))


@pytest.mark.parametrize("Q", sr.QS)
def test_whole_alphabet_table_is_the_plain_sampler_bit_for_bit(Q):
    """every pair (0, Q), at several periods and positions: the codes and probability bits of wn_sample_logits"""
    from music_amd import fast_generate as fg
    rows, _, u, T, _, _, _ = _inputs(Q)
    x = torch.from_numpy(rows).cuda()
    for period, pos, (k, p), temp in ((1, 0, (0, 1.0), T.tolist()), (16, 7, (5, 0.9), T.tolist()), (3, 2 ** 40, (40, 0.5), T.tolist()),
                                      (2, 1, (1, 1e-6), T.tolist()), (5, 3, (0, 1.0), None)):
        c0, p0 = fg.sample_logits(x, temperature=temp, top_k=k, top_p=p, u=u, want_probs=True)
        c1, p1 = fg.sample_logits(x, temperature=temp, top_k=k, top_p=p, u=u, want_probs=True, windows=[(0, Q)] * period, window_pos=pos)
        assert torch.equal(c0, c1) and torch.equal(p0.view(torch.int32), p1.view(torch.int32)), (period, pos, k, p)


@pytest.mark.parametrize("Q", [65, 256, 1000])
def test_window_position_rotates_the_table(Q):
    """window_pos = 5 is the table rotated by 5 at position 0, bit for bit; and a large position reduces mod the period"""
    from music_amd import fast_generate as fg
    rows, _, u, T, _, _, table = _inputs(Q)
    x = torch.from_numpy(rows).cuda()
    n = len(table)
    rot = [table[(5 + j) % n] for j in range(n)]
    for k, p in ((0, 1.0), (5, 0.9)):
        kw = dict(temperature=T.tolist(), top_k=k, top_p=p, u=u, want_probs=True)
        a = fg.sample_logits(x, windows=table, window_pos=5, **kw)
        b = fg.sample_logits(x, windows=rot, **kw)
        c = fg.sample_logits(x, windows=table, window_pos=5 + n * (2 ** 36), **kw)
        for other in (b, c):
            assert torch.equal(a[0], other[0]) and torch.equal(a[1].view(torch.int32), other[1].view(torch.int32))
    wins = wr.row_windows(Q, pos=5)
    _check_rows(rows, wins, wr.dead(rows, wins), T, 5, 0.9, u, a[0].cpu().numpy(), a[1].cpu().numpy())


@pytest.mark.parametrize("Q", [65, 256, 1000])
def test_generated_uniforms_and_window_position_are_independent(Q):
    """without u the uniform of row i is that of step step0 + i (seed, stream 0), its window pair (window_pos + i) mod period: moving
    one leaves the other alone"""
    from music_amd import fast_generate as fg
    rows, _, _, T, _, _, table = _inputs(Q)
    x = torch.from_numpy(rows).cuda()
    step0, seed = 2 ** 33 + 11, 9
    for pos in (0, 3):
        wins = wr.row_windows(Q, pos=pos)
        dead = wr.dead(rows, wins)
        for s0 in (step0, 4):
            codes, probs = fg.sample_logits(x, temperature=T.tolist(), top_k=5, top_p=0.9, seed=seed, step0=s0, want_probs=True,
                                            windows=table, window_pos=pos)
            u = np.array([sr.uniform(seed, s0 + i, 0) for i in range(sr.ROWS)])
            assert _check_rows(rows, wins, dead, T, 5, 0.9, u, codes.cpu().numpy(), probs.cpu().numpy()) <= sr.EXCUSED_CAP * sr.ROWS
    for bad in (dict(windows=[(0, Q + 1)]), dict(windows=[]), dict(windows=table, window_pos=-1), dict(window_pos=2)):
        with pytest.raises(ValueError):
            fg.sample_logits(x, **bad)
