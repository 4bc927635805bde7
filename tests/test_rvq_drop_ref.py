"""tests/rvq_drop_ref.py (quantiser dropout: a stage count per clip) against tests/rvq_ref.py: with every clip on all S stages the two
are the same numbers, with mixed counts every clip is what rvq_ref gives that clip alone at S = n_b (a brute-force loop), and a stage
nobody used leaves exact zeros in d_cb and the statistics.  No device."""
import numpy as np
import pytest

from tests import rvq_drop_ref as dr
from tests import rvq_ref

BETA = 0.25


def draw(S, K, Bw, B, Le, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, Bw, Le)), rng.standard_normal((S * K, Bw)) * 0.7, rng.standard_normal((B, Bw, Le))


@pytest.mark.parametrize("S", [1, 3, 8])
def test_all_stages_active_equals_the_chain_exactly(S):
    K, Bw, B, Le = 9, 5, 3, 7
    enc, cb, d_q = draw(S, K, Bw, B, Le, seed=S)
    for n in ([S] * B, [S + 3] * B):                                     # (a count above S is clamped to S)
        f, g = dr.forward(enc, cb, S, n, BETA), rvq_ref.forward(enc, cb, S, BETA)
        for k in ("idx", "q", "res", "r", "mse", "counts", "dist"):
            assert np.array_equal(f[k], g[k]), k
        assert f["vq_loss"] == g["vq_loss"] and (f["stage_frames"] == B * Le).all()
        assert dr.forward(enc, cb, S, n, BETA, ema=True)["vq_loss"] == rvq_ref.forward(enc, cb, S, BETA, ema=True)["vq_loss"]
        a, b = dr.backward(enc, cb, S, n, f["idx"], d_q, BETA, 1.5), rvq_ref.backward(enc, cb, S, g["idx"], d_q, BETA, 1.5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        a = dr.backward(enc, cb, S, n, f["idx"], d_q, BETA, 1.5, residuals=f["res"])
        b = rvq_ref.backward(enc, cb, S, g["idx"], d_q, BETA, 1.5, residuals=g["res"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(dr.lookup(cb, S, f["idx"], n), rvq_ref.lookup(cb, S, g["idx"]))
        assert np.array_equal(dr.stats(enc, cb, S, n, f["idx"]), rvq_ref.stats(enc, cb, S, g["idx"]))


@pytest.mark.parametrize("S,nstage", [(3, [1, 3, 2, 3]), (8, [8, 1, 5, 0]), (4, [1, 1, 1, 1]), (2, [2, 1, 2, 1])])
def test_mixed_counts_equal_a_per_clip_loop_over_the_chain(S, nstage):
    K, Bw, B, Le = 9, 5, 4, 7
    enc, cb, d_q = draw(S, K, Bw, B, Le, seed=10 + S)
    n = np.clip(nstage, 1, S)
    f = dr.forward(enc, cb, S, nstage, BETA)
    assert np.array_equal(f["n"], n)
    d_enc, d_cb = dr.backward(enc, cb, S, nstage, f["idx"], d_q, BETA, 0.5)
    stat = dr.stats(enc, cb, S, nstage, f["idx"])
    q_look = dr.lookup(cb, S, f["idx"], nstage)
    mse, counts, d_cb_loop, stat_loop = np.zeros(S), np.zeros((S, K), dtype=np.int64), np.zeros_like(d_cb), np.zeros_like(stat)
    for b in range(B):
        nb = int(n[b])
        one = rvq_ref.forward(enc[b:b + 1], cb[:nb * K], nb, BETA)         # the clip alone, on the first n_b codebooks
        assert np.array_equal(f["idx"][:nb, b], one["idx"][:, 0]) and (f["idx"][nb:, b] == -1).all()
        assert np.array_equal(f["q"][b], one["q"][0]) and np.array_equal(q_look[b], one["q"][0])
        assert np.array_equal(f["res"][:nb, b], one["res"][:, 0])
        assert all(np.array_equal(f["res"][s, b], one["res"][-1, 0]) for s in range(nb, S)), "the carried residual"
        mse[:nb] += one["mse"] / B                                          # the clip's own mean -> its share of the batch's
        counts[:nb] += one["counts"]
        # the clip alone scales by 2 / (Bw Le): 1 / B of that is the batch's 2 / (C Bw)
        e1, c1 = rvq_ref.backward(enc[b:b + 1], cb[:nb * K], nb, one["idx"], None, BETA, 0.5)
        assert np.allclose(d_enc[b], d_q[b] + e1[0] / B, rtol=0, atol=1e-15)
        d_cb_loop[:nb * K] += c1 / B
        stat_loop[:nb] += rvq_ref.stats(enc[b:b + 1], cb[:nb * K], nb, one["idx"])
    assert np.allclose(f["mse"], mse, rtol=1e-14, atol=0) and np.array_equal(f["counts"], counts)
    assert np.array_equal(f["stage_frames"], [(n > s).sum() * Le for s in range(S)]) and np.array_equal(f["counts"].sum(1), f["stage_frames"])
    assert np.allclose(d_cb, d_cb_loop, rtol=0, atol=1e-15)
    assert np.array_equal(stat[:, :K], counts) and np.allclose(stat, stat_loop, rtol=0, atol=1e-13)
    assert abs(f["vq_loss"] - (1 + BETA) * mse.sum()) <= 1e-14 * f["vq_loss"]
    assert np.isnan(f["dist"][f["idx"] < 0]).all() and np.isfinite(f["dist"][f["idx"] >= 0]).all()


def test_a_stage_nobody_used_leaves_exact_zeros():
    S, K, Bw, B, Le = 4, 6, 5, 3, 4
    enc, cb, d_q = draw(S, K, Bw, B, Le, seed=7)
    nstage = [2, 1, 2]
    f = dr.forward(enc, cb, S, nstage, BETA)
    d_enc, d_cb = dr.backward(enc, cb, S, nstage, f["idx"], d_q, BETA)
    stat = dr.stats(enc, cb, S, nstage, f["idx"])
    assert (d_cb[2 * K:] == 0).all() and not np.signbit(d_cb[2 * K:]).any() and (d_cb[:2 * K] != 0).any()
    assert (stat[2:] == 0).all() and (stat[:2, :K].sum(1) == [3 * Le, 2 * Le]).all()
    assert (f["mse"][2:] == 0).all() and (f["counts"][2:] == 0).all() and (f["idx"][2:] == -1).all() and (f["idx"][1, 1] == -1).all()
    assert np.array_equal(f["res"][3], f["res"][1]) and np.array_equal(f["res"][1, 1], f["res"][0, 1])
    # the commitment gradient sums the ACTIVE stages' residuals
    want = d_q + BETA * 2.0 / enc.size * np.stack([f["res"][:2, 0].sum(0), f["res"][0, 1], f["res"][:2, 2].sum(0)])
    assert np.allclose(d_enc, want, rtol=0, atol=1e-15)
