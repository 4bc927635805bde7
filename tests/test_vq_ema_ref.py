"""tests/vq_ema_ref.py alone: the EMA update is the decayed k-means centroid, an unused row does not move, the pairing of dead
codes and donors, and the independence from the order in which ranks' partial stats are summed.  No device is touched."""
import numpy as np

from tests import vq_ema_ref as er
from tests import vq_ref


def _batch(seed, B=3, Bw=5, Le=7, K=9):
    rng = np.random.default_rng(seed)
    enc, cb = rng.standard_normal((B, Bw, Le)), rng.standard_normal((K, Bw))
    return enc, cb, vq_ref.forward(enc, cb)["idx"]


def test_stats_count_and_sum_the_frames_of_every_code():
    enc, cb, idx = _batch(1)
    K = cb.shape[0]
    n, s = er.split(er.stats(enc, idx, K), K)
    assert n.sum() == idx.size and np.array_equal(n, np.bincount(idx.reshape(-1), minlength=K))
    frames = enc.transpose(0, 2, 1).reshape(-1, enc.shape[1])
    for k in range(K):
        np.testing.assert_allclose(s[k], frames[idx.reshape(-1) == k].sum(0), rtol=0, atol=1e-13)
    bad = idx.copy()
    bad[0, 0], bad[1, 1] = K, -1                     # codes outside [0, K) belong to no code
    assert er.split(er.stats(enc, bad, K), K)[0].sum() == idx.size - 2
    state = er.initial_state(cb)
    assert np.array_equal(er.split(state, K)[0], np.ones(K)) and np.array_equal(er.split(state, K)[1], cb)


def test_one_update_without_smoothing_is_the_decayed_kmeans_centroid():
    """state [n_prev | s_prev], eps = 0: c' = (g s_prev + (1 - g) s) / (g n_prev + (1 - g) n), the centroid of the old and the new
    frames weighted g : (1 - g)."""
    enc, cb, idx = _batch(2)
    enc0, _, _ = _batch(3)
    K, g = cb.shape[0], 0.8
    prev = er.stats(enc0, vq_ref.forward(enc0, cb)["idx"], K)
    n0, s0 = er.split(prev, K)
    seen = n0 > 0
    assert seen.sum() >= 3
    stat = er.stats(enc, idx, K)
    n, s = er.split(stat, K)
    out = er.update(stat, prev, K, g, eps=0.0)
    want = (g * s0 + (1 - g) * s)[seen] / (g * n0 + (1 - g) * n)[seen, None]
    np.testing.assert_allclose(out["cb"][seen], want, rtol=1e-12, atol=0)
    N1, m1 = er.split(out["state"], K)
    np.testing.assert_allclose(N1, g * n0 + (1 - g) * n, rtol=1e-15)
    np.testing.assert_allclose(m1, g * s0 + (1 - g) * s, rtol=1e-15, atol=1e-300)
    assert out["restarted"] == 0 and out["left"] == 0 and (out["donor"] == -1).all()
    assert abs(out["tot"] - N1.sum()) <= 1e-12 * N1.sum()


def test_an_unused_code_does_not_move_without_smoothing():
    rng = np.random.default_rng(4)
    enc, cb = rng.standard_normal((2, 6, 3)), rng.standard_normal((40, 6))
    idx = vq_ref.forward(enc, cb)["idx"]
    K = 40
    state = er.initial_state(cb)
    for _ in range(3):
        stat = er.stats(enc, idx, K)
        unused = er.split(stat, K)[0] == 0
        assert unused.sum() >= 34
        out = er.update(stat, state, K, 0.9, eps=0.0)
        assert np.abs(out["cb"][unused] - cb[unused]).max() <= 1e-12
        state = out["state"]
    # with smoothing the unused rows do move (towards 0): the rule, not an accident
    moved = er.update(stat, er.initial_state(cb), K, 0.9, eps=0.1)["cb"]
    assert np.abs(moved[unused] - cb[unused]).max() > 1e-3


def _pair(n, N, g=0.5, r=0.75):
    K = len(n)
    stat = er.join(n, (np.arange(K * 2, dtype=np.float64).reshape(K, 2) + 1.0) * (n[:, None] > 0))     # (no frames: no sum)
    state = er.join(N, np.full((K, 2), 7.0))
    return er.update(stat, state, K, g, eps=0.0, restart=r), er.split(stat, K), er.split(state, K)


def test_restart_pairing_order_ties_and_shortage():
    # N' = 0.5 N + 0.5 n:      k:  0     1     2     3     4     5     6
    n = np.array([0.0, 6.0, 0.0, 9.0, 6.0, 1.0, 0.0])
    N = np.array([1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 1.25])
    out, (n_, s), (N_, m) = _pair(n, N)
    assert np.allclose(out["N1"], [0.5, 3.5, 0.25, 5.0, 3.5, 1.0, 0.625])
    # dead: 0, 2, 6 (ascending); donors: 3 (n 9), then 1 and 4 (n 6, the smaller index first); code 5 (n = 1) never donates
    assert out["donor"].tolist() == [3, -1, 1, -1, -1, -1, 4] and out["restarted"] == 3 and out["left"] == 0
    N2, m2 = er.split(out["state"], 7)
    for j, k in ((0, 3), (2, 1), (6, 4)):
        assert np.array_equal(out["cb"][j], s[k] / n[k]) and N2[j] == 1.0 and np.array_equal(m2[j], out["cb"][j])
    for k in (1, 3, 4, 5):                                   # donors and bystanders: the plain update
        assert N2[k] == out["N1"][k] and np.array_equal(m2[k], 0.5 * m[k] + 0.5 * s[k])
        np.testing.assert_allclose(out["cb"][k], m2[k] / N2[k], rtol=1e-12)
    # a restarted row is the donor's BATCH mean, not its running centroid
    assert not np.allclose(out["cb"][0], out["cb"][3])
    # more dead codes than donors: the first ones in index order are served, the others keep the plain update
    n = np.array([0.0, 0.0, 5.0, 0.0, 1.0])
    N = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    out, (n_, s), (N_, m) = _pair(n, N)
    assert out["donor"].tolist() == [2, -1, -1, -1, -1] and out["restarted"] == 1 and out["left"] == 2
    N2, m2 = er.split(out["state"], 5)
    assert N2[1] == 0.5 and np.array_equal(m2[1], 0.5 * m[1]) and np.allclose(out["cb"][1], m[1] / N[1])
    # no donor at all (every live code has a single frame), and a dead code is never a donor however many frames it has
    out, _, _ = _pair(np.array([0.0, 1.0, 1.0]), np.array([1.0, 1.0, 1.0]))
    assert (out["donor"] == -1).all() and out["restarted"] == 0 and out["left"] == 1
    out, _, _ = _pair(np.array([2.0, 0.0, 0.0]), np.array([0.25, 2.0, 1.0]), r=1.25)      # N' = 1.125 (dead, n = 2), 1.0, 0.5
    assert (out["donor"] == -1).all() and out["left"] == 3
    # restart = 0: never
    out, _, _ = _pair(np.array([0.0, 9.0]), np.array([1e-9, 1.0]), r=0.0)
    assert (out["donor"] == -1).all() and out["restarted"] == 0 and out["left"] == 0


def test_the_order_in_which_ranks_stats_are_summed_does_not_matter():
    """Grid inputs (multiples of 1/8): every partial sum is exact, so any order of the ranks gives the same stat, hence the same
    update; the sum of the shards' stats is the stat of the whole batch."""
    rng = np.random.default_rng(6)
    K, Bw = 11, 4
    enc = rng.integers(-16, 17, size=(6, Bw, 5)) / 8.0
    cb = rng.integers(-16, 17, size=(K, Bw)) / 8.0
    idx = vq_ref.forward(enc, cb)["idx"]
    shards = [er.stats(enc[i:i + 2], idx[i:i + 2], K) for i in (0, 2, 4)] + [np.zeros(K * (Bw + 1))]      # (an empty shard: zeros)
    whole = er.stats(enc, idx, K)
    state = er.initial_state(cb)
    ref = er.update(whole, state, K, 0.99, 1e-5, 0.995)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        total = np.zeros_like(whole)
        for r in order:
            total = total + shards[r]
        assert np.array_equal(total, whole)
        out = er.update(total, state, K, 0.99, 1e-5, 0.995)
        assert np.array_equal(out["state"], ref["state"]) and np.array_equal(out["cb"], ref["cb"]) and np.array_equal(out["donor"], ref["donor"])
    assert ref["restarted"] >= 1
