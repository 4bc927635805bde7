"""CPU checks of tests/sampling_ref.py (the float64 restatement of the sampling rule the GPU tests compare against) on cases
small enough to work out by hand, and of the Python surface's argument checks (no device needed)."""
import numpy as np
import pytest

from tests import sampling_ref as sr


def test_ties_at_the_k_boundary_are_kept():
    l = np.array([1.0, 3.0, 2.0, 2.0, 0.0, 2.0], np.float32)
    row = sr.sample_row(l, 1.0, top_k=2)
    assert row.K.tolist() == [False, True, True, True, False, True]        # the 2nd largest is 2.0: all three twos stay
    e = np.exp(np.array([3.0, 2.0, 2.0, 2.0]) - 3.0)
    assert np.allclose(row.r[[1, 2, 3, 5]], e / e.sum(), atol=1e-15) and row.r[0] == 0.0 and row.r[4] == 0.0
    assert sr.sample_row(l, 1.0, top_k=1).N.tolist() == [False, True, False, False, False, False]
    assert sr.sample_row(l, 1.0, top_k=5).N.tolist() == [True, True, True, True, False, True]


def test_top_k_at_or_above_q_and_non_positive_is_off():
    l = np.array([0.5, -1.0, 2.0], np.float32)
    plain = sr.sample_row(l, 0.7)
    for k in (0, -3, 3, 10, None):
        row = sr.sample_row(l, 0.7, top_k=k)
        assert row.N.all() and np.array_equal(row.r, plain.r)
    e = np.exp((l.astype(np.float64) - 2.0) / 0.7)
    assert np.allclose(plain.r, e / e.sum(), atol=1e-15)


def test_top_p_with_an_exact_tie_at_tau():
    # probabilities 1/2, 1/8, 1/8, 1/8, 1/8 (logits ln 4 apart: exact enough in float64 to stay clear of every boundary)
    l = np.log(np.array([4.0, 1.0, 1.0, 1.0, 1.0]))
    assert sr.sample_row(l, 1.0, top_p=0.5).N.tolist() == [True, False, False, False, False]       # mass 0.5 >= 0.5
    row = sr.sample_row(l, 1.0, top_p=0.55)
    assert row.N.all()                                                   # tau is the tied value: all four ties are kept
    assert np.allclose(row.r, [0.5, 0.125, 0.125, 0.125, 0.125])
    assert sr.sample_row(l, 1.0, top_p=1.0).N.all() and sr.sample_row(l, 1.0, top_p=0.0).N.all()    # off
    # top-k first, then top-p on the renormalised rest
    l2 = np.log(np.array([4.0, 2.0, 1.0, 1.0]))
    row = sr.sample_row(l2, 1.0, top_k=2, top_p=0.7)                      # K = {4, 2}: p = 2/3, 1/3; 2/3 < 0.7: both
    assert row.N.tolist() == [True, True, False, False] and np.allclose(row.r, [2 / 3, 1 / 3, 0, 0])
    assert sr.sample_row(l2, 1.0, top_k=2, top_p=0.6).N.tolist() == [True, False, False, False]


def test_one_hot_row_and_a_single_entry():
    l = np.full(7, -np.inf, np.float32)
    l[4] = 0.25
    for kw in (dict(), dict(top_k=3), dict(top_p=0.3), dict(top_k=1, top_p=1e-6)):
        for u in (0.0, 0.5, 1 - 2.0 ** -24):
            row = sr.sample_row(l, 1.3, u=u, **kw)
            assert row.code == 4 and row.r[4] == 1.0 and row.r.sum() == 1.0
    for u in (0.0, 0.999):
        row = sr.sample_row(np.array([-3.0], np.float32), 0.5, top_k=1, top_p=0.5, u=u)
        assert row.code == 0 and row.r.tolist() == [1.0] and row.N.tolist() == [True]


def test_draw_and_the_fallback_to_the_largest_kept_index():
    r = np.array([0.0, 0.25, 0.0, 0.75, 0.0])
    N = np.array([False, True, False, True, False])
    assert [sr.draw(r, N, u) for u in (0.0, 0.2499, 0.25, 0.9999)] == [1, 1, 3, 3]
    short = r * (1 - 1e-7)                                              # a total that rounded below u
    assert sr.draw(short, N, 1 - 2.0 ** -24) == 3                       # the largest index IN N, not Q - 1 = 4
    assert sr.sample_row(np.array([0.0, 1.0, 5.0, 1.0]), 0, top_k=1).code == 2          # greedy: filters ignored
    g = sr.sample_row(np.array([5.0, 1.0, 5.0]), -1.0, top_k=1, top_p=0.1)
    assert g.code == 0 and g.N.all() and np.allclose(g.r.sum(), 1.0)


def test_near_boundary_rows_list_both_sides():
    l = np.log(np.array([4.0, 1.0, 1.0, 1.0, 1.0]))
    row = sr.sample_row(l, 1.0, top_p=0.5 + 1e-7)
    assert len(row.near) == 1 and row.N.all()
    sets = [a.tolist() for a in row.alt]
    assert [True, False, False, False, False] in sets and [True] * 5 in sets
    assert sr.sample_row(l, 1.0, top_p=0.6).near == []


def test_uniform_matches_the_generator_restated_in_the_parity_tests():
    def uniform(seed, step):                                            # tests/test_gpu_parity.py, utterance 0
        M = (1 << 64) - 1
        z = (seed + 0x9E3779B97F4A7C15 * (step + 1) + 0xD1B54A32D192ED03) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return (z >> 40) / 16777216.0
    for seed in (0, 7, 2 ** 63 + 5):
        for step in (0, 1, 299, 2 ** 33):
            assert sr.uniform(seed, step, 0) == uniform(seed, step)
    us = [sr.uniform(3, t, s) for t in range(50) for s in range(4)]
    assert len(set(us)) == len(us) and 0.0 <= min(us) and max(us) < 1.0


def test_python_surface_refuses_out_of_range_filters():
    import torch
    from music_amd import fast_generate as fg
    cpu = torch.device("cpu")
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            fg._Sampling(1, 1.0, None, bad, 0, None, cpu)
    with pytest.raises(ValueError, match="top_k"):
        fg._Sampling(1, 1.0, -1, None, 0, None, cpu)
    with pytest.raises(ValueError, match="top_p"):
        fg._Sampling(3, 1.0, None, [0.5, 0.9, 1.2], 0, None, cpu)
    with pytest.raises(ValueError, match="one entry per utterance"):
        fg._Sampling(3, [1.0, 2.0], None, None, 0, None, cpu)
    s = fg._Sampling(4, 0.8, None, None, 5, None, cpu)
    assert s.plain and s.table is None and abs(s.temperature - 0.8) < 1e-12 and s.seed == 5
    assert fg._Sampling(4, 0.8, None, None, 5, [0, 1, 2, 3], cpu).plain           # the default streams: no table
    s = fg._Sampling(4, 0.8, 40, 0.9, 5, None, cpu)
    assert not s.plain and s.table is None and (s.top_k, s.top_p) == (40, 0.9)
    s = fg._Sampling(2, [0.0, 0.5], 3, None, [1, 2 ** 64 - 1], [7, 7], cpu)
    assert not s.plain and s.table.numel() == 48
    tab = np.frombuffer(s.table.numpy().tobytes(), dtype=np.dtype([("t", "<f4"), ("p", "<f4"), ("k", "<i4"), ("s", "<u4"), ("seed", "<u8")]))
    assert tab["t"].tolist() == [0.0, 0.5] and tab["p"].tolist() == [1.0, 1.0] and tab["k"].tolist() == [3, 3]
    assert tab["s"].tolist() == [7, 7] and tab["seed"].tolist() == [1, 2 ** 64 - 1]
    with pytest.raises(ValueError, match="correct_queue"):
        fg._need_corrected(s, False)


def test_seeded_kernel_test_rows_stay_below_the_excusal_cap():
    """The kernel-level GPU test may excuse a row whose float64 head mass lies within 1e-5 of top_p at some candidate threshold,
    for at most 2 % of a case's rows.  Counted here with the reference alone, on the very rows that test uses."""
    worst = 0
    for Q in sr.QS:
        rows, _ = sr.make_rows(Q)
        T = sr.temperatures(sr.ROWS)
        for k in sr.top_ks(Q):
            for p in sr.TOP_P[1:]:
                near = sum(1 for i in range(sr.ROWS) if sr.sample_row(rows[i], T[i], k, p).near)
                assert near <= sr.EXCUSED_CAP * sr.ROWS, (Q, k, p, near)
                worst = max(worst, near)
    print("rows within 1e-5 of a top-p boundary: at most %d of %d per case" % (worst, sr.ROWS))
