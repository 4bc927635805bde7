"""CPU checks of tests/window_ref.py, the float64 rule of position-windowed sampling, and of the seeded rows and windows the GPU
test (tests/test_gpu_window_sampler.py) runs: few enough of them sit on a top-p boundary, few enough are dead inside their window."""
import numpy as np
import pytest

from tests import sampling_ref as sr
from tests import window_ref as wr


def test_a_maximum_outside_the_window_does_not_exist():
    l = np.array([9.0, 0.0, 1.0, 2.0, 50.0, np.nan], np.float32)
    ref = wr.windowed_row(l, 1, 4, 1.0, u=0.0)
    e = np.exp(np.array([0.0, 1.0, 2.0]) - 2.0)
    assert np.allclose(ref.r[1:4], e / e.sum(), rtol=0, atol=1e-15) and (ref.r[[0, 4, 5]] == 0).all()
    assert ref.code == 1 and list(np.nonzero(ref.N)[0]) == [1, 2, 3]
    assert wr.windowed_row(l, 1, 4, 1.0, u=0.999999).code == 3
    # greedy: the first-index argmax INSIDE the window, the plain softmax over it
    g = wr.windowed_row(l, 1, 4, 0.0)
    assert g.code == 3 and np.allclose(g.r[1:4], e / e.sum(), rtol=0, atol=1e-15) and g.r[4] == 0
    # u above the total: the largest index of the kept set inside the window
    assert wr.windowed_row(l, 1, 4, 1.0, top_k=2, u=1.0).code == 3
    assert wr.windowed_row(np.array([5.0, 3.0, 2.0, 1.0, 9.0]), 0, 4, 1.0, top_k=2, u=1.0).code == 1


def test_top_k_at_or_above_the_width_is_no_filter_at_that_position():
    l = np.array([0.5, -1.0, 2.0, 0.0, 3.0, 1.0, 7.0, 7.0], np.float32)
    full = wr.windowed_row(l, 2, 6, 0.8)
    for k in (4, 5, 8, 100):
        ref = wr.windowed_row(l, 2, 6, 0.8, top_k=k)
        assert (ref.N == full.N).all() and (ref.r == full.r).all() and ref.N.sum() == 4
    k3 = wr.windowed_row(l, 2, 6, 0.8, top_k=3)
    assert list(np.nonzero(k3.N)[0]) == [2, 4, 5]
    # the same top_k is a filter in a wide window and none in a narrow one
    assert wr.windowed_row(l, 0, 8, 1.0, top_k=4).N.sum() == 4 and wr.windowed_row(l, 0, 3, 1.0, top_k=4).N.sum() == 3


def test_a_window_of_one_entry():
    l = np.array([4.0, -2.0, 1.0], np.float32)
    for T, k, p in ((1.0, 0, 1.0), (0.5, 1, 0.5), (0.0, 0, 1.0), (1.3, 5, 1e-6)):
        for u in (0.0, 0.5, 1.0 - 2.0 ** -24):
            ref = wr.windowed_row(l, 1, 2, T, k, p, u if T > 0 else None)
            assert list(ref.r) == [0.0, 1.0, 0.0] and list(ref.N) == [False, True, False]
            assert (ref.code if T > 0 else wr.windowed_row(l, 1, 2, T).code) == 1


def test_window_table_is_the_list_of_the_sampler_test():
    for Q in sr.QS:
        tab = wr.window_table(Q)
        assert 1 <= len(tab) <= 16 and len(set(tab)) == len(tab) and tab[0] == (0, Q)
        assert all(0 <= lo < hi <= Q for lo, hi in tab)
    assert wr.window_table(1) == [(0, 1)]
    assert wr.window_table(256) == [(0, 256), (0, 1), (255, 256), (0, 128), (128, 256), (1, 6), (13, 14), (19, 21), (85, 170),
                                    (0, 64), (64, 128), (128, 192), (192, 256), (127, 129), (2, 254)]
    assert wr.entries_per_lane(64) == 1 and wr.entries_per_lane(65) == 2 and wr.entries_per_lane(1024) == 16
    # (Q - Q % NE - 1, Q): from the last entry of the last FULL lane to the end
    assert (63, 65) in wr.window_table(65) and (991, 1000) in wr.window_table(1000)


@pytest.mark.parametrize("Q", sr.QS)
def test_few_seeded_rows_sit_on_a_top_p_boundary_inside_their_window(Q):
    """The GPU test excuses a row whose sliced float64 head mass lies within 1e-5 of top_p, at most EXCUSED_CAP of a case's rows: the
    count, on the CPU, with the reference alone.  Rows dead inside their window are not excused (they take the "code inside the
    window" check only) - and are few."""
    rows, _ = sr.make_rows(Q)
    T = sr.temperatures(sr.ROWS)
    wins = wr.row_windows(Q)
    dead = wr.dead(rows, wins)
    assert dead.sum() <= 12 and (Q > 1 or dead.sum() == 0), dead.sum()
    worst = 0
    for k in (0, 1, 5):
        for p in sr.TOP_P[1:]:
            n = sum(bool(wr.windowed_row(rows[i], lo, hi, T[i], k, p).near) for i, (lo, hi) in enumerate(wins) if not dead[i])
            assert n <= sr.EXCUSED_CAP * sr.ROWS, (Q, k, p, n)
            worst = max(worst, n)
    print("Q = %d: %d windows, %d dead rows, at most %d of %d rows within 1e-5 of a top-p boundary" % (Q, len(set(wins)), dead.sum(),
                                                                                                    worst, sr.ROWS))


def test_hostile_rows_leave_the_window_alone():
    rows, _ = sr.make_rows(100)
    wins = wr.row_windows(100)
    bad = wr.hostile(rows, wins)
    for i, (lo, hi) in enumerate(wins):
        assert np.array_equal(bad[i, lo:hi], rows[i, lo:hi], equal_nan=True)
        out = np.concatenate([bad[i, :lo], bad[i, hi:]])
        if i % 2:
            assert np.isnan(out).all()
        elif np.isfinite(rows[i, lo:hi]).any():
            assert (out >= rows[i, lo:hi][np.isfinite(rows[i, lo:hi])].max() + 299).all()
