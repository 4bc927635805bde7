"""Float64 restatement of position-windowed sampling (include/wavenet_hip.h, wn_win_decode_batch / wn_win_sample_logits) on top of
tests/sampling_ref.py, and the seeded inputs of its kernel-level GPU test.  Not a test module.

The rule: the window [lo, hi) is applied FIRST - the row is the hi - lo logits l[lo .. hi) and sampling_ref.sample_row's rule runs
on that slice as if Q were hi - lo; everything outside has probability exactly 0 and influences nothing; codes are reported in the
full alphabet, lo + index."""
import numpy as np

from tests import sampling_ref as sr


def windowed_row(logits, lo, hi, T, top_k=0, top_p=1.0, u=None, band=1e-5):
    """sampling_ref.sample_row on logits[lo:hi], placed back into Q entries: ``K`` / ``N`` / every mask of ``alt`` are False and ``r``
    is 0 outside the window, ``code`` is the slice's code + lo (None without u)."""
    l = np.asarray(logits)
    Q = l.size
    assert 0 <= lo < hi <= Q
    ref = sr.sample_row(l[lo:hi], T, top_k, top_p, u, band)

    def back(v, fill):
        out = np.full(Q, fill, dtype=v.dtype)
        out[lo:hi] = v
        return out
    out = sr.Row()
    out.lo, out.hi = lo, hi
    out.K, out.N, out.r = back(ref.K, False), back(ref.N, False), back(ref.r, 0.0)
    out.alt = [back(m, False) for m in ref.alt]
    out.near = ref.near
    out.code = None if ref.code is None else ref.code + lo
    return out


# ---- the seeded inputs of tests/test_gpu_window_sampler.py: sampling_ref.make_rows(Q) with row i under window i mod period of
# window_table(Q); tests/test_window_ref.py counts on the CPU how many of them sit on a top-p boundary
def entries_per_lane(Q):
    """NE of the sampler's instantiation for Q (one wave, lane l owns entries NE l .. NE l + NE - 1)."""
    return 1 if Q <= 64 else 2 if Q <= 128 else 4 if Q <= 256 else 8 if Q <= 512 else 16


def window_table(Q):
    """Whole alphabet, single entries at both ends, halves, windows inside one lane and across a lane boundary, thirds, a window
    from the last lane's boundary to the end, quarters, a pair across the middle, all but two at each end: clamped to [0, Q],
    empty pairs and duplicates dropped, at most 16."""
    ne = entries_per_lane(Q)
    raw = [(0, Q), (0, 1), (Q - 1, Q), (0, Q // 2), (Q // 2, Q), (1, 6), (3 * ne + 1, 3 * ne + 2), (5 * ne - 1, 5 * ne + 1),
           (Q // 3, 2 * Q // 3), (Q - Q % ne - 1, Q)] + [(s * Q // 4, (s + 1) * Q // 4) for s in range(4)] + \
          [(Q // 2 - 1, Q // 2 + 1), (2, Q - 2)]
    out = []
    for lo, hi in raw:
        lo, hi = max(0, min(lo, Q)), max(0, min(hi, Q))
        if lo < hi and (lo, hi) not in out:
            out.append((lo, hi))
    return out[:16]


def row_windows(Q, n=sr.ROWS, pos=0):
    """The window of each of n rows: row i takes pair (pos + i) mod period of window_table(Q)."""
    tab = window_table(Q)
    return [tab[(pos + i) % len(tab)] for i in range(n)]


def dead(rows, wins):
    """Rows whose logits inside their window are all -inf (or NaN): the rule promises a code inside the window and nothing else."""
    return np.array([not np.isfinite(rows[i, lo:hi]).any() for i, (lo, hi) in enumerate(wins)])


def hostile(rows, wins):
    """The rows with everything OUTSIDE each row's window made hostile: even rows get the largest finite logit inside the window + 300
    there (0 + 300 where none is finite), odd rows NaN.  The windowed result may not notice."""
    out = rows.copy()
    for i, (lo, hi) in enumerate(wins):
        inside = rows[i, lo:hi]
        fin = inside[np.isfinite(inside)]
        v = np.float32((fin.max() if fin.size else 0.0) + 300.0) if i % 2 == 0 else np.float32(np.nan)
        out[i, :lo] = v
        out[i, hi:] = v
    return out
