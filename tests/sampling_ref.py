"""Float64 restatement of the decoder's sampling rule (include/wavenet_hip.h, wn_decode_batch_samp) and of its counter-based
uniform numbers.  Not a test module: the sampling tests import it.

Per row of Q logits l, temperature T > 0, top_k, top_p and a uniform number u in [0, 1):
  1. top-k (0 < top_k < Q): K = { i : l_i >= the top_k-th largest logit }, ties kept; otherwise K = everything.
  2. p_i = exp((l_i - max l) / T) / sum over K on K, 0 elsewhere.
  3. top-p (0 < top_p < 1): tau = the largest logit value v occurring in K with sum_{K, l_i >= v} p_i >= top_p,
     N = { i in K : l_i >= tau }; no such v (rounding): N = K; filter off: N = K.
  4. r = p / sum over N on N, 0 elsewhere; the code is the first index whose inclusive cumulative r exceeds u, the largest index
     in N when none does.
  5. T <= 0: first-index argmax, r = the plain softmax (filters ignored)."""
import numpy as np

M64 = (1 << 64) - 1


def uniform(seed, step, stream):
    """dec_uniform (music_amd/csrc/wn_decode.hip): splitmix64 finaliser of (seed, step, stream), 24 random bits."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(step) + 1) + 0xD1B54A32D192ED03 * (int(stream) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


class Row:
    """What the rule gives for one row: ``K`` / ``N`` (boolean masks), ``r`` (float64 distribution drawn from), ``code`` (for
    the u given, or None), and for the top-p filter the candidate thresholds whose float64 head mass lies within ``band`` of
    top_p (``near``) with the kept sets a rounded mass could turn them into (``alt``: list of masks, N itself first)."""


def sample_row(logits, temperature, top_k=0, top_p=1.0, u=None, band=1e-5):
    l = np.asarray(logits, dtype=np.float64)
    Q = l.size
    out = Row()
    if temperature is None or temperature <= 0:
        e = np.exp(l - l.max())
        out.K = out.N = np.ones(Q, bool)
        out.r = e / e.sum()
        out.code = int(np.argmax(l))                       # first index on ties
        out.near, out.alt = [], [out.N]
        return out
    T = float(temperature)
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    if top_k <= 0 or top_k >= Q:
        K = np.ones(Q, bool)
    else:
        K = l >= np.sort(l)[Q - top_k]
    e = np.where(K, np.exp((l - l.max()) / T), 0.0)
    p = e / e.sum()
    N, near, alt = K, [], []
    if 0.0 < top_p < 1.0:
        order = np.argsort(-l, kind="stable")
        order = order[K[order]]                             # K's entries, largest logit first
        ls, cs = l[order], np.cumsum(p[order])
        last = np.nonzero(np.append(ls[1:] != ls[:-1], True))[0]           # last entry of every run of equal values
        vals, mass = ls[last], cs[last]                     # distinct values, largest first, and their head masses
        ok = np.nonzero(mass >= top_p)[0]
        if ok.size:
            N = K & (l >= vals[ok[0]])
        # a mass within `band` of top_p may round to the other side: threshold j then gives way to j + 1, or takes over
        for j in np.nonzero(np.abs(mass - top_p) < band)[0]:
            near.append(float(vals[j]))
            alt.append(K & (l >= vals[j]))
            if j + 1 < vals.size:
                alt.append(K & (l >= vals[j + 1]))
    out.K, out.N, out.near = K, N, near
    out.alt = [N] + alt
    r = np.where(N, p, 0.0)
    out.r = r / r.sum()
    out.code = None if u is None else draw(out.r, N, u)
    return out


def draw(r, N, u):
    """Rule step 4 on a distribution r with kept set N."""
    c = np.cumsum(r)
    hit = np.nonzero(c > u)[0]
    return int(hit[0]) if hit.size else int(np.nonzero(N)[0][-1])


# ---- the seeded inputs of the kernel-level GPU test (tests/test_gpu_decode_sample.py); tests/test_sampling_ref.py checks on the
# CPU, with this reference alone, that few enough of them sit on a top-p boundary
QS = [1, 2, 63, 64, 65, 100, 256, 257, 512, 1000, 1024]
TOP_P = [1.0, 0.9, 0.5, 1e-6]
ROWS = 200
EXCUSED_CAP = 0.02                     # share of a case's rows that may sit within `band` of a top-p boundary
U_EDGE = [0.0, 0.5, 1 - 2.0 ** -24]


def top_ks(Q):
    return [0, 1, 2, 5, Q - 1, Q, Q + 7]


ROW_SEED = 2                           # chosen on the CPU (tests/test_sampling_ref.py): every case stays below EXCUSED_CAP


def make_rows(Q, seed=ROW_SEED):
    """ROWS rows of Q fp32 logits: random at several scales, exact duplicates (values on a coarse grid, and a block of copies
    of one value placed to straddle small k), rows with -inf entries, rows where one logit dominates; and one u per row
    (the three edge values, then random 24-bit uniforms)."""
    rng = np.random.default_rng(1000 * Q + seed)
    rows = np.empty((ROWS, Q), np.float32)
    for i in range(ROWS):
        kind = i % 5
        x = rng.standard_normal(Q) * [0.3, 1.0, 3.0, 10.0][(i // 5) % 4]
        if kind == 1:                                      # coarse grid: many exact ties everywhere
            x = np.round(x * 2) / 2
        elif kind == 2:                                    # a block of copies of one of the largest values
            srt = np.sort(x)[::-1]
            v = srt[min(Q - 1, int(rng.integers(0, 6)))]
            x[rng.integers(0, Q, size=min(Q, int(rng.integers(2, 9))))] = v
        elif kind == 3:                                    # -inf entries (at least one finite one stays)
            x[rng.random(Q) < [0.1, 0.5, 0.9][(i // 5) % 3]] = -np.inf
            x[int(rng.integers(0, Q))] = float(rng.standard_normal())
        elif kind == 4:                                    # one logit dominates
            x[int(rng.integers(0, Q))] += [8.0, 30.0, 120.0][(i // 5) % 3]
        rows[i] = x.astype(np.float32)
    u = np.array([U_EDGE[i] if i < 3 else int(rng.integers(0, 1 << 24)) / 16777216.0 for i in range(ROWS)])
    u = np.roll(u, 7 * (seed + 1))                          # the edge values meet different row kinds per seed
    return rows, u.astype(np.float32)


def temperatures(n, seed=0):
    return np.array([[0.5, 1.0, 1.7][(i + seed) % 3] for i in range(n)], np.float32)
