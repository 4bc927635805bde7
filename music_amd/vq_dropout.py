"""Quantiser dropout for the residual vq bottleneck (SoundStream, EnCodec, DAC): the host side.  During training every clip draws its
own stage count n in [1, S]; the stages behind n are skipped for that clip - in the quantised sum, in the loss and in the codebook's
gradient or EMA statistics (wn_rvq_fwd_n / wn_rvq_bwd_n / wn_rvq_bwd_stats_n) -, so ONE model serves every bitrate n log2 K and a
prefix of the stages decodes through tables that were trained on it.

``draw_stages``   the draw: a stateless counter hash of (seed, step, global clip index) - no torch RNG, nothing to checkpoint; a resumed
                  run and any data-parallel layout draw the same n for the same global clip
``stage_counts``  what ``stages=`` of forward / loss_and_grad / encode_codes may be -> None (all stages: the launches without
                  dropout) or B validated counts
``counts_of_codes``  the stage counts that (B, n, Le) codes with -1 in the absent stages describe, for decode_codes

Later stages see fewer frames - stage s expects a share 1 - p s / S of them -, so under ``vq_update="ema"`` a ``vq_restart``
threshold bites them sooner: their codes' running usage is smaller by that share.
"""
import numpy as np

_M64 = (1 << 64) - 1


def _splitmix64(x):
    """One splitmix64 output per uint64 of the array x (Steele, Lea, Flood 2014: the generator's finaliser on x + the golden-ratio
    increment); unsigned array arithmetic wraps modulo 2^64."""
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _splitmix64_int(x):
    """The same function of ONE value, on Python ints (the per-step key: no array to build)."""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_stages(seed, step, first_clip, B, S, p):
    """The stage counts (B,) int32 of clips first_clip .. first_clip + B - 1 of global step `step`: with probability p a clip draws n
    uniformly from 1 .. S, the others use all S (p = 1: SoundStream's rule, p = 0.5: DAC's).  A pure function of its arguments: clip
    g of step t hashes (seed, t, g) twice - one word decides whether it draws, the next one what."""
    seed, step, first_clip, B, S = int(seed), int(step), int(first_clip), int(B), int(S)
    if S < 1 or B < 0 or step < 0 or first_clip < 0:
        raise ValueError("music_amd.vq_dropout.draw_stages: S >= 1, B >= 0, step >= 0 and first_clip >= 0 are required")
    if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("music_amd.vq_dropout.draw_stages: p must lie in [0, 1], not %r" % (p,))
    clip = np.arange(first_clip, first_clip + B, dtype=np.uint64)
    key = np.uint64(_splitmix64_int((seed & _M64) ^ _splitmix64_int(step & _M64)))
    a = _splitmix64(key ^ _splitmix64(clip))
    b = _splitmix64(a)
    drops = (a >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < float(p)            # a uniform of [0, 1) from the top 53 bits
    n = 1 + ((b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * S).astype(np.int64)  # floor(u S) + 1: 1 .. S, each S-th of [0, 1)
    return np.where(drops, np.minimum(n, S), S).astype(np.int32)


def _as_ints(values, what):
    try:
        import torch
        if isinstance(values, torch.Tensor):
            if values.is_floating_point() or values.dtype == torch.bool or values.is_complex():
                raise ValueError("music_amd: %s must hold integers, not %s" % (what, values.dtype))
            values = values.detach().cpu().numpy()
    except ImportError:
        pass
    if isinstance(values, (str, bytes, dict, set)):
        raise ValueError("music_amd: %s must be an int or a sequence of ints, not %r" % (what, type(values).__name__))
    if isinstance(values, np.ndarray):
        if values.dtype.kind not in "iu":
            raise ValueError("music_amd: %s must hold integers, not %s" % (what, values.dtype))
        return values.astype(np.int64)
    try:
        values = list(values)
    except TypeError:
        raise ValueError("music_amd: %s must be an int or a sequence of ints, not %r" % (what, type(values).__name__))
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in values):
        raise ValueError("music_amd: %s must hold integers" % what)
    return np.asarray(values, dtype=np.int64)


def stage_counts(stages, B, S):
    """`stages` of forward / loss_and_grad: None, an int n (every clip uses n) or B ints, each in [1, S] -> None or (B,) int32.  None
    comes back for None and, on a model of ONE stage, for a value that means "all stages"; anything else raises ValueError."""
    if stages is None:
        return None
    B, S = int(B), int(S)
    if isinstance(stages, (bool, np.bool_)):
        raise ValueError("music_amd: stages must be None, an int or one int per clip, not a bool")
    if isinstance(stages, (int, np.integer)):
        n = np.full(B, int(stages), dtype=np.int64)
    else:
        n = _as_ints(stages, "stages")
        if n.ndim == 0:
            n = np.full(B, int(n), dtype=np.int64)
        if n.shape != (B,):
            raise ValueError("music_amd: stages must be an int or %d ints (one per clip), got shape %s" % (B, tuple(n.shape)))
    if n.size and (n.min() < 1 or n.max() > S):
        raise ValueError("music_amd: stages must lie in [1, %d] (vq_stages), got %d .. %d" % (S, n.min(), n.max()))
    if S == 1:
        return None                                         # one stage (or no quantiser): 1 means all of them
    return n.astype(np.int32)


def counts_of_codes(codes, S):
    """codes (B, n, Le) integers, 1 <= n <= S, with -1 in the absent stages -> None where no entry is -1 (a plain prefix), else the
    clips' stage counts (B,) int32.  A clip's -1 entries must form a stage suffix, identical over its frames, and never include
    stage 0; any other negative entry is refused (ValueError).  Codes >= 0 are the device's to check."""
    c = _as_ints(codes, "codes")
    if c.ndim != 3 or not 1 <= c.shape[1] <= int(S):
        raise ValueError("music_amd: vq_stages = %d: codes must be (B, n, Le) with 1 <= n <= %d, not %s" % (S, S, tuple(c.shape)))
    if not (c < 0).any():
        return None
    if (c < -1).any():
        raise ValueError("music_amd: a code lies below -1 (-1 marks an absent stage, codes lie in [0, K))")
    absent = c == -1
    per_stage = absent.all(axis=2)
    if (absent.any(axis=2) != per_stage).any():
        raise ValueError("music_amd: a clip's absent stages (-1) must be the same in all of its frames")
    if per_stage[:, 0].any():
        raise ValueError("music_amd: stage 0 cannot be absent (-1): every clip has at least one stage")
    n = (~per_stage).sum(axis=1)
    if (per_stage != (np.arange(c.shape[1])[None, :] >= n[:, None])).any():
        raise ValueError("music_amd: a clip's absent stages (-1) must form a suffix of the stages")
    return n.astype(np.int32)
