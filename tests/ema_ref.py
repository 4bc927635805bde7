"""Float64 reference of the EMA shadow (include/wavenet_hip.h, wn_ema_flat) and the error bound the tests hold it to, shared by
tests/test_ema_abi.py and tests/test_gpu_ema.py.

Rule: ema' = ema + w (p - ema), w = 1.0f - d_eff, d_eff = min(decay, (1 + T) / (10 + T)) with warm-up (in double from the float32
decay, rounded once to float32), else decay.  `kernel_w` restates that w on the host, independently of music_amd/ema.py.

Bound per step and element: 2^-23 (|e'| + 2 w |p - e|) - twice the worst case of the three float32 roundings (the difference, the
product, the sum: 2^-24 (w |p - e| (1 + 1) + |e'|) to first order; an fma only drops one of them).  An error already in the shadow
is carried on with the factor 1 - w <= 1, so over K steps the bound is the sum of the per-step bounds."""
import numpy as np


def kernel_w(decay, warmup, T):
    d = np.float64(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + float(T)) / (10.0 + float(T)))
    return np.float32(1.0) - np.float32(d)


class Ref64:
    """The float64 recurrence from a float32 start, fed the float32 parameters after every step, and its summed bound."""

    def __init__(self, start):
        self.e = np.asarray(start, dtype=np.float64).copy()
        self.bound = np.zeros_like(self.e)

    def step(self, p, w):
        p, w = np.asarray(p, dtype=np.float64), float(w)
        with np.errstate(invalid="ignore", over="ignore"):
            diff = p - self.e
            new = self.e + w * diff
            self.bound += 2.0 ** -23 * (np.abs(new) + 2.0 * w * np.abs(diff))
        self.e = new
        return self

    def check(self, got, what=""):
        """`got` (float32) within the bound wherever the reference is finite, non-finite exactly where it is not; the worst ratio."""
        got = np.asarray(got, dtype=np.float64)
        fin = np.isfinite(self.e) & np.isfinite(self.bound)
        assert np.array_equal(np.isfinite(got), fin), what
        if not fin.any():
            return 0.0
        err = np.abs(got[fin] - self.e[fin])
        assert (err <= self.bound[fin]).all(), (what, float((err / np.maximum(self.bound[fin], 1e-300)).max()))
        return float((err / np.maximum(self.bound[fin], 1e-300)).max())
