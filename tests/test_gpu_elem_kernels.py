"""GPU tests of the memory-bound helpers of wn_elem.hip and wn_generic.hip, one launch at a time, against float64 (run with -m gpu).

Chunk softmax (forward, backward, fused cross-entropy; the 256-wide and the any-q form), the gate and its derivative, the bucket
sums and the expansion of the conditioning table, the three flat optimizers, and the exact movers (one-hot, gradient gather,
mu-law).  Rules of tests/test_gpu_wgrad_kernels.py and tests/test_gpu_recompute_kernels.py: every test fills its own device
buffers and launches ONE entry point; every output buffer is larger than its tensor and NaN everywhere beforehand (integer
outputs: a sentinel), and afterwards exactly the declared elements have changed; every input holds NaN wherever
include/wavenet_hip.h says its values do not count (outside [t_lo, t_hi), rows >= rows, the gap between clips, behind element n);
no element is left out of a comparison; every launch is repeated into fresh buffers and must give the same bits.  With NaN
surroundings a stray store of a value computed from them disappears in the NaN-filled output, so one case per windowed kernel is
repeated with finite surroundings.  The reference is tests/elem_ref.py (the header's formulas in float64, held to float64 autograd
and torch.optim by tests/test_elem_ref.py) on the very float32 arrays the kernel reads.

The test ids name the regime: "wrap" = a thread, wave or workgroup takes more than one item in the kernel's grid-stride loop,
"sweep" = exactly one full sweep, everything else stays below one.  One coverage test per group restates the launchers' grid
formulas on the host and asserts that the labels are true.

Bars - the project's own:
  probabilities           1e-6 (256-wide) / 5e-7 (any q), absolute               tests/test_gpu_kernels.py
  dx of the fused CE      1e-5 / 1e-4 of max |ref|                               tests/test_gpu_kernels.py, test_gpu_nll_kernels.py
  loss                    1e-5 max(1, |ref|), the float64 sum of the partials; each partial is held to the same figure
  separate backward       on the y it was given, 1e-5 / 1e-4 of max |ref|
  gate                    z 5e-7, derivatives 2e-6 absolute, dz in [-1, 1]       tests/test_gpu_kernels.py
  bucket sums             n_j 2^-23 sum |terms| per element, n_j = columns of bucket j: the bound of ANY fixed-order fp32 sum
                          (an empty bucket must be exactly 0); on multiples of 1/8 below 2^10 the sums EQUAL float64
  optimizer state         8 2^-24 sum |terms| per element (m, v, square_avg, momentum buffers)
  optimizer p             on the device's own new state: 2^-23 |p'| + 8 2^-24 |update| - a cancellation in m is not charged twice.
                          The formulas evaluated in numpy float32 reach 0.33 of the state bars and 0.5 of this one; the 8 leaves
                          room for contraction into FMAs and the device's sqrtf and division.
  expansion, one-hot, gather, mu-law: torch.equal.
Before an optimizer launch the test asserts on the CPU that its inputs can see every term: the float64 reference with gscale, a
bias correction, eps or the momentum term dropped leaves at least a tenth of the elements beyond the bars.

Largest errors observed on an MI355X, as shares of the bar (test_zz_report prints them with -s; 256-wide / any q):
  softmax forward 0.24 / 0.53   fused CE probabilities 0.30 / 0.56, dx 0.04 / 0.007, loss 0.017 / 0.017   backward 0.04 / 0.006
  gate z 0.39, derivatives 0.19   bucket sums stretch 0.09, tile through LDS 0.25, tile strided 0.29
  Adam m 0.23, v 0.25, p 0.50   SGD buffer 0.13, p 0.50   RMSprop square_avg 0.21, buffer 0.39, p 0.49
The probabilities above half their bar are expf and one division against an absolute 5e-7 near 1; the p figures are the half ulp
of the last subtraction, half of the bar's first term by construction.

Answer-only mutations of the kernels that this file catches (each fails the tests named): softmax256_ce_k without `y = yn` or
without `v = vn` (test_softmax_ce[w256-*wrap*]), a forward stride of gridDim.x * 8 (test_softmax_fwd[*-32773rows-wrap]), the tile
bucket sum with per = nchunks / 4 (test_cond_grad[tile-lds-*]), a last stretch bucket ending at s0 + q (test_cond_grad[*ragged-tail*]),
Adam without rs (test_adam), RMSprop's eps under the root (test_rmsprop), SGD ignoring `first` (test_sgd[*first-step]), the
scrambled one-hot position computed as the proper one (test_onehot[scrambled-*]), mu-law `<=` as `<` (test_mulaw_encode_*), the
gate's derivative rows swapped (test_gate), softmaxq_ce_k's py from lane 0 (test_softmax_ce[q*])."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from tests import elem_ref

DEV = "cuda"
NAN = float("nan")
PAD = 64                                             # floats of frame in front of and behind every tensor (keeps 16-byte alignment)
PARTS = 1024                                         # WN_CE_NUM_PARTIALS
I32_MIN = -(1 << 31)
WORST = {}                                           # group -> (share of its bar, case)


def _note(group, share, case):
    if group not in WORST or share > WORST[group][0]:
        WORST[group] = (float(share), case)


def _st():
    return _lib.stream()


def _status(name, *args):
    """status of a call that is expected to be refused or to do nothing (no exception)"""
    return getattr(_lib.load(), name)(*args)


def _dev(a, fill=NAN):
    """numpy array -> flat device buffer [PAD of fill | a | PAD of fill]"""
    a = np.ascontiguousarray(a)
    t = np.full(PAD + a.size + PAD, fill, a.dtype)
    t[PAD:PAD + a.size] = a.reshape(-1)
    return torch.from_numpy(t).to(DEV)


def _out(n, dtype=np.float32, fill=NAN):
    return torch.from_numpy(np.full(PAD + n + PAD, fill, dtype)).to(DEV)


def _body(buf, n, shape=None, fill=None):
    """the tensor between the frames, on the host; asserts that both frames are untouched (fill: an integer buffer's sentinel)"""
    h = buf.cpu().numpy()
    assert h.size == n + 2 * PAD and (fill is None) == (h.dtype.kind == "f")
    for fr in (h[:PAD], h[PAD + n:]):
        assert (np.isnan(fr) if fill is None else fr == fill).all(), "a store outside the tensor"
    b = h[PAD:PAD + n]
    return b.reshape(shape) if shape is not None else b


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _twice(launch):
    """run `launch` (fresh buffers, returns host arrays) twice: the same bits both times"""
    torch.cuda.synchronize()
    first = launch()
    second = launch()
    for a, b in zip(first, second):
        if a is not None:
            assert _same(a, b), "two launches on the same inputs differ"
    return first


# ================================================================================================ chunk softmax
def _sm_grid(nrows):
    """sm_grid / gq_grid: workgroups of 4 waves, a wave per row"""
    return min(8192, max(1, (nrows + 3) // 4))


def _fwd_wraps(nrows):
    return nrows > _sm_grid(nrows) * 4


def _ce_waves(form):
    return 8 if form == "w256" else 4


def _ce_wraps(form, nrows):
    return nrows > PARTS * _ce_waves(form)


def _q_of(form):
    return 256 if form == "w256" else int(form[1:])


@functools.lru_cache(maxsize=4)
def _logits(n, q, seed=0):
    """(x, target): gain-3 normal logits; row r % 5 == 1 holds +-80 only, == 2 equal logits, == 3 a target 120 below the maximum"""
    rng = np.random.default_rng(1000 * q + n + seed)
    x = (rng.standard_normal((n, q)) * 3).astype(np.float32)
    tgt = rng.integers(0, q, n).astype(np.int64)
    r = np.arange(n)
    k = r[r % 5 == 1]
    x[k] = np.where(rng.integers(0, 2, (len(k), q)) == 1, 80.0, -80.0).astype(np.float32)
    x[r % 5 == 2] = np.float32(1.5)
    if q > 1:
        k = r[r % 5 == 3]
        x[k, tgt[k]] = np.float32(-60.0)
        x[k, (tgt[k] + 1) % q] = np.float32(60.0)
    x.setflags(write=False)
    tgt.setflags(write=False)
    return x, tgt


@functools.lru_cache(maxsize=2)
def _fwd_ref(n, q):
    x, _ = _logits(n, q)
    return elem_ref.softmax(x)


FWD_ROWS = [(1, "1row"), (3, "3rows"), (4, "4rows-one-workgroup"), (5, "5rows"), (1037, "1037rows"), (32768, "32768rows-sweep"),
            (32773, "32773rows-wrap")]
Q_ALL = [1, 7, 63, 64, 65, 100, 256, 1000]
FWD_CASES = [("w256", n, lab) for n, lab in FWD_ROWS]
FWD_CASES += [("q%d" % q, n, lab) for q in Q_ALL for n, lab in FWD_ROWS if n < 32768 or q in (7, 100)]
FWD_IDS = ["%s-%s" % (f, lab) for f, n, lab in FWD_CASES]
P_BAR = {True: 1e-6, False: 5e-7}
DX_BAR = {True: 1e-5, False: 1e-4}


def _fwd_call(form, x, y, n):
    if form == "w256":
        return ("wn_chunk_softmax256_fwd", x, y, n, _st())
    return ("wn_chunk_softmax_fwd", x, y, n, _q_of(form), _st())


def _bwd_call(form, y, dy, dx, n):
    if form == "w256":
        return ("wn_chunk_softmax256_bwd", y, dy, dx, n, _st())
    return ("wn_chunk_softmax_bwd", y, dy, dx, n, _q_of(form), _st())


def _ce_call(form, x, t, probs, dx, part, n, inv_n):
    if form == "w256":
        return ("wn_chunk_softmax256_ce", x, t, probs, dx, part, n, inv_n, _st())
    return ("wn_chunk_softmax_ce", x, t, probs, dx, part, n, _q_of(form), inv_n, _st())


@pytest.mark.parametrize("form,n,lab", FWD_CASES, ids=FWD_IDS)
def test_softmax_fwd(form, n, lab):
    q = _q_of(form)
    x, _ = _logits(n, q)
    xd = _dev(x)

    def launch():
        y = _out(n * q)
        call(*_fwd_call(form, ptr(xd, PAD), ptr(y, PAD), n))
        return (_body(y, n * q, (n, q)),)

    (y,) = _twice(launch)
    assert _same(_body(xd, n * q, (n, q)), x)
    assert not np.isnan(y).any()
    err = np.abs(y - _fwd_ref(n, q)).max()
    _note("softmax fwd %s" % ("256" if form == "w256" else "any q"), err / P_BAR[form == "w256"], "%s-%s" % (form, lab))
    assert err <= P_BAR[form == "w256"]


@pytest.mark.parametrize("form,n,lab", FWD_CASES, ids=FWD_IDS)
def test_softmax_bwd(form, n, lab):
    q = _q_of(form)
    y = _fwd_ref(n, q).astype(np.float32)                               # the probabilities the kernel is given, whatever made them
    dy = np.random.default_rng(n + q).standard_normal((n, q)).astype(np.float32)
    yd, dyd = _dev(y), _dev(dy)

    def launch():
        dx = _out(n * q)
        call(*_bwd_call(form, ptr(yd, PAD), ptr(dyd, PAD), ptr(dx, PAD), n))
        return (_body(dx, n * q, (n, q)),)

    (dx,) = _twice(launch)
    assert not np.isnan(dx).any()
    ref = elem_ref.softmax_bwd(y, dy)
    bar = DX_BAR[form == "w256"] * np.abs(ref).max()
    err = np.abs(dx - ref).max()
    if bar == 0:                                                        # q = 1: y = 1, dx = dy - dy = 0 exactly
        assert err == 0
        return
    _note("softmax bwd %s" % ("256" if form == "w256" else "any q"), err / bar, "%s-%s" % (form, lab))
    assert err <= bar


CE_ROWS = {"w256": [(1, "1row"), (7, "7rows"), (8, "8rows-one-workgroup"), (9, "9rows"), (8192, "8192rows-sweep"),
                    (8195, "8195rows-wrap"), (3 * 8192 + 1, "24577rows-wrap-three-and-four-trips")],
           "q": [(1, "1row"), (3, "3rows"), (4, "4rows-one-workgroup"), (5, "5rows"), (4096, "4096rows-sweep"), (4099, "4099rows-wrap"),
                 (2 * 4096 + 1, "8193rows-wrap-two-and-three-trips")]}
CE_CASES = [("w256", n, lab) for n, lab in CE_ROWS["w256"]]
CE_CASES += [("q%d" % q, n, lab) for q in Q_ALL for n, lab in CE_ROWS["q"] if n <= 4099 and n != 4096 or q in (7, 100, 256)]
CE_IDS = ["%s-%s" % (f, lab) for f, n, lab in CE_CASES]


def _part_ref(form, loss, inv_n):
    """the partial of every workgroup: rows r with (r / waves) % 1024 == wg, a wave per row"""
    wg = (np.arange(len(loss)) // _ce_waves(form)) % PARTS
    out = np.zeros(PARTS)
    np.add.at(out, wg, loss)
    return out * inv_n, np.bincount(wg, minlength=PARTS)


def _ce_launch(form, xd, td, n, want=(True, True, True), inv_n=None):
    """one fused launch into fresh NaN buffers -> (probs, dx, partials), None for an output passed as NULL"""
    q = _q_of(form)
    inv_n = np.float32(1.0 / n) if inv_n is None else inv_n
    probs, dx, part = (_out(n * q) if want[0] else None, _out(n * q) if want[1] else None, _out(PARTS) if want[2] else None)
    call(*_ce_call(form, ptr(xd, PAD), ptr(td, PAD), ptr(probs, PAD) if want[0] else None, ptr(dx, PAD) if want[1] else None,
                   ptr(part, PAD) if want[2] else None, n, float(inv_n)))
    return (_body(probs, n * q, (n, q)) if want[0] else None, _body(dx, n * q, (n, q)) if want[1] else None,
            _body(part, PARTS) if want[2] else None)


def _ce_check(form, lab, x, tgt, probs, dx, part):
    n, q = x.shape
    w = form == "w256"
    inv_n = float(np.float32(1.0 / n))
    rp, rl, rmean, rdx = elem_ref.softmax_ce(x, tgt, inv_n)
    grp = "256" if w else "any q"
    assert not np.isnan(probs).any()
    e = np.abs(probs - rp).max()
    _note("ce probs %s" % grp, e / P_BAR[w], "%s-%s" % (form, lab))
    assert e <= P_BAR[w]
    assert not np.isnan(dx).any()
    bar = DX_BAR[w] * np.abs(rdx).max()
    e = np.abs(dx - rdx).max()
    if bar == 0:
        assert e == 0
    else:
        _note("ce dx %s" % grp, e / bar, "%s-%s" % (form, lab))
        assert e <= bar
    pref, cnt = _part_ref(form, rl, inv_n)
    assert not np.isnan(part).any()                                     # all 1024 rewritten
    assert (part[cnt == 0] == 0).all()                                  # a workgroup without a row: exactly 0
    lbar = 1e-5 * max(1.0, abs(rmean))
    e = abs(part.astype(np.float64).sum() - rmean)
    _note("ce loss %s" % grp, e / lbar, "%s-%s" % (form, lab))
    assert e <= lbar
    assert np.abs(part - pref).max() <= lbar


@pytest.mark.parametrize("form,n,lab", CE_CASES, ids=CE_IDS)
def test_softmax_ce(form, n, lab):
    q = _q_of(form)
    x, tgt = _logits(n, q)
    xd, td = _dev(x), _dev(tgt, fill=-1)                                # a target read outside the tensor is a bad one: NaN
    probs, dx, part = _twice(lambda: _ce_launch(form, xd, td, n))
    _ce_check(form, lab, x, tgt, probs, dx, part)


@functools.lru_cache(maxsize=2)
def _ce_clean(form, n):
    q = _q_of(form)
    x, tgt = _logits(n, q)
    xd, td = _dev(x), _dev(tgt, fill=-1)
    return xd, _ce_launch(form, xd, td, n)


NULL_CASES = [("w256", 9), ("w256", 3 * 8192 + 1), ("q100", 5), ("q100", 2 * 4096 + 1)]


@pytest.mark.parametrize("null", ["probs", "dx", "loss_part"])
@pytest.mark.parametrize("form,n", NULL_CASES, ids=["%s-%drows%s" % (f, n, "-wrap" if _ce_wraps(f, n) else "") for f, n in NULL_CASES])
def test_softmax_ce_null_outputs(form, n, null):
    """each optional output NULL in turn: the others have the bits of the all-outputs launch"""
    xd, clean = _ce_clean(form, n)
    _, tgt = _logits(n, _q_of(form))
    td = _dev(tgt, fill=-1)
    want = tuple(k != null for k in ("probs", "dx", "loss_part"))
    got = _twice(lambda: _ce_launch(form, xd, td, n, want))
    for k, (g, c) in enumerate(zip(got, clean)):
        assert (g is None) == (not want[k])
        if g is not None:
            assert _same(g, c)


BAD_SHAPES = [("w256", 3 * 8192 + 1, 8192 + 5), ("q100", 2 * 4096 + 1, 4096 + 5), ("w256", 9, None), ("q7", 5, None)]
BAD_CASES = [(f, n, s, v, w) for f, n, s in BAD_SHAPES for v in ("q", "minus1", "2pow40")
             for w in ("first-row", "last-row", "second-trip-row") if s is not None or w != "second-trip-row"]


@pytest.mark.parametrize("form,n,second,value,where", BAD_CASES, ids=["%s-%drows-%s-%s" % (f, n, v, w) for f, n, s, v, w in BAD_CASES])
def test_softmax_ce_bad_target(form, n, second, value, where):
    """a target outside [0, q): NaN loss, that row's dx all NaN, every other row and partial bit-equal to the clean launch"""
    q = _q_of(form)
    xd, (cp, cdx, cpart) = _ce_clean(form, n)
    _, tgt = _logits(n, q)
    row = {"first-row": 0, "last-row": n - 1, "second-trip-row": second}[where]
    if where == "second-trip-row":
        assert row >= PARTS * _ce_waves(form)                           # reached on a wave's second trip
    bad = np.array(tgt)
    bad[row] = {"q": q, "minus1": -1, "2pow40": 1 << 40}[value]
    td = _dev(bad, fill=-1)
    probs, dx, part = _twice(lambda: _ce_launch(form, xd, td, n))
    assert _same(probs, cp)
    assert np.isnan(dx[row]).all()
    keep = np.arange(n) != row
    assert _same(dx[keep], cdx[keep])
    wg = (row // _ce_waves(form)) % PARTS
    assert np.isnan(part[wg]) and np.isnan(part.astype(np.float64).sum())
    keep = np.arange(PARTS) != wg
    assert _same(part[keep], cpart[keep])


def test_softmax_no_rows_write_nothing():
    """nrows = 0: every entry point returns 0 and launches nothing (NULL pointers accepted)"""
    s = _st()
    assert _status("wn_chunk_softmax256_fwd", None, None, 0, s) == 0
    assert _status("wn_chunk_softmax256_bwd", None, None, None, 0, s) == 0
    assert _status("wn_chunk_softmax256_ce", None, None, None, None, None, 0, 1.0, s) == 0
    for q in (1, 100):
        assert _status("wn_chunk_softmax_fwd", None, None, 0, q, s) == 0
        assert _status("wn_chunk_softmax_bwd", None, None, None, 0, q, s) == 0
        assert _status("wn_chunk_softmax_ce", None, None, None, None, None, 0, q, 1.0, s) == 0
    buf = _out(PARTS)                                                   # and with pointers: nothing written
    assert _status("wn_chunk_softmax256_ce", ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), 0, 1.0, s) == 0
    assert _status("wn_chunk_softmax_ce", ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), ptr(buf, PAD), 0, 7, 1.0, s) == 0
    torch.cuda.synchronize()
    assert np.isnan(_body(buf, PARTS)).all()


def test_softmax_cases_cover_the_stride_loops():
    for form, n, lab in FWD_CASES:
        assert ("wrap" in lab) == _fwd_wraps(n), (form, lab)
        assert ("sweep" in lab) == (n == _sm_grid(n) * 4 and n == 32768), (form, lab)
    for fam in ("w256", "q"):
        assert any(_fwd_wraps(n) for f, n, lab in FWD_CASES if f.startswith(fam))
        assert any(not _fwd_wraps(n) and n > 4 for f, n, lab in FWD_CASES if f.startswith(fam))
    for form, n, lab in CE_CASES:
        sweep = PARTS * _ce_waves(form)
        assert ("wrap" in lab) == _ce_wraps(form, n) == (n > sweep), (form, lab)
        assert ("sweep" in lab) == (n == sweep), (form, lab)
    # the 24577-row case of the 256-wide form: waves take three and four rows, so the prefetched row and target are handed over at
    # least twice, and the prefetch index is clamped to nrows - 1 on every wave's last trip
    trips = [len(range(w, 3 * 8192 + 1, 8192)) for w in range(8192)]
    assert sorted(set(trips)) == [3, 4]
    trips = [len(range(w, 2 * 4096 + 1, 4096)) for w in range(4096)]
    assert sorted(set(trips)) == [2, 3]
    for form, n, second in BAD_SHAPES:
        assert second is None or (_ce_wraps(form, n) and PARTS * _ce_waves(form) <= second < n)
    for form, n in NULL_CASES:
        assert (form, n) in [(f, m) for f, m, lab in CE_CASES]


# ================================================================================================ gate
GATE_GEO = [(1, 1, 1, "dp1-1row-1clip"), (5, 5, 3, "rows=dp-3clips"), (5, 3, 3, "rows<dp-3clips"), (5, 1, 1, "1row-of-dp5-1clip")]
GATE_SPECIAL = np.array([0.0, 15.0, -15.0, 81.0, -81.0, 104.0, -104.0], np.float32)


class _Gate:
    """fg [B][2 dp + 2][pitch] (two NaN rows between the clips), z / dz [B][dp + 1][pitch], dfg [B][2 dp + 3][pitch]; values only in
    rows [0, rows) and [dp, dp + rows), columns [t_lo, t_hi): NaN elsewhere, or finite junk with junk=True"""

    def __init__(self, w, t_lo, dp, rows, B, junk=False):
        rng = np.random.default_rng(w * 100 + t_lo * 10 + dp + rows + B)
        self.w, self.t_lo, self.t_hi, self.dp, self.rows, self.B = w, t_lo, t_lo + w, dp, rows, B
        self.pitch = pitch = t_lo + w + 3
        fill = (lambda s: rng.standard_normal(s).astype(np.float32)) if junk else (lambda s: np.full(s, NAN, np.float32))
        self.fg = fill((B, 2 * dp + 2, pitch))
        self.dz = fill((B, dp + 1, pitch))
        f = (rng.standard_normal((B, rows, w)) * 2).astype(np.float32)
        g = (rng.standard_normal((B, rows, w)) * 2).astype(np.float32)
        k = np.arange(f.size)
        f.reshape(-1)[::3] = GATE_SPECIAL[(k[::3] // 3) % 7]               # every pair of special values meets
        g.reshape(-1)[::3] = GATE_SPECIAL[(k[::3] // 21) % 7]
        self.f, self.g = f, g
        self.fg[:, :rows, t_lo:t_lo + w] = f
        self.fg[:, dp:dp + rows, t_lo:t_lo + w] = g
        self.d = rng.uniform(-1, 1, (B, rows, w)).astype(np.float32)
        self.dz[:, :rows, t_lo:t_lo + w] = self.d
        self.fgd, self.dzd = _dev(self.fg), _dev(self.dz)

    def fwd(self):
        z = _out(self.B * (self.dp + 1) * self.pitch)
        call("wn_gate_fwd", ptr(self.fgd, PAD), (2 * self.dp + 2) * self.pitch, self.dp, self.rows, ptr(z, PAD), (self.dp + 1) * self.pitch,
             self.pitch, self.t_lo, self.t_hi, self.B, _st())
        return (_body(z, z.numel() - 2 * PAD, (self.B, self.dp + 1, self.pitch)),)

    def bwd(self):
        dfg = _out(self.B * (2 * self.dp + 3) * self.pitch)
        call("wn_gate_bwd", ptr(self.fgd, PAD), (2 * self.dp + 2) * self.pitch, self.dp, self.rows, ptr(self.dzd, PAD),
             (self.dp + 1) * self.pitch, ptr(dfg, PAD), (2 * self.dp + 3) * self.pitch, self.pitch, self.t_lo, self.t_hi, self.B, _st())
        return (_body(dfg, dfg.numel() - 2 * PAD, (self.B, 2 * self.dp + 3, self.pitch)),)

    def check(self, group, case):
        rows, dp, lo, hi = self.rows, self.dp, self.t_lo, self.t_hi
        (z,) = _twice(self.fwd)
        mask = np.zeros(z.shape, bool)
        mask[:, :rows, lo:hi] = True
        assert np.array_equal(~np.isnan(z), mask)                       # finite inside, nothing moved outside
        e = np.abs(z[:, :rows, lo:hi] - elem_ref.gate(self.f, self.g)).max()
        _note("gate z" + group, e / 5e-7, case)
        assert e <= 5e-7
        (dfg,) = _twice(self.bwd)
        mask = np.zeros(dfg.shape, bool)
        mask[:, :rows, lo:hi] = True
        mask[:, dp:dp + rows, lo:hi] = True                             # the g rows sit dp * pitch behind the f rows
        assert np.array_equal(~np.isnan(dfg), mask)
        df, dg = elem_ref.gate_d(self.f, self.g)
        e = max(np.abs(dfg[:, :rows, lo:hi] - self.d * df).max(), np.abs(dfg[:, dp:dp + rows, lo:hi] - self.d * dg).max())
        _note("gate derivatives" + group, e / 2e-6, case)
        assert e <= 2e-6


@pytest.mark.parametrize("dp,rows,B,lab", GATE_GEO, ids=[g[3] for g in GATE_GEO])
@pytest.mark.parametrize("t_lo", [0, 5, 11], ids=["tlo0mod4", "tlo1mod4", "tlo3mod4"])
@pytest.mark.parametrize("w", [1, 255, 256, 257], ids=["1col", "255cols", "256cols-one-workgroup", "257cols-two-workgroups"])
def test_gate(w, t_lo, dp, rows, B, lab):
    _Gate(w, t_lo, dp, rows, B).check("", "%dcols-tlo%d-%s" % (w, t_lo, lab))


@pytest.mark.parametrize("w,t_lo", [(257, 5), (1, 11)], ids=["257cols", "1col"])
def test_gate_finite_surroundings(w, t_lo):
    """finite values where the inputs do not count: a store outside the window would now carry a number, not a NaN"""
    _Gate(w, t_lo, 5, 3, 3, junk=True).check(" (finite surroundings)", "%dcols" % w)


def test_gate_no_work_and_refusals():
    buf = _out(64)
    p, s = ptr(buf, PAD), _st()
    for rows, t_hi, B in ((0, 8, 1), (1, 4, 1), (1, 8, 0)):             # no rows / an empty window / no clips
        assert _status("wn_gate_fwd", p, 64, 1, rows, p, 64, 16, 4, t_hi, B, s) == 0
        assert _status("wn_gate_bwd", p, 64, 1, rows, p, 64, p, 64, 16, 4, t_hi, B, s) == 0
    assert _status("wn_gate_fwd", p, 64, 1, 2, p, 64, 16, 4, 8, 1, s) == -4          # rows > dp
    assert _status("wn_gate_bwd", p, 64, 1, 1, p, 64, None, 64, 16, 4, 8, 1, s) == -4
    torch.cuda.synchronize()
    assert np.isnan(_body(buf, 64)).all()


def test_gate_cases_cover_the_grid():
    """256 columns per workgroup: 255 / 256 stay in one, 257 opens a second whose threads past t_hi must return"""
    wg = lambda w: (w + 255) // 256
    assert [wg(w) for w in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert sorted({t % 4 for t in (0, 5, 11)}) == [0, 1, 3]
    assert any(r < d for d, r, b, l in GATE_GEO) and any(r == d > 1 for d, r, b, l in GATE_GEO) and any(d == 1 for d, r, b, l in GATE_GEO)


# ================================================================================================ bucket sums and expansion
def _tile_plan(le, L):
    """the rep / chunk / per arithmetic of cond_grad_k's tile form (le <= 64)"""
    rep = 64 // le
    chunk = rep * le
    nchunks = (L + chunk - 1) // chunk
    per = (nchunks + 3) // 4
    return dict(rep=rep, chunk=chunk, nchunks=nchunks, per=per)


def _tile_lengths(le):
    c = (64 // le) * le
    out = [(1, "1col"), (le - 1, "le-1"), (le, "le"), (c - 1, "chunk-1"), (c, "1chunk"), (c + 1, "chunk+1"), (3 * c, "3chunks-fewer-than-waves"),
           (4 * c, "4chunks-one-each"), (5 * c, "5chunks-uneven-deal"), (16 * c - 1, "16chunks-1-unrolled-trip-cut"), (16 * c, "16chunks"),
           (16 * c + 1, "16chunks+1"), (1103, "1103cols-ragged")]
    res = {}                                                            # lengths that coincide (le = 64: le = one chunk) run once
    for L, lab in out:
        if L >= 1:
            res[L] = res[L] + "=" + lab if L in res else lab
    return sorted(res.items())


COND_CASES = []                                      # (mode, le, q, L, label)
for _le in (1, 2, 5, 31, 32, 33, 63, 64):
    COND_CASES += [(2, _le, 0, L, "tile-lds-le%d-%s" % (_le, lab)) for L, lab in _tile_lengths(_le)]
for _le in (65, 100, 300):
    COND_CASES += [(2, _le, 0, L, "tile-strided-le%d-%s" % (_le, lab))
                   for L, lab in ((1, "1col"), (_le - 1, "le-1"), (_le, "le"), (_le + 1, "le+1"), (1103, "1103cols-ragged"))]
for _le, _q in ((7, 41), (31, 16), (1, 5), (8, 1)):
    COND_CASES += [(1, _le, _q, L, "stretch-le%d-q%d-%s" % (_le, _q, lab))
                   for L, lab in ((1, "1col"), (_le * _q, "exact"), (_le * _q + 13, "ragged-tail-in-last-bucket"), (max(1, _le * _q - _q - 1), "short"))]
COND_CASES += [(1, 5, 1000, 37, "stretch-le5-q1000-37cols-buckets-beyond-the-window"),
               (1, 3, 700, 1500, "stretch-le3-q700-1500cols-unrolled-segments"),
               (1, 3, 700, 2400, "stretch-le3-q700-2400cols-ragged-tail-unrolled")]
COND_IDS = [c[4] for c in COND_CASES]
COND_TLO = (36, 37, 39)                              # = 0, 1, 3 (mod 4)
COND_GEO = ((1, 1), (3, 24), (1, 24), (3, 1))        # (clips, rows)


def _cond_geo(i):
    return COND_TLO[i % 3], COND_GEO[i % 4]


class _Cond:
    """in [B][rows + 1][pitch] (a NaN row between the clips) with the window at [t_lo, t_lo + L); the table / the sums
    [B][rows][le + 3] + 5 floats between the clips"""

    def __init__(self, mode, le, q, L, t_lo, B, rows, exact=False, junk=False, seed=0):
        rng = np.random.default_rng(seed + 7 * le + L)
        self.mode, self.le, self.q, self.L, self.t_lo, self.B, self.rows = mode, le, max(q, 1), L, t_lo, B, rows
        self.pitch = t_lo + L + 5
        self.tp = le + 3
        self.tbs = rows * self.tp + 5
        if exact:
            self.win = (rng.integers(-8191, 8192, (B, rows, L)) / 8.0).astype(np.float32)        # multiples of 1/8 below 2^10
        else:
            self.win = rng.standard_normal((B, rows, L)).astype(np.float32)
        src = rng.standard_normal((B, rows + 1, self.pitch)).astype(np.float32) if junk else np.full((B, rows + 1, self.pitch), NAN, np.float32)
        src[:, :rows, t_lo:t_lo + L] = self.win
        self.src = _dev(src)

    def grad(self):
        out = _out(self.B * self.tbs)
        call("wn_cond_grad", ptr(self.src, PAD), (self.rows + 1) * self.pitch, self.pitch, self.rows, self.t_lo, self.t_lo + self.L, self.mode,
             self.le, self.q, ptr(out, PAD), self.tbs, self.tp, self.B, _st())
        return (self.table_view(_body(out, self.B * self.tbs)),)

    def table_view(self, flat):
        """[B][rows][tp] of the flat table buffer; asserts the 5 floats between the clips are NaN"""
        v = flat.reshape(self.B, self.tbs)
        assert np.isnan(v[:, self.rows * self.tp:]).all()
        return v[:, :self.rows * self.tp].reshape(self.B, self.rows, self.tp)


@pytest.mark.parametrize("i", range(len(COND_CASES)), ids=COND_IDS)
def test_cond_grad(i):
    mode, le, q, L, lab = COND_CASES[i]
    t_lo, (B, rows) = _cond_geo(i)
    c = _Cond(mode, le, q, L, t_lo, B, rows)
    (out,) = _twice(c.grad)
    assert np.isnan(out[:, :, le:]).all()                               # out_pitch > le: what lies behind column le stays
    got = out[:, :, :le]
    assert not np.isnan(got).any()
    ref = elem_ref.bucket_sums(c.win, mode, le, c.q)
    sabs, cnt = elem_ref.bucket_abs_sums(c.win, mode, le, c.q)
    bound = cnt * 2.0 ** -23 * sabs
    err = np.abs(got - ref)
    assert (got[..., cnt == 0] == 0).all()                              # a bucket without a column: exactly 0
    assert (err <= bound).all(), "worst %.3g of the bound" % (err[bound > 0] / bound[bound > 0]).max()
    if (bound > 0).any():
        _note("bucket sums %s" % ("stretch" if mode == 1 else "tile lds" if le <= 64 else "tile strided"),
              (err[bound > 0] / bound[bound > 0]).max(), lab)


@pytest.mark.parametrize("i", range(len(COND_CASES)), ids=COND_IDS)
def test_cond_grad_exact_inputs_equal_float64(i):
    mode, le, q, L, lab = COND_CASES[i]
    t_lo, (B, rows) = _cond_geo(i + 1)
    c = _Cond(mode, le, q, L, t_lo, B, rows, exact=True)
    (out,) = _twice(c.grad)
    assert np.isnan(out[:, :, le:]).all()
    assert np.array_equal(out[:, :, :le].astype(np.float64), elem_ref.bucket_sums(c.win, mode, le, c.q))


FINITE = [k for k, c in enumerate(COND_CASES) if c[4] in ("tile-lds-le5-5chunks-uneven-deal", "tile-strided-le100-1103cols-ragged",
                                                           "stretch-le7-q41-ragged-tail-in-last-bucket")]


@pytest.mark.parametrize("i", FINITE, ids=[COND_IDS[k] for k in FINITE])
def test_cond_grad_finite_surroundings(i):
    mode, le, q, L, lab = COND_CASES[i]
    c = _Cond(mode, le, q, L, 37, 3, 24, exact=True, junk=True)
    (out,) = _twice(c.grad)
    assert np.isnan(out[:, :, le:]).all()
    assert np.array_equal(out[:, :, :le].astype(np.float64), elem_ref.bucket_sums(c.win, mode, le, c.q))


@pytest.mark.parametrize("mode,le,q", [(1, 7, 41), (2, 5, 0), (2, 64, 0), (2, 100, 0)], ids=["stretch", "tile-lds-le5", "tile-lds-le64", "tile-strided"])
def test_cond_grad_empty_window(mode, le, q):
    """t_hi == t_lo with valid pointers: le zeros per row, the sum over nothing; with out (or in) NULL: -4, nothing launched"""
    c = _Cond(mode, le, q, 0, 37, 3, 24)
    (out,) = _twice(c.grad)
    assert np.isnan(out[:, :, le:]).all() and (out[:, :, :le] == 0).all()
    args = lambda i, o: ("wn_cond_grad", i, 25 * c.pitch, c.pitch, 24, 37, 37, mode, le, c.q, o, c.tbs, c.tp, 3, _st())
    o = _out(3 * c.tbs)
    assert _status(*args(ptr(c.src, PAD), None)) == -4 and "out" in _lib.load().wn_last_error().decode()
    assert _status(*args(None, ptr(o, PAD))) == -4
    torch.cuda.synchronize()
    assert np.isnan(_body(o, 3 * c.tbs)).all()


def test_cond_grad_refusals_and_no_work():
    c = _Cond(2, 5, 0, 40, 36, 1, 2, exact=True)
    o = _out(64)
    a = lambda mode, le, q, rows=2, B=1: ("wn_cond_grad", ptr(c.src, PAD), 3 * c.pitch, c.pitch, rows, 36, 76, mode, le, q, ptr(o, PAD), 2 * 8, 8, B, _st())
    for mode, le, q in ((0, 5, 1), (3, 5, 1), (1, 5, 0), (1, 5, -1), (2, 1025, 1), (1, 1025, 1)):
        assert _status(*a(mode, le, q)) == -4, (mode, le, q)
        assert _lib.load().wn_last_error().decode() != ""
    for q in (0, -1, 12345):                                            # the tile rule ignores q
        assert _status(*a(2, 5, q)) == 0
    torch.cuda.synchronize()
    got = _body(o, 64)
    assert np.array_equal(got[:16].reshape(2, 8)[:, :5].astype(np.float64), elem_ref.bucket_sums(c.win, 2, 5, 1)[0])
    o = _out(64)
    for rows, B, le in ((0, 1, 5), (2, 0, 5), (2, 1, 0)):               # no rows / clips / buckets: nothing written, NULL accepted
        assert _status("wn_cond_grad", None, 0, 0, rows, 36, 76, 2, le, 1, None, 0, 0, B, _st()) == 0
        assert _status(*a(2, le, 1, rows, B)) == 0
    torch.cuda.synchronize()
    assert np.isnan(_body(o, 64)).all()


EXPAND_W = ((1, "1col"), (3, "3cols"), (1023, "1023cols"), (1024, "1024cols-one-workgroup"), (1025, "1025cols-two-workgroups"), (1103, "1103cols"))
EXPAND_RULES = [(2, le, 0) for le in (1, 2, 5, 31, 64, 65, 300)] + [(1, 7, 41), (1, 31, 16), (1, 1, 5), (1, 8, 1), (1, 5, 1000), (1, 3, 700)]
EXPAND_CASES = [(m, le, q, w, "%s-le%d%s-%s" % ("stretch" if m == 1 else "tile", le, "-q%d" % q if m == 1 else "", lab))
                for m, le, q in EXPAND_RULES for w, lab in EXPAND_W]
EXPAND_CASES += [(1, 3, 700, 2400, "stretch-le3-q700-2400cols-three-workgroups")]


def _expand(c, tab, junk=False):
    n = c.B * (c.rows + 1) * c.pitch
    tabd = _dev(tab)

    def launch():
        out = _dev(np.random.default_rng(3).standard_normal(n).astype(np.float32)) if junk else _out(n)
        before = _body(out, n).copy()
        call("wn_cond_expand", ptr(tabd, PAD), c.tbs, c.tp, c.rows, c.t_lo, c.t_lo + c.L, c.mode, c.le, c.q, ptr(out, PAD),
             (c.rows + 1) * c.pitch, c.pitch, c.B, _st())
        return _body(out, n, (c.B, c.rows + 1, c.pitch)), before.reshape(c.B, c.rows + 1, c.pitch)

    return _twice(launch)


@pytest.mark.parametrize("i", range(len(EXPAND_CASES)), ids=[c[4] for c in EXPAND_CASES])
def test_cond_expand(i):
    mode, le, q, w, lab = EXPAND_CASES[i]
    t_lo, (B, rows) = _cond_geo(i)
    rows = min(rows, 5)
    c = _Cond(mode, le, q, w, t_lo, B, rows)
    val = np.random.default_rng(i).standard_normal((B, rows, le)).astype(np.float32)
    body = np.full((B, rows, c.tp), NAN, np.float32)                    # columns >= le and the gap between the clips: NaN
    body[:, :, :le] = val
    tab = np.full((B, c.tbs), NAN, np.float32)
    tab[:, :rows * c.tp] = body.reshape(B, rows * c.tp)
    out, _ = _expand(c, tab)
    mask = np.zeros(out.shape, bool)
    mask[:, :rows, t_lo:t_lo + w] = True
    assert np.array_equal(~np.isnan(out), mask)
    assert _same(out[:, :rows, t_lo:t_lo + w], elem_ref.bucket_expand(val, w, mode, le, c.q))


@pytest.mark.parametrize("mode,le,q,w", [(2, 5, 0, 1025), (1, 7, 41, 300)], ids=["tile", "stretch"])
def test_cond_expand_finite_surroundings(mode, le, q, w):
    c = _Cond(mode, le, q, w, 37, 3, 5)
    tab = np.random.default_rng(8).standard_normal((3, c.tbs)).astype(np.float32)
    val = tab[:, :5 * c.tp].reshape(3, 5, c.tp)[:, :, :le]
    out, before = _expand(c, tab, junk=True)
    want = before.copy()
    want[:, :5, 37:37 + w] = elem_ref.bucket_expand(val, w, mode, le, c.q)
    assert _same(out, want)


def test_cond_cases_cover_the_paths():
    by = {c[4]: c for c in COND_CASES}
    assert len(by) == len(COND_CASES)
    for le in (1, 2, 5, 31, 32, 33, 63, 64):
        rep = {1: 64, 2: 32, 5: 12, 31: 2, 32: 2, 33: 1, 63: 1, 64: 1}[le]

        def get(lab):
            hit = [c for c in COND_CASES if c[1] == le and c[0] == 2 and lab in c[4].split("-le%d-" % le)[1].split("=")]
            assert len(hit) == 1, (le, lab)
            return _tile_plan(le, hit[0][3])

        assert get("1chunk")["rep"] == rep and get("1chunk")["chunk"] == rep * le <= 64 < (rep + 1) * le
        assert get("1chunk")["nchunks"] == 1 and get("chunk+1")["nchunks"] == 2
        assert get("1col")["nchunks"] == 1
        if le > 1:
            assert any(c[1] == le and c[0] == 2 and c[3] == le - 1 for c in COND_CASES)           # a window shorter than one period
        p = get("3chunks-fewer-than-waves")
        assert p["nchunks"] == 3 and p["per"] == 1                      # wave 3 gets nothing
        p = get("4chunks-one-each")
        assert p["nchunks"] == 4 and p["per"] == 1
        p = get("5chunks-uneven-deal")
        assert p["nchunks"] == 5 and p["per"] == 2                      # waves 0, 1 two chunks, wave 2 one, wave 3 none
        # 16 chunks: every wave has four, so the unrolled-by-four loop is entered; one column less and the last trip's fourth
        # load of the last wave is cut by L for some lanes; one more opens a 17th chunk (per = 5)
        p = get("16chunks")
        assert p["nchunks"] == 16 and p["per"] == 4
        p = get("16chunks-1-unrolled-trip-cut")
        assert p["nchunks"] == 16 and p["per"] == 4
        assert get("16chunks+1")["per"] == 5
        p = get("1103cols-ragged")
        assert p["nchunks"] > 16 and (le == 1 or 1103 % p["chunk"] != 0)
    for mode, le, q, L, lab in COND_CASES:
        if "strided" in lab:
            assert mode == 2 and le > 64
        if "buckets-beyond-the-window" in lab:
            assert all(j * q >= L for j in range(1, le))                # every bucket but the first starts beyond the window
        if "unrolled-segments" in lab:
            assert q > 256 and L > 2 * q                                # the four-loads-in-flight loop runs in whole segments
        if "tail-unrolled" in lab:
            assert q > 256 and L - (le - 1) * q > q + 256               # ... and beyond s0 + q in the last bucket
        if "ragged-tail" in lab:
            assert L > le * q
    assert {_cond_geo(i)[0] % 4 for i in range(12)} == {0, 1, 3} and {_cond_geo(i)[1] for i in range(12)} == set(COND_GEO)
    for m, le, q, w, lab in EXPAND_CASES:                               # 1024 columns per cond_expand workgroup
        assert ("one-workgroup" in lab) == (w == 1024) and ("two-workgroups" in lab) == ((w + 1023) // 1024 == 2 and w == 1025)
    assert any(w % 4 for m, le, q, w, lab in EXPAND_CASES)


# ================================================================================================ optimizers
OPT_N = [(1, "1"), (255, "255"), (256, "256-one-workgroup"), (257, "257"), (524288, "524288-sweep"), (524289, "524289-wrap"),
         (2 * 524288 + 77, "1048653-wrap-two-and-three-trips")]
OPT_SWEEP = 2048 * 256
GS = 0.25
B1, B2, BC1, BC2 = 0.9, 0.999, 1 - 0.9 ** 3, 1 - 0.999 ** 3            # the bias corrections of step 3
E24, E23 = 2.0 ** -24, 2.0 ** -23
NV = 4096                                            # the non-vacuity condition is evaluated on at least this many elements


def _opt_inputs(n, seed):
    """p, g, first / second-moment-like state: |g| over ten decades (gscale * |g| from 2.5e-6 to 2.5e4), a state of the same scale
    (second moments from 1e-9 up), p of the size of a few updates so that the bar on p is about the update"""
    rng = np.random.default_rng(seed)
    m = max(n, NV)
    mag = 10.0 ** rng.uniform(-5, 5, m)
    g = (mag * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    prev = mag * GS * 10.0 ** rng.normal(0, 0.3, m)
    s1 = (prev * rng.standard_normal(m)).astype(np.float32)            # first moment / momentum buffer
    s2 = np.maximum(prev * prev, 1e-9).astype(np.float32)              # second moment / square average
    p = (rng.standard_normal(m) * 1e-2).astype(np.float32)
    return p, g, s1, s2


def _beyond(refs, alts, bars):
    """share of the elements where a reference with a term dropped lies beyond the bar of any output"""
    out = np.zeros(refs[0].shape, bool)
    for r, a, b in zip(refs, alts, bars):
        out |= np.abs(r - a) > b
    return out.mean()


def _opt_run(bufs, n, entry, args):
    """launch into fresh framed copies of the first n elements; None stays NULL.  Returns the buffers after the step."""
    def launch():
        d = [None if b is None else _dev(b[:n]) for b in bufs]
        call(entry, *[None if t is None else ptr(t, PAD) for t in d], n, *args, _st())
        return tuple(None if t is None else _body(t, n) for t in d)
    return _twice(launch)


def _opt_judge(group, case, got, ref, bar):
    assert not np.isnan(got).any()
    share = (np.abs(got - ref) / bar).max()
    _note(group, share, case)
    assert share <= 1.0, "%s %s: %.3g of the bar" % (group, case, share)


@pytest.mark.parametrize("eps", [1e-8, 1e-4], ids=["eps1e-8", "eps1e-4"])
@pytest.mark.parametrize("n,lab", OPT_N, ids=[l for n, l in OPT_N])
def test_adam(n, lab, eps):
    lr = 1e-3
    p, g, m, v = _opt_inputs(n, 11)
    f32 = lambda x: float(np.float32(x))
    ref = lambda **kw: elem_ref.adam_step(p, g, m, v, lr, B1, B2, kw.get("eps", eps), kw.get("bc1", BC1), kw.get("bc2", BC2), kw.get("gs", GS))
    rp, rm, rv = ref()
    gi = g.astype(np.float64) * GS
    bm = 8 * E24 * (np.abs(f32(B1) * m.astype(np.float64)) + np.abs((1 - f32(B1)) * gi))
    bv = 8 * E24 * (np.abs(f32(B2) * v.astype(np.float64)) + np.abs((1 - f32(B2)) * gi * gi))
    bp = E23 * np.abs(rp) + 8 * E24 * np.abs(rp - p)
    drops = dict(gscale=dict(gs=1.0), bc1=dict(bc1=1.0), bc2=dict(bc2=1.0))
    if eps == 1e-4:
        drops["eps"] = dict(eps=0.0)
    for name, kw in drops.items():
        share = _beyond((rp, rm, rv), ref(**kw), (bp, bm, bv))
        assert share >= 0.1, "dropping %s moves only %.3g of the elements beyond the bar" % (name, share)
    dp_, dg, dm, dv = _opt_run((p, g, m, v), n, "wn_adam_flat", (lr, B1, B2, eps, BC1, BC2, GS))
    assert _same(dg, g[:n])
    case = "n%s-%g" % (lab, eps)
    _opt_judge("adam m", case, dm, rm[:n], bm[:n])
    _opt_judge("adam v", case, dv, rv[:n], bv[:n])
    own = elem_ref.adam_p(p[:n], dm, dv, lr, eps, BC1, BC2)             # p on the device's own new moments
    _opt_judge("adam p", case, dp_, own, E23 * np.abs(own) + 8 * E24 * np.abs(own - p[:n]))


@pytest.mark.parametrize("variant", ["momentum0-null-buffer", "momentum0.9-first-step", "momentum0.9-later-step"])
@pytest.mark.parametrize("n,lab", OPT_N, ids=[l for n, l in OPT_N])
def test_sgd(n, lab, variant):
    lr = 1e-2
    mom = 0.0 if variant.startswith("momentum0-") else 0.9
    first = variant.endswith("first-step")
    p, g, buf, _ = _opt_inputs(n, 12)
    if mom == 0.0:
        buf = None
    elif first:
        buf = np.full_like(buf, NAN)                                    # torch has no buffer before the first step: whatever is there does not count
    f32 = lambda x: float(np.float32(x))
    ref = lambda gs=GS, m_=mom: elem_ref.sgd_step(p, g, buf, lr, m_, gs, first)
    rp, rb = ref()
    gi = g.astype(np.float64) * GS
    bp = E23 * np.abs(rp) + 8 * E24 * np.abs(rp - p)
    assert _beyond((rp,), (ref(gs=1.0)[0],), (bp,)) >= 0.1
    if mom and not first:
        bb = 8 * E24 * (np.abs(f32(mom) * buf) + np.abs(gi))
        ap, _ = elem_ref.sgd_step(p, g, buf, lr, 0.0, GS, first)        # the momentum term dropped
        assert _beyond((rp,), (ap,), (bp,)) >= 0.1
    elif mom:
        bb = 8 * E24 * np.abs(gi)
    dp_, dg, db = _opt_run((p, g, buf), n, "wn_sgd_flat", (lr, mom, GS, 1 if first else 0))
    assert _same(dg, g[:n])
    case = "n%s-%s" % (lab, variant)
    if mom:
        if first:
            assert _same(db, (g[:n] * np.float32(GS)))                  # equal to the scaled gradient
        _opt_judge("sgd buffer", case, db, rb[:n], bb[:n])
        own = p[:n].astype(np.float64) - f32(lr) * db
    else:
        assert db is None
        own = rp[:n]
    _opt_judge("sgd p", case, dp_, own, E23 * np.abs(own) + 8 * E24 * np.abs(own - p[:n]))


@pytest.mark.parametrize("variant", ["momentum0-null-buffer", "momentum0.9"])
@pytest.mark.parametrize("n,lab", OPT_N, ids=[l for n, l in OPT_N])
def test_rmsprop(n, lab, variant):
    lr, alpha, eps = 1e-3, 0.99, 1e-8
    mom = 0.9 if variant == "momentum0.9" else 0.0
    p, g, buf, sq = _opt_inputs(n, 13)
    buf = (buf / np.sqrt(sq)).astype(np.float32) if mom else None       # a buffer of g / avg's size
    f32 = lambda x: float(np.float32(x))
    ref = lambda gs=GS, e=eps, m_=mom: elem_ref.rmsprop_step(p, g, sq, buf if m_ else None, lr, alpha, e, m_, gs)
    rp, rs, rb = ref()
    gi = g.astype(np.float64) * GS
    bs = 8 * E24 * (np.abs(f32(alpha) * sq) + np.abs((1 - f32(alpha)) * gi * gi))
    bp = E23 * np.abs(rp) + 8 * E24 * np.abs(rp - p)
    for name, alt in (("gscale", ref(gs=1.0)), ("eps", ref(e=0.0))) + ((("momentum", ref(m_=0.0)),) if mom else ()):
        share = _beyond((rp, rs), alt[:2], (bp, bs))
        assert share >= 0.1, "dropping %s moves only %.3g of the elements beyond the bar" % (name, share)
    dp_, dg, ds, db = _opt_run((p, g, sq, buf), n, "wn_rmsprop_flat", (lr, alpha, eps, mom, GS))
    assert _same(dg, g[:n])
    case = "n%s-%s" % (lab, variant)
    _opt_judge("rmsprop square_avg", case, ds, rs[:n], bs[:n])
    step = gi[:n] / (np.sqrt(ds.astype(np.float64)) + f32(eps))         # on the device's own square average
    if mom:
        own_b = f32(mom) * buf[:n].astype(np.float64) + step
        _opt_judge("rmsprop buffer", case, db, own_b, 8 * E24 * (np.abs(f32(mom) * buf[:n]) + np.abs(step)))
        own = p[:n].astype(np.float64) - f32(lr) * db
    else:
        assert db is None
        own = p[:n].astype(np.float64) - f32(lr) * step
    _opt_judge("rmsprop p", case, dp_, own, E23 * np.abs(own) + 8 * E24 * np.abs(own - p[:n]))


def test_optimizer_refusals_and_no_work():
    buf = _out(64)
    p, s = ptr(buf, PAD), _st()
    assert _status("wn_sgd_flat", p, p, None, 8, 0.1, 0.9, 1.0, 0, s) == -4                       # momentum without its buffer
    assert _status("wn_rmsprop_flat", p, p, p, None, 8, 0.1, 0.99, 1e-8, 0.9, 1.0, s) == -4
    assert _status("wn_rmsprop_flat", p, p, None, None, 8, 0.1, 0.99, 1e-8, 0.0, 1.0, s) == -4    # no square_avg
    assert _status("wn_adam_flat", None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.1, 1.0, s) == 0
    assert _status("wn_sgd_flat", None, None, None, 0, 0.1, 0.0, 1.0, 1, s) == 0
    assert _status("wn_rmsprop_flat", None, None, p, None, 0, 0.1, 0.99, 1e-8, 0.0, 1.0, s) == 0
    torch.cuda.synchronize()
    assert np.isnan(_body(buf, 64)).all()


def test_optimizer_cases_cover_the_stride_loop():
    """2048 workgroups of 256 threads at most: a thread takes a second element from 524289 elements on"""
    for n, lab in OPT_N:
        grid = min(2048, (n + 255) // 256)
        assert ("wrap" in lab) == (n > grid * 256) == (n > OPT_SWEEP)
        assert ("sweep" in lab) == (n == OPT_SWEEP)
    trips = {len(range(i, 2 * 524288 + 77, OPT_SWEEP)) for i in (0, 76, 77, OPT_SWEEP - 1)}
    assert trips == {2, 3}


# ================================================================================================ exact movers
@pytest.mark.parametrize("B", [1, 3], ids=["1clip", "3clips"])
@pytest.mark.parametrize("t", [1, 255, 256, 257], ids=["t1", "t255", "t256", "t257"])
@pytest.mark.parametrize("q", [1, 2, 100, 256], ids=["q1", "q2", "q100", "q256"])
@pytest.mark.parametrize("layout", ["scrambled", "proper"])
def test_onehot(layout, q, t, B):
    rng = np.random.default_rng(q * 1000 + t + B)
    codes = rng.integers(0, q, (B, t)).astype(np.int32)
    k = rng.permutation(B * t)
    for j, bad in enumerate((-1, q, I32_MIN, q + 5)[:B * t - 1]):       # no one set for these
        codes.reshape(-1)[k[j]] = bad
    cd = _dev(codes, fill=0)                                            # a code read outside the tensor would set a one

    def launch():
        out = _out(B * q * t)
        call("wn_onehot", ptr(cd, PAD), ptr(out, PAD), B, q, t, 1 if layout == "scrambled" else 0, _st())
        return (_body(out, B * q * t, (B, q, t)),)

    (out,) = _twice(launch)
    assert ((out == 0) | (out == 1)).all()                              # every element of the tensor was written
    assert _same(out, elem_ref.onehot(codes, q, layout == "scrambled"))


def test_onehot_no_work_writes_nothing():
    out, cd = _out(64), _dev(np.zeros(8, np.int32), fill=0)
    for B, q, t in ((1, 0, 8), (1, -1, 8), (1, -(1 << 20), 8), (0, 4, 8), (1, 4, 0)):
        for scr in (0, 1):
            assert _status("wn_onehot", ptr(cd, PAD), ptr(out, PAD), B, q, t, scr, _st()) == 0
            assert _status("wn_onehot", None, None, B, q, t, scr, _st()) == 0
    assert _status("wn_onehot", ptr(cd, PAD), None, 1, 4, 8, 0, _st()) == -4
    torch.cuda.synchronize()
    assert np.isnan(_body(out, 64)).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257], ids=["n1", "n255", "n256-one-workgroup", "n257"])
def test_gather_grads(n):
    rng = np.random.default_rng(n)
    m = 3 * n + 5
    idx = rng.integers(-1, m, n).astype(np.int32)
    idx[0] = 0
    if n > 1:
        idx[n // 2], idx[n - 1] = -1, 0
    packed = np.full(m, NAN, np.float32)                                # NaN at every position no index refers to
    ref_pos = np.unique(idx[idx >= 0])
    packed[ref_pos] = rng.standard_normal(len(ref_pos)).astype(np.float32)
    pd, idd = _dev(packed), _dev(idx, fill=1)                           # an index read outside the tensor meets a NaN or the frame

    def launch():
        flat = _out(n)
        call("wn_gather_grads", ptr(pd, PAD), ptr(idd, PAD), ptr(flat, PAD), n, _st())
        return (_body(flat, n),)

    (flat,) = _twice(launch)
    assert _same(flat, elem_ref.gather(packed, idx))
    assert _status("wn_gather_grads", None, None, None, 0, _st()) == 0


def _thresholds(q, seed):
    """q - 1 ascending float32 thresholds in (-1, 1); from q = 256 on two of them are equal"""
    rng = np.random.default_rng(seed)
    thr = np.sort(rng.uniform(-1, 1, q - 1).astype(np.float32))
    if q >= 256:
        thr[q // 3 + 1] = thr[q // 3]
    return thr


def _samples(thr, n, seed):
    """thresholds first, then their float32 neighbours, +-0, +-inf, values outside the table, then random ones"""
    rng = np.random.default_rng(seed)
    one = np.float32(np.inf)
    pool = np.concatenate([thr[len(thr) // 2:], thr[:len(thr) // 2], np.nextafter(thr, -one), np.nextafter(thr, one),
                           np.array([0.0, -0.0, np.inf, -np.inf, -1.5, 1.5, thr[0] - 1, thr[-1] + 1], np.float32)]).astype(np.float32)
    if n <= len(pool):
        return pool[:n].copy()
    return np.concatenate([pool, rng.uniform(-1.1, 1.1, n - len(pool)).astype(np.float32)])


MULAW_N = [(1, "n1"), (257, "n257"), (524288 + 300, "n524588-wrap")]


@pytest.mark.parametrize("n,lab", MULAW_N, ids=[l for n, l in MULAW_N])
@pytest.mark.parametrize("q", [2, 3, 256, 1024], ids=["q2-one-threshold", "q3", "q256-equal-thresholds", "q1024-equal-thresholds"])
def test_mulaw_encode_q(q, n, lab):
    thr = _thresholds(q, q)
    x = _samples(thr, n, n)
    xd, td = _dev(x), _dev(thr)                                         # a threshold read outside the table is a NaN: never <= a sample

    def launch():
        codes = _out(n, np.int32, fill=-7777)
        call("wn_mulaw_encode_q", ptr(xd, PAD), ptr(td, PAD), q, ptr(codes, PAD), n, _st())
        return (_body(codes, n, fill=-7777),)

    (codes,) = _twice(launch)
    ref = elem_ref.mulaw_encode(x, thr)
    assert ref.min() >= 0 and ref.max() <= q - 1 and np.array_equal(ref, [(thr <= v).sum() for v in x[:300]] + list(ref[300:]))
    assert np.array_equal(codes, ref.astype(np.int32))


@pytest.mark.parametrize("n,lab", MULAW_N, ids=[l for n, l in MULAW_N])
def test_mulaw_encode_byte_entry(n, lab):
    """the 255-entry LDS copy of wn_mulaw_encode_tbl against the reference and, bit for bit, against the general entry at q = 256"""
    thr = _thresholds(256, 256)
    x = _samples(thr, n, n + 1)
    xd, td = _dev(x), _dev(thr)

    def launch():
        c8, c32 = _out(n, np.uint8, fill=0xAB), _out(n, np.int32, fill=-7777)
        call("wn_mulaw_encode_tbl", ptr(xd, PAD), ptr(td, PAD), ptr(c8, PAD), n, _st())
        call("wn_mulaw_encode_q", ptr(xd, PAD), ptr(td, PAD), 256, ptr(c32, PAD), n, _st())
        return _body(c8, n, fill=0xAB), _body(c32, n, fill=-7777)

    c8, c32 = _twice(launch)
    assert np.array_equal(c8, elem_ref.mulaw_encode(x, thr).astype(np.uint8))
    assert np.array_equal(c8.astype(np.int32), c32)


@pytest.mark.parametrize("n,lab", MULAW_N, ids=[l for n, l in MULAW_N])
@pytest.mark.parametrize("q", [2, 3, 256, 1024], ids=["q2", "q3", "q256", "q1024"])
def test_mulaw_decode(q, n, lab):
    rng = np.random.default_rng(q + n)
    table = np.sort(rng.uniform(-1, 1, q).astype(np.float32))
    codes = rng.integers(0, q, n).astype(np.int32)
    for j, c in enumerate((-5, q, 1 << 30, q - 1, 0, -1)):              # clamped to [0, q)
        if j < n:
            codes[(j * 37) % n] = c
    cd, tb = _dev(codes, fill=0), _dev(table)                           # an unclamped code reads a NaN of the table's frame

    def launch():
        audio = _out(n)
        call("wn_mulaw_decode_q", ptr(cd, PAD), ptr(tb, PAD), q, ptr(audio, PAD), n, _st())
        return (_body(audio, n),)

    (audio,) = _twice(launch)
    assert _same(audio, elem_ref.mulaw_decode(codes, table))
    if q == 256:                                                        # the byte entry: every code is in range by its type
        c8 = rng.integers(0, 256, n).astype(np.uint8)
        c8[0] = 255
        c8[n // 2] = 0
        c8d = _dev(c8, fill=0)

        def launch8():
            audio = _out(n)
            call("wn_mulaw_decode_lut", ptr(c8d, PAD), ptr(tb, PAD), ptr(audio, PAD), n, _st())
            return (_body(audio, n),)

        (a8,) = _twice(launch8)
        assert _same(a8, elem_ref.mulaw_decode(c8, table))


def test_mulaw_refusals_and_no_work():
    buf = _out(64)
    p, s = ptr(buf, PAD), _st()
    for q in (1, 0, -3):
        assert _status("wn_mulaw_encode_q", p, p, q, p, 8, s) == -4
        assert _status("wn_mulaw_decode_q", p, p, q, p, 8, s) == -4
    assert _status("wn_mulaw_encode_q", None, None, 2, None, 0, s) == 0
    assert _status("wn_mulaw_decode_q", None, None, 2, None, 0, s) == 0
    assert _status("wn_mulaw_encode_tbl", None, None, None, 0, s) == 0
    assert _status("wn_mulaw_decode_lut", None, None, None, 0, s) == 0
    torch.cuda.synchronize()
    assert np.isnan(_body(buf, 64)).all()


def test_mover_cases_cover_the_stride_loop():
    for n, lab in MULAW_N:
        assert ("wrap" in lab) == (n > min(2048, (n + 255) // 256) * 256)
    assert [(n + 255) // 256 for n in (1, 255, 256, 257)] == [1, 1, 1, 2]            # gather and one-hot: a thread per element


def test_zz_report():
    """the largest observed error of every group as a share of its bar (shown with -s)"""
    for k, (share, case) in sorted(WORST.items()):
        print("\n  elem worst %-28s %.3g of its bar at %s" % (k, share, case), end="")
    print()
