"""GPU tests of the causal layer computed from integer codes - wn_causal_fwd_codes (causal_fwd_codes_k) and wn_causal_wgrad_codes
(causal_wgrad_codes_k) - one launch at a time, against float64 (run with -m gpu).

Rules of tests/test_gpu_block_kernels.py: every test fills its own device buffers and launches ONE entry point; x0 and the slabs
are NaN beforehand (the gap between clips included), x0 must be NaN outside rows < n_rows x [1, T) afterwards and every slab
element written; dx holds NaN at column 0 and from T on, in the pair form P holds NaN below p_lo and from T on and Q at columns
< 1 + dn and from T on; padded rows of dx are zero; every case is launched twice and gives the same bits.

Reference: the dense one-hot the codes give under wn_onehot's rule (a code outside [0, 256) sets no one; the scrambled positions
are oracle.intops.one_hot_scrambled_positions, the proper ones oracle.intops.one_hot_proper), in numpy float64; one case per layout
holds it to what wn_onehot itself writes.
  forward   x0[b][r][s] = bias[r] + sum of W[r][q][0] over ones (q, s-1) + sum of W[r][q][1] over ones (q, s),  s in [1, T)
  gradient  dW[r][q][tap] = sum_{b, s in [1,T)} dx[b][r][s] in[b][q][s-1+tap]; the float64 sum over the slabs is compared, and
            the sum wn_reduce_slabs makes of them.

Bars, derived (not observed), per element:
  forward   the kernel starts from bias[r] and adds one fp32 weight per one, each addition rounded once: n additions give
            |got - ref| <= n 2^-24 (|bias| + sum |w|).  In the proper layout a column holds one one, so n <= 2 and the bar is
            2^-23 (|bias| + |w0| + |w1|); a column of the scrambled layout can hold any number of ones (it is a reshape), n then
            counts them, and is never taken below 2.
  gradient  a fixed-order fp32 sum of N terms: N 2^-23 sum |terms| (the bound of tests/test_gpu_wgrad_kernels.py's reduction
            sections), N = number of ones that reach the element + number of slabs; an element no one reaches is an exact zero.
            The pair form rounds P + Q once per term: N + 1.
  The 1e-5 of max-abs of tests/test_gpu_kernels.py stays as a second, coarser assert.

Largest errors observed on an MI355X over all cases of this file:
  forward                 0.98 of the derived per-element bar (the bar is sharp: two roundings of near-equal size); 4.3e-07 of max-abs
  gradient                0.17 of the bar; 3.3e-07 of max-abs
  gradient, pair form     0.21 of the bar; 2.1e-07 of max-abs"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from oracle import intops
from tests.test_gpu_block_kernels import NAN, _reduce, _same_bits, _written

DEV = "cuda"
LAYOUTS = {"scrambled": 1, "proper": 0}
SHAPES = [(32, 20), (64, 48), (64, 64)]                                     # (ch, R)
SHAPE_ID = ["ch%d-R%d" % s for s in SHAPES]
TS = [2, 3, 63, 64, 65, 66, 128, 129, 257, 1000]
BS = (1, 3)
MANY = (3, 5505)                                                            # B, T: 3 * 87 = 261 tiles > 256 workgroups
PATTERNS = ["uniform", "all-0", "all-255", "alternating", "run-over-a-tile-edge", "out-of-range"]
PATTERN_TS = [200, 512]                                                     # below 256, and a multiple of 256 (the scrambled layout's >> 8)
U = 2.0 ** -24
KERNELS = {"causal_%s_codes_k<%d>" % (k, ch) for k in ("fwd", "wgrad") for ch in (32, 64)}


def _route(kind, ch, q=256, T=2, batch=1):
    """Mirror of wn_causal_fwd_codes / wn_causal_wgrad_codes and their launchers: status of a refused call, None for an empty
    launch, else the kernel."""
    if q != 256:
        return -4
    if batch <= 0 or (T <= 1 if kind == "fwd" else T <= 0):
        return None
    if ch not in (32, 64):
        return -3
    return "causal_%s_codes_k<%d>" % (kind, ch)


def _slabs_formula(T, B):
    return 0 if T <= 0 or B <= 0 else min(256, -(-T // 64) * B)


def _codes(pattern, B, T, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, size=(B, T)).astype(np.int32)
    if pattern == "all-0":
        c[:] = 0
    elif pattern == "all-255":
        c[:] = 255
    elif pattern == "alternating":
        c[:] = np.where(np.arange(T) % 2 == 0, 0, 255)
    elif pattern == "run-over-a-tile-edge":
        c[:, 50:80] = 77                                                    # columns 50 .. 79 cross the tile edge at 64
        c[-1, 120:135] = 255
    elif pattern == "out-of-range":
        c[-1, ::7] = -1
        c[-1, 3::11] = 256
        c[-1, 5::13] = 1 << 20
        c[0, [0, 1, T - 2, T - 1]] = [-1, 256, 1 << 20, -1]
        c[0, 63:66] = [256, -1, 256]
    else:
        assert pattern == "uniform"
    return c


def _dense(codes, scr):
    """(B, 256, T) float64 one-hot under wn_onehot's rule: a code outside [0, 256) sets no one"""
    B, T = codes.shape
    out = np.zeros((B, 256 * T))
    for b in range(B):
        ok = (codes[b] >= 0) & (codes[b] < 256)
        safe = np.where(ok, codes[b], 0)
        if scr:
            out[b, intops.one_hot_scrambled_positions(safe)[ok]] = 1.0
        else:
            out[b] = (intops.one_hot_proper(safe) * ok[None, :]).reshape(-1)
    return out.reshape(B, 256, T)


def _pitch(T):
    return (T + 3) // 4 * 4 + 8


def _nan_dev(*shape):
    return torch.full(shape, NAN, device=DEV)


# ------------------------------------------------------------------------------------------------ forward
def _forward(scr, ch, R, T, B, bias, codes, dense, seed, tag, worst=None):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((R, 256, 2)).astype(np.float32)
    wt = np.zeros((2, 256, ch), np.float32)
    wt[:, :, :R] = w.transpose(2, 1, 0)
    bv = None
    if bias:
        bv = np.full(ch, NAN, np.float32)                                    # rows >= n_rows are not read
        bv[:R] = rng.standard_normal(R).astype(np.float32)
    pitch, rows = _pitch(T), ch + 1                                          # one NaN row between the clips
    cd, wtd = torch.from_numpy(codes).to(DEV), torch.from_numpy(wt).to(DEV)
    bd = torch.from_numpy(bv).to(DEV) if bias else None
    outs = []
    for _ in range(2):
        x0 = _nan_dev(B, rows, pitch)
        call("wn_causal_fwd_codes", ptr(cd), scr, ptr(wtd), ptr(bd), R, ptr(x0), rows * pitch, pitch, ch, 256, T, B, _lib.stream())
        torch.cuda.synchronize()
        outs.append(x0.cpu())
    assert _same_bits(outs[0], outs[1]), tag + ": a second launch gives other bits"
    got = outs[0]
    assert _written(got) == B * R * (T - 1), tag + ": x0 written outside rows < n_rows x [1, T), or not all of it"
    g = got[:, :R, 1:T].numpy().astype(np.float64)
    assert not np.isnan(g).any(), tag
    w64, b64 = w.astype(np.float64), (bv[:R].astype(np.float64) if bias else np.zeros(R))
    ref = b64[None, :, None] + np.matmul(w64[:, :, 0], dense[:, :, 0:T - 1]) + np.matmul(w64[:, :, 1], dense[:, :, 1:T])
    mag = np.abs(b64)[None, :, None] + np.matmul(np.abs(w64[:, :, 0]), dense[:, :, 0:T - 1]) + np.matmul(np.abs(w64[:, :, 1]), dense[:, :, 1:T])
    n = dense[:, :, 0:T - 1].sum(1) + dense[:, :, 1:T].sum(1)                # additions per output column
    if not scr:
        assert n.max() <= 2
    bar = np.maximum(n, 2)[:, None, :] * U * mag
    err = np.abs(g - ref)
    frac = float((err / np.where(bar > 0, bar, 1.0)).max())
    rel = float(err.max() / max(np.abs(ref).max(), 1e-300))
    if worst is not None:
        worst["fwd"] = max(worst.get("fwd", 0.0), frac)
        worst["fwd_rel"] = max(worst.get("fwd_rel", 0.0), rel)
    assert (err <= bar).all(), (tag, frac)
    assert rel <= 1e-5 or np.abs(ref).max() == 0, (tag, rel)


# ------------------------------------------------------------------------------------------------ weight gradient
def _launch_wgrad(cd, scr, dx, dxq, dn, p_lo, rows, pitch, ch, T, B):
    ns = _lib.causal_codes_slabs(T, B)
    slab = _nan_dev(ns + 1, ch, 512)                                         # one slab more: it must stay NaN
    call("wn_causal_wgrad_codes", ptr(cd), scr, ptr(dx), ptr(dxq), dn, p_lo, rows * pitch, pitch, ch, 256, T, B, ptr(slab), _lib.stream())
    torch.cuda.synchronize()
    assert _written(slab[ns:]) == 0, "a slab beyond wn_causal_wgrad_codes_slabs was written"
    assert _written(slab[:ns]) == ns * ch * 512, "a slab element was not written (or is NaN)"
    return slab[:ns].contiguous(), ns


def _grad_ref(d64, dense, T):
    """sum_b d[b][:, 1:T] x (tap 0 | tap 1 rows of the one-hot) -> [rows][512]"""
    return np.concatenate([np.matmul(d64[:, :, 1:T], dense[:, :, 0:T - 1].transpose(0, 2, 1)).sum(0),
                           np.matmul(d64[:, :, 1:T], dense[:, :, 1:T].transpose(0, 2, 1)).sum(0)], 1)


def _check_grad(slab, ns, ch, want, mag, count, extra, tag, key, worst):
    bar = (count[None, :] + ns + extra) * 2 * U * mag
    m = max(np.abs(want).max(), 1e-300)
    for name, got in (("slab sum", slab.double().sum(0).cpu().numpy()), ("wn_reduce_slabs", _reduce(slab, ns, ch, 512).numpy().astype(np.float64))):
        err = np.abs(got - want)
        frac = float((err / np.where(bar > 0, bar, 1.0)).max())
        if worst is not None:
            worst[key] = max(worst.get(key, 0.0), frac)
            worst[key + "_rel"] = max(worst.get(key + "_rel", 0.0), float(err.max() / m))
        assert (err <= bar).all(), (tag, name, frac)
        assert err.max() / m <= 1e-5 or np.abs(want).max() == 0, (tag, name)


def _wgrad(scr, ch, R, T, B, codes, dense, seed, tag, worst=None):
    rng = np.random.default_rng(seed)
    pitch, rows = _pitch(T), ch + 2
    dx = np.full((B, rows, pitch), NAN, np.float32)                          # NaN at column 0, from T on and between the clips
    dx[:, :R, 1:T] = rng.standard_normal((B, R, T - 1)).astype(np.float32)
    dx[:, R:ch, 1:T] = 0
    cd, dxd = torch.from_numpy(codes).to(DEV), torch.from_numpy(dx).to(DEV)
    slab, ns = _launch_wgrad(cd, scr, dxd, None, 0, 0, rows, pitch, ch, T, B)
    slab2, _ = _launch_wgrad(cd, scr, dxd, None, 0, 0, rows, pitch, ch, T, B)
    assert ns == _slabs_formula(T, B)
    assert _same_bits(slab, slab2), tag + ": a second launch gives other bits"
    d64 = np.nan_to_num(dx[:, :ch].astype(np.float64))
    count = np.concatenate([dense[:, :, 0:T - 1].sum((0, 2)), dense[:, :, 1:T].sum((0, 2))])
    _check_grad(slab, ns, ch, _grad_ref(d64, dense, T), _grad_ref(np.abs(d64), dense, T), count, 0, tag, "wgrad", worst)
    # the pair form: dx[s] = P[s] (s >= p_lo) + Q[s + dn]
    dn, p_lo = 3, 5
    P = np.full((B, rows, pitch), NAN, np.float32)
    Q = np.full((B, rows, pitch), NAN, np.float32)
    if p_lo < T:
        P[:, :R, p_lo:T] = rng.standard_normal((B, R, T - p_lo)).astype(np.float32)
        P[:, R:ch, p_lo:T] = 0
    if 1 + dn < T:
        Q[:, :R, 1 + dn:T] = rng.standard_normal((B, R, T - 1 - dn)).astype(np.float32)
        Q[:, R:ch, 1 + dn:T] = 0
    Pz, Qz = np.zeros((B, ch, T), np.float32), np.zeros((B, ch, T), np.float32)
    Pz[:, :, min(p_lo, T):T] = P[:, :ch, min(p_lo, T):T]
    if 1 + dn < T:
        Qz[:, :, 1:T - dn] = Q[:, :ch, 1 + dn:T]
    whole = np.full((B, rows, pitch), NAN, np.float32)
    whole[:, :ch, 1:T] = (Pz + Qz)[:, :, 1:T]                                 # float32(P + Q), built on the host
    Pd, Qd, wd = (torch.from_numpy(a).to(DEV) for a in (P, Q, whole))
    s_whole, _ = _launch_wgrad(cd, scr, wd, None, 0, 0, rows, pitch, ch, T, B)
    s_pair, _ = _launch_wgrad(cd, scr, Pd, Qd, dn, p_lo, rows, pitch, ch, T, B)
    s_pair2, _ = _launch_wgrad(cd, scr, Pd, Qd, dn, p_lo, rows, pitch, ch, T, B)
    assert _same_bits(s_pair, s_pair2), tag + ": a second pair-form launch gives other bits"
    assert _same_bits(s_pair, s_whole), tag + ": the pair form differs from the whole form on float32(P + Q)"
    p64 = Pz.astype(np.float64) + Qz.astype(np.float64)
    _check_grad(s_pair, ns, ch, _grad_ref(p64, dense, T), _grad_ref(np.abs(Pz).astype(np.float64) + np.abs(Qz), dense, T), count, 1,
                tag + " pair", "wgrad_pair", worst)


WORST = {}


def _report(tag):
    print(tag, " ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


# ================================================================================================ A. tile edges
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_forward_at_tile_edges(layout, shape, T):
    (ch, R), scr = shape, LAYOUTS[layout]
    for B in BS:
        codes = _codes("uniform", B, T, T + B)
        dense = _dense(codes, scr)
        for bias in (False, True):
            _forward(scr, ch, R, T, B, bias, codes, dense, T + R, "%s ch%d R%d T%d B%d bias%d" % (layout, ch, R, T, B, bias), WORST)
    _report("forward")


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_wgrad_at_tile_edges(layout, shape, T):
    (ch, R), scr = shape, LAYOUTS[layout]
    for B in BS:
        codes = _codes("uniform", B, T, T + B)
        _wgrad(scr, ch, R, T, B, codes, _dense(codes, scr), T + R, "%s ch%d R%d T%d B%d" % (layout, ch, R, T, B), WORST)
    _report("wgrad")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_more_tiles_than_workgroups(layout):
    """261 tiles: the gradient's 256 workgroups walk more than one tile each and the slab count is capped"""
    (B, T), scr = MANY, LAYOUTS[layout]
    assert -(-T // 64) * B == 261 and _lib.causal_codes_slabs(T, B) == 256
    codes = _codes("run-over-a-tile-edge", B, T, 5)
    dense = _dense(codes, scr)
    _forward(scr, 64, 48, T, B, True, codes, dense, 6, layout + " many tiles", WORST)
    _wgrad(scr, 64, 48, T, B, codes, dense, 7, layout + " many tiles", WORST)
    _wgrad(scr, 32, 20, T, B, codes, dense, 8, layout + " many tiles ch32", WORST)
    _report("many")


# ================================================================================================ B. code patterns
@pytest.mark.parametrize("T", PATTERN_TS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_code_patterns(layout, pattern, T):
    scr, B = LAYOUTS[layout], 2
    codes = _codes(pattern, B, T, len(pattern))
    dense = _dense(codes, scr)
    if pattern == "out-of-range":
        assert ((codes < 0) | (codes > 255)).sum() > 20 and dense.sum() == ((codes >= 0) & (codes < 256)).sum()
    for (ch, R), bias in (((64, 48), True), ((32, 20), False)):
        tag = "%s %s T%d ch%d" % (layout, pattern, T, ch)
        _forward(scr, ch, R, T, B, bias, codes, dense, T + ch, tag, WORST)
        _wgrad(scr, ch, R, T, B, codes, dense, T + ch + 1, tag, WORST)
    _report("patterns")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_reference_one_hot_is_what_wn_onehot_writes(layout):
    scr, B, T = LAYOUTS[layout], 2, 200
    codes = _codes("out-of-range", B, T, 3)
    out = _nan_dev(B, 256, T)
    call("wn_onehot", ptr(torch.from_numpy(codes).to(DEV)), ptr(out), B, 256, T, scr, _lib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), _dense(codes, scr))
    ok = (codes >= 0) & (codes < 256)
    fn = intops.one_hot_scrambled if scr else intops.one_hot_proper
    c0 = np.where(ok, codes, 0)[0]
    assert np.array_equal(_dense(c0[None], scr)[0], fn(c0).astype(np.float64))     # in-range codes: oracle.intops' own dense form


# ================================================================================================ C. plan, refusals, coverage
def test_slab_count():
    for T in (-3, 0, 1, 2, 63, 64, 65, 128, 129, 1000, 5440, 5441, 5505, 16000, 100000):
        for B in (-1, 0, 1, 2, 3, 7, 300):
            assert _lib.causal_codes_slabs(T, B) == _slabs_formula(T, B), (T, B)


def _raw(kind, ch=64, q=256, T=130, B=2, out=None):
    lib, pitch = _lib.load(), _pitch(130)
    cd = torch.zeros(2, 130, dtype=torch.int32, device=DEV)
    if kind == "fwd":
        wt = torch.zeros(2, 256, 64, device=DEV)
        rc = lib.wn_causal_fwd_codes(ptr(cd), 1, ptr(wt), None, 20, ptr(out), 64 * pitch, pitch, ch, q, T, B, _lib.stream())
    else:
        dx = torch.zeros(2, 64, pitch, device=DEV)
        rc = lib.wn_causal_wgrad_codes(ptr(cd), 1, ptr(dx), None, 0, 0, 64 * pitch, pitch, ch, q, T, B, ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", ["fwd", "wgrad"])
@pytest.mark.parametrize("what,over,status", [("q=255", dict(q=255), -4), ("q=512", dict(q=512), -4), ("ch48", dict(ch=48), -3),
                                              ("T=0", dict(T=0), 0), ("T=-1", dict(T=-1), 0), ("batch=0", dict(B=0), 0),
                                              ("batch=-1", dict(B=-1), 0)])
def test_refusals_and_empty_launches_write_nothing(kind, what, over, status):
    a = dict(ch=64, q=256, T=130, B=2)
    a.update(over)
    want = _route(kind, a["ch"], a["q"], a["T"], a["B"])
    assert not isinstance(want, str) and (want or 0) == status
    out = _nan_dev(2, 64, _pitch(130)) if kind == "fwd" else _nan_dev(4, 64, 512)
    assert _raw(kind, out=out, **over) == status
    assert _written(out) == 0


def test_one_sample_clips():
    """T = 1: no output column exists - the forward writes nothing; the gradient writes its wn_causal_wgrad_codes_slabs(1, B) = B
    slabs, as zeros"""
    out = _nan_dev(2, 64, _pitch(130))
    assert _route("fwd", 64, T=1) is None and _raw("fwd", T=1, out=out) == 0 and _written(out) == 0
    slab = _nan_dev(4, 64, 512)
    assert _lib.causal_codes_slabs(1, 2) == 2 and _raw("wgrad", T=1, out=slab) == 0
    assert (slab[:2] == 0).all().item() and _written(slab[2:]) == 0


def test_cases_reach_both_kernels_at_both_widths_and_layouts():
    reached = {(_route(k, ch, T=T, batch=B), lay) for k in ("fwd", "wgrad") for ch, _ in SHAPES for T in TS for B in BS for lay in LAYOUTS}
    assert reached == {(k, lay) for k in KERNELS for lay in LAYOUTS} and len(KERNELS) == 4
    assert {T % 64 for T in TS} >= {0, 1, 2, 63} and min(TS) == 2 and any(T < 64 for T in TS) and set(BS) == {1, 3}
    assert any(T < 256 for T in PATTERN_TS) and any(T % 256 == 0 for T in PATTERN_TS)
    assert any(R < ch for ch, R in SHAPES) and any(R == ch for ch, R in SHAPES)
