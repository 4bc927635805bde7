"""GPU tests of wn_chan_gemm's four kernels and of wn_pack_weights, one launch at a time, against float64 (run with -m gpu).

The rules of tests/test_gpu_fwd_kernels.py, for the kernels behind wn_launch_gemm (chan_gemm_k "narrow", chan_gemm_wide2_k,
chan_gemm_rw_k, chan_gemm_bst_k) and for pack_weights_k:
  - every test fills its device buffers itself and launches ONE entry point through _lib.call;
  - the reference is float64 on the CPU from include/wavenet_hip.h's formula
        out[b][m][t + out_shift] = resid[b][m][t] (t >= resid_lo) + mask(bias[m] + sum_tap sum_k W[m][tap, k] pre(in_tap[b][k][t + shift_tap]))
    computed from the very float32 inputs the kernel read; mask and relu_in come from given data and are exact: no element is excused;
  - every output buffer is NaN beforehand, slack included; afterwards every element of rows < m_valid on [t_lo, t_hi) takes part in
    the comparison and everything else is still NaN (counted: `_written`);
  - inputs hold NaN wherever their values do not count: in0 / in1 outside [in_lo, in_hi) (slack and the rows beyond a tap's 32 ks
    included), resid at columns < max(resid_lo, t_lo) and >= t_hi, mask outside [t_lo, t_hi), resid / mask / bias at rows >= m_valid;
  - every case is launched twice into fresh NaN buffers: same bits;
  - `_route` mirrors wn_launch_gemm's dispatch (the four launchers' preconditions, the rw / bst grid formulas, the compute-unit count
    of the device the tests run on); one test per section asserts that every case reaches the kernel and the regime its id names.

Bars: the project's own TOL[mode] of tests/test_gpu_kernels.py, relative to the reference tensor's max-abs
(1e-5 f16x3 / 1e-4 bf16x3 / 1e-2 f16x1 / 5e-2 bf16x1); bit equality for a repeated launch, for WN_GEMM_BST unset / 1 / 0, for the
0/1-input pack-order cases and for wn_pack_weights.

Largest error observed per kernel and mode, in units of the reference's max-abs (MI355X):
  narrow   f16x3 6.4e-7   bf16x3 6.2e-6   f16x1 3.3e-4   bf16x1 2.8e-3
  wide2    f16x3 3.6e-7   bf16x3 7.1e-6   f16x1 3.3e-4   bf16x1 2.7e-3
  rw       f16x3 4.8e-7   bf16x3 5.4e-6
  bst      f16x3 5.7e-7   bf16x3 5.1e-6"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from music_amd.engine import SLACK, pack_index
from tests.test_gpu_kernels import _packed, _buf, _view, TOL
from tests.test_gpu_block_kernels import _nanbuf, _written, _same_bits

DEV = "cuda"
MF, MB, M1F, M1B = _lib.F16X3, _lib.BF16X3, _lib.F16X1, _lib.BF16X1
MODE_ID = {MF: "f16x3", MB: "bf16x3", M1F: "f16x1", M1B: "bf16x1"}
X3, X1 = (MF, MB), (M1F, M1B)
ALL = X3 + X1
NAN = float("nan")
BACK = 512                       # floats behind every buffer, as _buf


def _cus():
    """compute units of the device the tests run on (wn_num_cus() reads the same number)"""
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ceil(a, b):
    return (a + b - 1) // b


# ================================================================================================ cases
def C(id, kernel, why, mt, ks0, t_lo, t_hi, ks1=0, s0=0, s1=0, in_lo=None, in_hi=None, B=2, m_valid=None, bias=False, resid=None,
      resid_lo=None, mask=False, relu=False, out="abs", ipitch=None, modes=X3, seed=0):
    """One wn_chan_gemm call.  kernel: the one it must reach; why(r): the regime its id names, on _route's result.
    resid: None, 'own' (a buffer of its own) or 'alias' (resid == out, identical strides).  out: 'abs' (absolute time, the inputs'
    pitch), 'compact' (column t - t_lo, pitch t_hi - t_lo), 'odd' (odd pitch and odd out_shift), 'user' (pitch t_hi, no slack
    columns: a user's [B][M][T] tensor).  ipitch: the inputs' pitch (default: a multiple of 256 with 256 columns to spare)."""
    sh = (s0, s1) if ks1 > 0 else (s0,)
    c = SimpleNamespace(id=id, kernel=kernel, why=why, mt=mt, ks0=ks0, ks1=ks1, s0=s0, s1=s1, t_lo=t_lo, t_hi=t_hi, B=B,
                        in_lo=t_lo + min(sh) if in_lo is None else in_lo, in_hi=t_hi + max(sh) if in_hi is None else in_hi,
                        m_valid=16 * mt if m_valid is None else m_valid, bias=bias, resid=resid,
                        resid_lo=t_lo if resid_lo is None else resid_lo, mask=mask, relu=relu, out=out, modes=modes, seed=seed)
    assert c.in_lo >= 0 and t_lo >= 0 and t_hi > t_lo and 0 < c.m_valid <= 16 * mt
    c.pitch = _ceil(max(t_hi, c.in_hi, 64), 256) * 256 + 256 if ipitch is None else ipitch
    assert c.pitch >= max(c.in_hi, 1)
    W = t_hi - t_lo
    if out == "abs":
        c.opitch, c.oshift = c.pitch, 0
    elif out == "compact":
        c.opitch, c.oshift = W, -t_lo
    elif out == "odd":
        c.opitch, c.oshift = (W + 3) | 1, -t_lo + (1 if t_lo % 2 == 0 else 2)
    else:
        c.opitch, c.oshift = t_hi, 0
    c.obs = 16 * mt * c.opitch
    assert resid != "alias" or c.oshift == 0
    return c


def _rw_items(nwg, ipw, total):
    """chan_gemm_rw_k's walk (swz = 1): per workgroup the items it multiplies, interleaved inside its XCD's contiguous range"""
    qn, rn = nwg >> 3, nwg & 7
    out = []
    for wg in range(nwg):
        xcd = wg & 7
        first = xcd * (qn + 1) if xcd < rn else rn * (qn + 1) + (xcd - rn) * qn
        cnt = qn + 1 if xcd < rn else qn
        i_lo, i_hi = first * ipw + (wg >> 3), min((first + cnt) * ipw, total)
        out.append(list(range(i_lo, i_hi, cnt)) if i_lo < i_hi else [])
    return out


def _route(c, mode, env=None):
    """Mirror of wn_launch_gemm (wn_gemm.hip, wn_gemm_rw.hip, wn_gemm_bst.hip): the kernel a call reaches and its launch geometry.
    env: the value of WN_GEMM_BST (None = unset)."""
    x3 = mode in X3
    t_base = c.t_lo & ~63                                        # wn_tile_origin
    ks = c.ks0 + c.ks1
    ncol = c.t_hi - t_base
    r = SimpleNamespace(c=c, mode=mode, t_base=t_base, KS=ks, ncol=ncol, weave=c.ks1 == c.ks0,
                        early=c.resid is not None and not c.mask)
    shifts = [(c.s0, c.ks0)] + ([(c.s1, c.ks1)] if c.ks1 > 0 else [])
    if x3 and c.mt == 4 and ks in (8, 4) and not c.relu and c.oshift == 0 and c.in_hi - c.in_lo >= 2:
        r.kernel = "rw"
        r.steps = _ceil(ncol, 32)
        r.total = r.steps * c.B
        r.ipw = max(1, _ceil(r.total, 512))
        r.nwg = _ceil(r.total, r.ipw)
        r.items = _rw_items(r.nwg, r.ipw, r.total)
        assert sorted(i for w in r.items for i in w) == list(range(r.total)), "the mirror of the rw walk loses or repeats items"
        r.n_items = {len(w) for w in r.items}
        # per tap: does an item exist that is cut by the low / by the high edge of the input window and still holds valid columns
        r.edge = []
        for sh, _ in shifts:
            lo = hi = False
            for i in range(r.steps):
                a = t_base + 32 * i + sh
                lo |= a < c.in_lo < a + 32
                hi |= a < c.in_hi < a + 32
            r.edge.append((lo, hi))
        return r
    if x3 and c.ks1 == 0 and c.resid is None and c.ks0 == 8 and c.mt >= 32 and c.mt % 3 == 0 and not (env and env[0] == "0"):
        r.kernel = "bst"
        r.ntx = _ceil(ncol, 128)
        r.ntiles = r.ntx * c.B
        r.npass = (c.mt // 3 + 7) // 8
        r.grid = _cus() if (env and env[0] == "1" and _cus() <= r.ntiles) else r.ntiles
        r.nfull = r.ntiles // r.grid
        r.left = r.ntiles - r.nfull * r.grid
        r.units = r.left * r.npass
        r.nt_ok = ((c.oshift | c.opitch) & 3) == 0 and (c.obs & 3) == 0        # and a 16-byte aligned `out` (asserted at the launch)
        r.interior = any(t_base + 128 * x >= c.t_lo and t_base + 128 * (x + 1) <= c.t_hi for x in range(r.ntx))
        return r
    if c.mt <= 4:
        r.kernel = "narrow"
        r.gx, r.gy = _ceil(ncol, 512), 1
        groups = [t_base + 64 * i for i in range(_ceil(ncol, 64))]
    else:
        r.kernel = "wide2"
        r.gx, r.gy = _ceil(ncol, 256), _ceil(c.mt, 16)
        groups = [t_base + 64 * i for i in range(4 * r.gx)]
    # per tap: the `inner` flags of the 64-column loader groups (plain loads) and whether a guarded group still holds valid columns
    r.inner = [{(g + sh >= c.in_lo and g + 64 + sh <= c.in_hi) for g in groups} for sh, _ in shifts]
    r.guarded_live = [any(not (g + sh >= c.in_lo and g + 64 + sh <= c.in_hi) and g + sh < c.in_hi and g + 64 + sh > c.in_lo for g in groups)
                      for sh, _ in shifts]
    return r


# ================================================================================================ one call: buffers, reference, check
def _canary_rows(B, rows, pitch, data, lo, hi, live_rows):
    """flat CPU buffer (SLACK in front, BACK behind) of [B][rows][pitch]: `data` on rows < live_rows x [lo, hi), NaN everywhere else"""
    t = torch.full((SLACK + B * rows * pitch + BACK,), NAN)
    v = t[SLACK:SLACK + B * rows * pitch].view(B, rows, pitch)
    lo = max(lo, 0)
    if hi > lo:
        v[:, :live_rows, lo:hi] = data[:, :live_rows, lo:hi]
    return t


class _Gemm:
    """The buffers of one case (shared by the modes: the inputs do not depend on the mode), the launch and the float64 reference"""

    def __init__(self, c):
        self.c = c
        rng = np.random.default_rng(1000 + c.seed)
        g = torch.Generator().manual_seed(2000 + c.seed)
        M, B, p = 16 * c.mt, c.B, c.pitch
        self.RI = RI = 32 * max(c.ks0, c.ks1)
        self.w = (rng.standard_normal((M, 32 * (c.ks0 + c.ks1))) * 0.1).astype(np.float32)
        self.pk = {}
        self.x0 = _canary_rows(B, RI, p, torch.randn(B, RI, p, generator=g), c.in_lo, c.in_hi, 32 * c.ks0)
        self.x1 = _canary_rows(B, RI, p, torch.randn(B, RI, p, generator=g), c.in_lo, c.in_hi, 32 * c.ks1) if c.ks1 > 0 else None
        self.x0d, self.x1d = self.x0.to(DEV), self.x1.to(DEV) if c.ks1 > 0 else None
        self.bias = self.res = self.msk = self.old = None
        if c.bias:
            self.bias = torch.full((M,), NAN)
            self.bias[:c.m_valid] = torch.randn(c.m_valid, generator=g)
            self.biasd = self.bias.to(DEV)
        if c.resid == "own":
            self.res = _canary_rows(B, M, p, torch.randn(B, M, p, generator=g), max(c.resid_lo, c.t_lo), c.t_hi, c.m_valid)
            self.resd = self.res.to(DEV)
        if c.resid == "alias":                                   # the old contents of `out`: data on the window, NaN elsewhere
            self.old = torch.randn(B, c.m_valid, c.t_hi - c.t_lo, generator=g)
        if c.mask:
            self.msk = _canary_rows(B, M, p, torch.randn(B, M, p, generator=g), c.t_lo, c.t_hi, c.m_valid)
            self.mskd = self.msk.to(DEV)
        self._ref = None

    def window(self, out):
        """the elements a launch must write: rows < m_valid on [t_lo, t_hi), as a [B][m_valid][t_hi - t_lo] view of the flat buffer"""
        c = self.c
        return torch.as_strided(out, (c.B, c.m_valid, c.t_hi - c.t_lo), (c.obs, c.opitch, 1), SLACK + c.t_lo + c.oshift)

    def reference(self):
        if self._ref is not None:
            return self._ref
        c = self.c
        B, mv, p = c.B, c.m_valid, c.pitch
        ts = torch.arange(c.t_lo, c.t_hi)
        wd = torch.from_numpy(self.w).double()[:mv]
        acc = torch.zeros(B, mv, len(ts), dtype=torch.float64)
        k0 = 0
        for x, ks, sh in ((self.x0, c.ks0, c.s0), (self.x1, c.ks1, c.s1)):
            if ks == 0:
                continue
            K = 32 * ks
            cols = ts + sh
            ok = (cols >= c.in_lo) & (cols < c.in_hi)              # columns outside the window read as 0
            a = torch.zeros(B, K, len(ts), dtype=torch.float64)
            a[:, :, ok] = x[SLACK:SLACK + B * self.RI * p].view(B, self.RI, p)[:, :K][:, :, cols[ok]].double()
            assert not torch.isnan(a).any()
            if c.relu:
                a.clamp_(min=0)
            acc += torch.matmul(wd[:, k0:k0 + K], a)
            k0 += K
        if c.bias:
            acc += self.bias[:mv].double()[None, :, None]
        if c.mask:
            m = self.msk[SLACK:SLACK + B * 16 * c.mt * p].view(B, 16 * c.mt, p)[:, :mv][:, :, ts]
            assert not torch.isnan(m).any()
            acc = torch.where(m > 0, acc, torch.zeros_like(acc))
        if c.resid is not None:
            if c.resid == "own":
                r = self.res[SLACK:SLACK + B * 16 * c.mt * p].view(B, 16 * c.mt, p)[:, :mv][:, :, ts].double()
            else:
                r = self.old.double().clone()
            r[:, :, ts < c.resid_lo] = 0
            assert not torch.isnan(r).any()
            acc += r                                               # the residual is added AFTER the mask
        self._ref = acc
        return acc

    def launch(self, mode):
        c = self.c
        if mode not in self.pk:
            self.pk[mode] = _packed(self.w, mode)
        out = torch.full((SLACK + c.B * c.obs + BACK,), NAN, device=DEV)
        assert ptr(out, SLACK) % 16 == 0
        rp, rbs, rpitch = None, 0, 0
        if c.resid == "own":
            rp, rbs, rpitch = ptr(self.resd, SLACK), 16 * c.mt * c.pitch, c.pitch
        elif c.resid == "alias":
            self.window(out).copy_(self.old.to(DEV))
            rp, rbs, rpitch = ptr(out, SLACK), c.obs, c.opitch
        call("wn_chan_gemm", ptr(self.x0d, SLACK), ptr(self.x1d, SLACK) if c.ks1 > 0 else None, self.RI * c.pitch, c.pitch, c.in_lo, c.in_hi,
             c.s0, c.s1, c.ks0, c.ks1, ptr(self.pk[mode]), c.mt, c.m_valid, ptr(out, SLACK), c.obs, c.opitch, c.oshift,
             ptr(self.biasd) if c.bias else None, rp, rbs, rpitch, c.resid_lo,
             ptr(self.mskd, SLACK) if c.mask else None, 16 * c.mt * c.pitch if c.mask else 0, c.pitch if c.mask else 0,
             c.t_lo, c.t_hi, 1 if c.relu else 0, c.B, mode, _lib.stream())
        torch.cuda.synchronize()
        return out

    def check(self, out, mode, kernel):
        c = self.c
        ref = self.reference()
        got = self.window(out).cpu().double()
        err = (got - ref).abs().max().item() / ref.abs().max().item()          # NaN (fails every <=) when a NaN leaked in
        print("OBS %s-%s %.2e   [%s]" % (kernel, MODE_ID[mode], err, c.id))
        assert _written(out) == ref.numel(), c.id + ": written outside rows < m_valid x [t_lo, t_hi) (or NaN inside)"
        assert err <= TOL[mode], (c.id, MODE_ID[mode], err)
        return err

    def run(self, mode, kernel):
        """launch, check against float64, launch again: same bits"""
        out = self.launch(mode)
        self.check(out, mode, kernel)
        assert _same_bits(out, self.launch(mode)), self.c.id + ": a second launch does not reproduce the bits"
        return out


_last = [None, None]


def _gemm(c):
    """the buffers and the reference of the case, kept while the same case runs in its next mode"""
    if _last[0] is not c:
        _last[0], _last[1] = c, None                # (drop the old buffers first)
        _last[1] = _Gemm(c)
    return _last[1]


def _table(cases):
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return [pytest.param(c, m, id="%s-%s" % (c.id, MODE_ID[m])) for c in cases for m in c.modes]


def _run_case(c, mode, monkeypatch):
    monkeypatch.delenv("WN_GEMM_BST", raising=False)
    assert _route(c, mode).kernel == c.kernel
    _gemm(c).run(mode, c.kernel)


def _covered(cases):
    for c in cases:
        for m in c.modes:
            r = _route(c, m)
            assert r.kernel == c.kernel, (c.id, MODE_ID[m], r.kernel)
            assert c.why(r), (c.id, MODE_ID[m], "does not reach the regime its id names")


def _as_x3(c, **over):
    """the route of the same call in f16x3 with some arguments changed: what a fallback case falls back FROM"""
    d = SimpleNamespace(**vars(c))
    for k, v in over.items():
        setattr(d, k, v)
    return _route(d, MF).kernel


# ================================================================================================ A. chan_gemm_k<.., 4, 1> ("narrow")
NARROW = [
    C("mt1", "narrow", lambda r: r.c.mt < 4 and r.c.m_valid < 16, 1, 2, 37, 400, m_valid=13, bias=True, modes=ALL),
    C("mt2_ks1", "narrow", lambda r: r.c.mt < 4 and r.KS == 1, 2, 1, 37, 400),
    C("mt3_ks3_mask", "narrow", lambda r: r.c.mt < 4 and r.KS % 2 == 1 and r.KS > 1, 3, 3, 37, 400, mask=True, m_valid=41),
    C("taps_2_1", "narrow", lambda r: r.c.mt == 4 and r.c.ks1 > 0 and not r.weave, 4, 2, 37, 400, ks1=1, s0=-3, modes=ALL),
    C("taps_1_2_relu", "narrow", lambda r: r.c.ks1 > r.c.ks0 and not r.weave, 4, 1, 37, 400, ks1=2, s1=4, relu=True),
    C("late_resid", "narrow", lambda r: r.c.resid and not r.early and r.weave, 2, 2, 37, 400, ks1=2, s1=3, resid="own", resid_lo=46,
      mask=True, m_valid=30),
    C("early_resid", "narrow", lambda r: r.c.resid and r.early, 3, 2, 37, 400, ks1=2, s0=-2, resid="own", resid_lo=46, bias=True),
    C("rw_shaped_x1", "narrow", lambda r: _as_x3(r.c) == "rw", 4, 4, 37, 400, ks1=4, s1=5, resid="own", resid_lo=42, modes=X1),
    C("rw_shaped_relu", "narrow", lambda r: _as_x3(r.c, relu=False) == "rw", 4, 8, 37, 400, relu=True),
    C("rw_shaped_out_shift", "narrow", lambda r: _as_x3(r.c, oshift=0) == "rw", 4, 4, 37, 400, ks1=4, s1=5, out="compact"),
    C("clip_below_a_wave", "narrow", lambda r: r.ncol < 64 and r.c.t_lo > r.t_base, 4, 3, 70, 97, bias=True),
    C("clip_three_workgroups", "narrow", lambda r: r.gx == 3, 4, 3, 37, 1400, B=1),
    C("causal_conv_user_input", "narrow", lambda r: r.KS == 16 and r.c.pitch % 4 != 0 and r.c.in_lo == 0, 4, 8, 1, 301, ks1=8, s0=-1,
      in_hi=301, ipitch=301, bias=True, m_valid=50, modes=ALL),
    C("alias", "narrow", lambda r: r.c.resid == "alias" and r.early, 3, 2, 37, 400, ks1=2, s1=2, resid="alias", resid_lo=42, modes=ALL),
    C("alias_mask", "narrow", lambda r: r.c.resid == "alias" and not r.early, 3, 3, 37, 400, resid="alias", resid_lo=42, mask=True),
    C("window_empty", "narrow", lambda r: r.c.in_hi == r.c.in_lo, 2, 2, 37, 400, in_lo=100, in_hi=100, bias=True),
    C("window_one_column", "narrow", lambda r: r.c.in_hi - r.c.in_lo == 1 and _as_x3(r.c, in_hi=r.c.in_lo + 2) == "rw", 4, 8, 37, 400,
      in_lo=101, in_hi=102),
]


@pytest.mark.parametrize("c,mode", _table(NARROW))
def test_narrow(c, mode, monkeypatch):
    _run_case(c, mode, monkeypatch)


def test_narrow_cases_cover_their_regimes():
    _covered(NARROW)
    ids = {c.id for c in NARROW}
    assert {"mt1", "mt2_ks1", "mt3_ks3_mask", "taps_2_1", "late_resid", "early_resid", "rw_shaped_x1", "clip_below_a_wave",
            "clip_three_workgroups", "alias", "window_empty", "window_one_column"} <= ids


# ================================================================================================ B. chan_gemm_wide2_k
WIDE2 = [
    C("two_taps_user_output", "wide2", lambda r: r.c.ks1 > 0 and r.c.opitch % 4 != 0 and r.c.t_lo == 0, 16, 2, 0, 1237, ks1=2, s1=1,
      in_lo=1, in_hi=1237, out="user", modes=ALL),
    C("mt20_ks2", "wide2", lambda r: r.c.mt % 16 != 0 and r.gy == 2 and r.c.mt % 16 <= 8 and r.KS == 2, 20, 2, 37, 600, m_valid=313,
      modes=ALL),
    C("ks1", "wide2", lambda r: r.KS == 1, 5, 1, 37, 600),
    C("ks3", "wide2", lambda r: r.KS == 3 and r.c.ks1 == 0, 6, 3, 37, 600),
    C("taps_2_1", "wide2", lambda r: r.KS == 3 and r.c.ks1 == 1, 5, 2, 37, 600, ks1=1, s0=-5),
    C("guarded_loader_groups", "wide2", lambda r: r.inner[0] == {True, False} and r.guarded_live[0], 5, 2, 0, 1024, in_lo=100, in_hi=900),
    C("epilogue_all", "wide2", lambda r: r.c.resid and r.c.mask and r.c.relu and r.c.oshift != 0 and r.c.m_valid % 16 != 0, 7, 3, 37, 600,
      resid="own", resid_lo=50, mask=True, relu=True, bias=True, out="compact", m_valid=103, in_lo=40, in_hi=590, modes=ALL),
    C("resid_only", "wide2", lambda r: r.c.resid and not r.c.mask, 5, 2, 37, 600, resid="own", resid_lo=45),
    C("mask_only_odd_output", "wide2", lambda r: r.c.mask and not r.c.resid and r.c.opitch % 2 == 1 and r.c.oshift % 2 == 1, 5, 2, 37,
      600, mask=True, out="odd"),
    C("alias", "wide2", lambda r: r.c.resid == "alias", 8, 2, 37, 600, ks1=2, s1=3, resid="alias", resid_lo=44, modes=ALL),
    C("alias_mask", "wide2", lambda r: r.c.resid == "alias" and r.c.mask, 5, 2, 37, 600, resid="alias", resid_lo=44, mask=True),
    C("window_empty", "wide2", lambda r: r.c.in_hi == r.c.in_lo, 5, 2, 37, 600, in_lo=100, in_hi=100, bias=True),
    C("window_one_column", "wide2", lambda r: r.c.in_hi - r.c.in_lo == 1, 5, 2, 37, 600, in_lo=101, in_hi=102),
    C("bst_shaped_x1", "wide2", lambda r: _as_x3(r.c) == "bst", 33, 8, 37, 600, modes=X1),
    C("bst_shaped_resid", "wide2", lambda r: _as_x3(r.c, resid=None) == "bst", 33, 8, 37, 600, resid="own"),
]


@pytest.mark.parametrize("c,mode", _table(WIDE2))
def test_wide2(c, mode, monkeypatch):
    _run_case(c, mode, monkeypatch)


def test_wide2_cases_cover_their_regimes():
    _covered(WIDE2)
    assert {r.KS for r in (_route(c, c.modes[0]) for c in WIDE2)} >= {1, 2, 3}


# ================================================================================================ C. chan_gemm_rw_k
def _parity(r, tap):
    sh = (r.c.s0, r.c.s1)[tap]
    return ((r.c.in_lo + sh) & 1, (r.c.in_hi + sh) & 1)


RW = [
    C("one_tap_ks8_dense_conv", "rw", lambda r: r.c.ks0 == 8 and r.c.ks1 == 0 and r.c.resid and r.c.m_valid < 64 and r.n_items == {1}, 4, 8,
      37, 700, m_valid=48, resid="own", bias=True),
    C("ks4_two_taps_mask", "rw", lambda r: r.KS == 4 and r.c.ks1 == 2 and r.c.mask, 4, 2, 37, 700, ks1=2, s1=6, resid="own", resid_lo=50,
      mask=True),
    C("ks4_one_tap_bias", "rw", lambda r: r.KS == 4 and r.c.ks1 == 0 and r.c.bias and not r.c.resid and not r.c.mask, 4, 4, 37, 700,
      bias=True, m_valid=61),
    C("causal_q64_user_input", "rw", lambda r: r.KS == 4 and 32 * r.c.ks0 == 64 and not r.c.resid and not r.c.mask and r.c.pitch % 4, 4, 2,
      1, 777, ks1=2, s0=-1, in_hi=777, ipitch=777, bias=True),
    C("two_items_per_wg", "rw", lambda r: r.ipw == 2 and r.total > 512 and 2 in r.n_items, 4, 4, 0, 5600, B=3, resid="own"),
    C("three_items_per_wg", "rw", lambda r: r.ipw == 3 and 3 in r.n_items, 4, 2, 0, 10990, ks1=2, s1=1, B=3, in_lo=0, in_hi=10990),
    C("fewer_than_8_wgs", "rw", lambda r: r.nwg < 8, 4, 8, 37, 200, B=1, resid="own"),
    C("wgs_not_a_multiple_of_8", "rw", lambda r: r.nwg > 8 and r.nwg % 8 != 0, 4, 4, 70, 390, ks1=4, s1=2, B=3),
    C("alias", "rw", lambda r: r.c.resid == "alias" and r.c.resid_lo % 2 == 1, 4, 4, 36, 700, ks1=4, s1=5, resid="alias", resid_lo=43),
    C("alias_mask", "rw", lambda r: r.c.resid == "alias" and r.c.mask, 4, 2, 37, 700, ks1=2, s1=3, resid="alias", resid_lo=44, mask=True),
    C("window_two_columns", "rw", lambda r: r.c.in_hi - r.c.in_lo == 2, 4, 8, 37, 700, in_lo=101, in_hi=103),
]
# a window edge of either parity under either tap: shift0 even, shift1 odd, the four parities of (in_lo, in_hi); both edges cut items
RW_PARITY = [C("parity_%d%d" % (a, b), "rw", lambda r: all(lo and hi for lo, hi in r.edge), 4, 4, 100, 900, ks1=4, s1=5, in_lo=104 + a,
               in_hi=880 + b, resid="own", resid_lo=111, seed=a * 2 + b) for a in (0, 1) for b in (0, 1)]


@pytest.mark.parametrize("c,mode", _table(RW + RW_PARITY))
def test_rw(c, mode, monkeypatch):
    _run_case(c, mode, monkeypatch)


def test_rw_cases_cover_their_regimes():
    _covered(RW + RW_PARITY)
    for tap in (0, 1):
        assert {_parity(_route(c, MF), tap) for c in RW_PARITY} == {(0, 0), (0, 1), (1, 0), (1, 1)}, tap
    n = set()
    for c in RW:
        n |= _route(c, MF).n_items
    assert {1, 2, 3} <= n                       # one, an even and an odd count above one: the padded last prefetch


# ================================================================================================ D. chan_gemm_bst_k
def _bst_case(mt, lay, fancy):
    kw = dict(mask=True, bias=True, relu=True, in_lo=140, in_hi=820) if fancy else {}
    return C("mt%d_%s%s" % (mt, lay, "_fancy" if fancy else ""), "bst", None, mt, 8, 132, 832, m_valid=16 * mt - 21, out=lay, **kw)


BST = [_bst_case(mt, lay, fancy) for mt, lay, fancy in
       ((33, "compact", 0), (33, "odd", 0), (36, "compact", 0), (36, "odd", 0), (36, "compact", 1), (51, "compact", 0), (51, "odd", 0))]
# an input window that is empty (the whole input NaN: the output is the bias) or one column wide
BST += [C("mt33_window_empty", "bst", None, 33, 8, 132, 832, in_lo=300, in_hi=300, bias=True, m_valid=507, out="compact"),
        C("mt33_window_one_column", "bst", None, 33, 8, 132, 832, in_lo=301, in_hi=302, m_valid=507, out="compact")]


@pytest.mark.parametrize("c,mode", _table(BST))
def test_bst(c, mode, monkeypatch):
    """WN_GEMM_BST unset (the production default: one workgroup per tile), 1 (one per compute unit) and 0 (chan_gemm_wide2_k): against
    float64, and the same bits from all three - the launcher promises the same order of terms"""
    g = _gemm(c)
    monkeypatch.delenv("WN_GEMM_BST", raising=False)
    assert _route(c, mode).kernel == "bst"
    out = g.run(mode, "bst")
    monkeypatch.setenv("WN_GEMM_BST", "1")
    assert _route(c, mode, "1").kernel == "bst"
    assert _same_bits(out, g.launch(mode)), c.id + ": WN_GEMM_BST=1 gives other bits than the default"
    monkeypatch.setenv("WN_GEMM_BST", "0")
    assert _route(c, mode, "0").kernel == "wide2"
    assert _same_bits(out, g.launch(mode)), c.id + ": chan_gemm_wide2_k (WN_GEMM_BST=0) gives other bits than chan_gemm_bst_k"


def _bst_big():
    """WN_GEMM_BST=1 with more tiles than compute units: whole tiles round-robin, then the leftover tiles dealt out by passes, some
    workgroups taking one (tile, pass) unit and some two.  The tile count follows the device: between 1 and 2 times its compute units"""
    cus = _cus()
    ntx = _ceil(cus + cus // 2 + cus // 8 + 1, 3)
    if (3 * ntx) % cus == 0:
        ntx += 1
    return C("persistent_leftover", "bst", None, 33, 8, 132, 128 + 128 * ntx - 40, B=3, m_valid=507, out="compact")


_big = []


@pytest.mark.parametrize("mode", X3, ids=[MODE_ID[m] for m in X3])
def test_bst_whole_tiles_plus_leftover(mode, monkeypatch):
    if not _big:
        _big.append(_bst_big())
    c = _big[0]
    r = _route(c, mode, "1")
    assert r.kernel == "bst" and r.grid == _cus() and r.nfull == 1 and 0 < r.left < r.grid and r.ntiles % r.grid != 0
    assert r.npass == 2 and r.grid < r.units < 2 * r.grid            # workgroups with one and with two leftover units
    g = _gemm(c)
    monkeypatch.setenv("WN_GEMM_BST", "1")
    out = g.launch(mode)
    g.check(out, mode, "bst")
    assert _same_bits(out, g.launch(mode)), "a second launch does not reproduce the bits"
    monkeypatch.delenv("WN_GEMM_BST")
    assert _same_bits(out, g.launch(mode)), "one workgroup per tile gives other bits than the persistent walk"


def test_bst_cases_cover_their_regimes():
    assert {c.mt for c in BST} == {33, 36, 51}
    for c in BST:
        for env in (None, "1"):
            r = _route(c, MF, env)
            assert r.kernel == "bst" and r.interior and r.ntiles <= _cus(), c.id
            assert r.nt_ok == (c.out == "compact"), c.id                      # streaming against plain stores
            assert (c.m_valid - 1) // 48 == (16 * c.mt - 1) // 48 and c.m_valid % 48 not in (0, 47), c.id     # m_valid cuts the last group of 3 tiles
        assert _route(c, MF, "0").kernel == "wide2"
    by_mt = {c.mt: _route(c, MF) for c in BST}
    assert by_mt[33].npass == 2 and (33 // 3) % 8 != 0                       # mt = 33: the last pass partly filled
    assert by_mt[51].npass == 3 and (51 // 3) % 8 == 1                       # mt = 51: three passes, one group in the last
    assert any(c.mask for c in BST) and {0, 1} <= {c.in_hi - c.in_lo for c in BST}


# ================================================================================================ E. the order of a pack's fragments
def _exact_w(M, K):
    """small integers, exact in bf16 (|v| <= 254), that differ between neighbouring rows and columns"""
    m, k = np.indices((M, K))
    return ((m * 37 + k * 11) % 509 - 254).astype(np.float32)


EXACT = [("narrow", 3, 3, ALL), ("wide2", 18, 3, ALL), ("rw", 4, 8, X3), ("rw", 4, 4, X3), ("bst", 33, 8, X3)]


@pytest.mark.parametrize("kernel,mt,ks0,mode", [pytest.param(k, mt, ks, m, id="%s-ks%d-%s" % (k, ks, MODE_ID[m]))
                                                for k, mt, ks, modes in EXACT for m in modes])
def test_pack_order_exact(kernel, mt, ks0, mode, monkeypatch):
    """in[k][t] = (t mod K == k), W small integers: out[m][t] must be W[m][t mod K] bit for bit - one term per sum, every product exact
    in all four modes.  A permuted fragment (rows, k-steps, lanes, the hi / lo blocks) cannot hide inside a tolerance here."""
    monkeypatch.delenv("WN_GEMM_BST", raising=False)
    M, K, B, t_lo, t_hi = 16 * mt, 32 * ks0, 2, 37, 37 + 3 * 32 * ks0 + 5
    c = C("exact", kernel, None, mt, ks0, t_lo, t_hi, B=B)
    assert _route(c, mode).kernel == kernel
    w = _exact_w(M, K)
    pk = _packed(w, mode)
    p = c.pitch
    x = torch.full((SLACK + B * K * p + BACK,), NAN)
    v = x[SLACK:SLACK + B * K * p].view(B, K, p)
    t = torch.arange(t_lo, t_hi)
    v[:, :, t_lo:t_hi] = (t[None, :] % K == torch.arange(K)[:, None]).float()[None]
    xd = x.to(DEV)
    out = _nanbuf(B, M, p)
    call("wn_chan_gemm", ptr(xd, SLACK), None, K * p, p, t_lo, t_hi, 0, 0, ks0, 0, ptr(pk), mt, M, ptr(out, SLACK), M * p, p, 0, None,
         None, 0, 0, 0, None, 0, 0, t_lo, t_hi, 0, B, mode, _lib.stream())
    torch.cuda.synchronize()
    want = torch.from_numpy(w)[:, t % K][None].expand(B, M, len(t)).contiguous()
    got = _view(out, B, M, p)[:, :, t_lo:t_hi].cpu().contiguous()
    assert _same_bits(got, want), "%s %s: %d elements are not W[m][t mod K]" % (kernel, MODE_ID[mode], int((got != want).sum()))
    assert _written(out) == want.numel()


# ================================================================================================ F. wn_pack_weights
def _pack_values(bf16, n, rng):
    """normals, exact ties of the 16-bit rounding (to even: down and up), +-0, magnitudes in f16's subnormal range, large ones"""
    ulp = 2.0 ** -8 if bf16 else 2.0 ** -11                     # half a 16-bit ulp at 1.0
    ties = [1 + ulp, 1 + 3 * ulp, -(1 + ulp), -(1 + 3 * ulp), 2 + 2 * ulp, 0.5 + 2.5 * ulp]
    special = ties + [0.0, -0.0, 6e-8, -6e-8, 3e-8, 2.5e-7, -7.1e-6, 6.0e-5, 6.1e-5, 1.0, -1.0, 1 / 3, 1e-3]
    special += [3.0e38, -1.7e38, 1e30, 65504.0, 65520.0, 1e5] if bf16 else [6e4, -6e4, 59999.0, 4097.0, 2049.0]
    v = rng.standard_normal(n).astype(np.float32)
    v[n // 4:n // 2] *= np.float32(1e-6)                        # f16 subnormals (and their lo pieces)
    v[n // 2:3 * n // 4] *= np.float32(1e30 if bf16 else 1.5e4)
    if not bf16:
        v = np.clip(v, -6e4, 6e4)
    pos = rng.permutation(n)[:len(special)]
    v[pos] = np.array(special, np.float32)
    return v


@pytest.mark.parametrize("chained", [False, True], ids=["natural", "chained"])
@pytest.mark.parametrize("mode", ALL, ids=[MODE_ID[m] for m in ALL])
def test_pack_weights_bits(mode, chained):
    """out[frag][hi: 512 | lo: 512 (x3 only)] = rne16(v), rne16(float32(v) - float32(hi)) in pack_index's order, idx -1 -> +0, nothing
    written beyond the last fragment: bit for bit against torch on the CPU"""
    bf16, x3 = mode in (MB, M1B), mode in X3
    M, K = 48, 32                                               # 3 fragments: an odd count
    rng = np.random.default_rng(5 + mode)
    flat = _pack_values(bf16, M * K + 100, rng)
    weff = rng.permutation(M * K + 100)[:M * K].reshape(M, K).astype(np.int64)
    weff[rng.random((M, K)) < 0.1] = -1                         # structural zeros
    weff[17, :] = -1
    idx = pack_index(weff, chained)
    n, hp = idx.size, 1024 if x3 else 512
    assert n == 3 * 512
    sent = 0x7B7B
    out = torch.full((3 * hp + 2048,), sent, dtype=torch.int16, device=DEV)
    fd, idd = torch.from_numpy(flat).to(DEV), torch.from_numpy(idx).to(DEV)
    call("wn_pack_weights", ptr(fd), ptr(idd), ptr(out), n, mode, _lib.stream())
    torch.cuda.synchronize()
    dt = torch.bfloat16 if bf16 else torch.float16
    it = torch.from_numpy(idx.astype(np.int64))
    v = torch.where(it >= 0, torch.from_numpy(flat)[it.clamp(min=0)], torch.zeros(()))
    hi = v.to(dt)
    lo = (v - hi.float()).to(dt)
    assert torch.isfinite(hi.float()).all()
    want = torch.full((3 * hp + 2048,), sent, dtype=torch.int16)
    wv = want[:3 * hp].view(3, hp)
    wv[:, :512] = hi.view(torch.int16).view(3, 512)
    if x3:
        wv[:, 512:] = lo.view(torch.int16).view(3, 512)
    got = out.cpu()
    bad = int((got != want).sum())
    assert bad == 0, "%d halfs differ (first at %d)" % (bad, int((got != want).nonzero()[0]))
    assert (got[:3 * hp].view(3, hp)[:, :512].reshape(-1)[it < 0] == 0).all()        # -1 is +0, not -0


def test_pack_weights_empty_and_refusals():
    lib = _lib.load()
    out = torch.full((2048,), 0x7B7B, dtype=torch.int16, device=DEV)
    flat = torch.ones(16, device=DEV)
    idx = torch.zeros(512, dtype=torch.int32, device=DEV)
    assert lib.wn_pack_weights(ptr(flat), ptr(idx), ptr(out), 0, MF, _lib.stream()) == 0
    assert lib.wn_pack_weights(None, None, None, 0, MB, _lib.stream()) == 0
    assert lib.wn_pack_weights(ptr(flat), ptr(idx), ptr(out), 100, MF, _lib.stream()) == -4          # n is not a multiple of 512
    assert lib.wn_pack_weights(ptr(flat), None, ptr(out), 512, MF, _lib.stream()) == -4
    torch.cuda.synchronize()
    assert (out == 0x7B7B).all()


# ================================================================================================ G. refusals and empty calls
def test_refusals_and_empty_calls():
    lib = _lib.load()
    B, mt, ks, p, t_lo, t_hi = 2, 2, 2, 512, 37, 300
    x = _buf(B, 32 * ks, p, 1.0, 1)
    pk = _packed(np.ones((16 * mt, 64), np.float32), MF)
    out = _nanbuf(B, 16 * mt, p)

    def gemm(in0=ptr(x, SLACK), in1=None, ks0=ks, ks1=0, wpack=ptr(pk), mt_=mt, o=ptr(out, SLACK), lo=t_lo, hi=t_hi, batch=B, mode=MF):
        return lib.wn_chan_gemm(in0, in1, 32 * ks * p, p, lo, hi, 0, 0, ks0, ks1, wpack, mt_, 16 * mt, o, 16 * mt * p, p, 0, None,
                                None, 0, 0, 0, None, 0, 0, lo, hi, 0, batch, mode, _lib.stream())

    assert gemm(ks0=0) == -4 and gemm(ks0=-1) == -4
    assert gemm(ks1=2, in1=None) == -4
    assert gemm(mt_=0) == -4 and gemm(mt_=-3) == -4
    assert gemm(in0=None) == -4 and gemm(wpack=None) == -4 and gemm(o=None) == -4
    assert b"must not be NULL" in lib.wn_last_error()
    assert gemm(mode=7) == -2 and gemm(mode=-1) == -2
    # nothing to do: 0 with NULL pointers, and nothing written with real ones
    for kw in (dict(hi=t_lo), dict(hi=t_lo - 5), dict(batch=0)):
        assert gemm(in0=None, wpack=None, o=None, **kw) == 0, kw
        assert gemm(**kw) == 0, kw
    torch.cuda.synchronize()
    assert _written(out) == 0, "a refused or an empty call wrote to `out`"
    assert gemm() == 0                                                                     # and the same arguments, whole, do run
    torch.cuda.synchronize()
    assert _written(out) == B * 16 * mt * (t_hi - t_lo)
