"""GPU tests of the forward block and of the two fused epilogues, one launch at a time, against float64 (run with -m gpu).

The rules of tests/test_gpu_block_kernels.py, for wn_resblock_fwd, wn_skip_epilogue_fwd and wn_skip_epilogue_bwd:
  - every test fills its device buffers itself and launches ONE entry point through _lib.call;
  - the reference is float64 on the CPU, computed with the formulas of include/wavenet_hip.h from the very float32 inputs the
    kernel read;
  - every output buffer is pre-filled with NaN, slack included; after the launch every element of the valid rows and the valid
    window takes part in the comparison and everything else is still NaN (counted: `_written`).  No element is excused: the gate
    and the forward ReLUs are continuous, the backward masks come from the given h / u and are exact;
  - inputs hold NaN wherever their values do not count: z, h, u outside [t_lo, t_hi) inside their rows; x_in outside
    [t_lo - d, t_hi), slack included (padded channel rows of x_in are zero by contract); bias entries beyond n_f / n_d / s_valid /
    q_valid; conditioning tables beyond cond_le;
  - every case is launched twice into fresh NaN buffers: same bits;
  - one test per section asserts, from the launchers' own host formulas and the compute-unit count of the device the tests run
    on, that every case reaches the regime its id names.

Bars (the project's own, not what these kernels turn out to do):
  block:     1e-5 (f16x3) / 2e-4 (bf16x3) of max(1, max|y|) for x_out, absolute for z - the bars of test_resblock_fwd;
  epilogues: 3 * TOL[mode] of the reference tensor's max-abs (3e-5 / 3e-4), against float64 and against the three wn_chan_gemm
             launches - the bars of test_skip_epilogue_fwd_fused / _bwd_fused;
  BARFORM = 2e-5 of max-abs between two forms of the same sums; bit equality where the launcher promises the same sums in the
  same order (a repeated launch, a fallback, WN_EPI_STAGGER=0, WN_EPI_BWD_SPLIT=0, WN_EPI_BWD_NT=1)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from music_amd.engine import SLACK, pack_positions
from tests.test_gpu_kernels import _packed, _buf, _view, _fg_pack, _res_ref, TOL
from tests.test_gpu_block_kernels import _nanbuf, _rel, _same_bits, _diag, _buckets, _written, _all_zero

DEV = "cuda"
MF, MB = _lib.F16X3, _lib.BF16X3
MODE_ID = {MF: "f16x3", MB: "bf16x3"}
NAN = float("nan")
BARFORM = 2e-5
BLOCK_BAR = {MF: 1e-5, MB: 2e-4}
BLOCK_COLS = 512                 # columns of one workgroup of resblock_fwd_nt_k (8 waves x 64)
EPI_COLS = 128                   # columns of one tile of both epilogues


def _cus():
    """compute units of the device the tests run on (wn_num_cus() reads the same number)"""
    return torch.cuda.get_device_properties(0).multi_processor_count


def _refused(code=-4):
    return pytest.raises(_lib.WavenetHipError, match=r"\(%d\)" % code)


def _nan_around(buf, b, rows, pitch, lo, hi):
    """NaN in the slack and in every column outside [lo, hi) of the rows of `buf`"""
    buf[:SLACK] = NAN
    buf[SLACK + b * rows * pitch:] = NAN
    v = _view(buf, b, rows, pitch)
    v[:, :, :max(lo, 0)] = NAN
    v[:, :, hi:] = NAN


# ================================================================================================ A. wn_resblock_fwd
def _block_grid(t_lo, t_hi, nb):
    """workgroups of a wn_resblock_fwd launch (launch_fwd_nt: 512-column tiles from t_lo & ~63, times the clips)"""
    return ((t_hi - (t_lo & ~63) + BLOCK_COLS - 1) // BLOCK_COLS) * nb


def _cond_on_mfma(chl, mode, le, pack):
    """launch_fwd_nt's rule for the CND instantiation (the conditioning bias as one more k-step)"""
    return bool(pack) and chl == 64 and mode == MF and le <= 32


class _Fwd:
    """One gated residual block's forward: inputs, the wn_resblock_fwd launch and the float64 reference of include/wavenet_hip.h
    ([f; g] = Wfg [x(t-d); x(t)] (+ bias) (+ table column bucket(t)); z = tanh f * sigmoid g; y = Wd z (+ bias) + x(t)).
    cond = (le, rule): rule 'stretch' / 'tile' through _buckets, or 'rot' - bytes only the pack form can take (the tile rule
    rotated by one bucket per period).  pairs: the B clips are those of a 32-channel model, two side by side per launch item
    (z_half_stride != 0, block-diagonal packs, table rows [f: A B | g: A B]); the reference stays B single clips."""

    def __init__(self, ch, R, D, d, t_lo, t_hi, z_lo=None, B=3, mode=MF, bias=False, cond=None, write_x=1, pairs=False, seed=0):
        assert t_lo >= d + 1 and t_hi > t_lo and (not pairs or (ch == 32 and B % 2 == 0))
        self.C = C = ch                                          # rows of one clip's x / x_out
        self.chl = chl = 64 if pairs else ch                     # `ch` of the launch
        self.nb = B // 2 if pairs else B                         # `batch` of the launch
        self.ZR = ZR = 64 if pairs else ch                       # rows of one clip's z slice (pairs: 32 more than the kernel writes)
        self.B, self.R, self.D, self.d, self.t_lo, self.t_hi, self.mode, self.write_x, self.pairs = B, R, D, d, t_lo, t_hi, mode, write_x, pairs
        self.z_lo = z_lo = t_lo if z_lo is None else z_lo
        assert t_lo <= z_lo < t_hi
        self.pitch = pitch = ((t_hi + 255) // 256) * 256 + 256
        rng = np.random.default_rng(seed)
        self.wf = (rng.standard_normal((D, R, 2)) * 0.3).astype(np.float32)
        self.wg = (rng.standard_normal((D, R, 2)) * 0.3).astype(np.float32)
        self.wd = (rng.standard_normal((R, D, 1)) * 0.3).astype(np.float32)
        self.pfg, wfg = _fg_pack(self.wf, self.wg, C, mode)
        wdp = np.zeros((C, C), np.float32)
        wdp[:R, :D] = self.wd[:, :, 0]
        if pairs:
            self.pfg = _packed(_diag(wfg, 2, 2), mode)
            wdp = _diag(wdp, 1, 1)
        self.pd = _packed(wdp, mode, chained=True)
        self.x = _buf(B, C, pitch, 1.0, 100 + seed)
        _nan_around(self.x, B, C, pitch, t_lo - d, t_hi)
        _view(self.x, B, C, pitch)[:, R:] = 0                    # padded channels are zero by contract
        self.bias, self.n_f, self.n_d = None, D, R
        if bias:
            self.bias_v = [rng.standard_normal(n).astype(np.float32) for n in (D, D, R)]
            self.bias = []
            for v in self.bias_v:
                if pairs:                                        # rows [A: 32 | B: 32], the model's one bias for both clips
                    b_ = torch.zeros(64)
                    b_[:len(v)] = b_[32:32 + len(v)] = torch.from_numpy(v)
                else:                                            # entries beyond n_f / n_d do not count
                    b_ = torch.full((ch,), NAN)
                    b_[:len(v)] = torch.from_numpy(v)
                self.bias.append(b_.to(DEV))
            if pairs:
                self.n_f = self.n_d = 64
        self.cond = None
        if cond is not None:
            le, rule = cond
            L = t_hi - t_lo
            if rule == "rot":
                tr = np.arange(L)
                idx, cmode, q = (tr + tr // le) % le, 2, 1
            else:
                idx, cmode, q = _buckets(L, le, rule)
            cp = le + 3                                          # cond_pitch > le, NaN beyond le
            g_ = torch.Generator().manual_seed(500 + seed)
            # columns pairwise far apart: column j of a row is (j - mid) * step up or down (+ noise of a fifth of a step)
            self.step = step = 0.25 if le <= 32 else 0.05
            ramp = (torch.arange(le, dtype=torch.float32) - (le - 1) / 2) * step
            tab = torch.full((B, 2 * C, cp), NAN)
            tab[:, :, :le] = 0
            for r0 in (0, C):
                sgn = torch.randint(0, 2, (B, D, 1), generator=g_).float() * 2 - 1
                tab[:, r0:r0 + D, :le] = sgn * ramp + 0.2 * step * torch.randn(B, D, le, generator=g_)
            self.tab_clip = tab                                  # [B][f rows | g rows][cp], what the reference adds
            if pairs:
                tab = tab.view(self.nb, 2, 2, C, cp).permute(0, 2, 1, 3, 4).reshape(self.nb, 4 * C, cp)
            self.tab = tab.contiguous().to(DEV)
            self.cond = dict(le=le, rule=rule, mode=cmode, q=q, cp=cp, idx=idx, idx_t=torch.from_numpy(idx).long())
            cidx = torch.zeros(_lib.COND_IDX_PAD + L + 64, dtype=torch.uint8)
            cidx[_lib.COND_IDX_PAD:_lib.COND_IDX_PAD + L] = torch.from_numpy(idx.astype(np.uint8))
            self.cidx = cidx.to(DEV)
            self.cpk = None
            if chl == 64:
                # the table once more as packed A fragments, [2ch rows][K = 32 buckets, zero beyond le] per clip (music_amd/model1.py)
                row, k = pack_positions(2 * chl // 16, 1, False)
                one = np.where(k < le, row * cp + k, -1).astype(np.int64)
                base = np.arange(self.nb, dtype=np.int64)[:, None] * (2 * chl * cp)
                pidx = torch.from_numpy(np.where(one[None, :] >= 0, base + one[None, :], -1).astype(np.int32).reshape(-1)).to(DEV)
                self.cpk = torch.zeros(pidx.numel() * 2, dtype=torch.int16, device=DEV)
                call("wn_pack_weights", ptr(self.tab), ptr(pidx), ptr(self.cpk), pidx.numel(), MF, _lib.stream())
                torch.cuda.synchronize()
        self._ref = None

    def grid(self):
        return _block_grid(self.t_lo, self.t_hi, self.nb)

    # -------- float64 reference: z and y on [t_lo, t_hi)
    def reference(self):
        if self._ref is not None:
            return self._ref
        B, C, R, D, d, t_lo, t_hi = self.B, self.C, self.R, self.D, self.d, self.t_lo, self.t_hi
        x = _view(self.x, B, C, self.pitch).cpu()[:, :R, t_lo - d:t_hi].double()
        assert not torch.isnan(x).any()
        wf, wg, wd = (torch.from_numpy(a).double() for a in (self.wf, self.wg, self.wd))
        if self.bias is None and self.cond is None:
            _, _, z, y = _res_ref(x, wf, wg, wd, d)
        else:
            f = F.conv1d(x, wf, dilation=d)
            g = F.conv1d(x, wg, dilation=d)
            bd = None
            if self.bias is not None:
                f = f + torch.from_numpy(self.bias_v[0]).double()[None, :, None]
                g = g + torch.from_numpy(self.bias_v[1]).double()[None, :, None]
                bd = torch.from_numpy(self.bias_v[2]).double()
            if self.cond is not None:
                t64 = self.tab_clip.double()
                f = f + t64[:, :D][:, :, self.cond["idx_t"]]
                g = g + t64[:, C:C + D][:, :, self.cond["idx_t"]]
            z = torch.tanh(f) * torch.sigmoid(g)
            y = F.conv1d(z, wd, bd) + x[:, :, d:]
        self._ref = (z, y)
        return self._ref

    # -------- one launch into NaN-filled outputs
    def launch(self, pack=False, cond=True, batch=None, t_hi=None, pitch=None, t_lo=None, ch=None, z_half=None):
        B, C, chl, ZR = self.B, self.C, self.chl, self.ZR
        p = self.pitch
        xo, zo = _nanbuf(B, C, p), _nanbuf(B, ZR, p)
        c = self.cond if cond else None
        pk = c is not None and pack and self.cpk is not None
        two = 2 if self.pairs else 1
        zh = (ZR * p if self.pairs else 0) if z_half is None else z_half
        b_ = self.bias
        call("wn_resblock_fwd", ptr(self.x, SLACK), ptr(xo, SLACK), ptr(zo, SLACK), two * C * p, two * ZR * p, p if pitch is None else pitch,
             ptr(self.pfg), ptr(self.pd), ptr(b_[0]) if b_ else None, ptr(b_[1]) if b_ else None, ptr(b_[2]) if b_ else None,
             self.n_f, self.n_d, chl if ch is None else ch, self.d, self.t_lo if t_lo is None else t_lo, self.t_hi if t_hi is None else t_hi,
             self.z_lo, self.write_x, ptr(self.tab) if c else None, 2 * chl * c["cp"] if c else 0, c["cp"] if c else 0,
             c["mode"] if c else 0, c["le"] if c else 0, c["q"] if c else 0, ptr(self.cpk) if pk else None, 2 * chl * 32 * 2 if pk else 0,
             ptr(self.cidx) if pk else None, zh, self.nb if batch is None else batch, self.mode, _lib.stream())
        torch.cuda.synchronize()
        return xo, zo

    # -------- comparison with float64 and the write windows; returns (err x_out, err z)
    def check(self, xo, zo, tag):
        B, C, R, D, ZR, t_lo, t_hi, z_lo, p = self.B, self.C, self.R, self.D, self.ZR, self.t_lo, self.t_hi, self.z_lo, self.pitch
        z, y = self.reference()
        gz = _view(zo, B, ZR, p).cpu()
        ez = (gz[:, :D, z_lo:t_hi].double() - z[:, :, z_lo - t_lo:]).abs().max().item()
        # the kernel writes all C rows of a clip on the window (include/wavenet_hip.h): padded rows exactly 0, nothing else touched
        assert _all_zero(gz[:, D:C, z_lo:t_hi]), tag + ": padded rows of z are not exactly 0"
        assert _written(zo) == B * C * (t_hi - z_lo), tag + ": z written outside rows [0, ch) x [z_lo, t_hi) (or NaN inside)"
        ey = 0.0
        if self.write_x:
            gx = _view(xo, B, C, p).cpu()
            ey = (gx[:, :R, t_lo:t_hi].double() - y).abs().max().item() / max(1.0, y.abs().max().item())
            assert _all_zero(gx[:, R:, t_lo:t_hi]), tag + ": padded rows of x_out are not exactly 0"
            assert _written(xo) == B * C * (t_hi - t_lo), tag + ": x_out written outside [t_lo, t_hi) (or NaN inside)"
        else:
            assert _written(xo) == 0, tag + ": write_x = 0 touched x_out"
        print("OBS block-%s x_out %.2e z %.2e   [%s]" % (MODE_ID[self.mode], ey, ez, tag))
        bar = BLOCK_BAR[self.mode]
        assert ey <= bar and ez <= bar, (tag, ey, ez)
        return ey, ez

    def run(self, tag, pack=False):
        """launch, check against float64, launch again: same bits"""
        xo, zo = self.launch(pack)
        self.check(xo, zo, tag)
        xo2, zo2 = self.launch(pack)
        assert _same_bits(xo, xo2) and _same_bits(zo, zo2), tag + ": a second launch does not reproduce the bits"
        return xo, zo


def _form_dev(a, b, ref, sl):
    """max |a - b| over the slice, in units of the reference's max-abs (1 at least for x_out, as the block's bar)"""
    return (a[sl].double() - b[sl].double()).abs().max().item() / ref.abs().max().item()


VARIANTS = ("plain", "bias", "last", "cond_stretch", "cond_tile", "bias_cond_tile")
SHAPES = ((64, 64, 64), (64, 48, 40), (32, 32, 32), (32, 20, 24))
DILATIONS = (1, 3, 64, 512)


def _window_of(d):
    """t_lo = 33 (mod 64) above d; 301 columns (t_hi = 2 mod 4), or 100 columns under the dilation larger than the window"""
    t_lo = 64 * ((d + 3 + 63) // 64) + 33
    return t_lo, t_lo + (100 if d == 512 else 301)


def _variant_table():
    """every variant x every shape x both modes; the dilation cycles so that each variant meets each d at both ch"""
    out = []
    for iv, v in enumerate(VARIANTS):
        for ish, (ch, R, D) in enumerate(SHAPES):
            for im, mode in enumerate((MF, MB)):
                out.append((v, ch, R, D, DILATIONS[(iv + ish // 2 + 2 * (ish % 2) + im) % 4], mode))
    return out


VARIANT_TABLE = _variant_table()


def _variant_case(v, ch, R, D, d, mode):
    t_lo, t_hi = _window_of(d)
    cond = (7, "stretch") if "stretch" in v else (31, "tile") if "tile" in v else None
    return _Fwd(ch, R, D, d, t_lo, t_hi, z_lo=t_lo + 45, mode=mode, bias="bias" in v, cond=cond, write_x=0 if v == "last" else 1,
                seed=ch + R + d)


# Observed worst over every block test of this file (each case prints its own with -s): f16x3 x_out 3.0e-7, z 2.2e-6 (bar 1e-5);
# bf16x3 x_out 1.1e-5, z 7.1e-5 (bar 2e-4).  test_resblock_fwd's own note: 1.8e-6 / 8.3e-5
@pytest.mark.parametrize("v,ch,R,D,d,mode", VARIANT_TABLE, ids=["%s-ch%d-R%d-D%d-d%d-%s" % (v, ch, R, D, d, MODE_ID[m])
                                                                  for v, ch, R, D, d, m in VARIANT_TABLE])
def test_block_variants_and_shapes(v, ch, R, D, d, mode):
    """wn_resblock_fwd: no bias / all three biases with n_f = D, n_d = R / write_x = 0 / the gathered conditioning under both
    rules / biases and conditioning, at 64 and 32 padded channels with full and short real channel counts, d = 1, 3, 64 and 512
    (larger than the 100-column window), z_lo inside a lane's four columns: z and x_out against float64, padded rows exactly 0,
    nothing else written (write_x = 0: x_out untouched), a second launch reproduces the bits."""
    _variant_case(v, ch, R, D, d, mode).run("%s ch%d R%d D%d d%d" % (v, ch, R, D, d))


WIN_TLO = (128, 128 + 63, 128 + 37)
WIN_WIDTHS = (1, 3, 5, 63, 64, 65, 511, 512, 513)


def _window_table():
    out, seen = [], set()
    for it, t_lo in enumerate(WIN_TLO):
        for iw, w in enumerate(WIN_WIDTHS):
            for iz, zoff in enumerate((0, 1, w - 1)):
                z_lo = min(t_lo + zoff, t_lo + w - 1)
                if (t_lo, w, z_lo) in seen:
                    continue
                seen.add((t_lo, w, z_lo))
                n = it + iw + iz
                out.append((t_lo, w, z_lo, (1, 3, 64)[n % 3], bool((iw + iz) % 2), (MF, MB)[(it + iz) % 2]))
    return out


WINDOW_TABLE = _window_table()


@pytest.mark.parametrize("t_lo,w,z_lo,d,bias,mode", WINDOW_TABLE, ids=["tlo%d-w%d-zlo+%d-d%d-%s-%s" % (t, w, z - t, d, "bias" if b else "plain", MODE_ID[m])
                                                                      for t, w, z, d, b, m in WINDOW_TABLE])
def test_block_windows(t_lo, w, z_lo, d, bias, mode):
    """t_lo at a tile origin, at its last column and odd mid-tile x windows of 1 ... 513 columns (narrower than a lane's vector, one
    wave tile / one workgroup tile and one column less or more) x z_lo = t_lo, t_lo + 1 (inside a lane's vector), t_hi - 1."""
    _Fwd(64, 48, 40, d, t_lo, t_lo + w, z_lo=z_lo, mode=mode, bias=bias, seed=t_lo + w).run("window tlo%d w%d zlo%d d%d" % (t_lo, w, z_lo, d))


def test_block_refusals_and_empty_calls():
    """-4 for t_lo < d + 1, for a pitch that is no multiple of 4 and for z_half_stride on the 32-channel block; t_hi <= t_lo and
    batch = 0 return 0 and write nothing."""
    c = _Fwd(64, 64, 64, 64, 128 + 5, 128 + 5 + 200, seed=1)
    with _refused():
        c.launch(t_lo=64)                                        # d + 1 = 65
    with _refused():
        c.launch(pitch=c.pitch + 2)
    c32 = _Fwd(32, 32, 32, 1, 64 + 5, 64 + 5 + 200, seed=2)
    with _refused():
        c32.launch(z_half=32 * c32.pitch)
    for kw in (dict(t_hi=c.t_lo), dict(t_hi=c.t_lo - 7), dict(batch=0)):
        xo, zo = c.launch(**kw)
        assert _written(xo) == 0 and _written(zo) == 0, kw


REMAP = [(64, 64, 64, 4, 128 + 5, 128 + 2100, 3, MF), (32, 20, 24, 64, 64 + 33, 64 + 2300, 3, MB)]


@pytest.mark.parametrize("ch,R,D,d,t_lo,t_hi,B,mode", REMAP, ids=["ch%d-grid%d" % (c[0], _block_grid(c[4], c[5], c[6])) for c in REMAP])
def test_block_workgroup_remap(ch, R, D, d, t_lo, t_hi, B, mode):
    """More than eight workgroups, their count no multiple of eight: wn_block's XCD remap must be a permutation.  A tile the remap
    leaves out stays NaN, a tile computed in another's place differs (every tile has its own data)."""
    c = _Fwd(ch, R, D, d, t_lo, t_hi, z_lo=t_lo + 1, B=B, mode=mode, bias=True, seed=5)
    assert c.grid() > 8 and c.grid() % 8 != 0
    c.run("remap ch%d grid %d" % (ch, c.grid()))


GATHER_LE = (1, 5, 31, 32, 33, 100)


@pytest.mark.parametrize("rule", ["stretch", "tile"])
@pytest.mark.parametrize("le", GATHER_LE)
@pytest.mark.parametrize("ch,R,D", [(64, 48, 40), (32, 20, 24)])
def test_block_gathered_conditioning(ch, R, D, le, rule):
    """The gathered conditioning bias: 1 ... 100 buckets under the stretch and the tile rule, cond_pitch = cond_le + 3 with NaN
    beyond cond_le, table columns pairwise far apart (a wrong bucket is off by orders of magnitude)."""
    d = (1, 3, 64)[le % 3]
    t_lo, t_hi = _window_of(d)
    mode = (MF, MB)[(le + (rule == "tile")) % 2]
    _Fwd(ch, R, D, d, t_lo, t_hi, z_lo=t_lo + 2, mode=mode, cond=(le, rule), seed=le).run("gather ch%d le%d %s" % (ch, le, rule))


MFMA_COND = [(le, rule) for le in (1, 5, 31, 32) for rule in ("stretch", "tile")] + [(32, "rot")]


def _mfma_case(le, rule, mode=MF):
    t_lo = 64 + 37
    return _Fwd(64, 48, 40, 5, t_lo, t_lo + 301, z_lo=t_lo + 3, mode=mode, cond=(le, rule), bias=(le == 5), seed=300 + le)


# the table reaches the product as f16 hi + lo (to 2^-22 of its magnitude, here <= 3.9).  Observed against the gather: x_out 1.6e-7,
# z 3.0e-7 (bar 2e-5); against float64: inside the figures above
@pytest.mark.parametrize("le,rule", MFMA_COND, ids=["le%d-%s" % c for c in MFMA_COND])
def test_block_conditioning_on_the_matrix_cores(le, rule):
    """The CND instantiation (ch = 64, f16x3, cond_pack + cond_idx, at most 32 buckets): the table times the 0/1 matrix built
    from id >> 3, (id & 7) >> 1, id & 1 as one more k-step.  Against float64, and against the gathered launch on the same inputs
    (BARFORM).  Under the tile rule 32 buckets stay locked to a lane's column positions (32 = 0 mod 4): 'rot' - the tile rule
    moved on by one bucket per period, bytes only this form can take - puts every bucket 0..31 at each of the four positions, as
    do the stretch rule's runs of nine columns and the tile rule with 31 buckets (asserted in the coverage test)."""
    c = _mfma_case(le, rule)
    assert _cond_on_mfma(c.chl, c.mode, le, c.cpk is not None)
    xo, zo = c.run("mfma le%d %s" % (le, rule), pack=True)
    if rule == "rot":
        return
    xg, zg = c.launch(pack=False)
    z, y = c.reference()
    B, p = c.B, c.pitch
    dx = _form_dev(_view(xo, B, 64, p).cpu(), _view(xg, B, 64, p).cpu(), y.abs().clamp(min=1.0), (slice(None), slice(None), slice(c.t_lo, c.t_hi)))
    dz = _form_dev(_view(zo, B, 64, p).cpu(), _view(zg, B, 64, p).cpu(), torch.ones(1), (slice(None), slice(None), slice(c.z_lo, c.t_hi)))
    print("OBS block-mfma-vs-gather x_out %.2e z %.2e   [le%d %s]" % (dx, dz, le, rule))
    assert dx <= BARFORM and dz <= BARFORM


@pytest.mark.parametrize("what,le,mode", [("bf16x3", 31, MB), ("le33", 33, MF)])
def test_block_conditioning_pack_falls_back_to_the_gather(what, le, mode):
    """A pack given where the launcher cannot use it (bf16x3; more than 32 buckets): the gather, bit for bit what passing no
    pack gives."""
    c = _mfma_case(le, "tile", mode)
    assert c.cpk is not None and not _cond_on_mfma(c.chl, mode, le, True)
    xo, zo = c.run("fallback " + what, pack=True)
    xg, zg = c.launch(pack=False)
    assert _same_bits(xo, xg) and _same_bits(zo, zg)


PAIRS = [(R, D, v) for R, D in ((32, 32), (24, 20)) for v in ("plain", "bias", "cond_stretch", "cond_tile")]


# observed against the 32-channel launches: x_out 8.7e-8, z 3.0e-7 (bar 2e-5)
@pytest.mark.parametrize("R,D,v", PAIRS, ids=["R%d-D%d-%s" % c for c in PAIRS])
def test_block_clip_pairs(R, D, v):
    """z_half_stride != 0: four clips of a 32-channel model as two launch items of the 64-channel block, block-diagonal packs
    (_diag), the conditioning through the pack with table rows [f: A B | g: A B]: against float64 per clip, and against the
    32-channel launches on the same inputs (BARFORM: 'to rounding', not bits).  The second clip's z rows lie z_half_stride floats
    behind the first's, the 32 rows below each clip's stay NaN."""
    d, t_lo = 7, 64 + 33
    cond = (8, "stretch") if "stretch" in v else (31, "tile") if "tile" in v else None
    kw = dict(z_lo=t_lo + 2, B=4, mode=MF, bias=v == "bias", cond=cond, seed=70 + R)
    c2 = _Fwd(32, R, D, d, t_lo, t_lo + 301, pairs=True, **kw)
    c1 = _Fwd(32, R, D, d, t_lo, t_lo + 301, pairs=False, **kw)
    assert _same_bits(c1.x, c2.x) and c2.chl == 64 and c2.nb == 2
    if cond:
        assert _cond_on_mfma(c2.chl, MF, cond[0], c2.cpk is not None)
    xo2, zo2 = c2.run("pairs R%d D%d %s" % (R, D, v), pack=True)
    xo1, zo1 = c1.run("single R%d D%d %s" % (R, D, v))
    assert torch.isnan(_view(zo2, 4, 64, c2.pitch)[:, 32:]).all()
    z, y = c1.reference()
    p = c1.pitch
    dx = _form_dev(_view(xo2, 4, 32, p).cpu(), _view(xo1, 4, 32, p).cpu(), y.abs().clamp(min=1.0), (slice(None), slice(None), slice(t_lo, c1.t_hi)))
    dz = _form_dev(_view(zo2, 4, 64, p).cpu()[:, :32], _view(zo1, 4, 32, p).cpu(), torch.ones(1), (slice(None), slice(None), slice(c1.z_lo, c1.t_hi)))
    print("OBS block-pairs-vs-32ch x_out %.2e z %.2e   [R%d D%d %s]" % (dx, dz, R, D, v))
    assert dx <= BARFORM and dz <= BARFORM


def test_block_case_tables_cover_what_they_claim():
    """the host formulas of launch_fwd_nt / wn_resblock_fwd put every case where its id says"""
    for v in VARIANTS:
        mine = [c for c in VARIANT_TABLE if c[0] == v]
        for ch in (64, 32):
            assert {c[5] for c in mine if c[1] == ch} == {MF, MB}, (v, ch)
            assert {c[4] for c in mine if c[1] == ch} == set(DILATIONS), (v, ch)
        assert {c[1:4] for c in mine} == set(SHAPES)
    t_lo, t_hi = _window_of(512)
    assert t_hi - t_lo < 512 and all(_window_of(d)[1] % 4 != 0 for d in DILATIONS)
    assert all((_window_of(d)[0] + 45) % 4 != 0 for d in DILATIONS)                    # z_lo inside a lane's vector
    assert {t % 64 for t in WIN_TLO} == {0, 63, 37}
    assert {c[1] for c in WINDOW_TABLE} == set(WIN_WIDTHS)
    for t_lo in WIN_TLO:
        for w in WIN_WIDTHS:
            zs = {c[2] for c in WINDOW_TABLE if c[0] == t_lo and c[1] == w}
            assert zs == {t_lo, min(t_lo + 1, t_lo + w - 1), t_lo + w - 1}
    assert all(c[0] >= c[3] + 1 for c in WINDOW_TABLE)
    assert any((c[0] + c[1]) % 4 for c in WINDOW_TABLE) and any(c[2] % 4 for c in WINDOW_TABLE) and any(c[1] < 4 for c in WINDOW_TABLE)
    assert {(c[4], c[5]) for c in WINDOW_TABLE} == {(b, m) for b in (False, True) for m in (MF, MB)}
    for c in REMAP:
        g = _block_grid(c[4], c[5], c[6])
        assert g > 8 and g % 8 != 0
    assert _block_grid(5 + 1, 1400, 2) == 6                                              # (what test_resblock_fwd launches at most)
    # buckets: every bucket that exists occurs; and where the docstrings say so, at each of a lane's four column positions
    t_lo, t_hi = 64 + 37, 64 + 37 + 301
    pos = (np.arange(t_lo, t_hi) % 4)
    for le, rule in MFMA_COND:
        tr = np.arange(t_hi - t_lo)
        idx = (tr + tr // le) % le if rule == "rot" else _buckets(t_hi - t_lo, le, rule)[0]
        assert set(idx.tolist()) == set(range(le)), (le, rule)
        pairs = {(int(b), int(p)) for b, p in zip(idx, pos)}
        every = pairs == {(b, p) for b in range(le) for p in range(4)}
        assert every == ((le, rule) != (32, "tile")), (le, rule)
        assert _cond_on_mfma(64, MF, le, True)
    assert {b >> 3 for b in range(32)} == {0, 1, 2, 3} and {(b & 7) >> 1 for b in range(32)} == {0, 1, 2, 3}
    assert not _cond_on_mfma(64, MB, 31, True) and not _cond_on_mfma(64, MF, 33, True) and not _cond_on_mfma(32, MF, 31, True)
    for le in GATHER_LE:
        for rule in ("stretch", "tile"):
            L = 301
            assert set(_buckets(L, le, rule)[0].tolist()) == set(range(le))
    c = _mfma_case(32, "rot")
    t = c.tab_clip[:, :, :32]
    rows = torch.cat([t[:, :c.D], t[:, 64:64 + c.D]], 1)                                # the real rows: pairwise far apart columns
    gap = (rows[:, :, :, None] - rows[:, :, None, :]).abs().amax(1) + torch.eye(32) * 1e9    # per clip and pair of columns: the widest row
    assert gap.min().item() >= c.step and rows.abs().max().item() <= 6.0


# ================================================================================================ B. wn_skip_epilogue_fwd
def _epi_tiles(t_lo, t_hi, B):
    t_base = t_lo & ~63
    ntx = (t_hi - t_base + EPI_COLS - 1) // EPI_COLS
    return t_base, ntx, ntx * B


def _fwd_regime(KZ):
    """(iterations one at a time, groups of six in the pipelined loop) of skip_epilogue_fwd_k"""
    NI = KZ // 64
    return NI % 6, NI // 6


def _mat(rng, rows, cols, r_valid, c_valid):
    m = np.zeros((rows, cols), np.float32)
    m[:r_valid, :c_valid] = rng.standard_normal((r_valid, c_valid)).astype(np.float32) * 0.08
    return m


class _EpiF:
    """u = bias_s + Ws z; h = bias_1 + P1 relu(u); o = bias_2 + P2 relu(h) on [t_lo, t_hi): inputs (z NaN outside the window,
    bias entries beyond the valid rows NaN), the fused launch, the three wn_chan_gemm launches and the float64 reference."""

    def __init__(self, B, KZ, S, Qv, t_lo, width, bias, mode, pitch=None, seed=0):
        self.B, self.KZ, self.S, self.Qv, self.t_lo, self.t_hi, self.mode, self.W = B, KZ, S, Qv, t_lo, t_lo + width, mode, width
        t_base, ntx, _ = _epi_tiles(t_lo, t_lo + width, B)
        self.need = t_base + EPI_COLS * ntx                      # the rows are read over whole tiles
        self.pitch = pitch = ((self.need + 255) // 256) * 256 + 256 if pitch is None else pitch
        rng = np.random.default_rng(11 + seed)
        self.ws, self.p1, self.p2 = _mat(rng, 256, KZ, S, KZ), _mat(rng, 256, 256, S, S), _mat(rng, 256, 256, Qv, S)
        self.pk_s, self.pk_1, self.pk_2 = _packed(self.ws, mode), _packed(self.p1, mode), _packed(self.p2, mode)
        self.pk_1c, self.pk_2c = _packed(self.p1, mode, chained=True), _packed(self.p2, mode, chained=True)
        self.z = _buf(B, KZ, pitch, 1.0, 3 + seed)
        _nan_around(self.z, B, KZ, pitch, t_lo, t_lo + width)
        self.bias = self.bias0 = None
        if bias:
            self.bias, self.bias0 = [], []
            for valid in (S, S, Qv):
                v = torch.from_numpy(rng.standard_normal(256).astype(np.float32))
                v0 = v.clone()
                v[valid:], v0[valid:] = NAN, 0.0
                self.bias.append(v.to(DEV))
                self.bias0.append(v0.to(DEV))                    # (for wn_chan_gemm, whose bias has no row count)
        self._ref = None

    def reference(self):
        if self._ref is None:
            B, t_lo, t_hi = self.B, self.t_lo, self.t_hi
            zz = _view(self.z, B, self.KZ, self.pitch).cpu()[:, :, t_lo:t_hi].double()
            assert not torch.isnan(zz).any()
            bb = [b_.cpu().double()[None, :, None] for b_ in self.bias0] if self.bias else [0.0] * 3
            ru = torch.einsum("mk,bkt->bmt", torch.from_numpy(self.ws).double(), zz) + bb[0]
            rh = torch.einsum("mk,bkt->bmt", torch.from_numpy(self.p1).double(), ru.clamp(min=0)) + bb[1]
            ro = torch.einsum("mk,bkt->bmt", torch.from_numpy(self.p2).double(), rh.clamp(min=0)) + bb[2]
            self._ref = (ru[:, :self.S], rh[:, :self.S], ro[:, :self.Qv])
        return self._ref

    def fused(self, pitch=None, ks=None, mode=None):
        B, KZ, W, p = self.B, self.KZ, self.W, self.pitch
        u, h = _nanbuf(B, 256, p), _nanbuf(B, 256, p)
        o = torch.full((B * 256 * W + 512,), NAN, device=DEV)
        b_ = self.bias
        call("wn_skip_epilogue_fwd", ptr(self.z, SLACK), KZ * p, p if pitch is None else pitch, KZ // 32 if ks is None else ks, ptr(self.pk_s),
             ptr(b_[0]) if b_ else None, ptr(u, SLACK), ptr(h, SLACK), 256 * p, ptr(self.pk_1c), ptr(b_[1]) if b_ else None, ptr(self.pk_2c),
             ptr(b_[2]) if b_ else None, ptr(o), 256 * W, W, self.S, self.Qv, self.t_lo, self.t_hi, B, self.mode if mode is None else mode,
             _lib.stream())
        torch.cuda.synchronize()
        return u, h, o

    def three(self):
        """the three wn_chan_gemm launches (zero-filled u / h: the second and third product read all 256 rows)"""
        B, KZ, W, p, t_lo, T, S, m = self.B, self.KZ, self.W, self.pitch, self.t_lo, self.t_hi, self.S, self.mode
        u, h = _buf(B, 256, p), _buf(B, 256, p)
        o = torch.zeros(B * 256 * W + 512, device=DEV)
        bs = [ptr(b_) for b_ in self.bias0] if self.bias else [None] * 3
        st = _lib.stream()
        call("wn_chan_gemm", ptr(self.z, SLACK), None, KZ * p, p, t_lo, T, 0, 0, KZ // 32, 0, ptr(self.pk_s), 16, S, ptr(u, SLACK), 256 * p,
             p, 0, bs[0], None, 0, 0, 0, None, 0, 0, t_lo, T, 0, B, m, st)
        call("wn_chan_gemm", ptr(u, SLACK), None, 256 * p, p, t_lo, T, 0, 0, 8, 0, ptr(self.pk_1), 16, S, ptr(h, SLACK), 256 * p,
             p, 0, bs[1], None, 0, 0, 0, None, 0, 0, t_lo, T, 1, B, m, st)
        call("wn_chan_gemm", ptr(h, SLACK), None, 256 * p, p, t_lo, T, 0, 0, 8, 0, ptr(self.pk_2), 16, self.Qv, ptr(o), 256 * W, W, -t_lo,
             bs[2], None, 0, 0, 0, None, 0, 0, t_lo, T, 1, B, m, st)
        torch.cuda.synchronize()
        return u, h, o

    def views(self, out):
        B, W, p, t_lo, t_hi = self.B, self.W, self.pitch, self.t_lo, self.t_hi
        u, h, o = out
        return (_view(u, B, 256, p).cpu()[:, :self.S, t_lo:t_hi], _view(h, B, 256, p).cpu()[:, :self.S, t_lo:t_hi],
                o[:B * 256 * W].view(B, 256, W).cpu()[:, :self.Qv])

    def check(self, out, tag, other=None):
        B, W, S, Qv = self.B, self.W, self.S, self.Qv
        bar = 3 * TOL[self.mode]
        for name, raw, rows in zip("uho", out, (S, S, Qv)):
            assert _written(raw) == B * rows * W, "%s: %s written outside its valid rows x [t_lo, t_hi) (or NaN inside)" % (tag, name)
        errs = {n: _rel(g, r) for n, g, r in zip("uho", self.views(out), self.reference())}
        print("OBS epi-fwd-%s " % MODE_ID[self.mode] + " ".join("%s %.2e" % kv for kv in errs.items()) + "   [%s]" % tag)
        assert all(v <= bar for v in errs.values()), (tag, errs)
        if other is not None:
            devs = {n: (g.double() - t.double()).abs().max().item() / r.abs().max().item()
                    for n, g, t, r in zip("uho", self.views(out), self.views(other), self.reference())}
            print("OBS epi-fwd-vs-three-%s " % MODE_ID[self.mode] + " ".join("%s %.2e" % kv for kv in devs.items()) + "   [%s]" % tag)
            assert all(v <= bar for v in devs.values()), (tag, devs)

    def run(self, tag, three=False):
        out = self.fused()
        self.check(out, tag, self.three() if three else None)
        out2 = self.fused()
        assert all(_same_bits(a, b) for a, b in zip(out, out2)), tag + ": a second launch does not reproduce the bits"
        return out


# Observed worst over every forward-epilogue test (bars 3e-5 / 3e-4): f16x3 u 7.0e-7, h 5.8e-7, o 7.5e-7; bf16x3 u 5.5e-6, h 8.2e-6,
# o 1.0e-5; against the three launches f16x3 8.4e-7, bf16x3 3.2e-6 (u identical).  test_skip_epilogue_fwd_fused prints the like
EPI_MODES = pytest.mark.parametrize("mode", [MF, MB], ids=[MODE_ID[MF], MODE_ID[MB]])
DEPTHS = {64: (1, 0), 384: (0, 1), 448: (1, 1), 704: (5, 1), 832: (1, 2)}      # KZ -> (one at a time, groups of six)


@EPI_MODES
@pytest.mark.parametrize("KZ", list(DEPTHS), ids=["KZ%d-pre%d-loop%d" % (k, a, b) for k, (a, b) in DEPTHS.items()])
def test_epilogue_fwd_depths(KZ, mode):
    """NI = 1, 6, 7, 11, 13 iterations: the one-at-a-time iterations only; the software-pipelined loop only; 1 + 6; 5 + 6; 1 + 12
    (its three weight register sets, two stages and the clamped it + 2 / it + 3 requests).  u, h, o against float64 and against
    the three wn_chan_gemm launches."""
    assert _fwd_regime(KZ) == DEPTHS[KZ]
    _EpiF(2, KZ, 256, 256, 37, 300, False, mode, seed=KZ).run("depth KZ%d" % KZ, three=True)


@EPI_MODES
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("S,Qv", [(256, 256), (250, 256), (256, 100), (17, 33)])
def test_epilogue_fwd_channels(S, Qv, bias, mode):
    """s_valid / q_valid at and below 256 (a row tile cut, whole waves without a valid row), with and without the three biases
    (their entries beyond the valid rows are NaN): rows beyond the valid counts stay NaN."""
    _EpiF(2, 128, S, Qv, 37, 300, bias, mode, seed=S + Qv).run("channels S%d Q%d bias%d" % (S, Qv, bias), three=True)


EPI_TLO = (128, 128 + 63, 37)
EPI_WIDTHS = (1, 127, 128, 129, 300)


@pytest.mark.parametrize("width", EPI_WIDTHS)
@pytest.mark.parametrize("t_lo", EPI_TLO)
def test_epilogue_fwd_windows(t_lo, width):
    """t_lo at a tile origin, at 64 k + 63 and at 37 x windows of 1 ... 300 columns; z is NaN outside [t_lo, t_hi) inside its rows
    (the header: ignored, NaN included)."""
    mode = (MF, MB)[(t_lo + width) % 2]
    _EpiF(3, 384, 250, 256, t_lo, width, True, mode, seed=t_lo + width).run("window tlo%d w%d" % (t_lo, width))


def test_epilogue_fwd_tightest_pitch_and_refusals():
    """A window that ends on a tile edge with pitch = t_base + 128 ntx, the tightest the launcher takes; 4 floats less, an odd
    ks_skip: -4; an x1 mode: refused as a bad mode (-2, the code every launcher gives a mode it does not have)."""
    t_lo, width = 128 + 7, 3 * 128 - 7
    need = 128 + 3 * 128
    c = _EpiF(2, 128, 256, 256, t_lo, width, True, MF, pitch=need, seed=4)
    assert c.need == c.pitch == need and c.t_hi == need
    c.run("tightest pitch")
    for kw, code in ((dict(pitch=need - 4), -4), (dict(ks=3), -4), (dict(mode=_lib.F16X1), -2), (dict(mode=_lib.BF16X1), -2)):
        with _refused(code):
            c.fused(**kw)


def _big_shape():
    """B = 3 clips of cus // 3 + 1 tiles: one tile more than a round, whatever the device"""
    ntx = _cus() // 3 + 1
    return 3, 64 + 5, ntx * EPI_COLS - 5 - 11, ntx               # t_lo = 69 (t_base 64), the last tile 11 columns short


# observed at 256 compute units (258 tiles of 11 008 columns): u 5.2e-7, h 5.1e-7, o 5.5e-7; 0.5 s
def test_epilogue_fwd_more_tiles_than_compute_units(monkeypatch):
    """ntx * batch > compute units: the first round is staggered, with the pipelined loop under it (KZ = 384).  Against float64
    and bit for bit against the same launch under WN_EPI_STAGGER=0 (the variable is read at every launch)."""
    B, t_lo, width, ntx = _big_shape()
    assert _epi_tiles(t_lo, t_lo + width, B) == (64, ntx, 3 * ntx) and 3 * ntx > _cus() and _fwd_regime(384) == (0, 1)
    c = _EpiF(B, 384, 256, 256, t_lo, width, False, MF, seed=9)
    monkeypatch.delenv("WN_EPI_STAGGER", raising=False)
    out = c.run("more tiles than CUs")
    monkeypatch.setenv("WN_EPI_STAGGER", "0")
    plain = c.fused()
    assert all(_same_bits(a, b) for a, b in zip(out, plain)), "the staggered first round changes bits"


def test_epilogue_fwd_case_tables_cover_what_they_claim():
    cus = _cus()
    assert {_fwd_regime(k) for k in DEPTHS} == {(1, 0), (0, 1), (1, 1), (5, 1), (1, 2)}
    assert _fwd_regime(128)[1] == 0 and _fwd_regime(192)[1] == 0                       # (what test_skip_epilogue_fwd_fused reaches)
    assert _fwd_regime(384)[1] == 1                                                    # the window tests run the pipelined loop too
    for t_lo in EPI_TLO:
        for w in EPI_WIDTHS:
            assert _epi_tiles(t_lo, t_lo + w, 3)[2] <= cus, "a small case would be staggered"
    assert {t % 64 for t in EPI_TLO} == {0, 63, 37}
    B, t_lo, width, ntx = _big_shape()
    assert _epi_tiles(t_lo, t_lo + width, B)[2] == 3 * ntx > cus and 3 * ntx - cus <= 3


# ================================================================================================ C. wn_skip_epilogue_bwd
def _bwd_regime(mt_z, ntiles, cus, split_env=True):
    """(dZ passes, tiles of the partly filled last round, is it dealt out by passes) of wn_launch_skip_epilogue_bwd"""
    npass = (mt_z // 3 + 7) // 8
    rest = ntiles % cus
    return npass, rest, ntiles > cus and rest > 0 and rest * npass <= cus and split_env


class _EpiB:
    """dh = (P2^T d_o) [h > 0]; du = (P1^T dh) [u > 0]; dz = Ws^T du on [t_lo, t_hi): inputs (h, u NaN outside the window), the
    fused launch, the three wn_chan_gemm launches and the float64 reference.
    d_o is of order 1e-3 in bf16x3 (the backward's mode, a gradient's magnitude) and of order 1 in f16x3: an f16 operand's lo piece
    is a normal number only from 2^-3 on, and at 1e-3 the rounding of the operands alone (hi = f16(x), lo = f16(x - hi), exact
    products, float64 sums, on the inputs of the 480 / 448-row case with s_valid = 17) leaves dz 6.4e-5 of max-abs off - twice the
    bar before the kernel has done anything; at order 1 it leaves 4.2e-7.  That is why gradients run in bf16x3 (header)."""

    def __init__(self, B, MZ, zv, S, t_lo, width, mode, pitch=None, seed=0):
        self.B, self.MZ, self.zv, self.S, self.t_lo, self.t_hi, self.mode, self.W = B, MZ, zv, S, t_lo, t_lo + width, mode, width
        t_base, ntx, _ = _epi_tiles(t_lo, t_lo + width, B)
        self.need = t_base + EPI_COLS * ntx
        self.pitch = pitch = ((self.need + 255) // 256) * 256 + 256 if pitch is None else pitch
        rng = np.random.default_rng(13 + seed)
        self.p2, self.p1, self.ws = _mat(rng, 256, 256, 256, S), _mat(rng, 256, 256, S, S), _mat(rng, 256, MZ, S, zv)     # [Q][S], [S][S], [S][rows of z]
        T_ = lambda m: np.ascontiguousarray(m.T)
        self.pk_p2T, self.pk_p1T, self.pk_sT = _packed(T_(self.p2), mode), _packed(T_(self.p1), mode), _packed(T_(self.ws), mode)
        self.pk_p1Tc, self.pk_sTc = _packed(T_(self.p1), mode, chained=True), _packed(T_(self.ws), mode, chained=True)
        g = torch.Generator(device="cpu").manual_seed(5 + seed)
        self.dO = (torch.randn(B, 256, width, generator=g) * (1e-3 if mode == MB else 1.0)).to(DEV).contiguous()
        self.h, self.u = _buf(B, 256, pitch, 1.0, 6 + seed), _buf(B, 256, pitch, 1.0, 7 + seed)
        for m in (self.h, self.u):
            _nan_around(m, B, 256, pitch, t_lo, t_lo + width)
        self._ref = None

    def reference(self):
        if self._ref is None:
            B, p, t_lo, t_hi = self.B, self.pitch, self.t_lo, self.t_hi
            hv, uv = (_view(m, B, 256, p).cpu()[:, :, t_lo:t_hi] for m in (self.h, self.u))
            assert not torch.isnan(hv).any() and not torch.isnan(uv).any()
            rh = torch.einsum("qs,bqt->bst", torch.from_numpy(self.p2).double(), self.dO.cpu().double()) * (hv > 0)
            ru = torch.einsum("rs,brt->bst", torch.from_numpy(self.p1).double(), rh) * (uv > 0)
            rz = torch.einsum("sm,bst->bmt", torch.from_numpy(self.ws).double(), ru)
            self._ref = (rh[:, :self.S], ru[:, :self.S], rz[:, :self.zv])
        return self._ref

    def fused(self, pitch=None, mt_z=None):
        B, MZ, W, p = self.B, self.MZ, self.W, self.pitch
        dh, du, dz = _nanbuf(B, 256, p), _nanbuf(B, 256, p), _nanbuf(B, MZ, p)
        call("wn_skip_epilogue_bwd", ptr(self.dO), 256 * W, W, ptr(self.h, SLACK), ptr(self.u, SLACK), 256 * p, p if pitch is None else pitch,
             ptr(dh, SLACK), ptr(du, SLACK), ptr(dz, SLACK), MZ * p, ptr(self.pk_p2T), ptr(self.pk_p1Tc), ptr(self.pk_sTc),
             MZ // 16 if mt_z is None else mt_z, self.zv, self.S, self.t_lo, self.t_hi, B, self.mode, _lib.stream())
        torch.cuda.synchronize()
        return dh, du, dz

    def three(self):
        """the three wn_chan_gemm launches (zero-filled dh / du: the products read all 256 rows)"""
        B, MZ, W, p, t_lo, T, S, m = self.B, self.MZ, self.W, self.pitch, self.t_lo, self.t_hi, self.S, self.mode
        dh, du, dz = _buf(B, 256, p), _buf(B, 256, p), _buf(B, MZ, p)
        st = _lib.stream()
        call("wn_chan_gemm", ptr(self.dO), None, 256 * W, W, 0, W, -t_lo, 0, 8, 0, ptr(self.pk_p2T), 16, S, ptr(dh, SLACK), 256 * p, p, 0, None,
             None, 0, 0, 0, ptr(self.h, SLACK), 256 * p, p, t_lo, T, 0, B, m, st)
        call("wn_chan_gemm", ptr(dh, SLACK), None, 256 * p, p, t_lo, T, 0, 0, 8, 0, ptr(self.pk_p1T), 16, S, ptr(du, SLACK), 256 * p,
             p, 0, None, None, 0, 0, 0, ptr(self.u, SLACK), 256 * p, p, t_lo, T, 0, B, m, st)
        call("wn_chan_gemm", ptr(du, SLACK), None, 256 * p, p, t_lo, T, 0, 0, 8, 0, ptr(self.pk_sT), MZ // 16, self.zv, ptr(dz, SLACK), MZ * p,
             p, 0, None, None, 0, 0, 0, None, 0, 0, t_lo, T, 0, B, m, st)
        torch.cuda.synchronize()
        return dh, du, dz

    def views(self, out):
        B, p, t_lo, t_hi = self.B, self.pitch, self.t_lo, self.t_hi
        return tuple(_view(t, B, rows, p).cpu()[:, :valid, t_lo:t_hi]
                     for t, rows, valid in zip(out, (256, 256, self.MZ), (self.S, self.S, self.zv)))

    def check(self, out, tag, other=None):
        B, W = self.B, self.W
        bar = 3 * TOL[self.mode]
        names = ("dh", "du", "dz")
        for name, raw, rows in zip(names, out, (self.S, self.S, self.zv)):
            assert _written(raw) == B * rows * W, "%s: %s written outside its valid rows x [t_lo, t_hi) (or NaN inside)" % (tag, name)
        errs = {n: _rel(g, r) for n, g, r in zip(names, self.views(out), self.reference())}
        print("OBS epi-bwd-%s " % MODE_ID[self.mode] + " ".join("%s %.2e" % kv for kv in errs.items()) + "   [%s]" % tag)
        assert all(v <= bar for v in errs.values()), (tag, errs)
        if other is not None:
            devs = {n: (g.double() - t.double()).abs().max().item() / r.abs().max().item()
                    for n, g, t, r in zip(names, self.views(out), self.views(other), self.reference())}
            print("OBS epi-bwd-vs-three-%s " % MODE_ID[self.mode] + " ".join("%s %.2e" % kv for kv in devs.items()) + "   [%s]" % tag)
            assert all(v <= bar for v in devs.values()), (tag, devs)

    def run(self, tag, three=False):
        out = self.fused()
        self.check(out, tag, self.three() if three else None)
        out2 = self.fused()
        assert all(_same_bits(a, b) for a, b in zip(out, out2)), tag + ": a second launch does not reproduce the bits"
        return out


# Observed worst over every backward-epilogue test (bars 3e-4 / 3e-5): bf16x3 dh 7.6e-6, du 9.4e-6, dz 1.1e-5; f16x3 (d_o of order 1)
# dh 4.8e-7, du 5.7e-7, dz 6.4e-7; against the three launches bf16x3 5.1e-6, f16x3 7.2e-7 (dh identical).  With d_o of order 1e-3
# f16x3 gave dz 5.2e-5 (480 / 448 rows) and 4.6e-5 (1920) at s_valid = 17: the format's floor there, see _EpiB
ROWS = [(48, 48), (192, 192), (480, 448), (480, 440), (432, 432), (1920, 1920)]
ROWS_S = (256, 250, 17)


@EPI_MODES
@pytest.mark.parametrize("MZ,zv", ROWS, ids=["MZ%d-valid%d" % r for r in ROWS])
def test_epilogue_bwd_row_padding(MZ, zv, mode):
    """16 mt_z rows of dz of which z_valid are real: one group of 48 rows (seven waves skip the dZ product), four groups, the
    engine's padding of seven 64-row blocks to 480 (448 real; 440: a row tile cut), two passes of which the second has one group,
    five passes.  Rows >= z_valid of dz and >= s_valid of dh / du stay NaN.  Against float64 and the three wn_chan_gemm launches."""
    S = ROWS_S[(ROWS.index((MZ, zv)) + (mode == MB)) % 3]
    _EpiB(2, MZ, zv, S, 37, 300, mode, seed=MZ + zv).run("rows MZ%d valid%d S%d" % (MZ, zv, S), three=True)


@pytest.mark.parametrize("width", EPI_WIDTHS)
@pytest.mark.parametrize("t_lo", EPI_TLO)
def test_epilogue_bwd_windows(t_lo, width):
    """the windows of the forward epilogue's test; h and u are NaN outside [t_lo, t_hi) inside their rows (read over whole tiles:
    they only gate results that are never stored)"""
    mode = (MB, MF)[(t_lo + width) % 2]
    _EpiB(3, 192, 192, 250, t_lo, width, mode, seed=t_lo + width).run("window tlo%d w%d" % (t_lo, width))


def test_epilogue_bwd_tightest_pitch_and_refusals():
    """pitch = t_base + 128 ntx is taken, 4 floats less and an mt_z that is no multiple of 3 are refused (-4)"""
    t_lo, width = 128 + 7, 3 * 128 - 7
    need = 128 + 3 * 128
    c = _EpiB(2, 192, 192, 256, t_lo, width, MB, pitch=need, seed=4)
    assert c.need == c.pitch == need
    c.run("tightest pitch")
    for kw in (dict(pitch=need - 4), dict(mt_z=11), dict(mt_z=10)):
        with _refused():
            c.fused(**kw)


# observed at 256 compute units (258 tiles, rest 2, 4 short workgroups): dh 4.8e-6, du 6.9e-6, dz 8.4e-6; 0.6 s each
@pytest.mark.parametrize("MZ,zv,S", [(432, 432, 256), (480, 448, 250)], ids=["MZ432", "MZ480-valid448"])
def test_epilogue_bwd_partly_filled_last_round(MZ, zv, S, monkeypatch):
    """One tile more than a round of the device: the last round's tiles are dealt out by dZ passes (n_whole, p0, store_sd, the
    mz >= mt_z break; only pass 0 stores dh / du).  Against float64, and bit for bit against WN_EPI_BWD_SPLIT=0 (every tile whole)
    and WN_EPI_BWD_NT=1 (streaming dZ stores): all three form the same sums in the same order."""
    B, t_lo, width, ntx = _big_shape()
    cus = _cus()
    npass, rest, split = _bwd_regime(MZ // 16, 3 * ntx, cus)
    assert npass == 2 and 1 <= rest <= 3 and split
    c = _EpiB(B, MZ, zv, S, t_lo, width, MB, seed=MZ)
    for v in ("WN_EPI_BWD_SPLIT", "WN_EPI_BWD_NT"):
        monkeypatch.delenv(v, raising=False)
    out = c.run("partly filled last round MZ%d" % MZ)
    monkeypatch.setenv("WN_EPI_BWD_SPLIT", "0")
    whole = c.fused()
    assert all(_same_bits(a, b) for a, b in zip(out, whole)), "tiles dealt out by passes differ from whole tiles"
    monkeypatch.delenv("WN_EPI_BWD_SPLIT")
    monkeypatch.setenv("WN_EPI_BWD_NT", "1")
    nt = c.fused()
    assert all(_same_bits(a, b) for a, b in zip(out, nt)), "streaming dZ stores change bits"


def test_epilogue_bwd_case_tables_cover_what_they_claim():
    cus = _cus()
    groups = lambda MZ: MZ // 48
    assert [(_bwd_regime(MZ // 16, 1, cus)[0], groups(MZ)) for MZ, _ in ROWS] == [(1, 1), (1, 4), (2, 10), (2, 10), (2, 9), (5, 40)]
    assert all(MZ % 48 == 0 and zv <= MZ for MZ, zv in ROWS) and groups(432) - 8 == 1   # the second pass of 432 rows: one group
    assert {zv % 16 for _, zv in ROWS} == {0, 8} and {MZ - zv for MZ, zv in ROWS} == {0, 32, 40}
    for mode in (MF, MB):                                                              # every s_valid meets both modes' case lists
        assert {ROWS_S[(i + (mode == MB)) % 3] for i in range(len(ROWS))} == set(ROWS_S)
    for t_lo in EPI_TLO:
        for w in EPI_WIDTHS:
            assert not _bwd_regime(12, _epi_tiles(t_lo, t_lo + w, 3)[2], cus)[2]        # the small cases: every tile whole
    B, t_lo, width, ntx = _big_shape()
    ntiles = _epi_tiles(t_lo, t_lo + width, B)[2]
    for MZ in (432, 480):
        npass, rest, split = _bwd_regime(MZ // 16, ntiles, cus)
        assert ntiles > cus and npass == 2 and 1 <= rest <= 3 and split
        assert not _bwd_regime(MZ // 16, ntiles, cus, split_env=False)[2]
    for n in range(32, 305):                                                           # ... on any device of 32 to 304 compute units
        nt = 3 * (n // 3 + 1)
        for mt_z in (27, 30, 120):
            npass, rest, split = _bwd_regime(mt_z, nt, n)
            assert rest in (1, 2, 3) and split, (n, mt_z)
