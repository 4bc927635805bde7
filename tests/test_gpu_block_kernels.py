"""GPU tests of the one-launch backward blocks, one launch at a time, against float64 (run with -m gpu).

Every test fills its device buffers itself, launches ONE entry point through _lib.call and compares with float64 torch autograd
on the CPU computed from the very float32 inputs the kernel read, so only that launch's arithmetic is measured.  Geometry is
hostile on purpose (alignments, windows and hand-over forms a dilation ladder never produces); everything around an output
window is pre-filled with NaN and must still be NaN afterwards, inputs hold NaN wherever include/wavenet_hip.h says their
values do not count.  No element is left out of a comparison.

Bars (the project's own, not what these kernels turn out to do):
  BAR64  = 1e-4 of the reference tensor's max-abs - what test_resblock_bwd_and_dx holds the same arithmetic (f16x3, bf16x3) to;
  BARFORM = 2e-5 of max-abs between two forms of the same sums - what tests/test_gpu_switches.py holds the whole model to;
  torch.equal where the header promises the same sums (wn_shift_add, wn_gather_grads2, a repeated launch)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from music_amd.engine import SLACK
from tests.test_gpu_kernels import _packed, _buf, _view, _fg_pack, _res_ref

DEV = "cuda"
CH = 64
MF, MB = _lib.F16X3, _lib.BF16X3
NAN = float("nan")
BAR64 = 1e-4
BARFORM = 2e-5


# ------------------------------------------------------------------------------------------------ helpers
def _nanbuf(b, rows, pitch):
    t = _buf(b, rows, pitch)
    t.fill_(NAN)                                    # slack in front and behind included
    return t


def _reduce(slab, ns, rows, cols):
    """wn_reduce_slabs over ns slabs of rows x cols -> dense tensor (fixed order: bit-reproducible)."""
    n = rows * cols
    out = torch.full((n + 8,), NAN, device=DEV)
    desc = torch.tensor([[0, 0, ns, n, 4, n]], dtype=torch.int64, device=DEV)
    call("wn_reduce_slabs", ptr(desc), 1, (n + 3) // 4, ptr(slab), ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out[4:4 + n].view(rows, cols).cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rel(got, ref):
    """max |got - ref| / max |ref|; NaN (which fails every <=) when anything in got is NaN."""
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def _written(buf):
    return int((~torch.isnan(buf)).sum().item())


def _all_zero(t):
    return t.numel() == 0 or (t == 0).all().item()


def _chain_ok_one_item_less(t_lo, t_hi, B, d):
    """is there still a chain form with one 32-column item less?  (False at the chain_ok boundary)"""
    return _lib.pq_chain_ok(t_lo, t_hi - 32, B, d)


def _diag(m32, rb, cb):
    """[rb*32][cb*32] blocks of 32 x 32 -> [rb*64][cb*64] with every block doubled on the diagonal (music_amd/engine.py's pair packs)"""
    out = np.zeros((rb * 64, cb * 64), np.float32)
    for a in range(rb):
        for b in range(cb):
            for c in range(2):
                out[a * 64 + c * 32:a * 64 + (c + 1) * 32, b * 64 + c * 32:b * 64 + (c + 1) * 32] = m32[a * 32:(a + 1) * 32, b * 32:(b + 1) * 32]
    return out


def _fold_pair(W, rb, cb):
    """The gradient of a weight that sits twice on the diagonal of a clip pair's [rb*64][cb*64] matrix: wn_gather_grads2 adds the
    two copies -> [rb*32][cb*32]; exactly the float32 sum of the two blocks.  (The off-diagonal blocks hold products of one clip's
    rows with the other clip's: the header has wn_gather_grads2 read the two diagonal copies only, nobody reads those.)"""
    pos = np.arange(rb * 64 * cb * 64, dtype=np.int64).reshape(rb * 64, cb * 64)
    i1 = np.zeros((rb * 32, cb * 32), np.int32)
    i2 = np.zeros((rb * 32, cb * 32), np.int32)
    for a in range(rb):
        for b in range(cb):
            i1[a * 32:(a + 1) * 32, b * 32:(b + 1) * 32] = pos[a * 64:a * 64 + 32, b * 64:b * 64 + 32]
            i2[a * 32:(a + 1) * 32, b * 32:(b + 1) * 32] = pos[a * 64 + 32:a * 64 + 64, b * 64 + 32:b * 64 + 64]
    n = i1.size
    flat = torch.full((n + 8,), NAN, device=DEV)
    Wd, i1d, i2d = W.to(DEV).contiguous(), torch.from_numpy(i1.reshape(-1)).to(DEV), torch.from_numpy(i2.reshape(-1)).to(DEV)
    call("wn_gather_grads2", ptr(Wd), ptr(i1d), ptr(i2d), ptr(flat), n, _lib.stream())
    torch.cuda.synchronize()
    got = flat[:n].cpu().view(rb * 32, cb * 32)
    w = W.reshape(-1)
    want = (w[torch.from_numpy(i1.reshape(-1)).long()] + w[torch.from_numpy(i2.reshape(-1)).long()]).view(rb * 32, cb * 32)
    assert torch.equal(got, want) and torch.isnan(flat[n:]).all(), "wn_gather_grads2 is not packed[idx] + packed[idx2]"
    return got


def _chain_plan(t_lo, t_hi, batch, d):
    """Host view of the chain plan: per workgroup the (clip, t0, flags) triples it walks."""
    lib = _lib.load()
    nwg = _lib.pq_slabs(t_lo, t_hi, batch, d, True)
    out = (ctypes.c_int * (3 * 4096))()
    plan = []
    for wg in range(nwg):
        n = lib.wn_resblock_bwd_pq_chain_items(t_lo, t_hi, batch, d, wg, out, 4096)
        assert 0 <= n <= 4096
        plan.append([(out[3 * k], out[3 * k + 1], out[3 * k + 2]) for k in range(n)])
    return plan


def _buckets(L, le, rule):
    """bucket of column t - t_lo, and the (mode, q) that make wn_cond_grad / wn_resblock_bwd_ms use the same rule"""
    tr = np.arange(L)
    if rule == "stretch":
        q = max(1, L // le)
        return np.minimum(tr // q, le - 1), 1, q
    return tr % le, 2, 1


# ------------------------------------------------------------------------------------------------ the gated block
class _Gated:
    """Inputs of one gated residual block's backward (64 padded channels, no biases unless `bias`), the launches of
    wn_resblock_bwd_pq / wn_resblock_bwd_ms on them and the float64 reference of include/wavenet_hip.h's formulas.
    hand: 'last' (p_in = NULL), 'pair' (p_in below p_lo = NaN, q_in zero beyond t_hi) or 'whole' (q_in = NULL).
    clip_pairs: the B clips are those of a model with <= 32 channels, two side by side per launch item (dz_half_stride != 0,
    block-diagonal packs, the second clip's dz-crop rows in a slice of their own); the reference stays B single clips."""

    def __init__(self, B, R, D, d, t_lo, t_hi, z_lo, hand, dn=0, p_lo=None, seed=0, sat=False, cond=None, bias=False,
                 clip_pairs=False):
        assert t_lo >= d + 1 and t_lo <= z_lo < t_hi and hand in ("last", "pair", "whole")
        assert not clip_pairs or (B % 2 == 0 and R <= 32 and D <= 32 and cond is None and not bias)
        self.pairs = clip_pairs
        self.C = C = 32 if clip_pairs else CH                    # rows of one clip's tensors
        self.nb = B // 2 if clip_pairs else B                    # `batch` of the launch
        self.ZR = ZR = 48 if clip_pairs else CH                  # rows of one clip's dz slice (pairs: more than the 32 the kernel reads)
        self.B, self.R, self.D, self.d, self.t_lo, self.t_hi, self.z_lo, self.hand = B, R, D, d, t_lo, t_hi, z_lo, hand
        self.dn = dn if hand == "pair" else 0
        self.p_lo = t_lo if p_lo is None else p_lo
        self.pitch = pitch = ((t_hi + max(d, dn) + 32 + 255) // 256) * 256 + 256
        rng = np.random.default_rng(seed)
        self.wf = (rng.standard_normal((D, R, 2)) * 0.3).astype(np.float32)
        self.wg = (rng.standard_normal((D, R, 2)) * 0.3).astype(np.float32)
        self.wd = (rng.standard_normal((R, D, 1)) * 0.3).astype(np.float32)
        self.pfg, wfg = _fg_pack(self.wf, self.wg, C, MF)
        wdT = np.zeros((C, C), np.float32)
        wdT[:D, :R] = self.wd[:, :, 0].T
        wpq = np.zeros((2 * C, 2 * C), np.float32)               # rows [0, C) = W1^T (-> P), [C, 2C) = W0^T (-> Q), K = (df | dg)
        for h, src in enumerate((self.wf, self.wg)):
            wpq[:R, h * C:h * C + D] = src[:, :, 1].T
            wpq[C:C + R, h * C:h * C + D] = src[:, :, 0].T
        if clip_pairs:
            self.pfg = _packed(_diag(wfg, 2, 2), MF)
            wdT, wpq = _diag(wdT, 1, 1), _diag(wpq, 2, 2)
        self.pdT = _packed(wdT, MB)
        self.ppq = _packed(wpq, MB)
        self.x = _buf(B, C, pitch, 1.0, 100 + seed)
        xv = _view(self.x, B, C, pitch)
        xv[:, R:] = 0                                            # padded channels are zero by contract
        if sat:                                                  # pre-activations of +-40 .. +-90 in a few columns
            for k, col in enumerate((t_lo - d + 1, t_lo + 2, (t_lo + t_hi) // 2, t_hi - 3)):
                xv[:, :, col] *= 4.0 + 1.5 * k
        self.dz = _buf(B, ZR, pitch, 1e-3, 200 + seed)
        zv = _view(self.dz, B, ZR, pitch)
        zv[:, D:] = 0
        zv[:, :, :z_lo] = NAN                                    # the crop counts from z_lo on
        self.p_in = self.q_in = None
        self.gy = None
        if hand != "last":
            self.p_in = _buf(B, C, pitch, 1e-3, 300 + seed)
            pv = _view(self.p_in, B, C, pitch)
            pv[:, R:] = 0
            pv[:, :, :self.p_lo] = NAN                           # rows of p_in below p_lo count as zero
            ts = torch.arange(t_lo, t_hi)
            gy = torch.nan_to_num(pv.cpu()[:, :R, t_lo:t_hi].double(), nan=0.0) * (ts >= self.p_lo)
            if hand == "pair":
                self.q_in = _buf(B, C, pitch, 1e-3, 400 + seed)
                qv = _view(self.q_in, B, C, pitch)
                qv[:, R:] = 0
                qv[:, :, t_hi:] = 0                              # q buffers read as zero beyond t_hi
                gy = gy + qv.cpu()[:, :R, t_lo + dn:t_hi + dn].double()
            self.gy = gy
        self.bias = None
        if bias:
            self.bias = [torch.zeros(CH, device=DEV), torch.zeros(CH, device=DEV)]
            for b_ in self.bias:
                b_[:D] = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(DEV)
        self.cond = None
        if cond is not None:
            le, rule = cond
            idx, mode, q = _buckets(t_hi - t_lo, le, rule)
            self.cond = dict(le=le, mode=mode, q=q, idx=torch.from_numpy(idx).long())
            tab = torch.zeros(B, 2 * CH, le)
            g_ = torch.Generator().manual_seed(500 + seed)
            tab[:, :D] = torch.randn(B, D, le, generator=g_) * 0.5
            tab[:, CH:CH + D] = torch.randn(B, D, le, generator=g_) * 0.5
            self.tab = tab.to(DEV).contiguous()
            cidx = torch.zeros(_lib.COND_IDX_PAD + (t_hi - t_lo) + 64, dtype=torch.uint8)
            cidx[_lib.COND_IDX_PAD:_lib.COND_IDX_PAD + (t_hi - t_lo)] = torch.from_numpy(idx.astype(np.uint8))
            self.cidx = cidx.to(DEV)

    # -------- float64 reference
    def reference(self):
        B, R, D, d, t_lo, t_hi, z_lo = self.B, self.R, self.D, self.d, self.t_lo, self.t_hi, self.z_lo
        x = _view(self.x, B, self.C, self.pitch).cpu()[:, :R, t_lo - d:t_hi].double().requires_grad_(True)
        twf, twg, twd = (torch.from_numpy(a).double().requires_grad_(True) for a in (self.wf, self.wg, self.wd))
        tab = None
        if self.cond is None and self.bias is None:
            f, g, z, y = _res_ref(x, twf, twg, twd, d)
        else:
            f = F.conv1d(x, twf, dilation=d)
            g = F.conv1d(x, twg, dilation=d)
            if self.bias is not None:
                f = f + self.bias[0].cpu().double()[None, :D, None]
                g = g + self.bias[1].cpu().double()[None, :D, None]
            if self.cond is not None:
                tab = self.tab.cpu().double().requires_grad_(True)
                f = f + tab[:, :D][:, :, self.cond["idx"]]
                g = g + tab[:, CH:CH + D][:, :, self.cond["idx"]]
            z = torch.tanh(f) * torch.sigmoid(g)
            y = F.conv1d(z, twd) + x[:, :, d:]
        f.retain_grad()
        g.retain_grad()
        gz = torch.zeros_like(z)
        gz[:, :, z_lo - t_lo:] = _view(self.dz, B, self.ZR, self.pitch).cpu()[:, :D, z_lo:t_hi].double()
        loss = (z * gz).sum()
        if self.gy is not None:
            loss = loss + (y * self.gy).sum()
        loss.backward()
        gf, gg = f.grad, g.grad
        wf64, wg64 = torch.from_numpy(self.wf).double(), torch.from_numpy(self.wg).double()
        P = torch.einsum("dr,bdt->brt", wf64[:, :, 1], gf) + torch.einsum("dr,bdt->brt", wg64[:, :, 1], gg)
        if self.gy is not None:
            P = P + self.gy
        Q = torch.einsum("dr,bdt->brt", wf64[:, :, 0], gf) + torch.einsum("dr,bdt->brt", wg64[:, :, 0], gg)
        return dict(dx=x.grad, gwf=twf.grad, gwg=twg.grad, gwd=twd.grad if self.gy is not None else None, gf=gf, gg=gg, P=P, Q=Q,
                    gtab=tab.grad if tab is not None else None)

    # -------- launches
    def launch_pq(self, chain):
        """one wn_resblock_bwd_pq launch into NaN-filled outputs and slabs (a conditioned block: its bucket-sum slabs too)"""
        B, C, nb, pitch, t_lo, t_hi = self.B, self.C, self.nb, self.pitch, self.t_lo, self.t_hi
        p_out, q_out = _nanbuf(B, C, pitch), _nanbuf(B, C, pitch)
        ns = _lib.pq_slabs(t_lo, t_hi, nb, self.d, chain)
        slab_fg = torch.full((ns * 4 * CH * CH,), NAN, device=DEV)
        slab_d = torch.full((ns * CH * CH,), NAN, device=DEV) if self.p_in is not None else None
        c = self.cond
        cslab = torch.full((_lib.load().wn_resblock_bwd_pq_cond_floats(t_lo, t_hi, nb),), NAN, device=DEV) if c else None
        call("wn_resblock_bwd_pq", ptr(self.x, SLACK), ptr(self.p_in, SLACK) if self.p_in is not None else None,
             ptr(self.q_in, SLACK) if self.q_in is not None else None, self.dn, self.p_lo, ptr(self.dz, SLACK), ptr(p_out, SLACK),
             ptr(q_out, SLACK), CH * pitch, (2 if self.pairs else 1) * self.ZR * pitch, pitch, ptr(self.pfg), ptr(self.pdT), ptr(self.ppq),
             CH, self.d, t_lo, t_hi, self.z_lo, ptr(slab_fg), ptr(slab_d), ptr(self.tab) if c else None, 2 * CH * c["le"] if c else 0,
             c["le"] if c else 0, c["le"] if c else 0, ptr(self.cidx) if c else None, ptr(cslab), self.ZR * pitch if self.pairs else 0,
             1 if chain else 0, nb, MF, MB, _lib.stream())
        torch.cuda.synchronize()
        Wfg = _reduce(slab_fg, ns, 2 * CH, 2 * CH)
        Wd = _reduce(slab_d, ns, CH, CH) if slab_d is not None else None
        if self.pairs:                                           # the two diagonal copies of every weight, added by wn_gather_grads2
            Wfg = _fold_pair(Wfg, 2, 2)
            Wd = _fold_pair(Wd, 1, 1) if Wd is not None else None
        return dict(p_raw=p_out.cpu(), q_raw=q_out.cpu(), P=_view(p_out, B, C, pitch).cpu(), Q=_view(q_out, B, C, pitch).cpu(),
                    slab_fg=slab_fg.cpu(), slab_d=slab_d.cpu() if slab_d is not None else None, ns=ns, Wfg=Wfg, Wd=Wd,
                    cslab=cslab.cpu() if c else None, cslab_dev=cslab, p_dev=p_out, q_dev=q_out)

    def dy_plain(self, seed=7):
        """dx_{i+1} as the ONE float32 tensor the other block kernels take: the pair summed as the kernel sums it (fp32),
        finite junk outside [t_lo, t_hi)"""
        B, pitch, t_lo, t_hi = self.B, self.pitch, self.t_lo, self.t_hi
        dy = _buf(B, CH, pitch, 1e-3, 900 + seed)
        ts = torch.arange(t_lo, t_hi)
        v = torch.nan_to_num(_view(self.p_in, B, CH, pitch).cpu()[:, :, t_lo:t_hi], nan=0.0) * (ts >= self.p_lo).float()
        if self.q_in is not None:
            v = v + _view(self.q_in, B, CH, pitch).cpu()[:, :, t_lo + self.dn:t_hi + self.dn]
        _view(dy, B, CH, pitch)[:, :, t_lo:t_hi] = v.to(DEV)
        return dy

    def launch_ms(self):
        assert not self.pairs
        B, pitch, t_lo, t_hi = self.B, self.pitch, self.t_lo, self.t_hi
        dfg = _nanbuf(B, 2 * CH, pitch)
        dy = self.dy_plain() if self.p_in is not None else None
        ns = _lib.ms_slabs(t_lo, t_hi, B)
        slab_fg = torch.full((ns * 4 * CH * CH,), NAN, device=DEV)
        slab_d = torch.full((ns * CH * CH,), NAN, device=DEV) if dy is not None else None
        c = self.cond
        call("wn_resblock_bwd_ms", ptr(self.x, SLACK), ptr(dy, SLACK) if dy is not None else None, ptr(self.dz, SLACK), ptr(dfg, SLACK),
             CH * pitch, CH * pitch, 2 * CH * pitch, pitch, ptr(self.pfg), ptr(self.pdT),
             ptr(self.bias[0]) if self.bias else None, ptr(self.bias[1]) if self.bias else None, self.D, CH, self.d, t_lo, t_hi,
             self.z_lo, ptr(slab_fg), ptr(slab_d), ptr(self.tab) if c else None, 2 * CH * c["le"] if c else 0, c["le"] if c else 0,
             c["mode"] if c else 0, c["le"] if c else 0, c["q"] if c else 0, B, MF, MB, _lib.stream())
        torch.cuda.synchronize()
        return dict(dfg_dev=dfg, dfg_raw=dfg.cpu(), dfg=_view(dfg, B, 2 * CH, pitch).cpu(), dy=dy, ns=ns, slab_fg=slab_fg.cpu(),
                    slab_d=slab_d.cpu() if slab_d is not None else None, Wfg=_reduce(slab_fg, ns, 2 * CH, 2 * CH),
                    Wd=_reduce(slab_d, ns, CH, CH) if slab_d is not None else None)

    def shift_add(self, o):
        """wn_shift_add of a pair-form launch's (P, Q): dx whole on [t_lo - d, t_hi); equal to the float32 expression"""
        B, C, pitch, t_lo, t_hi, d = self.B, self.C, self.pitch, self.t_lo, self.t_hi, self.d
        out = _nanbuf(B, C, pitch)
        call("wn_shift_add", ptr(o["p_dev"], SLACK), ptr(o["q_dev"], SLACK), ptr(out, SLACK), C * pitch, pitch, C, d, t_lo, t_lo - d,
             t_hi, B, _lib.stream())
        torch.cuda.synchronize()
        assert _written(out) == B * C * (t_hi - t_lo + d), "wn_shift_add wrote outside [t_lo - d, t_hi)"
        got = _view(out, B, C, pitch).cpu()[:, :, t_lo - d:t_hi]
        ts = torch.arange(t_lo - d, t_hi)
        zero = torch.zeros(())
        want = torch.where(ts >= t_lo, o["P"][:, :, t_lo - d:t_hi], zero) + torch.where(ts + d < t_hi, o["Q"][:, :, t_lo:t_hi + d], zero)
        assert torch.equal(got, want), "wn_shift_add differs from p[t] (t >= p_lo) + q[t + dn] (t + dn < t_hi) in float32"
        return got

    # -------- comparisons
    def check_wgrads(self, o, ref, tag):
        R, D, C = self.R, self.D, self.C
        assert not torch.isnan(o["slab_fg"]).any(), tag + ": a slab_fg element was not overwritten (or is NaN)"
        W = o["Wfg"].double()
        errs = {}
        for name, r0, gw in (("dWf", 0, ref["gwf"]), ("dWg", C, ref["gwg"])):
            got = torch.cat([W[r0:r0 + D, :R], W[r0:r0 + D, C:C + R]], 1)
            errs[name] = _rel(got, torch.cat([gw[:, :, 0], gw[:, :, 1]], 1))
        keep = torch.zeros(2 * C, 2 * C, dtype=torch.bool)
        for r0 in (0, C):
            for c0 in (0, C):
                keep[r0:r0 + D, c0:c0 + R] = True
        assert _all_zero(W[~keep]), tag + ": padded rows / columns of dWfg are not exactly 0"
        if ref["gwd"] is not None:
            assert not torch.isnan(o["slab_d"]).any(), tag + ": a slab_d element was not overwritten (or is NaN)"
            Wd = o["Wd"].double()
            errs["dWd"] = _rel(Wd[:R, :D], ref["gwd"][:, :, 0])
            assert _all_zero(Wd[R:]) and _all_zero(Wd[:, D:]), tag + ": padded rows / columns of dWd are not exactly 0"
        return errs

    def check_pq(self, o, ref, chain, tag):
        """one wn_resblock_bwd_pq launch against float64 + its write windows; returns the errors"""
        B, C, R, d, t_lo, t_hi = self.B, self.C, self.R, self.d, self.t_lo, self.t_hi
        errs = self.check_wgrads(o, ref, tag)
        if chain:
            assert _written(o["q_raw"]) == 0, tag + ": the chain form touched q_out"
            assert _written(o["p_raw"]) == B * C * (t_hi - t_lo + d), tag + ": p_out written outside [t_lo - d, t_hi) (or NaN inside)"
            dx = o["P"][:, :, t_lo - d:t_hi]
        else:
            assert _written(o["p_raw"]) == B * C * (t_hi - t_lo), tag + ": p_out written outside [t_lo, t_hi) (or NaN inside)"
            assert _written(o["q_raw"]) == B * C * (t_hi - t_lo), tag + ": q_out written outside [t_lo, t_hi) (or NaN inside)"
            errs["P"] = _rel(o["P"][:, :R, t_lo:t_hi], ref["P"])
            errs["Q"] = _rel(o["Q"][:, :R, t_lo:t_hi], ref["Q"])
            assert _all_zero(o["P"][:, R:, t_lo:t_hi]) and _all_zero(o["Q"][:, R:, t_lo:t_hi]), tag + ": padded rows of P / Q not 0"
            dx = self.shift_add(o)
        errs["dx"] = _rel(dx[:, :R], ref["dx"])
        assert _all_zero(dx[:, R:]), tag + ": padded rows of dx are not exactly 0"
        print(tag, " ".join("%s %.2e" % kv for kv in errs.items()))
        assert all(torch.isfinite(torch.tensor(v)) and v <= BAR64 for v in errs.values()), (tag, errs)
        return errs, dx

    def run_pq(self, chain, tag, ref=None):
        """launch, check against float64, launch again: same bits"""
        ref = self.reference() if ref is None else ref
        o = self.launch_pq(chain)
        errs, dx = self.check_pq(o, ref, chain, tag)
        o2 = self.launch_pq(chain)
        for k in ("p_raw", "q_raw", "slab_fg", "slab_d", "cslab", "Wfg", "Wd"):
            assert o[k] is None or _same_bits(o[k], o2[k]), tag + ": a second launch does not reproduce the bits of " + k
        return o, dx, ref


def _inst(hand, chain, cond=False):
    """the template instantiation <HAS_DY, COND, QIN, CHAIN> of resblock_bwd_pq_k a case reaches (wn_respq.hip's dispatch)"""
    return "HAS_DY%d-COND%d-QIN%d-CHAIN%d" % (hand != "last", cond, hand != "whole", chain)


# The six unconditioned instantiations.  Observed worst against float64 over this test and the geometry, chain-regime,
# saturated-gate and clip-pair tests below (bar BAR64 = 1e-4):
#   P 1.7e-5, Q 1.5e-5, dx 1.4e-5, dWf 1.4e-5, dWg 1.1e-5, dWd 7.0e-6
@pytest.mark.parametrize("hand,chain", [(h, c) for h in ("last", "pair", "whole") for c in (0, 1)],
                         ids=[_inst(h, c) for h in ("last", "pair", "whole") for c in (0, 1)])
def test_pq_every_unconditioned_instantiation(hand, chain):
    """wn_resblock_bwd_pq: {last block, pair in, whole in} x {pair out, chain out}: P, Q (pair out), dx, dWf, dWg, dWd against
    float64; wn_shift_add(P, Q) exact and against dx; write windows; a second launch reproduces the bits."""
    c = _Gated(B=2, R=64, D=64, d=64, t_lo=64 + 37, t_hi=1499, z_lo=64 + 37 + 301, hand=hand, dn=32, p_lo=64 + 37 + 9, seed=1)
    if chain:
        assert _lib.pq_chain_ok(c.t_lo, c.t_hi, c.B, c.d)
    c.run_pq(chain, _inst(hand, chain))


def _geometry():
    """t_lo at 0, 1, 31, 32, 33, 63 modulo 64 x spans of one 32-column item, one less, one more and a long one whose t_hi is no
    multiple of 4 x {pair out, chain out} x {pair in, whole in, last block}.  Inside every (hand, output form) the offsets below
    cycle with (alignment + span), so p_lo > t_lo, z_lo > t_lo by a non-multiple of 32 and z_lo = t_lo each meet every hand in
    both forms at the one-item spans; dn != d, batch 1 and 3, 48 / 40 real channels."""
    out = []
    for ir, res in enumerate((0, 1, 31, 32, 33, 63)):
        for iw, width in enumerate((31, 32, 33, 1203)):
            for chain in (0, 1):
                for ih, hand in enumerate(("pair", "whole", "last")):
                    n = ir + iw
                    d = ((32, 64)[n % 2] if width > 100 else 32) if chain else (3, 7, 32, 50)[(n + ih) % 4]
                    dn = (5, 64, 2, 96)[n % 4]
                    dn += int(dn == d)
                    t_lo = 64 * ((d + 3 + 63) // 64) + res
                    p_off = min((5, 40, 0)[n % 3], width // 2)
                    z_off = min((13, 0, 45)[(ir + 2 * iw) % 3], width // 2)
                    B = (1, 3)[(ir + ih) % 2]
                    R, D = ((64, 64), (48, 40))[(iw + ih + chain) % 2]
                    out.append(pytest.param(B, R, D, d, dn, t_lo, t_lo + width, t_lo + p_off, t_lo + z_off, hand, chain,
                                            id="tlo%d-w%d-d%d-plo%d-%s" % (t_lo, width, d, p_off, _inst(hand, chain))))
    return out


# (observed errors: above test_pq_every_unconditioned_instantiation; every case prints its own figures with -s)
@pytest.mark.parametrize("B,R,D,d,dn,t_lo,t_hi,p_lo,z_lo,hand,chain", _geometry())
def test_pq_hostile_geometry(B, R, D, d, dn, t_lo, t_hi, p_lo, z_lo, hand, chain):
    assert dn != d and t_lo >= d + 3
    c = _Gated(B=B, R=R, D=D, d=d, t_lo=t_lo, t_hi=t_hi, z_lo=z_lo, hand=hand, dn=dn, p_lo=p_lo, seed=t_lo + t_hi)
    if chain:
        assert _lib.pq_chain_ok(t_lo, t_hi, B, d)
    c.run_pq(chain, "tlo%d thi%d d%d %s" % (t_lo, t_hi, d, _inst(hand, chain)))


# The regimes of the chain plan, asserted on the host view of the plan so that they cannot rot.  Chain against pair form,
# observed worst 2.0e-7 of max-abs (bar BARFORM = 2e-5); chains of one item and whole chains of a 'last' block: identical
@pytest.mark.parametrize("regime,B,d,t_lo,t_hi,hand", [
    ("s1_segments", 2, 32, 32 + 5, 1500, "pair"),               # d = 32: one residue class; 2 chains cut into segments with halo items
    ("one_item_chains", 3, 512, 515, 1021, "whole"),            # exactly d / 32 = 16 items: the chain_ok boundary
    ("unequal_chains", 3, 64, 70, 64 + 32 * 21 - 5, "pair"),    # 21 items in 2 residue classes: chains of 11 and 10, in segments
    ("whole_chains", 16, 512, 520, 1120, "last"),               # 16 x 16 = 256 chains: a workgroup takes whole chains
    ("whole_chains_dy", 16, 512, 520, 1120, "pair"),
], ids=lambda v: v if isinstance(v, str) and "_" in v else None)
def test_pq_chain_plan_regimes(regime, B, d, t_lo, t_hi, hand):
    assert _lib.pq_chain_ok(t_lo, t_hi, B, d)
    plan = _chain_plan(t_lo, t_hi, B, d)
    items = [it for wg in plan for it in wg]
    halos = [it for it in items if it[2] & 1]
    t_base, s = t_lo & ~31, d // 32
    steps = (t_hi - t_base + 31) // 32
    lens = {}
    for b, t0, fl in items:
        if not fl & 1:
            lens[(b, ((t0 - t_base) // 32) % s)] = lens.get((b, ((t0 - t_base) // 32) % s), 0) + 1
    assert sum(lens.values()) == B * steps and len(lens) == B * s
    if regime == "s1_segments":
        assert s == 1 and B * s < 256 and len(plan) >= 2 * B * s and len(halos) == len(plan) - B * s and halos
    elif regime == "one_item_chains":
        assert steps == s and not _chain_ok_one_item_less(t_lo, t_hi, B, d) and all(fl == 6 for _, _, fl in items)
    elif regime == "unequal_chains":
        assert steps % s != 0 and len(set(lens.values())) == 2 and B * s < 256 and halos
    else:
        assert B * s >= 256 and len(plan) == 256 and not halos
    c = _Gated(B=B, R=64, D=64, d=d, t_lo=t_lo, t_hi=t_hi, z_lo=t_lo + 45, hand=hand, dn=96, p_lo=t_lo + 3, seed=len(regime))
    o_c, dx_c, ref = c.run_pq(1, regime + " " + _inst(hand, 1))
    o_p, dx_p, _ = c.run_pq(0, regime + " " + _inst(hand, 0), ref)
    # chain form against pair form of the same case: the project's form-against-form bar
    devs = {"dx": (dx_c.double() - dx_p.double()).abs().max().item() / dx_p.abs().max().item(),
            "dWfg": (o_c["Wfg"].double() - o_p["Wfg"].double()).abs().max().item() / o_p["Wfg"].abs().max().item()}
    if o_p["Wd"] is not None:
        devs["dWd"] = (o_c["Wd"].double() - o_p["Wd"].double()).abs().max().item() / o_p["Wd"].abs().max().item()
    print(regime, "chain vs pair", devs)
    assert all(v <= BARFORM for v in devs.values()), devs


# Saturated gates, one launch
@pytest.mark.parametrize("hand,chain", [("pair", 0), ("pair", 1), ("last", 0), ("whole", 1)],
                         ids=[_inst(h, c) for h, c in (("pair", 0), ("pair", 1), ("last", 0), ("whole", 1))])
def test_pq_saturated_gates(hand, chain):
    """f, g pre-activations of +-40 .. +-90 in a few columns: every output finite and within the bar (a saturated gate must give
    a zero derivative, not inf * 0)."""
    c = _Gated(B=2, R=64, D=64, d=32, t_lo=32 + 9, t_hi=1107, z_lo=32 + 9, hand=hand, dn=64, seed=9, sat=True)
    ref = c.reference()
    pre = max(F.conv1d(_view(c.x, 2, CH, c.pitch).cpu()[:, :, c.t_lo - 32:c.t_hi].double(), torch.from_numpy(w).double(), dilation=32)
              .abs().max().item() for w in (c.wf, c.wg))
    print("largest pre-activation %.1f" % pre)
    assert 40.0 <= pre <= 90.0, "the case does not saturate its gates as meant"
    o, dx, _ = c.run_pq(chain, "saturated " + _inst(hand, chain), ref)
    assert torch.isfinite(dx).all() and torch.isfinite(o["Wfg"]).all()


# wn_resblock_bwd_ms against float64, each tensor by its own max-abs; observed worst: df 5.6e-6, dg 6.3e-6, dWf 7.9e-6, dWg 6.9e-6, dWd 4.4e-6 (bar 1e-4);
# the fused launch against bwd_ms + GEMM: 3.2e-7 (bar 2e-5)
@pytest.mark.parametrize("variant", ["plain", "bias", "last", "cond_stretch", "cond_tile", "bias_cond_tile"])
@pytest.mark.parametrize("R,D,B", [(64, 64, 2), (48, 40, 3)])
def test_bwd_ms_against_float64(variant, R, D, B):
    """wn_resblock_bwd_ms: [df; dg], dWf, dWg, dWd against float64 - with and without biases, dy = NULL, a conditioning table in
    modes 1 and 2; writes stay in [t_lo, t_hi); a second launch reproduces the bits; and (plain) the data gradient that one
    wn_chan_gemm makes of its dfg against wn_resblock_bwd_pq's P, Q on the same inputs."""
    d, t_lo, t_hi = 5, 64 + 33, 64 + 33 + 1203
    cond = (7, "stretch") if "stretch" in variant else (31, "tile") if "tile" in variant else None
    c = _Gated(B=B, R=R, D=D, d=d, t_lo=t_lo, t_hi=t_hi, z_lo=t_lo + 45, hand="last" if variant == "last" else "pair", dn=3,
               p_lo=t_lo + 5, seed=17, cond=cond, bias="bias" in variant)
    ref = c.reference()
    o = c.launch_ms()
    tag = "bwd_ms %s R%d D%d" % (variant, R, D)
    errs = c.check_wgrads(o, ref, tag)
    errs["df"] = _rel(o["dfg"][:, :D, t_lo:t_hi], ref["gf"])
    errs["dg"] = _rel(o["dfg"][:, CH:CH + D, t_lo:t_hi], ref["gg"])
    print(tag, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v <= BAR64 for v in errs.values()), errs
    # the kernel writes all 2 x 64 rows of [df; dg] on [t_lo, t_hi) (the GEMM behind it reads them all): padded rows exactly 0
    assert _all_zero(o["dfg"][:, D:CH, t_lo:t_hi]) and _all_zero(o["dfg"][:, CH + D:, t_lo:t_hi]), tag + ": padded rows of [df; dg] not 0"
    assert not torch.isnan(o["dfg"][:, :, t_lo:t_hi]).any()
    assert _written(o["dfg_raw"]) == B * 2 * CH * (t_hi - t_lo), tag + ": dfg written outside [t_lo, t_hi)"
    o2 = c.launch_ms()
    for k in ("dfg_raw", "slab_fg", "slab_d", "Wfg", "Wd"):
        assert o[k] is None or _same_bits(o[k], o2[k]), tag + ": a second launch does not reproduce the bits of " + k
    if variant == "plain":
        # P = W1^T [df;dg] + dy, Q = W0^T [df;dg] by one wn_chan_gemm on dfg, against the fused launch's (P, Q)
        pitch = c.pitch
        pq = _nanbuf(B, 2 * CH, pitch)
        dfg = o["dfg_dev"]                                       # NaN outside [t_lo, t_hi): in_lo / in_hi keep the GEMM off it
        call("wn_chan_gemm", ptr(dfg, SLACK), None, 2 * CH * pitch, pitch, t_lo, t_hi, 0, 0, 2 * CH // 32, 0, ptr(c.ppq), 2 * CH // 16,
             2 * CH, ptr(pq, SLACK), 2 * CH * pitch, pitch, 0, None, None, 0, 0, 0, None, 0, 0, t_lo, t_hi, 0, B, MB, _lib.stream())
        torch.cuda.synchronize()
        g = _view(pq, B, 2 * CH, pitch).cpu()
        of = c.launch_pq(0)
        P2 = g[:, :CH, t_lo:t_hi] + _view(o["dy"], B, CH, pitch).cpu()[:, :, t_lo:t_hi]
        devs = {"P": (P2.double() - of["P"][:, :, t_lo:t_hi].double()).abs().max().item() / ref["P"].abs().max().item(),
                "Q": (g[:, CH:, t_lo:t_hi].double() - of["Q"][:, :, t_lo:t_hi].double()).abs().max().item() / ref["Q"].abs().max().item(),
                "dWfg": (of["Wfg"].double() - o["Wfg"].double()).abs().max().item() / o["Wfg"].abs().max().item(),
                "dWd": (of["Wd"].double() - o["Wd"].double()).abs().max().item() / o["Wd"].abs().max().item()}
        print(tag, "fused vs bwd_ms + GEMM", devs)
        assert all(v <= BARFORM for v in devs.values()), devs


# The conditioned block.  Observed worst: P 1.1e-5, Q 1.2e-5, dx 9.7e-6, dWf 8.2e-6, dWg 7.3e-6, dWd 4.5e-6, d cond 7.5e-6 against float64 (bar 1e-4);
# d cond against wn_cond_grad on bwd_ms's [df; dg] 4.2e-6 (bar 2e-5)
@pytest.mark.parametrize("le", [1, 5, 31, 32])
@pytest.mark.parametrize("rule", ["stretch", "tile"])
@pytest.mark.parametrize("has_dy", [0, 1], ids=[_inst("last", 0, True), _inst("pair", 0, True)])
def test_pq_conditioned_block(le, rule, has_dy):
    """The conditioned form of wn_resblock_bwd_pq (table column bucket(t) added to [f; g], buckets as bytes): P, Q, dx, the weight
    gradients and - through cslab and ONE wn_resblock_bwd_pq_cond_reduce over two launches with different t_lo - d cond against
    float64 autograd, and against wn_cond_grad on the [df; dg] wn_resblock_bwd_ms writes for the same inputs.  Each block launch
    runs twice into NaN-filled outputs and slabs: same bits in P, Q, both weight-gradient slabs and cslab."""
    B, t_hi = 3, 1400
    hand = "pair" if has_dy else "last"
    cases = [_Gated(B=B, R=48, D=40, d=d, t_lo=t_lo, t_hi=t_hi, z_lo=t_lo + 13, hand=hand, dn=7, p_lo=t_lo + 5, seed=31 + t_lo,
                    cond=(le, rule)) for d, t_lo in ((4, 64 + 31), (9, 128 + 5))]
    refs, outs = [], []
    for c in cases:
        o, _, ref = c.run_pq(0, "cond le%d %s t_lo%d %s" % (le, rule, c.t_lo, _inst(hand, 0, True)))      # (launched twice: same bits, cslab included)
        refs.append(ref)
        outs.append(o)
    cslab = torch.cat([o["cslab_dev"] for o in outs])            # the two launches' regions, as one reduce takes them
    offs = [0, outs[0]["cslab_dev"].numel()]

    def reduce():
        out = torch.full((2, B, 2 * CH, le), NAN, device=DEV)
        call("wn_resblock_bwd_pq_cond_reduce", ptr(cslab), (ctypes.c_int64 * 2)(*offs), (ctypes.c_int * 2)(*[c.t_lo for c in cases]), 2,
             t_hi, B, le, ptr(out), B * 2 * CH * le, 2 * CH * le, le, _lib.stream())
        torch.cuda.synchronize()
        return out.cpu()
    got = reduce()
    assert torch.equal(got, reduce())
    for l, (c, ref) in enumerate(zip(cases, refs)):
        D = c.D
        e = _rel(got[l], ref["gtab"])
        keep = torch.zeros(2 * CH, dtype=torch.bool)
        keep[:D] = keep[CH:CH + D] = True
        assert _all_zero(got[l][:, ~keep])
        # ... and the unfused route: wn_resblock_bwd_ms's [df; dg] -> wn_cond_grad
        m = c.launch_ms()
        cg = torch.full((B, 2 * CH, le), NAN, device=DEV)
        dfg = m["dfg_dev"]
        call("wn_cond_grad", ptr(dfg, SLACK), 2 * CH * c.pitch, c.pitch, 2 * CH, c.t_lo, t_hi, c.cond["mode"], le, c.cond["q"], ptr(cg),
             2 * CH * le, le, B, _lib.stream())
        torch.cuda.synchronize()
        dev = (got[l].double() - cg.cpu().double()).abs().max().item() / ref["gtab"].abs().max().item()
        print("d cond le%d %s launch %d: vs float64 %.2e, vs wn_cond_grad %.2e" % (le, rule, l, e, dev))
        assert e <= BAR64 and dev <= BARFORM


# ------------------------------------------------------------------------------------------------ the encoder block
class _Enc:
    """One encoder block (h = Wdil [relu x(t-d); relu x(t)], y = Wd relu(h) + x(t)); 64 padded channels for the backward."""

    def __init__(self, B, R, D, d, t_lo, t_hi, ch=CH, seed=0, bias=False, mode=MF):
        self.B, self.R, self.D, self.d, self.t_lo, self.t_hi, self.ch = B, R, D, d, t_lo, t_hi, ch
        self.pitch = pitch = ((t_hi + 2 * max(d, 64) + 32 + 255) // 256) * 256 + 256
        rng = np.random.default_rng(seed)
        self.wdil = (rng.standard_normal((D, R, 2)) * 0.2).astype(np.float32)
        self.wd = (rng.standard_normal((R, D, 1)) * 0.2).astype(np.float32)
        w = np.zeros((ch, 2 * ch), np.float32)
        w[:D, :R], w[:D, ch:ch + R] = self.wdil[:, :, 0], self.wdil[:, :, 1]
        self.p_dil = _packed(w, mode)
        wdd = np.zeros((ch, ch), np.float32)
        wdd[:R, :D] = self.wd[:, :, 0]
        self.p_dc = _packed(wdd, mode, chained=True)
        self.p_dT = _packed(np.ascontiguousarray(wdd.T), MB)
        wq = np.zeros((2 * ch, ch), np.float32)                  # [W1^T; W0^T] over dh
        wq[:R, :D], wq[ch:ch + R, :D] = self.wdil[:, :, 1].T, self.wdil[:, :, 0].T
        self.p_pq = _packed(wq, MB)
        self.x = _buf(B, ch, pitch, 1.0, 100 + seed)
        _view(self.x, B, ch, pitch)[:, R:] = 0
        self.bias = None
        if bias:
            self.bias = [torch.zeros(ch, device=DEV), torch.zeros(ch, device=DEV)]
            self.bias[0][:D] = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(DEV)
            self.bias[1][:R] = torch.from_numpy(rng.standard_normal(R).astype(np.float32)).to(DEV)
        # the stored pre-activation the backward masks with: an INPUT of the backward kernels (any values; independent of x here)
        self.h = _buf(B, ch, pitch, 1.0, 600 + seed)
        _view(self.h, B, ch, pitch)[:, D:] = 0

    def hand(self, kind, dn, p_lo, seed=0):
        """dy as handed in: 'pair' (p_in NaN below p_lo, q_in zero beyond t_hi) or 'whole' (q_in = NULL)"""
        B, R, pitch, t_lo, t_hi = self.B, self.R, self.pitch, self.t_lo, self.t_hi
        self.p_lo, self.dn = p_lo, dn if kind == "pair" else 0
        self.p_in = _buf(B, CH, pitch, 1e-3, 300 + seed)
        pv = _view(self.p_in, B, CH, pitch)
        pv[:, R:] = 0
        pv[:, :, :p_lo] = NAN
        ts = torch.arange(t_lo, t_hi)
        gy = torch.nan_to_num(pv.cpu()[:, :R, t_lo:t_hi].double(), nan=0.0) * (ts >= p_lo)
        self.q_in = None
        if kind == "pair":
            self.q_in = _buf(B, CH, pitch, 1e-3, 400 + seed)
            qv = _view(self.q_in, B, CH, pitch)
            qv[:, R:] = 0
            qv[:, :, t_hi:] = 0
            gy = gy + qv.cpu()[:, :R, t_lo + dn:t_hi + dn].double()
        self.gy = gy

    def reference_bwd(self):
        """float64; the ReLU masks from the signs of the SAME float32 x and h the kernel reads (h is fed in, not recomputed)"""
        B, R, D, d, t_lo, t_hi = self.B, self.R, self.D, self.d, self.t_lo, self.t_hi
        x = _view(self.x, B, CH, self.pitch).cpu()[:, :R, t_lo - d:t_hi].double().requires_grad_(True)
        hh = _view(self.h, B, CH, self.pitch).cpu()[:, :D, t_lo:t_hi].double().requires_grad_(True)
        wdil, wd = (torch.from_numpy(a).double().requires_grad_(True) for a in (self.wdil, self.wd))
        y = F.conv1d(torch.relu(hh), wd) + x[:, :, d:]
        (y * self.gy).sum().backward()
        dh = hh.grad.clone()
        (F.conv1d(torch.relu(x), wdil, dilation=d) * dh).sum().backward()
        xm = (x.detach() > 0).double()
        w64 = torch.from_numpy(self.wdil).double()
        P = self.gy + xm[:, :, d:] * torch.einsum("dr,bdt->brt", w64[:, :, 1], dh)
        Q = xm[:, :, :-d] * torch.einsum("dr,bdt->brt", w64[:, :, 0], dh)
        return dict(dh=dh, gwdil=wdil.grad, gwd=wd.grad, dx=x.grad, P=P, Q=Q)

    def check_slabs(self, slab_dil, slab_d, ns, ref, tag):
        R, D = self.R, self.D
        assert not torch.isnan(slab_dil).any() and not torch.isnan(slab_d).any(), tag + ": a slab element was not overwritten (or is NaN)"
        W = _reduce(slab_dil, ns, CH, 2 * CH).double()
        Wd = _reduce(slab_d, ns, CH, CH).double()
        errs = {"dWdil": _rel(torch.cat([W[:D, :R], W[:D, CH:CH + R]], 1), torch.cat([ref["gwdil"][:, :, 0], ref["gwdil"][:, :, 1]], 1)),
                "dWd": _rel(Wd[:R, :D], ref["gwd"][:, :, 0])}
        keep = torch.zeros(CH, 2 * CH, dtype=torch.bool)
        keep[:D, :R] = keep[:D, CH:CH + R] = True
        assert _all_zero(W[~keep]) and _all_zero(Wd[R:]) and _all_zero(Wd[:, D:]), tag + ": padded rows / columns of a slab sum not 0"
        return errs, W, Wd


# Encoder block, forward.  Observed worst: f16x3 x_out 2.6e-7, h 3.0e-7 (bar 1e-5); bf16x3 x_out 7.0e-6, h 5.8e-6 (bar 2e-4), of max(1, max-abs)
@pytest.mark.parametrize("mode", [MF, MB], ids=["f16x3", "bf16x3"])
@pytest.mark.parametrize("ch,R,D,d,bias", [(32, 32, 32, 1, False), (32, 20, 24, 3, True), (64, 64, 64, 32, False), (64, 48, 40, 5, True),
                                           (64, 64, 64, 512, True)])
def test_enc_resblock_fwd(ch, R, D, d, bias, mode):
    """wn_enc_resblock_fwd: x_out and the stored h against float64, biases on / off, real channels below the padding; nothing
    written outside [t_lo, t_hi); a second launch reproduces the bits."""
    B = 2
    t_lo = 64 * ((d + 3 + 63) // 64) + 33
    t_hi = t_lo + 1203
    e = _Enc(B, R, D, d, t_lo, t_hi, ch=ch, seed=d, bias=bias, mode=mode)
    pitch = e.pitch

    def run():
        xo, ho = _nanbuf(B, ch, pitch), _nanbuf(B, ch, pitch)
        call("wn_enc_resblock_fwd", ptr(e.x, SLACK), ptr(xo, SLACK), ptr(ho, SLACK), ch * pitch, ch * pitch, pitch, ptr(e.p_dil), ptr(e.p_dc),
             ptr(e.bias[0]) if bias else None, ptr(e.bias[1]) if bias else None, D, R, ch, d, t_lo, t_hi, B, mode, _lib.stream())
        torch.cuda.synchronize()
        return xo, ho
    xo, ho = run()
    x = _view(e.x, B, ch, pitch).cpu()[:, :R, t_lo - d:t_hi].double()
    h = F.conv1d(torch.relu(x), torch.from_numpy(e.wdil).double(), e.bias[0].cpu().double()[:D] if bias else None, dilation=d)
    y = F.conv1d(torch.relu(h), torch.from_numpy(e.wd).double(), e.bias[1].cpu().double()[:R] if bias else None) + x[:, :, d:]
    gx, gh = _view(xo, B, ch, pitch).cpu(), _view(ho, B, ch, pitch).cpu()
    ey = (gx[:, :R, t_lo:t_hi].double() - y).abs().max().item()
    eh = (gh[:, :D, t_lo:t_hi].double() - h).abs().max().item()
    print("enc fwd ch%d d%d mode %d: err x_out %.2e h %.2e, scales %.2f %.2f" % (ch, d, mode, ey, eh, y.abs().max().item(), h.abs().max().item()))
    tol = 1e-5 if mode == MF else 2e-4                          # the forward bar of test_resblock_fwd
    assert ey <= tol * max(1.0, y.abs().max().item()) and eh <= tol * max(1.0, h.abs().max().item())
    # the kernel writes all ch rows on [t_lo, t_hi) and nothing else: padded rows (zero weights, no bias) exactly 0
    for got, raw, rows in ((gx, xo, R), (gh, ho, D)):
        assert _all_zero(got[:, rows:, t_lo:t_hi]) and not torch.isnan(got[:, :, t_lo:t_hi]).any()
        assert _written(raw) == B * ch * (t_hi - t_lo)
    xo2, ho2 = run()
    assert _same_bits(xo, xo2) and _same_bits(ho, ho2), "a second launch does not reproduce the bits"


# Encoder block, backward without the data gradient.  Observed worst: dh 6.5e-6, dWdil 7.3e-6, dWd 5.1e-6 (bar 1e-4)
@pytest.mark.parametrize("R,D,B,d,y_off", [(64, 64, 2, 4, 0), (48, 40, 3, 7, 45), (64, 64, 1, 64, 301)])
def test_enc_resblock_bwd(R, D, B, d, y_off):
    """wn_enc_resblock_bwd: dh = (Wd^T dy) [h > 0] and both slab sums against float64; dy counts as 0 below y_lo > t_lo (NaN there)."""
    t_lo = 64 * ((d + 3 + 63) // 64) + 31
    t_hi = t_lo + 1203
    e = _Enc(B, R, D, d, t_lo, t_hi, seed=40 + d)
    e.hand("whole", 0, t_lo + y_off)
    ref = e.reference_bwd()
    pitch = e.pitch

    def run():
        dh = _nanbuf(B, CH, pitch)
        ns = _lib.enc_slabs(t_lo, t_hi, B)
        s1, s2 = torch.full((ns * 2 * CH * CH,), NAN, device=DEV), torch.full((ns * CH * CH,), NAN, device=DEV)
        call("wn_enc_resblock_bwd", ptr(e.x, SLACK), ptr(e.p_in, SLACK), ptr(e.h, SLACK), ptr(dh, SLACK), CH * pitch, CH * pitch, CH * pitch,
             pitch, ptr(e.p_dT), CH, d, t_lo, t_hi, t_lo + y_off, ptr(s1), ptr(s2), B, MB, _lib.stream())
        torch.cuda.synchronize()
        return dh, s1, s2, ns
    dh, s1, s2, ns = run()
    tag = "enc bwd R%d D%d d%d" % (R, D, d)
    errs, _, _ = e.check_slabs(s1, s2, ns, ref, tag)
    g = _view(dh, B, CH, pitch).cpu()
    errs["dh"] = _rel(g[:, :D, t_lo:t_hi], ref["dh"])
    print(tag, errs)
    assert all(v <= BAR64 for v in errs.values()), errs
    # all 64 rows of dh are written on [t_lo, t_hi) and nothing else: padded rows exactly 0
    assert _all_zero(g[:, D:, t_lo:t_hi]) and _written(dh) == B * CH * (t_hi - t_lo)
    dh2, s1b, s2b, _ = run()
    assert _same_bits(dh, dh2) and _same_bits(s1, s1b) and _same_bits(s2, s2b)


def _enc_pq_cases():
    out = []
    for kind in ("pair", "whole"):
        out += [pytest.param(0, 5, 64 + 33, 1203, kind, id="form0-d5-%s" % kind),
                pytest.param(0, 64, 128 + 1, 33, kind, id="form0-d64-w33-%s" % kind)]
        for d, t_lo, w in ((32, 64 + 31, 1203), (64, 128 + 63, 1500), (512, 515, 1021 - 515)):
            out.append(pytest.param(1, d, t_lo, w, kind, id="form1-d%d-%s" % (d, kind)))
        # form 2: d < 32; a clip of a single item; t_lo - d in the 32-column tile below t_lo's
        for d, t_lo, w in ((1, 64 + 1, 1203), (2, 64 + 40, 20), (5, 64 + 3, 1203), (16, 64 + 32, 31), (31, 96 + 30, 1203)):
            out.append(pytest.param(2, d, t_lo, w, kind, id="form2-d%d-tlo%d-w%d-%s" % (d, t_lo, w, kind)))
    return out


# Encoder block, the whole backward in one launch.  Observed worst over the three forms: P 6.5e-6, Q 9.2e-6, dx 7.7e-6, dWdil 9.8e-6, dWd 8.4e-6 (bar 1e-4)
@pytest.mark.parametrize("form,d,t_lo,width,kind", _enc_pq_cases())
def test_enc_resblock_bwd_pq(form, d, t_lo, width, kind):
    """wn_enc_resblock_bwd_pq, forms 0 (pair out), 1 (chain, d % 32 == 0) and 2 (LDS hand-over, d < 32), pair in and whole in:
    P, Q (form 0), dx, dWdil, dWd against float64; write windows; repeated launch."""
    B, R, D = (3, 48, 40) if (d + t_lo) % 2 else (2, 64, 64)
    t_hi = t_lo + width
    e = _Enc(B, R, D, d, t_lo, t_hi, seed=60 + d + form)
    e.hand(kind, 7 if d != 7 else 9, t_lo + min(5, width // 2), seed=form)
    ref = e.reference_bwd()
    pitch = e.pitch
    if form == 1:
        assert _lib.pq_chain_ok(t_lo, t_hi, B, d)
    if form == 2 and width <= 32:
        assert (t_hi - 1) // 32 == t_lo // 32, "not a single item"
    ns = _lib.enc_slabs(t_lo, t_hi, B) if form == 0 else _lib.pq_slabs(t_lo, t_hi, B, d if form == 1 else 32, True)

    def run():
        po, qo = _nanbuf(B, CH, pitch), _nanbuf(B, CH, pitch)
        s1, s2 = torch.full((ns * 2 * CH * CH,), NAN, device=DEV), torch.full((ns * CH * CH,), NAN, device=DEV)
        call("wn_enc_resblock_bwd_pq", ptr(e.x, SLACK), ptr(e.p_in, SLACK), ptr(e.q_in, SLACK) if e.q_in is not None else None, e.dn,
             e.p_lo, ptr(e.h, SLACK), ptr(po, SLACK), ptr(qo, SLACK), CH * pitch, CH * pitch, pitch, ptr(e.p_dT), ptr(e.p_pq), CH, d,
             t_lo, t_hi, ptr(s1), ptr(s2), form, B, MB, _lib.stream())
        torch.cuda.synchronize()
        return po, qo, s1, s2
    po, qo, s1, s2 = run()
    tag = "enc pq form%d d%d t_lo%d w%d %s" % (form, d, t_lo, width, kind)
    errs, _, _ = e.check_slabs(s1, s2, ns, ref, tag)
    Pg, Qg = _view(po, B, CH, pitch).cpu(), _view(qo, B, CH, pitch).cpu()
    if form == 0:
        assert _written(po) == B * CH * width and _written(qo) == B * CH * width, tag + ": P / Q written outside [t_lo, t_hi)"
        errs["P"] = _rel(Pg[:, :R, t_lo:t_hi], ref["P"])
        errs["Q"] = _rel(Qg[:, :R, t_lo:t_hi], ref["Q"])
        assert _all_zero(Pg[:, R:, t_lo:t_hi]) and _all_zero(Qg[:, R:, t_lo:t_hi])
        out = _nanbuf(B, CH, pitch)
        call("wn_shift_add", ptr(po, SLACK), ptr(qo, SLACK), ptr(out, SLACK), CH * pitch, pitch, CH, d, t_lo, t_lo - d, t_hi, B, _lib.stream())
        torch.cuda.synchronize()
        dx = _view(out, B, CH, pitch).cpu()[:, :, t_lo - d:t_hi]
    else:
        assert _written(qo) == 0, tag + ": a chain form touched q_out"
        assert _written(po) == B * CH * (width + d), tag + ": p_out written outside [t_lo - d, t_hi) (or NaN inside)"
        dx = Pg[:, :, t_lo - d:t_hi]
    errs["dx"] = _rel(dx[:, :R], ref["dx"])
    assert _all_zero(dx[:, R:])
    print(tag, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(v <= BAR64 for v in errs.values()), errs
    po2, qo2, s1b, s2b = run()
    assert _same_bits(po, po2) and _same_bits(qo, qo2) and _same_bits(s1, s1b) and _same_bits(s2, s2b)


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("dn,p_off,lo_off,B,rows", [(5, 0, 5, 2, 64), (64, 7, 64, 3, 48), (1, 40, 0, 1, 5), (700, 3, 2, 2, 16)])
def test_shift_add_exact(dn, p_off, lo_off, B, rows):
    """wn_shift_add: out[t] = p[t] (t >= p_lo) + q[t + dn] (t + dn < t_hi) on [t_lo, t_hi), exactly the float32 expression; p below
    p_lo and q from t_hi on hold NaN (they do not count); nothing else is written."""
    pitch, t_hi = 1536, 1021
    p_lo = 100 + p_off
    t_lo = p_lo - lo_off
    p, q = _buf(B, rows, pitch, 1.0, 1), _buf(B, rows, pitch, 1.0, 2)
    _view(p, B, rows, pitch)[:, :, :p_lo] = NAN
    _view(q, B, rows, pitch)[:, :, t_hi:] = NAN
    out = _nanbuf(B, rows, pitch)
    call("wn_shift_add", ptr(p, SLACK), ptr(q, SLACK), ptr(out, SLACK), rows * pitch, pitch, rows, dn, p_lo, t_lo, t_hi, B, _lib.stream())
    torch.cuda.synchronize()
    ts = torch.arange(t_lo, t_hi)
    pv, qv = _view(p, B, rows, pitch).cpu(), _view(q, B, rows, pitch).cpu()
    qs = torch.zeros(B, rows, t_hi - t_lo)
    n = max(0, t_hi - dn - t_lo)
    qs[:, :, :n] = qv[:, :, t_lo + dn:t_lo + dn + n]
    want = torch.where(ts >= p_lo, pv[:, :, t_lo:t_hi], torch.zeros(())) + qs
    got = _view(out, B, rows, pitch).cpu()
    assert torch.equal(got[:, :, t_lo:t_hi], want)
    assert _written(out) == B * rows * (t_hi - t_lo)


@pytest.mark.parametrize("pool,n_out,t0,rows,B", [(4, 250, 37, 24, 2), (7, 100, 64, 5, 3), (320, 3, 5, 16, 1), (64, 17, 33, 64, 2)])
def test_avgpool_fwd_bwd(pool, n_out, t0, rows, B):
    """wn_avgpool / wn_avgpool_bwd against F.avg_pool1d and its autograd in float64: pool sizes that do and do not divide the span
    (the tail up to t_hi gets zero gradient), canaries around both outputs."""
    span = pool * n_out + (0 if pool == 4 else pool // 2)
    t_hi = t0 + span
    pitch = ((t_hi + 255) // 256) * 256 + 256
    src = _buf(B, rows + 3, pitch, 1.0, pool)
    out = torch.full((B, rows + 2, n_out + 5), NAN, device=DEV)
    call("wn_avgpool", ptr(src, SLACK), (rows + 3) * pitch, pitch, t0, pool, n_out, rows, ptr(out), (rows + 2) * (n_out + 5), n_out + 5, B,
         _lib.stream())
    torch.cuda.synchronize()
    x = _view(src, B, rows + 3, pitch).cpu()[:, :rows, t0:t_hi].double().requires_grad_(True)
    want = F.avg_pool1d(x, pool)
    assert want.shape[-1] == n_out
    got = out.cpu()
    e = (got[:, :rows, :n_out].double() - want).abs().max().item()
    print("avgpool %d: err %.2e" % (pool, e))
    assert e <= 1e-6 * max(1.0, want.abs().max().item())       # a float32 mean of `pool` terms (2^-24 per term, pool <= 320); observed 1.3e-7
    assert torch.isnan(got[:, rows:]).all() and torch.isnan(got[:, :, n_out:]).all()
    g = torch.Generator().manual_seed(pool)
    denc = torch.randn(B, rows, n_out, generator=g)
    want.backward(denc.double())
    dd = denc.to(DEV).contiguous()
    dout = _nanbuf(B, rows + 3, pitch)
    call("wn_avgpool_bwd", ptr(dd), rows * n_out, n_out, t0, pool, n_out, rows, ptr(dout, SLACK), (rows + 3) * pitch, pitch, t_hi, B,
         _lib.stream())
    torch.cuda.synchronize()
    gd = _view(dout, B, rows + 3, pitch).cpu()
    e = (gd[:, :rows, t0:t_hi].double() - x.grad).abs().max().item()
    assert e <= 1e-6 * x.grad.abs().max().item(), e
    assert (gd[:, :rows, t0 + pool * n_out:t_hi] == 0).all()
    assert _written(dout) == B * rows * (t_hi - t0)


def test_gather_grads2_exact():
    """wn_gather_grads2: flat[i] = packed[idx[i]] + packed[idx2[i]], an index < 0 adds nothing; exact."""
    g = torch.Generator().manual_seed(3)
    n, m = 5003, 4096
    packed = torch.randn(m, generator=g)
    idx = torch.randint(-1, m, (n,), generator=g).int()
    idx2 = torch.randint(-1, m, (n,), generator=g).int()
    idx[:7], idx2[:7] = -1, -1
    out = torch.full((n + 16,), NAN, device=DEV)
    pk, i1, i2 = packed.to(DEV), idx.to(DEV), idx2.to(DEV)
    call("wn_gather_grads2", ptr(pk), ptr(i1), ptr(i2), ptr(out), n, _lib.stream())
    torch.cuda.synchronize()
    a = torch.where(idx >= 0, packed[idx.long().clamp(min=0)], torch.zeros(()))
    b = torch.where(idx2 >= 0, packed[idx2.long().clamp(min=0)], torch.zeros(()))
    assert torch.equal(out[:n].cpu(), a + b) and torch.isnan(out[n:]).all()


# ------------------------------------------------------------------------------------------------ clip pairs
# observed worst against float64: P 8.3e-6, Q 1.1e-5, dx 8.7e-6, dWf 5.9e-6, dWg 6.2e-6, dWd 5.2e-6 (bar 1e-4)
@pytest.mark.parametrize("hand,chain,d", [("pair", 0, 3), ("last", 0, 32), ("whole", 0, 7), ("pair", 1, 32), ("whole", 1, 64), ("last", 1, 32)],
                         ids=["d%d-pairs-%s" % (d, _inst(h, c)) for h, c, d in (("pair", 0, 3), ("last", 0, 32), ("whole", 0, 7), ("pair", 1, 32),
                                                                                 ("whole", 1, 64), ("last", 1, 32))])
def test_pq_clip_pairs(hand, chain, d):
    """dz_half_stride != 0: two clips of a 32-channel model (24 / 20 real channels) side by side on the 64-channel block, block-diagonal
    packs, the second clip's dz-crop rows in its own slice.  Equals the float64 reference of four single clips: P, Q (pair out), dx,
    write windows, padded rows exactly 0; dWf, dWg, dWd = the two diagonal blocks of the reduced slabs added by wn_gather_grads2
    (exact against the float32 sum; the off-diagonal blocks are cross-clip products nobody reads); a second launch reproduces the bits."""
    t_lo = 64 * ((d + 3 + 63) // 64) + 33
    c = _Gated(B=4, R=24, D=20, d=d, t_lo=t_lo, t_hi=t_lo + 1203, z_lo=t_lo + 45, hand=hand, dn=96, p_lo=t_lo + 5, seed=77 + d,
               clip_pairs=True)
    if chain:
        assert _lib.pq_chain_ok(c.t_lo, c.t_hi, c.nb, d)
    c.run_pq(chain, "clip pairs d%d %s" % (d, _inst(hand, chain)))
