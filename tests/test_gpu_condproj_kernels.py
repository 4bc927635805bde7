"""wn_cond_proj_fwd / wn_cond_proj_bwd (music_amd/csrc/wn_condproj.hip) alone, through ctypes, against a float64 restatement of
include/wavenet_hip.h written here: the N + 1 projections of the pooled encoding out of a flat parameter buffer into the block
tables (per clip and as clip pairs) and the final table, and their backward (d enc, dW and db into a flat gradient buffer).

Two kinds of input per geometry:
  exact    every input a multiple of 1/8 in [-2, 2]: every product is a multiple of 1/64 and every partial sum of up to 65 535
           terms is exact in fp32 in any order, with or without FMA - the result must EQUAL the float64 one after the cast;
  random   normal inputs: |got - ref| <= gamma (sum |a_j| |b_j| + |bias|) per element, gamma = (K + 2) u / (1 - (K + 2) u),
           u = 2^-24, K the length of that element's reduction - the standard bound of an fp32 dot product in any order.
Every output lies in a NaN-filled buffer: padding rows must come back 0, everything around the outputs (canaries in front and
behind, the gaps between the parameters in the flat gradient) must stay NaN, and a second launch must give the same bits.  The
padding rows of d_tab hold NaN: they must not be read."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64

# (Bw, Le, Dd, CH, Sd, B, N, pair): every value of the issue's lists appears, the extremes meet (512 x 70; 1 x 1)
CASES = [
    (1, 1, 8, 32, 32, 1, 1, False),
    (512, 70, 32, 32, 512, 2, 3, True),
    (16, 3, 64, 64, 256, 3, 3, False),
    (48, 25, 80, 96, 32, 3, 1, False),          # the general plan's padding (Dd 80 in 96 rows)
    (64, 32, 32, 32, 256, 8, 3, True),
    (64, 33, 64, 64, 256, 2, 1, False),
    (16, 25, 8, 32, 32, 8, 3, True),            # padding rows in the pair layout
    (512, 70, 64, 64, 512, 1, 1, False),
]
IDS = ["bw%d_le%d_dd%d_ch%d_sd%d_b%d_n%d_%s" % (c[:7] + ("pair" if c[7] else "clip",)) for c in CASES]


def gamma(K):
    return (K + 2) * U / (1 - (K + 2) * U)


def draw(rng, shape, exact):
    if exact:
        return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


class Geometry:
    """One case's parameters in a flat buffer with a NaN pad in front, gaps between the stages and NaN behind."""

    def __init__(self, case, exact, seed):
        self.Bw, self.Le, self.Dd, self.CH, self.Sd, self.B, self.N, self.pair = case
        Bw, Le, Dd, Sd, B, N = self.Bw, self.Le, self.Dd, self.Sd, self.B, self.N
        rng = np.random.default_rng(seed)
        self.W = draw(rng, (N, 2 * Dd, Bw), exact)
        self.b = draw(rng, (N, 2 * Dd), exact)
        self.Wf = draw(rng, (Sd, Bw), exact)
        self.bf = draw(rng, (Sd,), exact)
        self.enc = draw(rng, (B, Bw, Le), exact)
        self.d_en = draw(rng, (N, B, 2 * Dd, Le), exact)          # reference row order: gate rows first
        self.d_enf = draw(rng, (B, Sd, Le), exact)
        self.w_off, gap = 7, 3
        self.b_off = self.w_off + 2 * Dd * Bw
        self.stride = 2 * Dd * Bw + 2 * Dd + gap
        self.wf_off = self.w_off + N * self.stride + 5
        self.bf_off = self.wf_off + Sd * Bw + 2
        self.total = self.bf_off + Sd + 9
        flat = np.full(self.total, np.nan, dtype=np.float32)
        for i in range(N):
            flat[self.w_off + i * self.stride:][:2 * Dd * Bw] = self.W[i].reshape(-1)
            flat[self.b_off + i * self.stride:][:2 * Dd] = self.b[i]
        flat[self.wf_off:][:Sd * Bw] = self.Wf.reshape(-1)
        flat[self.bf_off:][:Sd] = self.bf
        self.flat = flat
        self.offsets = (self.w_off, self.b_off, self.stride, self.wf_off, self.bf_off)
        self.dims = (N, Dd, self.CH, Sd, Bw, Le, B)

    def table(self, en, pair, fill):
        """en (N, B, 2Dd, Le) in the reference's row order -> the block table of include/wavenet_hip.h, other rows = fill"""
        N, B, Dd, CH, Le = self.N, self.B, self.Dd, self.CH, self.Le
        rows, nt = (4 * CH, B // 2) if pair else (2 * CH, B)
        tab = np.full((N, nt, rows, Le), fill, dtype=en.dtype)
        for b in range(B):
            t, h = (b >> 1, b & 1) if pair else (b, 0)
            tab[:, t, h * CH:h * CH + Dd] = en[:, b, Dd:]                                    # filter rows c in [Dd, 2Dd)
            g0 = (2 * CH if pair else CH) + h * CH
            tab[:, t, g0:g0 + Dd] = en[:, b, :Dd]                                            # gate rows c in [0, Dd)
        return tab


def guarded(n, fill=float("nan")):
    """(whole buffer, view of its n floats between two guards of NaN)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n]
    if fill == fill:
        view.fill_(fill)
    return buf, view


def guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def compare(got, ref, bound, exact, what):
    got64 = np.asarray(got, dtype=np.float64)
    if exact:
        assert np.array_equal(got, ref.astype(np.float32)), "%s: not exact (largest difference %.3e)" % (what, np.abs(got64 - ref).max())
        return 0.0
    assert np.isfinite(got64).all(), what
    err = np.abs(got64 - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("  %s: largest error %.3e, largest error / bound %.3f" % (what, err.max(), ratio))
    assert (err <= bound).all(), (what, ratio)
    return ratio


def fwd_reference(g):
    W, b, Wf, bf, enc = (np.asarray(a, dtype=np.float64) for a in (g.W, g.b, g.Wf, g.bf, g.enc))
    en = np.einsum("nck,bkl->nbcl", W, enc) + b[:, None, :, None]
    enf = np.einsum("ck,bkl->bcl", Wf, enc) + bf[None, :, None]
    gm = gamma(g.Bw)
    en_bound = gm * (np.einsum("nck,bkl->nbcl", np.abs(W), np.abs(enc)) + np.abs(b)[:, None, :, None])
    enf_bound = gm * (np.einsum("ck,bkl->bcl", np.abs(Wf), np.abs(enc)) + np.abs(bf)[None, :, None])
    return en, enf, en_bound, enf_bound


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cond_proj_fwd(case, exact):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    g = Geometry(case, exact, seed=17)
    en, enf_ref, en_bound, enf_bound = fwd_reference(g)
    flat, enc = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.enc).cuda()
    N, B, CH, Le, Sd = g.N, g.B, g.CH, g.Le, g.Sd
    n_tab, n_enf = N * B * 2 * CH * Le, B * Sd * Le
    variants = [(True, False)] + ([(True, True), (False, True)] if g.pair else [])
    for want_clip, want_pair in variants:
        runs = []
        for _ in range(2):
            tb, tab = guarded(n_tab) if want_clip else (None, None)
            pb, tabp = guarded(n_tab) if want_pair else (None, None)
            eb, enf = guarded(n_enf)
            call("wn_cond_proj_fwd", ptr(enc), ptr(flat), *g.offsets, ptr(tab), ptr(tabp), ptr(enf), *g.dims, _lib.stream())
            torch.cuda.synchronize()
            assert guards_intact(eb, n_enf) and (tb is None or guards_intact(tb, n_tab)) and (pb is None or guards_intact(pb, n_tab))
            runs.append([t.cpu().numpy() if t is not None else None for t in (tab, tabp, enf)])
        for a, b in zip(*runs):
            assert a is None or np.array_equal(a, b), "two launches differ"                   # (NaN nowhere: checked below)
        tab, tabp, enf = runs[0]
        what = "fwd %s%s" % ("clip" if want_clip else "", "+pair" if want_pair and want_clip else "pair" if want_pair else "")
        compare(enf.reshape(B, Sd, Le), enf_ref, enf_bound, exact, what + " enf")
        for got, pair in ((tab, False), (tabp, True)):
            if got is None:
                continue
            ref = g.table(en, pair, 0.0)
            bound = g.table(en_bound, pair, 0.0)
            got = got.reshape(ref.shape)
            pad = g.table(np.ones_like(en), pair, 0.0) == 0.0
            assert pad.sum() == N * B * 2 * (CH - g.Dd) * Le
            assert (got[pad] == 0.0).all(), "padding rows are not zero"
            compare(got, ref, bound, exact, what + (" pair table" if pair else " clip table"))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cond_proj_bwd(case, exact):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    g = Geometry(case, exact, seed=29)
    N, B, Dd, CH, Le, Sd, Bw = g.N, g.B, g.Dd, g.CH, g.Le, g.Sd, g.Bw
    W, Wf, enc, d_en, d_enf = (np.asarray(a, dtype=np.float64) for a in (g.W, g.Wf, g.enc, g.d_en, g.d_enf))
    R = N * 2 * Dd + Sd
    denc_ref = np.einsum("nck,nbcl->bkl", W, d_en) + np.einsum("ck,bcl->bkl", Wf, d_enf)
    denc_bound = gamma(R) * (np.einsum("nck,nbcl->bkl", np.abs(W), np.abs(d_en)) + np.einsum("ck,bcl->bkl", np.abs(Wf), np.abs(d_enf)))
    gk = gamma(B * Le)
    ref = np.full(g.total, np.nan)
    bound = np.zeros(g.total)
    dW, dWb = np.einsum("nbcl,bkl->nck", d_en, enc), gk * np.einsum("nbcl,bkl->nck", np.abs(d_en), np.abs(enc))
    db, dbb = d_en.sum((1, 3)), gk * np.abs(d_en).sum((1, 3))
    for i in range(N):
        ref[g.w_off + i * g.stride:][:2 * Dd * Bw], bound[g.w_off + i * g.stride:][:2 * Dd * Bw] = dW[i].reshape(-1), dWb[i].reshape(-1)
        ref[g.b_off + i * g.stride:][:2 * Dd], bound[g.b_off + i * g.stride:][:2 * Dd] = db[i], dbb[i]
    ref[g.wf_off:][:Sd * Bw] = np.einsum("bcl,bkl->ck", d_enf, enc).reshape(-1)
    bound[g.wf_off:][:Sd * Bw] = gk * np.einsum("bcl,bkl->ck", np.abs(d_enf), np.abs(enc)).reshape(-1)
    ref[g.bf_off:][:Sd], bound[g.bf_off:][:Sd] = d_enf.sum((0, 2)), gk * np.abs(d_enf).sum((0, 2))
    is_param = ~np.isnan(ref)

    flat, enc_d, d_enf_d = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.enc).cuda(), torch.from_numpy(g.d_enf).cuda()
    for pair in ([False, True] if g.pair else [False]):
        d_tab = torch.from_numpy(g.table(g.d_en, pair, np.float32("nan"))).cuda()            # padding rows: NaN, never to be read
        runs = []
        for _ in range(2):
            eb, d_enc = guarded(B * Bw * Le)
            gb, grad = guarded(g.total)
            call("wn_cond_proj_bwd", ptr(d_tab), 1 if pair else 0, ptr(d_enf_d), ptr(enc_d), ptr(flat), *g.offsets, ptr(d_enc), ptr(grad),
                 *g.dims, _lib.stream())
            torch.cuda.synchronize()
            assert guards_intact(eb, B * Bw * Le) and guards_intact(gb, g.total)
            runs.append((d_enc.cpu().numpy(), grad.cpu().numpy()))
        d_enc, grad = runs[0]
        assert np.array_equal(d_enc, runs[1][0]) and np.array_equal(grad[is_param], runs[1][1][is_param]), "two launches differ"
        assert np.isnan(grad[~is_param]).all(), "flat_grad was written outside the projections' parameters"
        what = "bwd %s" % ("pair" if pair else "clip")
        compare(d_enc.reshape(B, Bw, Le), denc_ref, denc_bound, exact, what + " d_enc (K = %d)" % R)
        compare(grad[is_param], ref[is_param], bound[is_param], exact, what + " dW, db (K = %d)" % (B * Le))
