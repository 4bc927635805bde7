"""wn_gcond_proj_fwd / wn_gcond_proj_bwd (music_amd/csrc/wn_gcond.hip) alone, through ctypes, against a float64 restatement of
include/wavenet_hip.h written here: the learned projections with a global class term, en_i[b] = W_i enc[b] + b_i + G_i emb[cls[b]],
and its backward (d enc, dW, db, dG and d emb into a flat gradient buffer).  The method is tests/test_gpu_condproj_kernels.py's:

  exact    every input a multiple of 1/8 in [-2, 2]: every product is a multiple of 1/64 and every partial sum of up to 65 535
           terms is exact in fp32 in any order - the result must EQUAL the float64 one.  d emb's longest reduction has
           (clips of one class) R Le terms: every case keeps that <= 65 535 (asserted);
  random   normal inputs: |got - ref| <= gamma(K) sum |a_j| |b_j| per element, gamma(K) = (K + 2) u / (1 - (K + 2) u), u = 2^-24,
           K the number of elementary terms of that element's reduction (valid for any summation order): Bw + E forward,
           B Le for dW, db and dG, R for d enc, (clips of the class) R Le for d emb.
Outputs lie in NaN-filled guarded buffers, padding rows of d_tab hold NaN (never to be read), the gaps of the flat gradient must stay
NaN, a second launch must give the same bits.  Beyond that: d enc, dW and db carry wn_cond_proj_bwd's bits, the d emb rows of
absent classes are exactly 0, all G = 0 gives wn_cond_proj_fwd's bits, and a class outside [0, n_cls) turns its clip's columns
into NaN and nothing else."""
import numpy as np
import pytest
import torch

from tests.test_gpu_condproj_kernels import Geometry, compare, draw, gamma, guarded, guards_intact

pytestmark = pytest.mark.gpu

# (Bw, Le, Dd, CH, Sd, B, N, pair), E, n_cls, cls: the smallest shapes at which each index path can go wrong
CASES = [
    ((1, 1, 8, 32, 32, 1, 1, False), 1, 1, [0]),
    ((16, 3, 64, 64, 256, 3, 3, False), 17, 5, [4, 0, 4]),
    ((64, 32, 32, 32, 256, 8, 3, True), 64, 8, [5, 2, 7, 0, 3, 6, 1, 4]),
    ((48, 25, 80, 96, 32, 3, 1, False), 20, 2, [1, 1, 1]),
    ((16, 25, 8, 32, 32, 8, 3, True), 5, 3, [0, 1, 2, 0, 1, 2, 2, 2]),
    ((64, 33, 64, 64, 256, 2, 1, False), 65, 1024, [1023, 0]),
    ((512, 70, 32, 32, 512, 2, 3, True), 128, 2, [1, 0]),
]
IDS = ["bw%d_le%d_dd%d_ch%d_sd%d_b%d_n%d_%s_e%d_cls%d" % (c[0][:7] + ("pair" if c[0][7] else "clip", c[1], c[2])) for c in CASES]


class GGeometry(Geometry):
    """The learned projections' geometry with the global block behind it in the flat buffer: G_i, G_f and the embedding, gaps of NaN
    between them."""

    def __init__(self, case, exact, seed):
        base, self.E, self.n_cls, cls = case
        super().__init__(base, exact, seed)
        N, Dd, Sd, E = self.N, self.Dd, self.Sd, self.E
        rng = np.random.default_rng(seed + 1000)
        self.G = draw(rng, (N, 2 * Dd, E), exact)
        self.Gf = draw(rng, (Sd, E), exact)
        self.emb = draw(rng, (self.n_cls, E), exact)
        self.cls = np.asarray(cls, dtype=np.int32)
        assert self.cls.shape == (self.B,)
        self.gw_off = self.total + 4
        self.gstride = 2 * Dd * E + 6
        self.gwf_off = self.gw_off + N * self.gstride + 1
        self.emb_off = self.gwf_off + Sd * E + 3
        self.total = self.emb_off + self.n_cls * E + 5
        self.flat = self.fill(np.full(self.total, np.nan, dtype=np.float32), self.flat, self.G, self.Gf, self.emb)
        self.flat_g0 = self.fill(np.full(self.total, np.nan, dtype=np.float32), self.flat, 0 * self.G, 0 * self.Gf, self.emb)
        self.goffsets = (self.gw_off, self.gstride, self.gwf_off, self.emb_off, E, self.n_cls)
        self.R = N * 2 * Dd + Sd
        in_range = self.cls[(self.cls >= 0) & (self.cls < self.n_cls)]
        assert np.bincount(in_range, minlength=1).max() * self.R * self.Le <= 65535

    def fill(self, flat, learned, G, Gf, emb):
        n = min(len(learned), self.gw_off - 4)
        flat[:n] = learned[:n]
        for i in range(self.N):
            flat[self.gw_off + i * self.gstride:][:G[i].size] = G[i].reshape(-1)
        flat[self.gwf_off:][:Gf.size] = Gf.reshape(-1)
        flat[self.emb_off:][:emb.size] = emb.reshape(-1)
        return flat

    def place(self, dG, dGf, demb):
        """the global block's three tensors at their offsets of a NaN-filled flat vector (float64)"""
        v = np.full(self.total, np.nan)
        for i in range(self.N):
            v[self.gw_off + i * self.gstride:][:dG[i].size] = dG[i].reshape(-1)
        v[self.gwf_off:][:dGf.size] = dGf.reshape(-1)
        v[self.emb_off:][:demb.size] = demb.reshape(-1)
        return v


def fwd_reference(g, cls=None):
    cls = g.cls if cls is None else cls
    W, b, Wf, bf, enc, G, Gf, emb = (np.asarray(a, dtype=np.float64) for a in (g.W, g.b, g.Wf, g.bf, g.enc, g.G, g.Gf, g.emb))
    ok = (cls >= 0) & (cls < g.n_cls)
    v = np.where(ok[:, None], emb[np.where(ok, cls, 0)], np.nan)                       # (B, E): NaN rows for classes out of range
    en = np.einsum("nck,bkl->nbcl", W, enc) + b[:, None, :, None] + np.einsum("nce,be->nbc", G, v)[..., None]
    enf = np.einsum("ck,bkl->bcl", Wf, enc) + bf[None, :, None] + np.einsum("ce,be->bc", Gf, v)[..., None]
    gm = gamma(g.Bw + g.E)
    av = np.abs(np.nan_to_num(v))
    en_bound = gm * (np.einsum("nck,bkl->nbcl", np.abs(W), np.abs(enc)) + np.abs(b)[:, None, :, None]
                     + np.einsum("nce,be->nbc", np.abs(G), av)[..., None])
    enf_bound = gm * (np.einsum("ck,bkl->bcl", np.abs(Wf), np.abs(enc)) + np.abs(bf)[None, :, None]
                      + np.einsum("ce,be->bc", np.abs(Gf), av)[..., None])
    return en, enf, en_bound, enf_bound


def run_fwd(g, flat, cls, want_clip, want_pair, entry="wn_gcond_proj_fwd"):
    """one launch into fresh guarded buffers -> (tab, tab_pair, enf) as numpy (None where not asked for)"""
    from music_amd import _lib
    from music_amd._lib import call, ptr
    n_tab, n_enf = g.N * g.B * 2 * g.CH * g.Le, g.B * g.Sd * g.Le
    tb, tab = guarded(n_tab) if want_clip else (None, None)
    pb, tabp = guarded(n_tab) if want_pair else (None, None)
    eb, enf = guarded(n_enf)
    extra = (ptr(cls),) + g.goffsets if entry == "wn_gcond_proj_fwd" else ()
    call(entry, ptr(g.enc_d), ptr(flat), *g.offsets, ptr(tab), ptr(tabp), ptr(enf), *g.dims, *extra, _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(eb, n_enf) and (tb is None or guards_intact(tb, n_tab)) and (pb is None or guards_intact(pb, n_tab))
    return [t.cpu().numpy() if t is not None else None for t in (tab, tabp, enf)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gcond_proj_fwd(case, exact):
    g = GGeometry(case, exact, seed=17)
    en, enf_ref, en_bound, enf_bound = fwd_reference(g)
    flat, flat_g0, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.flat_g0).cuda(), torch.from_numpy(g.cls).cuda()
    g.enc_d = torch.from_numpy(g.enc).cuda()
    N, B, CH, Le, Sd = g.N, g.B, g.CH, g.Le, g.Sd
    variants = [(True, False)] + ([(True, True), (False, True)] if g.pair else [])
    for want_clip, want_pair in variants:
        runs = [run_fwd(g, flat, cls, want_clip, want_pair) for _ in range(2)]
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
        # all G = 0: the learned projections' bits
        zero = run_fwd(g, flat_g0, cls, want_clip, want_pair)
        learned = run_fwd(g, flat_g0, None, want_clip, want_pair, entry="wn_cond_proj_fwd")
        for a, b in zip(zero, learned):
            assert a is None or np.array_equal(a, b), "G = 0 does not give wn_cond_proj_fwd's bits"


def bwd_reference(g, cls=None):
    """(reference, bound) of the global block as flat float64 vectors (NaN / 0 elsewhere)"""
    cls = g.cls if cls is None else cls
    G, Gf, emb, d_en, d_enf = (np.asarray(a, dtype=np.float64) for a in (g.G, g.Gf, g.emb, g.d_en, g.d_enf))
    ok = (cls >= 0) & (cls < g.n_cls)
    v = np.where(ok[:, None], emb[np.where(ok, cls, 0)], np.nan)
    s, sf = d_en.sum(3), d_enf.sum(2)                                                   # (N, B, 2Dd), (B, Sd)
    a_s, a_sf = np.abs(d_en).sum(3), np.abs(d_enf).sum(2)
    dG, dGf = np.einsum("nbc,be->nce", s, v), np.einsum("bc,be->ce", sf, v)
    gk = gamma(g.B * g.Le)
    dG_b, dGf_b = gk * np.einsum("nbc,be->nce", a_s, np.abs(np.nan_to_num(v))), gk * np.einsum("bc,be->ce", a_sf, np.abs(np.nan_to_num(v)))
    per_clip = np.einsum("nce,nbc->be", G, s) + np.einsum("ce,bc->be", Gf, sf)          # (B, E)
    per_clip_abs = np.einsum("nce,nbc->be", np.abs(G), a_s) + np.einsum("ce,bc->be", np.abs(Gf), a_sf)
    demb, demb_b = np.zeros((g.n_cls, g.E)), np.zeros((g.n_cls, g.E))
    for b in range(g.B):
        if ok[b]:
            demb[cls[b]] += per_clip[b]
            demb_b[cls[b]] += per_clip_abs[b]
    count = np.bincount(cls[ok], minlength=g.n_cls)
    demb_b *= np.array([gamma(int(c) * g.R * g.Le) for c in count])[:, None]
    return g.place(dG, dGf, demb), np.nan_to_num(g.place(dG_b, dGf_b, demb_b)), count


def run_bwd(g, flat, cls, d_tab, pair, entry="wn_gcond_proj_bwd"):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    n_enc = g.B * g.Bw * g.Le
    eb, d_enc = guarded(n_enc)
    gb, grad = guarded(g.total)
    extra = (ptr(cls),) + g.goffsets if entry == "wn_gcond_proj_bwd" else ()
    call(entry, ptr(d_tab), 1 if pair else 0, ptr(g.d_enf_d), ptr(g.enc_d), ptr(flat), *g.offsets, ptr(d_enc), ptr(grad), *g.dims, *extra,
         _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(eb, n_enc) and guards_intact(gb, g.total)
    return d_enc.cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gcond_proj_bwd(case, exact):
    g = GGeometry(case, exact, seed=29)
    ref, bound, count = bwd_reference(g)
    is_global = ~np.isnan(ref)
    flat, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.cls).cuda()
    g.enc_d, g.d_enf_d = torch.from_numpy(g.enc).cuda(), torch.from_numpy(g.d_enf).cuda()
    for pair in ([False, True] if g.pair else [False]):
        d_tab = torch.from_numpy(g.table(g.d_en, pair, np.float32("nan"))).cuda()            # padding rows: NaN, never to be read
        runs = [run_bwd(g, flat, cls, d_tab, pair) for _ in range(2)]
        d_enc, grad = runs[0]
        # d enc, dW, db: wn_cond_proj_bwd's bits (its own test holds them against float64), and nothing else but the global block
        d_enc_l, grad_l = run_bwd(g, flat, None, d_tab, pair, entry="wn_cond_proj_bwd")
        is_learned = ~np.isnan(grad_l)
        assert is_learned.sum() == g.R * (g.Bw + 1) and not (is_learned & is_global).any()
        assert np.array_equal(d_enc, d_enc_l) and np.array_equal(grad[is_learned], grad_l[is_learned]), "not wn_cond_proj_bwd's bits"
        written = is_learned | is_global
        assert np.isnan(grad[~written]).all(), "flat_grad was written outside the parameters"
        assert np.array_equal(d_enc, runs[1][0]) and np.array_equal(grad[written], runs[1][1][written]), "two launches differ"
        what = "bwd %s" % ("pair" if pair else "clip")
        compare(grad[is_global], ref[is_global], bound[is_global], exact, what + " dG, d_emb")
        demb = grad[g.emb_off:][:g.n_cls * g.E].reshape(g.n_cls, g.E)
        absent = count == 0
        assert (demb[absent] == 0.0).all() and not np.signbit(demb[absent]).any(), "an absent class's d_emb row is not exactly 0"


@pytest.mark.parametrize("bad", [5, -1, 2 ** 31 - 1], ids=["n_cls", "minus1", "intmax"])
def test_a_class_out_of_range_is_not_dereferenced(bad):
    g = GGeometry(((16, 3, 64, 64, 256, 3, 3, False), 17, 5, [4, bad, 0]), True, seed=41)
    flat, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.cls).cuda()
    g.enc_d, g.d_enf_d = torch.from_numpy(g.enc).cuda(), torch.from_numpy(g.d_enf).cuda()
    en, enf_ref, _, _ = fwd_reference(g)
    assert np.isnan(en[:, 1]).all() and np.isnan(enf_ref[1]).all() and not np.isnan(en[:, [0, 2]]).any()
    tab, _, enf = run_fwd(g, flat, cls, True, False)                                      # (asserts the guards)
    ref = g.table(en, False, 0.0)
    assert np.array_equal(tab.reshape(ref.shape), ref.astype(np.float32), equal_nan=True)    # clip 1: NaN; padding 0; others exact
    assert np.array_equal(enf.reshape(enf_ref.shape), enf_ref.astype(np.float32), equal_nan=True)
    # backward: that clip's share turns dG into NaN, d emb has no row for it, everything else is untouched by it
    ref, _, count = bwd_reference(g)
    d_tab = torch.from_numpy(g.table(g.d_en, False, np.float32("nan"))).cuda()
    d_enc, grad = run_bwd(g, flat, cls, d_tab, False)
    d_enc_l, grad_l = run_bwd(g, flat, None, d_tab, False, entry="wn_cond_proj_bwd")
    is_learned, is_global = ~np.isnan(grad_l), np.zeros(g.total, dtype=bool)
    is_global[g.emb_off:g.emb_off + g.n_cls * g.E] = True
    assert np.array_equal(d_enc, d_enc_l) and np.array_equal(grad[is_learned], grad_l[is_learned])
    assert np.array_equal(grad[is_global], ref[is_global].astype(np.float32)) and list(count) == [1, 0, 0, 0, 1]
    assert np.isnan(grad[~(is_learned | is_global)]).all()
