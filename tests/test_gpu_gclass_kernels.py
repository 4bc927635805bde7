"""wn_gclass_fwd / wn_gclass_bwd (music_amd/csrc/wn_gcond.hip) alone, through ctypes, one entry per launch, against their float64
restatement tests/gclass_ref.py.  The method is tests/test_gpu_gcond_kernels.py's:

  exact    every input a multiple of 1/8 in [-2, 2]: every product is a multiple of 1/64 and every partial sum (at most
           3 clips x 4096 rows here) is exact in fp32 in any order - the result must EQUAL the float64 one;
  random   normal inputs: |got - ref| <= gamma(K) sum |a_j| |b_j| per element, K the terms of that element's sum: E forward,
           B for dG, (clips of the class) R for d emb.
Outputs lie in NaN-filled guarded buffers; everything the entries are documented to ignore holds NaN (the flat buffer outside G and
the embedding - the learned projections' region included -, the padding rows of d_tab, flat_grad outside the global block, which must
stay NaN); a second launch must give the same bits.  Against wn_gcond_proj_fwd / _bwd with bw = 1, le = 1 and zero W_i, b_i (a zero
bracket added to x is x) every output is bit-equal.  A class outside [0, n_cls) turns its own clip into NaN and nothing else."""
import numpy as np
import pytest
import torch

from tests import gclass_ref as ref
from tests.test_gpu_condproj_kernels import compare, draw, guarded, guards_intact

pytestmark = pytest.mark.gpu

# (Dd, CH, Sd, B, N, pair, E, n_cls, cls): n_stages 1 / 3 / 30, dd 32 / 48 (in 64 rows) / 64, sd 100 / 256, ge 1 / 7 / 64 / 512,
# batch 1 / 2 / 3 / 8 with pair tables on the even ones, n_cls 1 / 5 with a repeated class and classes nobody has
CASES = [
    (32, 32, 100, 1, 1, False, 1, 1, [0]),
    (48, 64, 256, 3, 3, False, 7, 5, [4, 0, 4]),
    (64, 64, 256, 8, 30, True, 64, 5, [3, 1, 3, 0, 1, 1, 3, 0]),
    (48, 64, 100, 2, 3, True, 512, 5, [2, 2]),
    (32, 32, 256, 2, 30, True, 7, 1, [0, 0]),
    (64, 64, 100, 3, 1, False, 64, 5, [1, 4, 1]),
    (32, 64, 100, 8, 3, True, 512, 5, [0, 1, 2, 3, 3, 2, 1, 0]),
]
IDS = ["dd%d_ch%d_sd%d_b%d_n%d_%s_e%d_cls%d" % (c[:5] + ("pair" if c[5] else "clip",) + c[6:8]) for c in CASES]


class Geometry:
    """One case in a flat buffer: the learned projections' region of bw = 1 in front (what wn_gcond_proj_* reads: zeros for the
    bit comparison, NaN for wn_gclass_*, which never looks at it), then G_i, G_f and the embedding with gaps of NaN between them."""

    def __init__(self, case, exact, seed):
        self.Dd, self.CH, self.Sd, self.B, self.N, self.pair, self.E, self.n_cls, cls = case
        Dd, Sd, B, N, E = self.Dd, self.Sd, self.B, self.N, self.E
        rng = np.random.default_rng(seed)
        self.G, self.Gf, self.emb = draw(rng, (N, 2 * Dd, E), exact), draw(rng, (Sd, E), exact), draw(rng, (self.n_cls, E), exact)
        self.d_en, self.d_enf = draw(rng, (N, B, 2 * Dd), exact), draw(rng, (B, Sd), exact)
        self.cls = np.asarray(cls, dtype=np.int32)
        assert self.cls.shape == (B,)
        self.w_off = 7
        self.b_off = self.w_off + 2 * Dd
        self.stride = 4 * Dd + 3
        self.wf_off = self.w_off + N * self.stride + 5
        self.bf_off = self.wf_off + Sd + 2
        self.gw_off = self.bf_off + Sd + 9
        self.gstride = 2 * Dd * E + 6
        self.gwf_off = self.gw_off + N * self.gstride + 1
        self.emb_off = self.gwf_off + Sd * E + 3
        self.total = self.emb_off + self.n_cls * E + 5
        self.offsets = (self.w_off, self.b_off, self.stride, self.wf_off, self.bf_off)
        self.goffsets = (self.gw_off, self.gstride, self.gwf_off, self.emb_off, E, self.n_cls)
        self.R = N * 2 * Dd + Sd
        self.flat = self.place(self.G, self.Gf, self.emb, np.float32)                       # NaN wherever wn_gclass_* must not look
        self.flat_w0 = self.flat.copy()                                                      # ... zero learned projections
        for i in range(N):
            self.flat_w0[self.w_off + i * self.stride:][:4 * Dd] = 0.0
        self.flat_w0[self.wf_off:][:Sd] = 0.0
        self.flat_w0[self.bf_off:][:Sd] = 0.0

    def place(self, G, Gf, emb, dtype=np.float64):
        """the global block's three tensors at their offsets of a NaN-filled flat vector"""
        v = np.full(self.total, np.nan, dtype=dtype)
        for i in range(self.N):
            v[self.gw_off + i * self.gstride:][:G[i].size] = G[i].reshape(-1)
        v[self.gwf_off:][:Gf.size] = Gf.reshape(-1)
        v[self.emb_off:][:emb.size] = emb.reshape(-1)
        return v

    def table(self, en, pair, fill):
        return ref.table(en, self.CH, pair, fill)


def run_fwd(g, flat, cls, want_clip, want_pair, entry="wn_gclass_fwd"):
    """one launch into fresh guarded buffers -> (tab, tab_pair, enf) as numpy (None where not asked for)"""
    from music_amd import _lib
    from music_amd._lib import call, ptr
    n_tab, n_enf = g.N * g.B * 2 * g.CH, g.B * g.Sd
    tb, tab = guarded(n_tab) if want_clip else (None, None)
    pb, tabp = guarded(n_tab) if want_pair else (None, None)
    eb, enf = guarded(n_enf)
    if entry == "wn_gclass_fwd":
        call(entry, ptr(flat), ptr(tab), ptr(tabp), ptr(enf), g.N, g.Dd, g.CH, g.Sd, g.B, ptr(cls), *g.goffsets, _lib.stream())
    else:
        call(entry, ptr(g.enc_d), ptr(flat), *g.offsets, ptr(tab), ptr(tabp), ptr(enf), g.N, g.Dd, g.CH, g.Sd, 1, 1, g.B, ptr(cls),
             *g.goffsets, _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(eb, n_enf) and (tb is None or guards_intact(tb, n_tab)) and (pb is None or guards_intact(pb, n_tab))
    return [t.cpu().numpy() if t is not None else None for t in (tab, tabp, enf)]


def run_bwd(g, flat, cls, d_tab, pair, entry="wn_gclass_bwd"):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    gb, grad = guarded(g.total)
    if entry == "wn_gclass_bwd":
        call(entry, ptr(d_tab), 1 if pair else 0, ptr(g.d_enf_d), ptr(flat), ptr(grad), g.N, g.Dd, g.CH, g.Sd, g.B, ptr(cls), *g.goffsets,
             _lib.stream())
    else:
        d_enc = torch.empty(g.B, dtype=torch.float32, device="cuda")
        call(entry, ptr(d_tab), 1 if pair else 0, ptr(g.d_enf_d), ptr(g.enc_d), ptr(flat), *g.offsets, ptr(d_enc), ptr(grad), g.N, g.Dd,
             g.CH, g.Sd, 1, 1, g.B, ptr(cls), *g.goffsets, _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(gb, g.total)
    return grad.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gclass_fwd(case, exact):
    g = Geometry(case, exact, seed=17)
    en, enf_ref, en_bound, enf_bound = ref.gclass_fwd(g.G, g.Gf, g.emb, g.cls)
    flat, flat_w0, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.flat_w0).cuda(), torch.from_numpy(g.cls).cuda()
    g.enc_d = torch.from_numpy(draw(np.random.default_rng(3), (g.B, 1, 1), exact)).cuda()
    variants = [(True, False)] + ([(True, True), (False, True)] if g.pair else [])
    for want_clip, want_pair in variants:
        runs = [run_fwd(g, flat, cls, want_clip, want_pair) for _ in range(2)]
        for a, b in zip(*runs):
            assert a is None or same_bits(a, b), "two launches differ"
        tab, tabp, enf = runs[0]
        what = "fwd %s%s" % ("clip" if want_clip else "", "+pair" if want_pair and want_clip else "pair" if want_pair else "")
        compare(enf.reshape(g.B, g.Sd), enf_ref, enf_bound, exact, what + " enf")
        for got, pair in ((tab, False), (tabp, True)):
            if got is None:
                continue
            want, bound = g.table(en, pair, 0.0), g.table(en_bound, pair, 0.0)
            got = got.reshape(want.shape)
            pad = g.table(np.ones_like(en), pair, 0.0) == 0.0
            assert pad.sum() == g.N * g.B * 2 * (g.CH - g.Dd)
            assert (got[pad] == 0.0).all() and not np.signbit(got[pad]).any(), "padding rows are not exact zeros"
            compare(got, want, bound, exact, what + (" pair table" if pair else " clip table"))
        # the projections with the class term, bw = 1, le = 1, zero W and b: the same bits
        full = run_fwd(g, flat_w0, cls, want_clip, want_pair, entry="wn_gcond_proj_fwd")
        for a, b in zip(runs[0], full):
            assert a is None or same_bits(a, b), "not wn_gcond_proj_fwd's bits"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gclass_bwd(case, exact):
    g = Geometry(case, exact, seed=29)
    (dG, dGf, demb), (dG_b, dGf_b, demb_b), count = ref.gclass_bwd(g.G, g.Gf, g.emb, g.cls, g.d_en, g.d_enf)
    want, bound = g.place(dG, dGf, demb), np.nan_to_num(g.place(dG_b, dGf_b, demb_b))
    is_global = ~np.isnan(want)
    assert is_global.sum() == g.R * g.E + g.n_cls * g.E
    assert (count == 0).any() == (g.n_cls > len(set(g.cls.tolist())))
    flat, flat_w0, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.flat_w0).cuda(), torch.from_numpy(g.cls).cuda()
    g.d_enf_d = torch.from_numpy(g.d_enf).cuda()
    g.enc_d = torch.from_numpy(draw(np.random.default_rng(3), (g.B, 1, 1), exact)).cuda()
    for pair in ([False, True] if g.pair else [False]):
        d_tab = torch.from_numpy(g.table(g.d_en, pair, np.float32("nan"))).cuda()            # padding rows: NaN, never to be read
        runs = [run_bwd(g, flat, cls, d_tab, pair) for _ in range(2)]
        grad = runs[0]
        assert np.isnan(grad[~is_global]).all(), "flat_grad was written outside the global block"
        assert same_bits(grad[is_global], runs[1][is_global]), "two launches differ"
        compare(grad[is_global], want[is_global], bound[is_global], exact, "bwd %s dG, d_emb" % ("pair" if pair else "clip"))
        rows = grad[g.emb_off:][:g.n_cls * g.E].reshape(g.n_cls, g.E)
        absent = count == 0
        assert (rows[absent] == 0.0).all() and not np.signbit(rows[absent]).any(), "an absent class's d_emb row is not exactly 0"
        full = run_bwd(g, flat_w0, cls, d_tab, pair, entry="wn_gcond_proj_bwd")
        assert same_bits(grad[is_global], full[is_global]), "not wn_gcond_proj_bwd's bits"


@pytest.mark.parametrize("bad", [5, -1, 2 ** 31 - 1], ids=["n_cls", "minus1", "intmax"])
def test_a_class_out_of_range_is_not_dereferenced(bad):
    g = Geometry((48, 64, 256, 4, 3, True, 7, 5, [4, bad, 0, 4]), True, seed=41)
    flat, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.cls).cuda()
    g.d_enf_d = torch.from_numpy(g.d_enf).cuda()
    en, enf_ref, _, _ = ref.gclass_fwd(g.G, g.Gf, g.emb, g.cls)
    assert np.isnan(en[:, 1]).all() and np.isnan(enf_ref[1]).all() and not np.isnan(en[:, [0, 2, 3]]).any()
    tab, tabp, enf = run_fwd(g, flat, cls, True, True)                                    # (asserts the guards)
    for got, pair in ((tab, False), (tabp, True)):
        want = g.table(en, pair, 0.0)                                                     # clip 1: NaN; padding 0; the others exact
        assert np.array_equal(got.reshape(want.shape), want.astype(np.float32), equal_nan=True)
    assert np.array_equal(enf.reshape(enf_ref.shape), enf_ref.astype(np.float32), equal_nan=True)
    # backward: that clip's share turns dG into NaN, d emb has no row for it and is what the other clips give
    (dG, dGf, demb), _, count = ref.gclass_bwd(g.G, g.Gf, g.emb, g.cls, g.d_en, g.d_enf)
    assert np.isnan(dG).all() and np.isnan(dGf).all() and list(count) == [1, 0, 0, 0, 2]
    want = g.place(dG, dGf, demb)
    for pair in (False, True):
        d_tab = torch.from_numpy(g.table(g.d_en, pair, np.float32("nan"))).cuda()
        grad = run_bwd(g, flat, cls, d_tab, pair)
        assert np.array_equal(grad, want.astype(np.float32), equal_nan=True)


def test_refusals_and_the_empty_call_on_the_device():
    """-4 with function and argument named before any launch; batch 0 returns 0 with NULLs (tests/test_gclass_abi.py sweeps every
    argument without a device; here: the device buffers stay as they were)"""
    from music_amd import _lib
    from music_amd._lib import ptr
    lib = _lib.load()
    g = Geometry(CASES[1], True, seed=5)
    flat, cls = torch.from_numpy(g.flat).cuda(), torch.from_numpy(g.cls).cuda()
    gb, grad = guarded(g.total)
    eb, enf = guarded(g.B * g.Sd)
    tb, tab = guarded(g.N * g.B * 2 * g.CH)
    st = _lib.stream()
    assert lib.wn_gclass_fwd(ptr(flat), ptr(tab), ptr(tab), ptr(enf), g.N, g.Dd, g.CH, g.Sd, g.B, ptr(cls), *g.goffsets, st) == -4
    assert "wn_gclass_fwd" in lib.wn_last_error().decode() and "'batch'" in lib.wn_last_error().decode()      # odd batch, pair table
    assert lib.wn_gclass_bwd(ptr(tab), 0, ptr(enf), ptr(flat), ptr(grad), g.N, g.Dd, g.CH, g.Sd, g.B, None, *g.goffsets, st) == -4
    assert "wn_gclass_bwd" in lib.wn_last_error().decode() and "'cls'" in lib.wn_last_error().decode()
    assert lib.wn_gclass_fwd(None, None, None, None, g.N, g.Dd, g.CH, g.Sd, 0, None, *g.goffsets, st) == 0
    assert lib.wn_gclass_bwd(None, 0, None, None, None, g.N, g.Dd, g.CH, g.Sd, 0, None, *g.goffsets, st) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (gb, eb, tb))
