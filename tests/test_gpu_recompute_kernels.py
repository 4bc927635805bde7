"""GPU tests of wn_resblock_bwd (resblock_bwd_k, the recompute half of the gated block's backward), one launch at a time,
against float64 (run with -m gpu).

Rules of tests/test_gpu_block_kernels.py: every test fills its own device buffers and launches ONE entry point; dfg and z are NaN
everywhere beforehand (slack and the gap between clips included) and must be NaN outside [t_lo, t_hi) afterwards; the inputs hold
NaN wherever include/wavenet_hip.h says their values do not count (x_in below t_lo - d and from t_hi on, dy outside the window, dz
below z_lo and from t_hi on, bias rows >= n_f, table columns >= cond_le, the gaps between clips); no element is left out of a
comparison; every case is launched twice into fresh buffers and must give the same bits.  The reference is tests/recompute_ref.py
(the header's formulas in float64, itself held to float64 autograd by tests/test_recompute_ref.py), evaluated from the very float32
arrays the kernel reads.

`_route` mirrors wn_launch_resblock_bwd's dispatch; test_cases_reach_every_instantiation asserts that the parametrisation reaches
all eight resblock_bwd_k instantiations by name.

Bars - the project's own, each tensor against its reference's max-abs:
  df, dg  x3 pairs  BAR64 = 1e-4 (tests/test_gpu_block_kernels.py)      x1 pairs  TOL[BF16X1] = 5e-2 (tests/test_gpu_kernels.py)
  z       F16X3 1e-5 (test_resblock_bwd_and_dx)   BF16X3 2e-4 (test_resblock_fwd)   F16X1 / BF16X1  TOL = 1e-2 / 5e-2
The x1 bars cannot see a subtly wrong x1 instantiation, so every x1 instantiation also runs on operands that both 16-bit formats
hold exactly (multiples of 2^-6 below 1/2: the products are exact, accumulation and gate are fp32 as in x3) and is held to the
x3 bars there.

Largest errors observed on an MI355X (df / dg / z as fractions of the reference's max-abs, over all cases of the instantiation;
"exact": the exactly representable operands):
  resblock_bwd_k<F16, 3, BF16, 3, 32>    6.6e-06 / 9.6e-06 / 1.3e-06
  resblock_bwd_k<F16, 3, BF16, 3, 64>    6.5e-06 / 7.2e-06 / 1.9e-06
  resblock_bwd_k<BF16, 3, BF16, 3, 32>   2.1e-05 / 2.1e-05 / 4.3e-05
  resblock_bwd_k<BF16, 3, BF16, 3, 64>   3.0e-05 / 2.7e-05 / 6.2e-05
  resblock_bwd_k<F16, 1, BF16, 1, 32>    3.0e-03 / 3.0e-03 / 3.3e-03     exact 2.2e-07 / 2.9e-07 / 2.7e-07
  resblock_bwd_k<F16, 1, BF16, 1, 64>    2.7e-03 / 3.0e-03 / 4.6e-03     exact 3.2e-07 / 3.5e-07 / 2.8e-07
  resblock_bwd_k<BF16, 1, BF16, 1, 32>   1.4e-02 / 9.5e-03 / 2.6e-02     exact 2.2e-07 / 2.9e-07 / 2.7e-07
  resblock_bwd_k<BF16, 1, BF16, 1, 64>   1.7e-02 / 1.4e-02 / 2.9e-02     exact 3.2e-07 / 3.5e-07 / 2.8e-07

Two things the kernel's structure decides, found by mutating it:
  - The `t >= t_lo` half of the dy mask cannot change any output: a dy column enters the Wd^T product's column of the same t
    only, and columns below t_lo are never stored.  No case can see it dropped (NaN in dy below t_lo stays in columns that the
    masked stores leave out).
  - With NaN where the inputs do not count, everything the kernel computes outside the window is NaN as well, and an unmasked
    store of it disappears in the NaN-filled outputs.  The *_finite_surroundings tests repeat the launches with finite values
    there; they are the ones that catch a plain 4-column store of z or dfg."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import ptr
from music_amd.engine import SLACK
from tests import recompute_ref
from tests.test_gpu_kernels import _packed, _fg_pack, TOL
from tests.test_gpu_block_kernels import BAR64, NAN, _same_bits, _written, _all_zero

DEV = "cuda"
F16X3, F16X1, BF16X3, BF16X1 = _lib.F16X3, _lib.F16X1, _lib.BF16X3, _lib.BF16X1
PAIRS = {"f16x3": (F16X3, BF16X3), "f16x1": (F16X1, BF16X1), "bf16x3": (BF16X3, BF16X3), "bf16x1": (BF16X1, BF16X1)}
SHAPES = [(32, 32, 32), (32, 20, 16), (64, 64, 64), (64, 48, 40)]                      # (ch, R, D)
SHAPE_ID = ["ch%d-R%d-D%d" % s for s in SHAPES]
VARIANTS = ["plain", "bias", "table1", "table2", "nody"]
_T = {F16X3: "F16, 3", F16X1: "F16, 1", BF16X3: "BF16, 3", BF16X1: "BF16, 1"}
INSTANTIATIONS = {"resblock_bwd_k<%s, %s, %d>" % (_T[mf], _T[mb], ch) for mf, mb in PAIRS.values() for ch in (32, 64)}


def _route(mf, mb, ch, pitch=4, t_lo=0, t_hi=1, batch=1):
    """Mirror of wn_resblock_bwd / wn_launch_resblock_bwd: the status of a refused call, None for an empty launch, else the
    instantiation the call reaches."""
    if pitch % 4 != 0:
        return -4
    if t_hi <= t_lo or batch <= 0:
        return None
    if (mf, mb) not in PAIRS.values():
        return -2
    if ch not in (32, 64):
        return -3
    return "resblock_bwd_k<%s, %s, %d>" % (_T[mf], _T[mb], ch)


def _flat(a):
    """numpy float32 array -> flat device buffer with NaN slack in front and behind"""
    t = np.full(SLACK + a.size + 512, NAN, np.float32)
    t[SLACK:SLACK + a.size] = a.reshape(-1)
    return torch.from_numpy(t).to(DEV)


def _rel(got, ref):
    """max |got - ref| / max |ref| (NaN, which fails every <=, when got holds a NaN); an all-zero reference wants exact zeros"""
    m = np.abs(ref).max()
    e = np.abs(got.astype(np.float64) - ref).max()
    if m == 0:
        return 0.0 if e == 0 else float("inf")
    return e / m


class _Block:
    """Inputs of one wn_resblock_bwd call, its launch into NaN-filled outputs and the float64 reference.
    cond = (rule, le); dy=False passes dy = NULL; exact: x, weights and dy are multiples of 2^-6 in [-1/2, 1/2].
    junk: the columns of x_in, dy and dz that do not count hold finite random values instead of NaN.  With NaN there the kernel's
    own values outside the window are NaN too, and a stray store of them into the NaN-filled outputs would go unseen."""
    GAP = dict(x=2, dz=1, dfg=3, z=1, tab=1)                  # NaN rows between the clips: every batch stride > rows * pitch

    def __init__(self, pair, ch, R, D, d, t_lo, t_hi, z_lo, B=2, bias=False, cond=None, dy=True, exact=False, seed=0,
                 junk=False):
        assert t_lo >= d and t_hi > t_lo and z_lo >= t_lo                  # x[t_lo - d] exists; the tile origin - d stays in the slack
        self.mf, self.mb = PAIRS[pair]
        self.pair, self.ch, self.R, self.D, self.d, self.B = pair, ch, R, D, d, B
        self.t_lo, self.t_hi, self.z_lo, self.exact = t_lo, t_hi, z_lo, exact
        self.pitch = pitch = (t_hi + 512 + 255) // 256 * 256              # the launch's 512-column tiles end below t_hi + 512
        rng = np.random.default_rng(seed)
        if exact:
            draw = lambda *s: (rng.integers(-32, 33, size=s) / 64.0).astype(np.float32)
            self.wf, self.wg, self.wd = draw(D, R, 2), draw(D, R, 2), draw(R, D, 1)
        else:
            draw = lambda *s: rng.standard_normal(s).astype(np.float32)
            self.wf, self.wg, self.wd = draw(D, R, 2) * 0.3, draw(D, R, 2) * 0.3, draw(R, D, 1) * 0.3
        self.pfg, _ = _fg_pack(self.wf, self.wg, ch, self.mf)
        wdT = np.zeros((ch, ch), np.float32)
        wdT[:D, :R] = self.wd[:, :, 0].T
        self.pdT = _packed(wdT, self.mb)
        G = self.GAP
        self.x = np.full((B, ch + G["x"], pitch), NAN, np.float32)
        self.x[:, :R, t_lo - d:t_hi] = draw(B, R, t_hi - t_lo + d)
        self.x[:, R:ch, t_lo - d:t_hi] = 0                                # padded rows are zero inside the windows (the layout's contract)
        self.dy = None
        if dy:
            self.dy = np.full((B, ch + G["x"], pitch), NAN, np.float32)   # dy shares x's batch stride
            self.dy[:, :R, t_lo:t_hi] = draw(B, R, t_hi - t_lo) * (1.0 if exact else 1e-3)
            self.dy[:, R:ch, t_lo:t_hi] = 0
        self.dz = np.full((B, ch + G["dz"], pitch), NAN, np.float32)      # z_lo >= t_hi: NaN throughout
        if z_lo < t_hi:
            self.dz[:, :D, z_lo:t_hi] = rng.standard_normal((B, D, t_hi - z_lo)).astype(np.float32) * (0.25 if exact else 1e-3)
            self.dz[:, D:ch, z_lo:t_hi] = 0
        self.bias = None
        if bias:
            self.bias = np.full((2, ch), NAN, np.float32)                 # rows >= n_f = D are not read
            self.bias[:, :D] = rng.standard_normal((2, D)).astype(np.float32)
        self.cond = None
        if cond is not None:
            rule, le = cond
            self.cond = dict(mode=rule, le=le, q=max(1, (t_hi - t_lo) // le) if rule == 1 else 0, pitch=le + 5)
            self.tab = np.full((B, 2 * ch + G["tab"], le + 5), NAN, np.float32)      # columns >= cond_le are not read
            for r0 in (0, ch):
                self.tab[:, r0:r0 + D, :le] = rng.standard_normal((B, D, le)).astype(np.float32) * 0.5
                self.tab[:, r0 + D:r0 + ch, :le] = 0
        if junk:
            for a in (self.x, self.dy, self.dz):
                if a is not None:
                    a[np.isnan(a)] = rng.standard_normal(int(np.isnan(a).sum())).astype(np.float32)
        self.dev = dict(x=_flat(self.x), dz=_flat(self.dz), dy=_flat(self.dy) if dy else None,
                        bias=torch.from_numpy(self.bias).to(DEV) if bias else None,
                        tab=torch.from_numpy(self.tab).to(DEV) if cond is not None else None)

    def route(self):
        return _route(self.mf, self.mb, self.ch, self.pitch, self.t_lo, self.t_hi, self.B)

    def reference(self):
        c = self.cond
        kw = dict(tab=self.tab, tab_g_row=self.ch, cond_mode=c["mode"], cond_le=c["le"], cond_q=c["q"]) if c else {}
        if self.bias is not None:
            kw.update(bias_f=self.bias[0], bias_g=self.bias[1])
        return recompute_ref.recompute_bwd(self.x, self.wf, self.wg, self.wd, self.d, self.t_lo, self.t_hi, self.z_lo, dy=self.dy,
                                           dz=self.dz, **kw)

    def call(self, dfg, z, **over):
        """the raw status of one wn_resblock_bwd call on this case's buffers; `over` replaces arguments by name"""
        ch, pitch, G, v, c = self.ch, self.pitch, self.GAP, self.dev, self.cond
        a = dict(x=ptr(v["x"], SLACK), dy=ptr(v["dy"], SLACK) if v["dy"] is not None else None, dz=ptr(v["dz"], SLACK),
                 dfg=ptr(dfg, SLACK), z=ptr(z, SLACK) if z is not None else None, x_bs=(ch + G["x"]) * pitch,
                 dz_bs=(ch + G["dz"]) * pitch, dfg_bs=(2 * ch + G["dfg"]) * pitch, z_bs=(ch + G["z"]) * pitch, pitch=pitch,
                 wfg=ptr(self.pfg), wdT=ptr(self.pdT), bias_f=ptr(v["bias"][0]) if v["bias"] is not None else None,
                 bias_g=ptr(v["bias"][1]) if v["bias"] is not None else None, n_f=self.D, ch=ch, d=self.d, t_lo=self.t_lo,
                 t_hi=self.t_hi, z_lo=self.z_lo, cond=ptr(v["tab"]) if c else None,
                 cond_bs=(2 * ch + G["tab"]) * c["pitch"] if c else 0, cond_pitch=c["pitch"] if c else 0,
                 cond_mode=c["mode"] if c else 0, cond_le=c["le"] if c else 0, cond_q=c["q"] if c else 0, batch=self.B,
                 mode_fwd=self.mf, mode_bwd=self.mb)
        assert set(over) <= set(a)
        a.update(over)
        rc = _lib.load().wn_resblock_bwd(*a.values(), _lib.stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        G = self.GAP
        return (_flat(np.full((self.B, 2 * self.ch + G["dfg"], self.pitch), NAN, np.float32)),
                _flat(np.full((self.B, self.ch + G["z"], self.pitch), NAN, np.float32)))

    def launch(self, store_z=True):
        dfg, z = self.outputs()
        rc = self.call(dfg, z if store_z else None)
        assert rc == 0, (rc, _lib.load().wn_last_error().decode())
        if not store_z:
            assert _written(z) == 0
        return dfg.cpu(), z.cpu()

    def bars(self):
        x3 = self.exact or self.mf in (F16X3, BF16X3)
        half = self.mf in (F16X3, F16X1)
        if x3:
            return BAR64, (1e-5 if half else 2e-4)
        return TOL[BF16X1], TOL[self.mf]

    def check(self, tag):
        """two launches, same bits; exactly the windows written; padded rows exact zeros; every written element compared"""
        B, ch, D, t_lo, t_hi, G = self.B, self.ch, self.D, self.t_lo, self.t_hi, self.GAP
        L = t_hi - t_lo
        dfg_raw, z_raw = self.launch()
        dfg2, z2 = self.launch()
        assert _same_bits(dfg_raw, dfg2) and _same_bits(z_raw, z2), tag + ": a second launch gives other bits"
        assert _written(dfg_raw) == B * 2 * ch * L, tag + ": dfg written outside its window, or not all of it"
        assert _written(z_raw) == B * ch * L, tag + ": z written outside its window, or not all of it"
        dfg = dfg_raw[SLACK:SLACK + B * (2 * ch + G["dfg"]) * self.pitch].view(B, 2 * ch + G["dfg"], self.pitch)[:, :2 * ch, t_lo:t_hi]
        z = z_raw[SLACK:SLACK + B * (ch + G["z"]) * self.pitch].view(B, ch + G["z"], self.pitch)[:, :ch, t_lo:t_hi]
        assert not torch.isnan(dfg).any() and not torch.isnan(z).any(), tag + ": NaN inside a window"
        assert _all_zero(dfg[:, D:ch]) and _all_zero(dfg[:, ch + D:]) and _all_zero(z[:, D:]), tag + ": a padded row is not zero"
        rf, rg, rz = self.reference()
        e = (_rel(dfg[:, :D].numpy(), rf), _rel(dfg[:, ch:ch + D].numpy(), rg), _rel(z[:, :D].numpy(), rz))
        dbar, zbar = self.bars()
        print("%s %s: df %.3g dg %.3g z %.3g (bars %g / %g)" % (self.route(), tag, e[0], e[1], e[2], dbar, zbar))
        assert e[0] <= dbar and e[1] <= dbar and e[2] <= zbar, (tag, e, dbar, zbar)
        return dfg_raw


# ================================================================================================ A. every instantiation
# d = 5, t_lo = 69 (t_lo % 4 = 1, tile origin 64), 601 columns: two workgroup tiles, the second ragged; the crop starts inside a
# lane's 4 columns.  table1: 601 // 7 = 85 columns per bucket, 7 * 85 = 595 < 601 - the clamp takes the last 6 columns.
# table2: 601 is no multiple of 100 (64 channels) or 31 (32 channels).
INST_GEOM = dict(d=5, t_lo=69, t_hi=670, z_lo=199)


def _variant(ch, variant):
    return dict(plain={}, bias=dict(bias=True), table1=dict(cond=(1, 7)), table2=dict(cond=(2, 100 if ch == 64 else 31)),
                nody=dict(dy=False), exact=dict(bias=True, cond=(1, 7)))[variant]


def _inst(pair, shape, variant, exact=False, junk=False):
    ch, R, D = shape
    return _Block(pair, ch, R, D, B=2, exact=exact, junk=junk, seed=len(variant) + R, **INST_GEOM, **_variant(ch, variant))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_every_instantiation(pair, shape, variant):
    _inst(pair, shape, variant).check("%s-%s" % (SHAPE_ID[SHAPES.index(shape)], variant))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_z_null_gives_the_same_dfg_bits(pair, shape):
    """z = NULL (the caller kept the forward's z): dfg has the bits of the launch that stored z, and z is not touched"""
    c = _inst(pair, shape, "table1")
    with_z = c.check("z-null")
    without, _ = c.launch(store_z=False)
    assert _same_bits(with_z, without)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_no_stray_store_with_finite_surroundings(pair, shape):
    """the same launch with finite values where the inputs do not count: what the kernel computes outside [t_lo, t_hi) is finite
    then, and a store of it outside the window shows in the NaN-filled dfg and z (a plain 4-column store of z does)"""
    _inst(pair, shape, "table1", junk=True).check("finite-surroundings")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("pair", ["f16x1", "bf16x1"])
def test_x1_on_exactly_representable_operands_meets_the_x3_bars(pair, shape):
    c = _inst(pair, shape, "exact", exact=True)
    for a in (c.x, c.dy, c.wf, c.wg, c.wd):                                  # both 16-bit formats hold every operand
        v = torch.from_numpy(a[~np.isnan(a)])
        assert torch.equal(v.half().float(), v) and torch.equal(v.bfloat16().float(), v)
    assert c.bars() == (BAR64, 1e-5 if pair == "f16x1" else 2e-4)
    c.check("exact")


def test_cases_reach_every_instantiation():
    t_lo, t_hi = INST_GEOM["t_lo"], INST_GEOM["t_hi"]
    reached = {_route(*PAIRS[pair], ch, 4, t_lo, t_hi, 2) for pair in PAIRS for ch, _, _ in SHAPES}
    assert reached == INSTANTIATIONS and len(INSTANTIATIONS) == 8
    assert {ch for ch, _, _ in SHAPES} == {32, 64} and any(R < ch and D < R for ch, R, D in SHAPES)
    L = t_hi - t_lo
    assert (t_hi - (t_lo & ~63)) > 512 and t_lo % 4 != 0 and INST_GEOM["z_lo"] % 4 != 0       # two tiles, unaligned window and crop
    for ch in (32, 64):                                                     # the variants reach the argument-dependent branches
        (r1, le1), (r2, le2) = _variant(ch, "table1")["cond"], _variant(ch, "table2")["cond"]
        assert r1 == 1 and le1 * (L // le1) < L and r2 == 2 and L % le2 != 0
        assert _variant(ch, "bias")["bias"] and _variant(ch, "nody")["dy"] is False and _variant(ch, "plain") == {}
    assert _variant(64, "table2")["cond"][1] > 64


# ================================================================================================ B. geometry
# (id, d, t_lo, t_hi, z_lo, B); the workgroup tile is 512 columns from t_lo & ~63, a wave owns 64 columns, a lane 4.
GEOM = [
    ("tlo%4=0", 2, 68, 218, 105, 2), ("tlo%4=1", 2, 69, 219, 106, 2), ("tlo%4=2", 2, 70, 220, 107, 2), ("tlo%4=3", 2, 71, 221, 108, 2),
    ("tlo%64=63", 2, 127, 300, 160, 2),
    ("one-column", 2, 70, 71, 70, 2), ("five-columns", 2, 70, 75, 72, 2),
    ("one-past-a-tile", 2, 70, 577, 300, 2), ("two-tiles-and-a-rest", 2, 70, 1125, 600, 1),
    ("zlo=tlo", 2, 72, 230, 72, 2), ("zlo-lane+1", 2, 72, 230, 101, 2), ("zlo-lane+2", 2, 72, 230, 102, 2),
    ("zlo-lane+3", 2, 72, 230, 103, 2), ("zlo-last-column", 2, 72, 230, 229, 2), ("zlo=thi", 2, 72, 230, 230, 2),
    ("zlo>thi", 2, 72, 230, 239, 2),
    ("d1-below-origin", 1, 128, 330, 150, 2), ("d3-below-origin", 3, 129, 330, 150, 2), ("d64-below-origin", 64, 67, 270, 90, 2),
    ("d512-below-origin", 512, 515, 720, 600, 2),
    ("B1", 4, 77, 290, 133, 1), ("B3", 4, 77, 290, 133, 3),
]


def _geom(g, shape, junk=False):
    _, d, t_lo, t_hi, z_lo, B = g
    return _Block("f16x3", *shape, d, t_lo, t_hi, z_lo, B=B, bias=True, cond=(2, 7), seed=t_lo + d, junk=junk)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[SHAPE_ID[1], SHAPE_ID[3]])
@pytest.mark.parametrize("g", GEOM, ids=[g[0] for g in GEOM])
def test_geometry(g, shape):
    _geom(g, shape).check(g[0])


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[SHAPE_ID[1], SHAPE_ID[3]])
@pytest.mark.parametrize("g", GEOM, ids=[g[0] for g in GEOM])
def test_geometry_no_stray_store_with_finite_surroundings(g, shape):
    _geom(g, shape, junk=True).check(g[0] + " finite-surroundings")


def test_geometry_cases_are_what_their_ids_say():
    by = {g[0]: g for g in GEOM}
    assert [by["tlo%%4=%d" % k][2] % 4 for k in range(4)] == [0, 1, 2, 3] and by["tlo%64=63"][2] % 64 == 63
    assert by["one-column"][3] - by["one-column"][2] == 1 and by["five-columns"][3] - by["five-columns"][2] == 5
    _, _, lo, hi, _, _ = by["five-columns"]
    assert lo // 64 == (hi - 1) // 64 and lo // 4 != (hi - 1) // 4              # one wave's 64 columns, two lanes
    _, _, lo, hi, _, _ = by["one-past-a-tile"]
    assert hi == (lo & ~63) + 512 + 1
    _, _, lo, hi, _, _ = by["two-tiles-and-a-rest"]
    assert 2 * 512 < hi - (lo & ~63) < 3 * 512 and (hi - (lo & ~63)) % 64 not in (0, 63) and hi - lo <= 1100
    assert by["zlo=tlo"][4] == by["zlo=tlo"][2] and by["zlo=tlo"][2] % 4 == 0
    assert [by["zlo-lane+%d" % k][4] % 4 for k in (1, 2, 3)] == [1, 2, 3]
    assert by["zlo-last-column"][4] == by["zlo-last-column"][3] - 1 and by["zlo=thi"][4] == by["zlo=thi"][3] and by["zlo>thi"][4] > by["zlo>thi"][3]
    for k in (1, 3, 64, 512):
        _, d, lo, _, _, _ = by["d%d-below-origin" % k]
        assert d == k and 0 <= lo - d < (lo & ~63)
    assert {by["B1"][5], by["B3"][5]} == {1, 3} and max(g[5] for g in GEOM) <= 3 and max(g[3] - g[2] for g in GEOM) <= 1100
    for g in GEOM:
        assert _route(F16X3, BF16X3, 64, 4, g[2], g[3], g[5]) == "resblock_bwd_k<F16, 3, BF16, 3, 64>"
    for name in ("zlo-last-column", "zlo=thi", "zlo>thi"):                      # z_lo >= t_hi: the whole of dz is NaN
        assert bool(np.isnan(_geom(by[name], SHAPES[1]).dz).all()) == (by[name][4] >= by[name][3])


# ================================================================================================ C. refusals and empty launches
@pytest.mark.parametrize("what,over,status", [
    ("unsupported-pair", dict(mode_fwd=F16X3, mode_bwd=F16X3), -2),
    ("bf16-recompute-f16-gradient", dict(mode_fwd=BF16X3, mode_bwd=F16X3), -2),
    ("ch48", dict(ch=48), -3),
    ("pitch-not-a-multiple-of-4", dict(pitch=1026), -4),
    ("t_hi=t_lo", dict(t_hi=72), 0),
    ("t_hi<t_lo", dict(t_hi=40), 0),
    ("batch=0", dict(batch=0), 0),
])
def test_refusals_and_empty_launches_write_nothing(what, over, status):
    c = _Block("f16x3", 64, 48, 40, 2, 72, 230, 101, B=2, bias=True, cond=(2, 7))
    a = dict(mode_fwd=c.mf, mode_bwd=c.mb, ch=c.ch, pitch=c.pitch, t_lo=c.t_lo, t_hi=c.t_hi, batch=c.B)
    a.update(over)
    want = _route(a["mode_fwd"], a["mode_bwd"], a["ch"], a["pitch"], a["t_lo"], a["t_hi"], a["batch"])
    assert (want if isinstance(want, int) else 0) == status and not isinstance(want, str)
    dfg, z = c.outputs()
    assert c.call(dfg, z, **over) == status
    assert _written(dfg) == 0 and _written(z) == 0
