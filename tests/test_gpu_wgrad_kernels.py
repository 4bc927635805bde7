"""GPU tests of the weight-gradient launches, one launch at a time, against float64 (run with -m gpu).

wn_wgrad (the three code paths of wn_wgrad.hip), wn_reduce_slabs and wn_bias_grad, each on buffers the test fills itself.  The
reference is the defining sum of include/wavenet_hip.h evaluated in float64 (torch.einsum) on the very float32 inputs the kernel
read; ReLU is applied to the float32 values, so there is no tie.  Every buffer is larger than its tensor and NaN wherever the
header says the values do not count: the operands everywhere outside [t_lo + shift, t_hi + shift) of each row (the slack in front
of the first row and the tail behind the last included), the slab buffer everywhere with one slab more than wn_wgrad_slabs()
says, `out` around every written range.  After the launch exactly the declared elements are non-NaN, and a second launch into
fresh buffers gives the same bits.  No element is left out of a comparison.

The test ids name the kernel form the dispatch rule of wn_wgrad.hip selects (restated on the host in Geo.form):
  big    mt >= 16 and nt_total >= 16: wgrad_big_k, LDS-shared fragments, a plain and a guarded time loop per workgroup chunk;
  split8 one 64 x 64 block: wgrad_k with the chunk split eight ways in time;
  tiled  everything else: wgrad_k, four blocks per workgroup, two time shares;
and whether the guarded loads must be taken (Geo.guard, from tb_lo / tb_hi as the kernels form them): plain / guarded / mixed.

Bars
  BF16X3: 5e-5 of the reference's max-abs, this kernel's bar in test_gpu_kernels.py (test_wgrad_compact_relu).
  F16X3, F16X1, BF16X1: four times the error of the operand rounding alone - hi = round16(x), lo = round16(x - hi), products
  hi hi + hi lo + lo hi (x3) or hi hi (x1) summed in float64 on the test's own inputs (_emulated); the factor covers the fp32
  accumulation over B (t_hi - t_lo) terms in the kernel's order.  The inputs are scaled so that the emulated F16X3 error of
  every case stays under a quarter of 5e-5 (asserted): B = activations of 1, A = gradients of 1e-2 - at the 1e-3 of the
  existing tests the lo halves of A are f16 denormals and a one-column window emulates to 1.9e-5.
  wn_reduce_slabs / wn_bias_grad: the bound of any fixed-order fp32 sum of N terms, N 2^-23 sum |terms|, per element."""
import functools
from dataclasses import dataclass, replace

import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from music_amd.engine import SLACK
from tests.helpers import nan_rows

DEV = "cuda"
NAN = float("nan")
BAR_BF16X3 = 5e-5
A_SCALE, B_SCALE = 1e-2, 1.0
MODE_NAME = {_lib.BF16X3: "bf16x3", _lib.F16X3: "f16x3", _lib.BF16X1: "bf16x1", _lib.F16X1: "f16x1"}
WORST = {}                                          # mode name -> (worst observed, its emulated figure, case)


# ------------------------------------------------------------------------------------------------ one wn_wgrad call
@dataclass(frozen=True)
class Geo:
    """Geometry of ONE wn_wgrad call.  A has 16 mt rows, every tap of B 16 ntp rows; row-pitched operands share one pitch and
    a_cols = b_cols = pitch (end_at_cols: pitch = t_hi, the window ends where the rows end); compact: A is [B][16 mt][W]
    with a_pitch = a_cols = W = t_hi - t_lo and a_shift = -t_lo.  C: ldc columns (0: just the 16 ntp taps written), c_rows rows
    per slab (0: 16 mt), c_pad floats more per slab, written from column c_col0 on."""
    name: str
    mt: int
    ntp: int
    taps: int = 1
    shifts: tuple = (0, 0)
    t_lo: int = 96
    t_hi: int = 700
    chunk: int = 256
    B: int = 2
    compact: bool = False
    relu: int = 0
    end_at_cols: bool = False
    ldc: int = 0
    c_rows: int = 0
    c_pad: int = 0
    c_col0: int = 0
    seed: int = 0

    # ---- derived
    @property
    def W(self):
        return self.t_hi - self.t_lo

    @property
    def width(self):
        return 16 * self.ntp * self.taps

    @property
    def ld(self):
        return self.ldc or self.width

    @property
    def rows(self):
        return self.c_rows or 16 * self.mt

    @property
    def stride(self):
        return self.rows * self.ld + self.c_pad

    @property
    def pitch(self):
        if self.end_at_cols:
            return self.t_hi
        return (self.t_hi + max(0, *self.shifts[:self.taps]) + 36 + 3) // 4 * 4

    @property
    def chunk_eff(self):
        """the launcher's chunk: at least 128, rounded up to a multiple of 128"""
        return (max(self.chunk, 128) + 127) // 128 * 128

    @property
    def t_base(self):
        return self.t_lo & ~31

    @property
    def n_chunks(self):
        return -(-(self.t_hi - self.t_base) // self.chunk_eff)

    def form(self):
        nt = self.ntp * self.taps
        if self.mt >= 16 and nt >= 16:
            return "big"
        return "split8" if ((nt + 3) // 4) * ((self.mt + 3) // 4) == 1 else "tiled"

    def guard(self):
        """must the guarded loads be taken?  [tb_lo, tb_hi] = the k-steps whose 32 samples are addressable in every operand
        row; wgrad_k decides per k-step, wgrad_big_k per workgroup chunk (first and last k-step of the chunk)."""
        sh = self.shifts[:self.taps]
        a_shift, a_cols = (-self.t_lo, self.W) if self.compact else (0, self.pitch)
        tb_lo = -min(a_shift, *sh)
        tb_hi = min(a_cols - a_shift, self.pitch - max(sh)) - 32
        if self.form() == "big":
            plain = []
            for j in range(self.n_chunks):
                tc0 = self.t_base + j * self.chunk_eff
                tc1 = min(tc0 + self.chunk_eff, self.t_hi)
                last = tc0 + ((tc1 - 1 - tc0) & ~31)
                plain.append(tc0 >= tb_lo and last <= tb_hi)
        else:
            plain = [tb_lo <= tb <= tb_hi for tb in range(self.t_base, self.t_hi, 32)]
        return "plain" if all(plain) else "mixed" if any(plain) else "guarded"

    def declared(self):
        """bool [stride]: the elements of one slab this call writes"""
        m = torch.zeros(self.stride, dtype=torch.bool)
        m[:self.rows * self.ld].view(self.rows, self.ld)[:16 * self.mt, self.c_col0:self.c_col0 + self.width] = True
        return m


@functools.lru_cache(maxsize=None)
def _inputs(g):
    """(A window [B][16 mt][W], per tap the B window [B][16 ntp][W] aligned with it, float64 reference [16 mt][width]).
    Window column i is time t_lo + i; a tap whose column t_lo + i + shift lies below 0 reads zero there."""
    gen = torch.Generator().manual_seed(1000 + g.seed)
    a = torch.randn(g.B, 16 * g.mt, g.W, generator=gen) * A_SCALE
    gen = torch.Generator().manual_seed(2000 + g.seed + g.c_col0)
    bs = []
    for j in range(g.taps):
        v = torch.randn(g.B, 16 * g.ntp, g.W, generator=gen) * B_SCALE
        v[:, :, :max(0, -(g.t_lo + g.shifts[j]))] = 0
        bs.append(v)
    ref = torch.cat([torch.einsum("bmt,bnt->mn", a.double(), (v.clamp(min=0) if g.relu else v).double()) for v in bs], 1)
    return a, tuple(bs), ref


def _rel(got, ref):
    """max |got - ref| / max |ref|; NaN (which fails every <=) when anything in got is NaN"""
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


@functools.lru_cache(maxsize=None)
def _emulated(g, mode):
    """error of the operand rounding alone against the float64 reference, relative to its max-abs: wn_split16's hi / lo
    (torch's casts round to nearest even as it does; x - hi is exact in float32), the mode's products, float64 sums"""
    dt = torch.bfloat16 if mode in (_lib.BF16X3, _lib.BF16X1) else torch.float16
    x3 = mode in (_lib.BF16X3, _lib.F16X3)

    def split(x):
        hi = x.to(dt).float()
        lo = (x - hi).to(dt).float()
        return hi.double(), lo.double()

    a, bs, ref = _inputs(g)
    ah, al = split(a)
    cols = []
    for v in bs:
        bh, bl = split(v.clamp(min=0) if g.relu else v)
        c = torch.einsum("bmt,bnt->mn", ah, bh)
        if x3:
            c = c + torch.einsum("bmt,bnt->mn", ah, bl) + torch.einsum("bmt,bnt->mn", al, bh)
        cols.append(c)
    return _rel(torch.cat(cols, 1), ref)


def _bar(g, mode):
    if mode == _lib.F16X3:
        assert _emulated(g, mode) <= BAR_BF16X3 / 4, "rescale the inputs: emulated f16x3 error %.3g" % _emulated(g, mode)
    return BAR_BF16X3 if mode == _lib.BF16X3 else 4 * _emulated(g, mode)


def _operands(g):
    """device buffers of the call: NaN everywhere outside the window of each row"""
    a, bs, _ = _inputs(g)
    if g.compact:
        da = nan_rows(a, g.W, 0, SLACK)
    else:
        da = nan_rows(a, g.pitch, g.t_lo, SLACK)
    db = [nan_rows(v, g.pitch, g.t_lo + g.shifts[j], SLACK) for j, v in enumerate(bs)]
    return da.to(DEV), [t.to(DEV) for t in db]


def _wgrad_args(g, da, db, slab, mode):
    a_head = (16 * g.mt * g.W, g.W, -g.t_lo, g.W) if g.compact else (16 * g.mt * g.pitch, g.pitch, 0, g.pitch)
    return (ptr(da, SLACK), *a_head, ptr(db[0], SLACK), ptr(db[1], SLACK) if g.taps == 2 else None, 16 * g.ntp * g.pitch,
            g.pitch, g.shifts[0], g.shifts[1], g.pitch, g.ntp, g.mt, g.relu, ptr(slab, g.c_col0), g.ld, g.stride, g.t_lo,
            g.t_hi, g.chunk, g.B, mode, _lib.stream())


def _n_slabs(g):
    """wn_wgrad_slabs, checked against the launcher's rule restated here"""
    ns = _lib.wgrad_slabs(g.t_lo, g.t_hi, g.chunk, g.B)
    assert ns == g.B * g.n_chunks, (ns, g.B, g.n_chunks)
    return ns


def _reduce(slab, ns, stride):
    """wn_reduce_slabs over ns whole slabs (NaN columns sum to NaN) into a NaN-surrounded buffer -> CPU [stride + 8]"""
    out = torch.full((stride + 8,), NAN, device=DEV)
    desc = torch.tensor([[0, 0, ns, stride, 4, stride]], dtype=torch.int64, device=DEV)
    call("wn_reduce_slabs", ptr(desc), 1, (stride + 3) // 4, ptr(slab), ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out.cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_slabs(g, slab, ns, declared, tag):
    s = slab.view(ns + 1, g.stride)
    assert torch.isnan(s[ns]).all(), tag + ": the slab behind the last one was written"
    written = ~torch.isnan(s[:ns])
    assert int(written.any(1).sum()) == ns, tag + ": %d slabs written, wn_wgrad_slabs says %d" % (int(written.any(1).sum()), ns)
    assert torch.equal(written, declared.expand(ns, -1)), tag + ": written elements differ from the declared ones (or NaN inside)"
    assert torch.isfinite(s[:ns][:, declared]).all(), tag + ": a slab element is not finite"


def _check_out(g, out, declared, tag):
    assert torch.isnan(out[:4]).all() and torch.isnan(out[4 + g.stride:]).all(), tag + ": wn_reduce_slabs wrote outside [out_off, out_off + n)"
    body = out[4:4 + g.stride]
    assert torch.equal(~torch.isnan(body), declared), tag + ": columns outside the written width are not NaN (or NaN inside)"
    got = body[declared]
    assert torch.isfinite(got).all(), tag + ": result is not finite"
    return got


def _run(g, mode):
    """one wn_wgrad launch + wn_reduce_slabs, every canary checked -> (slab, out, C [16 mt][width])"""
    tag = g.name
    da, db = _operands(g)
    ns = _n_slabs(g)
    slab = torch.full(((ns + 1) * g.stride,), NAN, device=DEV)
    call("wn_wgrad", *_wgrad_args(g, da, db, slab, mode))
    torch.cuda.synchronize()
    declared = g.declared()
    sc = slab.cpu()
    _check_slabs(g, sc, ns, declared, tag)
    out = _reduce(slab, ns, g.stride)
    got = _check_out(g, out, declared, tag).view(16 * g.mt, g.width)
    return sc, out, got


def _note(mode, err, emu, name):
    k = MODE_NAME[mode]
    if k not in WORST or err > WORST[k][0]:
        WORST[k] = (err, emu, name)


def _case(g, mode):
    _, _, ref = _inputs(g)
    bar = _bar(g, mode)
    emu = _emulated(g, mode)
    s1, o1, got = _run(g, mode)
    err = _rel(got, ref)
    _note(mode, err, emu, g.name)
    print("  wgrad %-24s %-6s %-7s %s: rel err %.3g (operand rounding alone %.3g, bar %.3g)"
          % (g.name, g.form(), g.guard(), MODE_NAME[mode], err, emu, bar))
    assert err <= bar, (g.name, err, bar)
    s2, o2, _ = _run(g, mode)
    assert _same_bits(s1, s2) and _same_bits(o1, o2), g.name + ": a repeated launch gives other bits"


# ------------------------------------------------------------------------------------------------ the case table
FORMS = [
    # split8: one 64 x 64 block
    Geo("dWd64", 4, 4, seed=1),
    Geo("dWd32-ldc64", 2, 2, ldc=64, c_rows=64, seed=2),
    Geo("dWfg32-d1", 4, 2, 2, (-1, 0), seed=3),
    Geo("dWfg32-d5", 4, 2, 2, (-5, 0), seed=4),
    Geo("dWfg32-d64", 4, 2, 2, (-64, 0), seed=5),
    # tiled
    Geo("dWfg64", 8, 4, 2, (-4, 0), seed=6),
    Geo("ragged3x5", 3, 5, c_pad=12, seed=7),
    Geo("ch160", 10, 10, seed=8),
    # big
    Geo("p1", 16, 16, t_hi=600, seed=9),
    Geo("p2-compact-relu", 16, 16, t_hi=600, compact=True, relu=1, seed=10),
    Geo("skip16x24", 16, 24, t_hi=600, relu=1, seed=11),
    Geo("rows17x16", 17, 16, t_hi=600, seed=12),
]
BASE = {"split8": Geo("s8", 4, 2, 2, (-5, 0)), "tiled": Geo("ti", 3, 5), "big": Geo("bg", 16, 16)}
X3 = (_lib.BF16X3, _lib.F16X3)


def _table():
    cases = [(g, m) for g in FORMS for m in X3]
    for f, base in BASE.items():
        # window: t_lo % 32 in {0, 1, 31} x spans {1, 31, 32, 33, chunk, chunk + 1} at the smallest chunk; batch 1 and 3
        for i, t_lo in enumerate((64, 65, 95)):
            for j, span in enumerate((1, 31, 32, 33, 128, 129)):
                g = replace(base, name="%s-lo%d-w%d" % (base.name, t_lo, span), t_lo=t_lo, t_hi=t_lo + span, chunk=128,
                            B=(1, 3)[(i + j) % 2], seed=100 + 10 * i + j)
                cases.append((g, X3[(i + j // 2) % 2]))
        # chunk: clamped (1, 100), kept (128, 384, 2048), rounded up (130)
        for j, chunk in enumerate((1, 100, 128, 130, 384, 2048)):
            g = replace(base, name="%s-chunk%d" % (base.name, chunk), t_lo=70, t_hi=70 + (700 if f != "big" else 500), chunk=chunk,
                        B=(3, 1)[j % 2], seed=200 + j)
            cases.append((g, X3[j % 2]))
        # the window ends where the rows end; compact A of an odd width; tap 0 below column 0
        cases.append((replace(base, name=base.name + "-ends-at-cols", t_lo=40, t_hi=555, end_at_cols=True, seed=300), _lib.BF16X3))
        cases.append((replace(base, name=base.name + "-compact-W333", t_lo=77, t_hi=410, compact=True, relu=1, B=3, seed=301), _lib.BF16X3))
        cases.append((replace(base, name=base.name + "-compact-W45", t_lo=31, t_hi=76, compact=True, B=1, seed=302), _lib.F16X3))
        cases.append((replace(base, name=base.name + "-compact-W29", t_lo=33, t_hi=62, compact=True, B=3, seed=308), _lib.BF16X3))
        # one case per form in the plain 16-bit modes
        cases.append((replace(base, name=base.name + "-x1", seed=303), _lib.BF16X1))
        cases.append((replace(base, name=base.name + "-x1", seed=303), _lib.F16X1))
    # t_lo < d: tap 0 reads columns below 0 as zero (the big form needs two taps of 8 tiles for that)
    cases.append((Geo("s8-tlo3-d5", 4, 2, 2, (-5, 0), t_lo=3, t_hi=300, seed=304), _lib.BF16X3))
    cases.append((Geo("ti-tlo3-d5", 8, 4, 2, (-5, 0), t_lo=3, t_hi=300, seed=305), _lib.F16X3))
    cases.append((Geo("bg-tlo3-d5", 16, 8, 2, (-5, 0), t_lo=3, t_hi=300, B=1, seed=306), _lib.BF16X3))
    cases.append((Geo("bg-tlo1-d64", 16, 8, 2, (-64, 0), t_lo=1, t_hi=150, B=3, relu=1, seed=307), _lib.F16X3))
    return cases


def _id(g, mode):
    return "%s-%s-%s-%s" % (g.name, g.form(), g.guard(), MODE_NAME[mode])


CASES = _table()


@pytest.mark.parametrize("g,mode", CASES, ids=[_id(g, m) for g, m in CASES])
def test_wgrad(g, mode):
    _case(g, mode)


def test_wgrad_case_table_covers_what_it_claims():
    """the host-side predicates put every case where its name says, and every (form, guard) pair that exists is run"""
    assert [g.form() for g in FORMS] == ["split8"] * 5 + ["tiled"] * 3 + ["big"] * 4
    assert all(g.form() == f for f, g in BASE.items())
    seen = {(g.form(), g.guard()) for g, _ in CASES}
    assert seen == {(f, k) for f in BASE for k in ("plain", "guarded", "mixed")}, seen
    for f in BASE:
        assert {m for g, m in CASES if g.form() == f} == set(MODE_NAME), f
        assert {g.B for g, _ in CASES if g.form() == f} >= {1, 2, 3}
        assert {g.t_lo % 32 for g, _ in CASES if g.form() == f} >= {0, 1, 31}
    ch160 = FORMS[7]
    assert ((ch160.ntp + 3) // 4) * ((ch160.mt + 3) // 4) == 9                 # last y-group: three inactive waves
    assert len({_id(g, m) for g, m in CASES}) == len(CASES)


@pytest.mark.parametrize("mode", X3, ids=[MODE_NAME[m] for m in X3])
def test_wgrad_three_taps_two_calls_into_one_c(mode):
    """the general plan's filter width 3: taps 0 and 1 in one call, tap 2 in a second one (b1 = NULL, c moved 2 n columns on),
    both into slabs of ldc = 3 n; the second call leaves the first call's columns bit for bit"""
    n, d = 96, 3
    g1 = Geo("taps01", 6, 6, 2, (-2 * d, -d), t_lo=50, t_hi=650, ldc=3 * n, seed=400)
    g2 = replace(g1, name="tap2", taps=1, shifts=(0, 0), c_col0=2 * n)
    assert g1.form() == "tiled" and g2.form() == "tiled" and g1.stride == g2.stride == 96 * 3 * n
    a1, b1, ref1 = _inputs(g1)
    a2, b2, ref2 = _inputs(g2)
    assert torch.equal(a1, a2)                                                 # one A, three taps of B
    ref = torch.cat([ref1, ref2], 1)
    ns = _n_slabs(g1)
    assert ns == _n_slabs(g2)

    def run():
        slab = torch.full(((ns + 1) * g1.stride,), NAN, device=DEV)
        da, db = _operands(g1)
        call("wn_wgrad", *_wgrad_args(g1, da, db, slab, mode))
        torch.cuda.synchronize()
        first = slab.cpu()
        _check_slabs(g1, first, ns, g1.declared(), "taps 0, 1")
        da2, db2 = _operands(g2)
        call("wn_wgrad", *_wgrad_args(g2, da2, db2, slab, mode))
        torch.cuda.synchronize()
        both = slab.cpu()
        full = replace(g1, ntp=9)                                              # all 3 n columns declared
        assert torch.equal(full.declared(), g1.declared() | g2.declared())
        _check_slabs(full, both, ns, full.declared(), "taps 0, 1, 2")
        d1 = g1.declared().expand(ns, -1)
        assert _same_bits(both.view(ns + 1, -1)[:ns][d1], first.view(ns + 1, -1)[:ns][d1]), "the second call changed the first call's columns"
        out = _reduce(slab, ns, g1.stride)
        return both, out, _check_out(full, out, full.declared(), "three taps").view(96, 3 * n)

    s1, o1, got = run()
    errs = [_rel(got[:, :2 * n], ref1), _rel(got[:, 2 * n:], ref2)]
    bars = [_bar(g1, mode), _bar(g2, mode)]
    print("  wgrad three taps %s: rel err %.3g / %.3g (bars %.3g / %.3g)" % (MODE_NAME[mode], errs[0], errs[1], bars[0], bars[1]))
    for g, e in zip((g1, g2), errs):
        _note(mode, e, _emulated(g, mode), "three-taps-" + g.name)
    assert errs[0] <= bars[0] and errs[1] <= bars[1] and _rel(got, ref) <= max(bars)
    s2, o2, _ = run()
    assert _same_bits(s1, s2) and _same_bits(o1, o2)


def test_wgrad_no_work_and_refusal():
    """batch = 0 and t_hi <= t_lo return 0 and write nothing; a slab stride smaller than C returns -4 and writes nothing"""
    lib = _lib.load()
    g = Geo("nowork", 4, 4, t_lo=96, t_hi=300)
    da, db = _operands(g)
    slab = torch.full((4 * g.stride,), NAN, device=DEV)
    for what, gg in (("batch = 0", replace(g, B=0)), ("t_hi == t_lo", replace(g, t_hi=96)), ("t_hi < t_lo", replace(g, t_hi=64))):
        assert _lib.wgrad_slabs(gg.t_lo, gg.t_hi, gg.chunk, gg.B) == 0, what
        args = list(_wgrad_args(g, da, db, slab, _lib.BF16X3))
        args[18:22] = [gg.t_lo, gg.t_hi, gg.chunk, gg.B]
        assert lib.wn_wgrad(*args) == 0, what
        torch.cuda.synchronize()
        assert torch.isnan(slab).all(), what + ": something was written"
    args = list(_wgrad_args(g, da, db, slab, _lib.BF16X3))
    assert args[17] == g.stride == 64 * 64
    args[17] = g.stride - 1
    assert lib.wn_wgrad(*args) == -4
    assert b"stride" in lib.wn_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(slab).all(), "the refused call wrote something"


@pytest.fixture(scope="module", autouse=True)
def _worst_errors_per_mode():
    """after the module: the worst figure of every mode over the wn_wgrad cases (the figures of DESIGN.md section 2)"""
    yield
    for k, (err, emu, name) in sorted(WORST.items()):
        print("\n  wgrad worst %-6s: %.3g of max-abs (operand rounding alone %.3g) at %s" % (k, err, emu, name), end="")


# ------------------------------------------------------------------------------------------------ wn_reduce_slabs
# (n, n_slabs): the scalar tail (n % 4), the 8-way unrolled loop and its remainder (n_slabs % 8), large ops for the search
REDUCE_OPS = [(1, 1), (3, 2), (4, 7), (5, 8), (4096, 9), (4099, 16), (1, 17), (3, 8), (4, 9), (5, 17), (4096, 8), (4099, 7),
              (4, 1), (5, 2)]


def _reduce_table(ops, seed):
    """descriptor table + NaN-surrounded slab buffer (NaN between an op's n and its stride and between the ops) + the
    layout of `out` (NaN between the ops' ranges, out_off not a multiple of 4 for most) + float64 sums and bounds"""
    gen = torch.Generator().manual_seed(seed)
    desc, vals = [], []
    vec, soff = 0, 3
    ooff = 1
    for k, (n, ns) in enumerate(ops):
        stride = n + (0, 3, 5)[k % 3]
        desc.append([vec, soff, ns, stride, ooff, n])
        vals.append(torch.randn(ns, n, generator=gen))
        vec += (n + 3) // 4
        soff += ns * stride + (2, 0, 7)[k % 3]
        ooff += n + (1, 2, 3, 5)[k % 4]
    slab = torch.full((soff + 16,), NAN)
    for (_, so, ns, stride, _, n), v in zip(desc, vals):
        slab[so:so + ns * stride].view(ns, stride)[:, :n] = v
    return desc, vec, slab, ooff + 8, vals


def _reduce_launch(desc, total_vec, slab, out_len):
    out = torch.full((out_len,), NAN, device=DEV)
    dd = torch.tensor(desc, dtype=torch.int64, device=DEV)
    call("wn_reduce_slabs", ptr(dd), len(desc), total_vec, ptr(slab), ptr(out), _lib.stream())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("order", ["table", "one-op", "large-first"])
def test_reduce_slabs_descriptor_table(order):
    ops = {"table": REDUCE_OPS, "one-op": [(4099, 17)], "large-first": REDUCE_OPS[5:] + REDUCE_OPS[:5]}[order]
    assert order == "one-op" or (len(ops) >= 12 and {n for n, _ in ops} == {1, 3, 4, 5, 4096, 4099}
                                 and {s for _, s in ops} == {1, 2, 7, 8, 9, 16, 17})
    desc, total_vec, slab, out_len, vals = _reduce_table(ops, 7)
    assert any(d[4] % 4 for d in desc) and (order == "one-op" or any(d[3] > d[5] for d in desc)) and desc[0][0] == 0
    assert all(desc[k + 1][0] - desc[k][0] == (desc[k][5] + 3) // 4 for k in range(len(desc) - 1))
    sd = slab.to(DEV)
    out = _reduce_launch(desc, total_vec, sd, out_len)
    keep = torch.zeros(out_len, dtype=torch.bool)
    worst = 0.0
    for (_, _, ns, _, oo, n), v in zip(desc, vals):
        keep[oo:oo + n] = True
        got = out[oo:oo + n].double()
        assert torch.isfinite(got).all(), (order, n, ns, "not finite")
        bound = ns * 2.0 ** -23 * v.double().abs().sum(0)
        excess = ((got - v.double().sum(0)).abs() / bound).max().item()
        worst = max(worst, excess)
        assert excess <= 1.0, (order, n, ns, excess)
    assert torch.equal(~torch.isnan(out), keep), order + ": written outside the ops' [out_off, out_off + n)"
    print("  reduce_slabs %s: %d ops, worst |got - ref64| = %.3g of the bound n_slabs 2^-23 sum |slab|" % (order, len(ops), worst))
    assert _same_bits(out, _reduce_launch(desc, total_vec, sd, out_len)), order + ": a repeated launch gives other bits"


# ------------------------------------------------------------------------------------------------ wn_bias_grad
BIAS_CASES = [(rows, w, B, lay) for rows in (1, 37, 256) for w in (1, 255, 256, 257, 1500) for B in (1, 3)
              for lay in ("pitched", "compact") if lay == "pitched" or w % 2 == 1]


@pytest.mark.parametrize("rows,w,B,lay", BIAS_CASES, ids=["rows%d-w%d-B%d-%s" % c for c in BIAS_CASES])
def test_bias_grad(rows, w, B, lay):
    """out[row] = sum_{b, t} a[b][row][t + a_shift] on a row-pitched a (a_shift = 0) and on the compact one of the
    post_process_2.bias call (a_pitch = W odd, a_shift = -t_lo); NaN everywhere outside the window, out[rows:] stays NaN"""
    t_lo = 77
    gen = torch.Generator().manual_seed(rows * 7 + w)
    win = torch.randn(B, rows, w, generator=gen)
    if lay == "compact":
        a, pitch, shift = nan_rows(win, w, 0, SLACK), w, -t_lo
    else:
        pitch = (t_lo + w + 36 + 3) // 4 * 4
        a, shift = nan_rows(win, pitch, t_lo, SLACK), 0
    a = a.to(DEV)
    ref = win.double().sum((0, 2))
    bound = B * w * 2.0 ** -23 * win.double().abs().sum((0, 2))

    def run():
        out = torch.full((rows + 9,), NAN, device=DEV)
        call("wn_bias_grad", ptr(a, SLACK), rows * pitch, pitch, shift, rows, t_lo, t_lo + w, B, ptr(out, 3), _lib.stream())
        torch.cuda.synchronize()
        return out.cpu()

    out = run()
    assert torch.isnan(out[:3]).all() and torch.isnan(out[3 + rows:]).all(), "written outside out[0, rows)"
    got = out[3:3 + rows].double()
    assert torch.isfinite(got).all()
    excess = ((got - ref).abs() / bound).max().item()
    print("  bias_grad rows %d w %d B %d %s: worst %.3g of the bound N 2^-23 sum |a|" % (rows, w, B, lay, excess))
    assert excess <= 1.0
    assert _same_bits(out, run())


def test_bias_grad_no_work_writes_nothing():
    """no clips or no columns: returns 0 and leaves `out` alone, as wn_wgrad does with its slabs"""
    out = torch.full((8,), NAN, device=DEV)
    a = torch.zeros(256, device=DEV)
    lib = _lib.load()
    for rows, t_hi, B in ((0, 20, 1), (4, 10, 1), (4, 5, 1), (4, 20, 0)):
        assert lib.wn_bias_grad(ptr(a), 64, 16, 0, rows, 10, t_hi, B, ptr(out), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (rows, t_hi, B)
