"""wn_phase_tab_fwd / wn_phase_tab_bwd (music_amd/csrc/wn_phase.hip) alone, through ctypes, one entry per launch, against their
float64 restatement tests/phase_ref.py.

  forward    every written float EQUALS the reference: a copy of a parameter, or, with the class term's addends, the correctly
             rounded fp32 sum of two floats; padding rows are exact +0; the NaN guards around every buffer are intact;
  backward   |got - ref| <= n 2^-24 sum |terms| per output, n the number of terms of that output's sum (batch for dT, P for the
             frame sums): the worst case of a sequential fp32 sum of n terms, nothing measured;
  both       a second launch gives the same bits; flat_grad outside the tables stays NaN.
Geometry: n_stages 1 / 3, dd 16 / 20 / 64 (ch 32 / 32 / 64), sd 20 / 256, batch 1 .. 4 with both layouts where it is even, P 1, 2, 3,
5, 8, 16, positions 0, P - 1 and 2^40 + 1, a rotation of its own per stage (negative ones and ones beyond P included), each with and
without the class addends.  The flat buffer holds NaN wherever the entries must not look."""
import itertools

import numpy as np
import pytest
import torch

from tests import phase_ref as ref
from tests.test_gpu_condproj_kernels import draw, guarded, guards_intact

pytestmark = pytest.mark.gpu

SHAPES = [(n, dd, ch, sd) for n in (1, 3) for dd, ch in ((16, 32), (20, 32), (64, 64)) for sd in (20, 256)]
ROT = [5, -7, 33, 0]                       # distinct per stage (the last one in use is the output stage's)


def positions(B, P, k):
    cand = [0, P - 1, 2 ** 40 + 1]
    return [cand[(b + k) % 3] for b in range(B)]


class Geometry:
    def __init__(self, shape, B, P, k, seed=0):
        self.N, self.Dd, self.CH, self.Sd = shape
        self.B, self.P = B, P
        N, Dd, Sd = self.N, self.Dd, self.Sd
        rng = np.random.default_rng(seed + 1000 * k)
        self.T, self.Tf = draw(rng, (N, 2 * Dd, P), False), draw(rng, (Sd, P), False)
        self.add_en, self.add_enf = draw(rng, (N, B, 2 * Dd), False), draw(rng, (B, Sd), False)
        self.d_en, self.d_enf = draw(rng, (N, B, 2 * Dd, P), False), draw(rng, (B, Sd, P), False)
        self.pos = np.asarray(positions(B, P, k), dtype=np.int64)
        self.rot = np.asarray([ROT[(i + k) % 4] + i for i in range(N)] + [ROT[(N + k) % 4] - 2], dtype=np.int32)
        self.pw_off, self.stride = 11, 2 * Dd * P + 3
        self.pwf_off = self.pw_off + N * self.stride + 4
        self.total = self.pwf_off + Sd * P + 6
        self.offs = (self.pw_off, self.stride, self.pwf_off)
        self.flat = self.place(self.T, self.Tf, np.float32)

    def place(self, T, Tf, dtype=np.float64):
        v = np.full(self.total, np.nan, dtype=dtype)
        for i in range(self.N):
            v[self.pw_off + i * self.stride:][:T[i].size] = T[i].reshape(-1)
        v[self.pwf_off:][:Tf.size] = Tf.reshape(-1)
        return v

    def dev(self):
        self.flat_d, self.pos_d, self.rot_d = (torch.from_numpy(a).cuda() for a in (self.flat, self.pos, self.rot))
        return self


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def run_fwd(g, want_clip, want_pair, addends):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    n_tab, n_enf = g.N * g.B * 2 * g.CH * g.P, g.B * g.Sd * g.P
    tb, tab = guarded(n_tab) if want_clip else (None, None)
    pb, tabp = guarded(n_tab) if want_pair else (None, None)
    eb, enf = guarded(n_enf)
    a_tab = a_pair = a_enf = None
    if addends:                                                  # the class term in wn_gclass_fwd's le = 1 layouts, padding rows +0
        en1 = g.add_en[..., None]
        a_tab = torch.from_numpy(ref.table(en1, g.CH, False, 0.0)).cuda() if want_clip else None
        a_pair = torch.from_numpy(ref.table(en1, g.CH, True, 0.0)).cuda() if want_pair else None
        a_enf = torch.from_numpy(g.add_enf).cuda()
    call("wn_phase_tab_fwd", ptr(g.flat_d), *g.offs, ptr(g.pos_d), ptr(g.rot_d), ptr(a_tab), ptr(a_pair), ptr(a_enf), ptr(tab), ptr(tabp),
         ptr(enf), g.N, g.Dd, g.CH, g.Sd, g.P, g.B, _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(eb, n_enf) and (tb is None or guards_intact(tb, n_tab)) and (pb is None or guards_intact(pb, n_tab))
    return [t.cpu().numpy() if t is not None else None for t in (tab, tabp, enf)]


def run_bwd(g, pair, sums):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    gb, grad = guarded(g.total)
    n1, n2 = g.N * g.B * 2 * g.CH, g.B * g.Sd
    (sb, s_tab), (fb, s_enf) = (guarded(n1), guarded(n2)) if sums else ((None, None), (None, None))
    d_tab = torch.from_numpy(ref.table(g.d_en, g.CH, pair, np.float32(0.0))).cuda()
    d_enf = torch.from_numpy(g.d_enf).cuda()
    call("wn_phase_tab_bwd", ptr(d_tab), 1 if pair else 0, ptr(d_enf), ptr(grad), *g.offs, ptr(g.pos_d), ptr(g.rot_d), ptr(s_tab),
         ptr(s_enf), g.N, g.Dd, g.CH, g.Sd, g.P, g.B, _lib.stream())
    torch.cuda.synchronize()
    assert guards_intact(gb, g.total) and (not sums or (guards_intact(sb, n1) and guards_intact(fb, n2)))
    return [t.cpu().numpy() if t is not None else None for t in (grad, s_tab, s_enf)]


def check_fwd(g, addends):
    en, enf_ref = ref.tab_fwd(g.T, g.Tf, g.pos, g.rot, *((g.add_en, g.add_enf) if addends else ()))
    variants = [(True, False)] + ([(True, True), (False, True)] if g.B % 2 == 0 else [])
    for want_clip, want_pair in variants:
        runs = [run_fwd(g, want_clip, want_pair, addends) for _ in range(2)]
        for a, b in zip(*runs):
            assert a is None or same_bits(a, b), "two launches differ"
        tab, tabp, enf = runs[0]
        assert same_bits(enf.reshape(enf_ref.shape), enf_ref), "enf"
        for got, pair in ((tab, False), (tabp, True)):
            if got is None:
                continue
            want = ref.table(en, g.CH, pair, np.float32(0.0))
            assert same_bits(got.reshape(want.shape), want), "table (pair %s): not the reference's bits (padding: +0)" % pair


def check_bwd(g, sums):
    (dT, dTf), (bT, bTf), (s_en, s_enf), (bs_en, bs_enf) = ref.tab_bwd(g.d_en, g.d_enf, g.pos, g.rot)
    want, bound = g.place(dT, dTf), np.nan_to_num(g.place(bT, bTf))
    mine = ~np.isnan(want)
    assert mine.sum() == (g.N * 2 * g.Dd + g.Sd) * g.P
    for pair in ([False, True] if g.B % 2 == 0 else [False]):
        runs = [run_bwd(g, pair, sums) for _ in range(2)]
        grad = runs[0][0]
        assert np.isnan(grad[~mine]).all(), "flat_grad was written outside the phase tables"
        for a, b in zip(*runs):
            assert a is None or same_bits(a[~np.isnan(a)], b[~np.isnan(b)]), "two launches differ"
        err = np.abs(grad[mine].astype(np.float64) - want[mine])
        assert np.isfinite(err).all() and (err <= bound[mine]).all(), ("dT", float((err / np.maximum(bound[mine], 1e-300)).max()))
        if sums:
            w_tab, b_tab = (ref.table(a[..., None], g.CH, pair, 0.0)[..., 0] for a in (s_en, bs_en))       # padding rows: sums of zeros
            err = np.abs(runs[0][1].reshape(w_tab.shape).astype(np.float64) - w_tab)
            assert (err <= b_tab).all(), "frame sums of the block tables"
            err = np.abs(runs[0][2].reshape(s_enf.shape).astype(np.float64) - s_enf)
            assert (err <= bs_enf).all(), "frame sums of enf"


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 16])
def test_phase_tables_forward_and_backward(P, B):
    seen = set()
    for k, (shape, cls) in enumerate(itertools.product(SHAPES, (False, True))):
        g = Geometry(shape, B, P, k, seed=100 * P + B).dev()
        seen.update(g.pos.tolist())
        check_fwd(g, cls)
        check_bwd(g, cls)
    assert seen == {0, P - 1, 2 ** 40 + 1}


def test_a_negative_position_makes_its_clip_nan_and_is_no_index():
    g = Geometry((3, 20, 32, 20), 4, 5, 1, seed=9)
    g.pos[2] = -(2 ** 40) - 3
    g.dev()
    en, enf_ref = ref.tab_fwd(g.T, g.Tf, g.pos, g.rot)
    assert np.isnan(en[:, 2]).all() and np.isnan(enf_ref[2]).all() and not np.isnan(en[:, [0, 1, 3]]).any()
    tab, tabp, enf = run_fwd(g, True, True, False)
    for got, pair in ((tab, False), (tabp, True)):
        want = ref.table(en, g.CH, pair, np.float32(0.0))
        assert np.array_equal(got.reshape(want.shape), want, equal_nan=True)
    assert np.array_equal(enf.reshape(enf_ref.shape), enf_ref, equal_nan=True)
    grad = run_bwd(g, False, False)[0]
    want = g.place(*ref.tab_bwd(g.d_en, g.d_enf, g.pos, g.rot)[0])
    assert np.isnan(grad).all() and np.isnan(want).all()          # its share turns every dT into NaN; the rest stays NaN


def test_refusals_and_the_empty_call_on_the_device():
    from music_amd import _lib
    from music_amd._lib import ptr
    lib = _lib.load()
    g = Geometry((3, 20, 32, 20), 3, 5, 0).dev()
    gb, grad = guarded(g.total)
    eb, enf = guarded(g.B * g.Sd * g.P)
    tb, tab = guarded(g.N * g.B * 2 * g.CH * g.P)
    st, dims = _lib.stream(), (g.N, g.Dd, g.CH, g.Sd, g.P)
    head = (ptr(g.flat_d),) + g.offs + (ptr(g.pos_d), ptr(g.rot_d))
    assert lib.wn_phase_tab_fwd(*head, None, None, None, ptr(tab), ptr(tab), ptr(enf), *dims, g.B, st) == -4       # odd batch, pair table
    assert "wn_phase_tab_fwd" in lib.wn_last_error().decode() and "'batch'" in lib.wn_last_error().decode()
    assert lib.wn_phase_tab_bwd(ptr(tab), 0, ptr(enf), ptr(grad), *g.offs, None, ptr(g.rot_d), None, None, *dims, g.B, st) == -4
    assert "wn_phase_tab_bwd" in lib.wn_last_error().decode() and "'pos'" in lib.wn_last_error().decode()
    assert lib.wn_phase_tab_fwd(None, *g.offs, None, None, None, None, None, None, None, None, *dims, 0, st) == 0
    assert lib.wn_phase_tab_bwd(None, 0, None, None, *g.offs, None, None, None, None, *dims, 0, st) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (gb, eb, tb))
