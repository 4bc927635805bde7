"""wn_vq_fwd / wn_vq_bwd / wn_vq_lookup (music_amd/csrc/wn_vq.hip) alone, through ctypes, against tests/vq_ref.py in float64.

Two kinds of input per geometry:
  grid     every input a multiple of 1/8 in [-2, 2]: a squared difference is a multiple of 1/64 <= 16 and any partial sum of up to
           512 of them is exact in fp32 in any order (tests/test_vq_ref.py checks that claim), so idx, q and counts must EQUAL the
           float64 ones in every frame - with exact ties planted (duplicated codebook rows, a frame ON a duplicated row, a frame
           midway between c and -c) that must go to the smallest index;
  normal   a frame whose float64 relative margin (second-best - best) / best exceeds BAND = 4 (Bw + 2) 2^-24 must get the float64
           argmin, and every frame's code must lie within BAND of the minimum.
Sums are held to gamma(n) = (n + 2) u / (1 - (n + 2) u), u = 2^-24, of tests/test_gpu_condproj_kernels.py, n the length of the
reduction: the mse over Bw terms per frame and at most C frames per workgroup, d_c[k] over the frames of code k, d_enc over its
two terms; where the scale 1 / (C Bw) is a power of two, grid inputs give every one of them exactly.
Outputs lie between guards; flat_grad holds NaN in the codebook's rows and a canary everywhere else."""
import numpy as np
import pytest
import torch

from tests import vq_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
CANARY = 123.0
BETA = 0.25
CB_OFF = 5                    # the codebook's offset in the flat buffers: rows are not 16-byte aligned

# (Bw, K, B, Le): Bw crosses the 64 lanes (1, 7 | 64 | 65, 512), K the 8 waves' code split (2 | 17, 64, 1024), B Le the 4-frame tile
CASES = [(1, 2, 1, 1), (1, 17, 3, 3), (1, 1024, 3, 70), (7, 2, 3, 1), (7, 17, 2, 4), (7, 64, 3, 70), (7, 1024, 3, 3),
         (64, 2, 2, 4), (64, 17, 3, 70), (64, 64, 3, 3), (64, 1024, 3, 1), (64, 1024, 3, 70), (65, 2, 3, 3), (65, 17, 1, 1),
         (65, 64, 2, 4), (65, 1024, 3, 70), (512, 2, 3, 70), (512, 17, 3, 3), (512, 64, 1, 1), (512, 1024, 2, 4)]
IDS = ["bw%d_k%d_b%d_le%d" % c for c in CASES]


def gamma(n):
    return (n + 2) * U / (1 - (n + 2) * U)


def guarded(n, dtype=torch.float32, fill=None):
    guard = float("nan") if dtype == torch.float32 else -7
    buf = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.fill_(fill)

    def intact():
        ends = torch.cat([buf[:GUARD], buf[GUARD + n:]])
        return bool(torch.isnan(ends).all()) if dtype == torch.float32 else bool((ends == -7).all())
    return view, intact


def draw(case, grid, seed):
    Bw, K, B, Le = case
    rng = np.random.default_rng(seed)
    if grid:
        enc = rng.integers(-16, 17, size=(B, Bw, Le)) / 8.0
        cb = rng.integers(-16, 17, size=(K, Bw)) / 8.0
        d_q = rng.integers(-16, 17, size=(B, Bw, Le)) / 8.0
        if K >= 4:
            cb[K - 1] = cb[0]                       # duplicated rows: ties wherever one of them is nearest
            cb[K // 2] = cb[1]
            enc[0, :, 0] = cb[1]                    # ... and one frame ON a duplicated row: distance 0 to codes 1 and K / 2
        else:
            cb[1] = -cb[0]                          # a frame midway between the two codes
            enc[0, :, 0] = 0.0
    else:
        enc, cb, d_q = rng.standard_normal((B, Bw, Le)), rng.standard_normal((K, Bw)), rng.standard_normal((B, Bw, Le))
    return enc.astype(np.float32), cb.astype(np.float32), d_q.astype(np.float32)


def run_fwd(enc, cb, with_counts=True):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0]
    flat = torch.full((CB_OFF + K * Bw + 3,), float("nan"), dtype=torch.float32, device="cuda")
    flat[CB_OFF:CB_OFF + K * Bw] = torch.from_numpy(cb.reshape(-1)).cuda()
    enc_d = torch.from_numpy(enc).cuda()
    q, q_ok = guarded(B * Bw * Le)
    idx, idx_ok = guarded(B * Le, torch.int32)
    counts, counts_ok = guarded(K, torch.int32, fill=99)                 # stale values: the call clears them
    part, part_ok = guarded(_lib.VQ_NUM_PARTIALS)
    call("wn_vq_fwd", ptr(enc_d), ptr(flat), CB_OFF, ptr(q), ptr(idx), ptr(counts) if with_counts else None, ptr(part), K, Bw, Le, B,
         _lib.stream())
    torch.cuda.synchronize()
    assert q_ok() and idx_ok() and counts_ok() and part_ok(), "a guard was overwritten"
    if not with_counts:
        assert bool((counts == 99).all())
    return dict(q=q.cpu().numpy().reshape(B, Bw, Le), idx=idx.cpu().numpy().reshape(B, Le).astype(np.int64),
                counts=counts.cpu().numpy().astype(np.int64), part=part.cpu().numpy(), flat=flat, enc_d=enc_d, idx_d=idx)


def run_bwd(f, enc, cb, d_q, alias, g_scale=1.0):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0]
    total = f["flat"].numel()
    grad, grad_ok = guarded(total, fill=CANARY)
    grad[CB_OFF:CB_OFF + K * Bw] = float("nan")
    d_q_d, dq_ok = guarded(B * Bw * Le)
    d_q_d.copy_(torch.from_numpy(d_q.reshape(-1)).cuda())
    d_enc, de_ok = (d_q_d, dq_ok) if alias else guarded(B * Bw * Le)
    call("wn_vq_bwd", ptr(f["enc_d"]), ptr(f["idx_d"]), ptr(d_q_d), ptr(f["flat"]), CB_OFF, BETA, g_scale, ptr(d_enc), ptr(grad), K, Bw,
         Le, B, _lib.stream())
    torch.cuda.synchronize()
    assert grad_ok() and dq_ok() and de_ok(), "a guard was overwritten"
    grad = grad.cpu().numpy()
    rest = np.ones(total, dtype=bool)
    rest[CB_OFF:CB_OFF + K * Bw] = False
    assert (grad[rest] == CANARY).all(), "flat_grad was written outside the codebook"
    d_c = grad[CB_OFF:CB_OFF + K * Bw].reshape(K, Bw)
    assert np.isfinite(d_c).all(), "not all K rows of d_c were written"
    if not alias:
        assert np.array_equal(d_q_d.cpu().numpy(), d_q.reshape(-1)), "d_q was modified"
    return d_enc.cpu().numpy().reshape(B, Bw, Le), d_c


def check_bwd(f, enc, cb, d_q, exact, what):
    (B, Bw, Le), K = enc.shape, cb.shape[0]
    C = B * Le
    runs = [run_bwd(f, enc, cb, d_q, alias) for alias in (False, False, True)]
    for r in runs[1:]:                                                    # a second launch, and d_enc = d_q: the same bits
        assert np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]), what
    d_enc, d_c = runs[0]
    ref_enc, ref_c = vq_ref.backward(enc, cb, f["idx"], d_q, BETA)
    unused = f["counts"] == 0
    assert (d_c[unused] == 0).all(), "%s: an unused code's gradient is not exactly 0" % what
    e64, c64, s = enc.astype(np.float64), cb.astype(np.float64), 2.0 / (C * Bw)
    q64 = c64[f["idx"]].transpose(0, 2, 1)
    if exact:
        assert np.array_equal(d_enc, ref_enc.astype(np.float32)) and np.array_equal(d_c, ref_c.astype(np.float32)), what
        return
    # d_enc: the difference, its product with the coefficient (rounded once itself), the sum
    b_enc = gamma(2) * (np.abs(d_q.astype(np.float64)) + BETA * s * np.abs(e64 - q64))
    abs_c = np.zeros_like(c64)
    np.add.at(abs_c, f["idx"].reshape(-1), np.abs(q64 - e64).transpose(0, 2, 1).reshape(-1, Bw))
    b_c = gamma(f["counts"].max() + 1) * s * abs_c
    for got, ref, bound, name in ((d_enc, ref_enc, b_enc, "d_enc"), (d_c, ref_c, b_c, "d_c")):
        err = np.abs(got.astype(np.float64) - ref)
        print("  %s %s: largest error %.3e, largest error / bound %.3f" % (what, name, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (what, name)


def check_mse(f, dist_chosen, C, Bw, exact, what):
    got = f["part"].astype(np.float64).sum()
    ref = dist_chosen.sum() / (C * Bw)
    print("  %s mse: %.9g (float64 %.9g)" % (what, got, ref))
    if exact:
        assert got == ref, (what, got, ref)
    else:
        assert abs(got - ref) <= gamma(Bw + C + 2) * ref, (what, got, ref)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_grid_inputs_equal_float64_in_every_frame(case):
    Bw, K, B, Le = case
    C = B * Le
    enc, cb, d_q = draw(case, True, seed=11)
    ref = vq_ref.forward(enc, cb, BETA)
    assert (vq_ref.margins(ref["dist"]) == 0).any(), "no tie was planted"
    f, f2 = run_fwd(enc, cb), run_fwd(enc, cb)
    for k in ("q", "idx", "counts", "part"):
        assert np.array_equal(f[k], f2[k]), "two launches differ in %s" % k
    assert np.array_equal(f["idx"], ref["idx"]), "idx differs in %d frames" % (f["idx"] != ref["idx"]).sum()
    # the planted tie went to the smallest index (code 0 only where the drawn rows 0 and 1 coincide)
    assert vq_ref.margins(ref["dist"])[0, 0] == 0 and f["idx"][0, 0] <= (1 if K >= 4 else 0)
    assert np.array_equal(f["q"], ref["q"].astype(np.float32)) and np.array_equal(f["counts"], ref["counts"])
    assert f["counts"].sum() == C
    pow2 = (C * Bw) & (C * Bw - 1) == 0
    chosen = np.take_along_axis(ref["dist"], ref["idx"][..., None], -1)
    check_mse(f, chosen, C, Bw, pow2, "grid")
    check_bwd(f, enc, cb, d_q, pow2, "grid")
    f3 = run_fwd(enc, cb, with_counts=False)                               # counts is optional
    assert np.array_equal(f3["idx"], f["idx"]) and np.array_equal(f3["part"], f["part"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_normal_inputs_outside_the_rounding_band(case):
    Bw, K, B, Le = case
    C = B * Le
    band = 4 * (Bw + 2) * U
    enc, cb, d_q = draw(case, False, seed=23)
    ref = vq_ref.forward(enc, cb, BETA)
    f = run_fwd(enc, cb)
    margin = vq_ref.margins(ref["dist"])
    clear = margin > band
    print("  %d of %d frames inside the band of %.2e" % ((~clear).sum(), C, band))
    assert np.array_equal(f["idx"][clear], ref["idx"][clear])
    chosen = np.take_along_axis(ref["dist"], f["idx"][..., None], -1)[..., 0]
    best = ref["dist"].min(-1)
    assert (chosen <= best * (1 + band)).all()
    assert np.array_equal(f["q"], cb[f["idx"]].transpose(0, 2, 1)) and np.array_equal(f["counts"], np.bincount(f["idx"].reshape(-1), minlength=K))
    check_mse(f, chosen, C, Bw, False, "normal")
    check_bwd(f, enc, cb, d_q, False, "normal")


def test_an_upstream_scale_reaches_both_loss_gradients_only():
    case = (64, 17, 2, 4)                                                  # C Bw = 512: every scale a power of two
    enc, cb, d_q = draw(case, True, seed=31)
    f = run_fwd(enc, cb)
    d_enc, d_c = run_bwd(f, enc, cb, d_q, False, g_scale=4.0)
    ref_enc, ref_c = vq_ref.backward(enc, cb, f["idx"], d_q, BETA, g=4.0)
    assert np.array_equal(d_enc, ref_enc.astype(np.float32)) and np.array_equal(d_c, ref_c.astype(np.float32))
    d_enc0, d_c0 = run_bwd(f, enc, cb, d_q, False, g_scale=0.0)            # vq_loss left out of the objective
    assert np.array_equal(d_enc0, d_q) and (d_c0 == 0).all()


@pytest.mark.parametrize("case", [(7, 17, 2, 4), (65, 1024, 3, 70)], ids=["small", "large"])
def test_lookup_and_its_out_of_range_flag(case):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    Bw, K, B, Le = case
    rng = np.random.default_rng(41)
    cb = rng.standard_normal((K, Bw)).astype(np.float32)
    codes = rng.integers(0, K, size=(B, Le)).astype(np.int32)
    flat = torch.full((CB_OFF + K * Bw,), float("nan"), dtype=torch.float32, device="cuda")
    flat[CB_OFF:] = torch.from_numpy(cb.reshape(-1)).cuda()

    def lookup(codes, with_flag=True):
        q, q_ok = guarded(B * Bw * Le)
        bad, bad_ok = guarded(1, torch.int32, fill=5)
        codes_d = torch.from_numpy(codes).cuda()
        call("wn_vq_lookup", ptr(codes_d), ptr(flat), CB_OFF, ptr(q), ptr(bad) if with_flag else None, K, Bw, Le, B,
             _lib.stream())
        torch.cuda.synchronize()
        assert q_ok() and bad_ok()
        return q.cpu().numpy().reshape(B, Bw, Le), int(bad.item())

    q, bad = lookup(codes)
    assert bad == 0 and np.array_equal(q, cb[codes].transpose(0, 2, 1))
    for wrong in (K, -1, 1 << 30):                      # never read: the frame is NaN, the flag is up, the others are untouched
        c2 = codes.copy()
        c2[B - 1, Le // 2] = wrong
        q2, bad = lookup(c2)
        assert bad == 1 and np.isnan(q2[B - 1, :, Le // 2]).all()
        q2[B - 1, :, Le // 2] = q[B - 1, :, Le // 2]
        assert np.array_equal(q2, q)
        q3, _ = lookup(c2, with_flag=False)
        assert np.isnan(q3[B - 1, :, Le // 2]).all()
