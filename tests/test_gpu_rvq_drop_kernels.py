"""wn_rvq_fwd_n / wn_rvq_bwd_n / wn_rvq_bwd_stats_n / wn_rvq_lookup_n (music_amd/csrc/wn_vq.hip: quantiser dropout, a stage count per
clip) alone, through ctypes, one launch at a time against tests/rvq_drop_ref.py in float64.

Inputs are the grid of tests/test_gpu_rvq_kernels.py (multiples of 1/8, every distance exact in fp32 in any order; a tie planted in the
last stage), so idx must EQUAL the float64 argmin in every active frame and stage and be -1 in every inactive one - no case left out.
Shapes: (B, Le) = (3, 5) and (2, 7) (tiles straddle clips, C % 4 != 0), (1, 1), (4, 4) (a tile = a clip) and (5, 300) (375 tiles on 256
workgroups); Bw = 1, 16, 65, 512; K = 2, 5 (fewer codes than waves), 37, 512; S = 1, 3, 8.  Stage counts: all S (every output buffer
has the bits of the entry without _n), all 1, alternating 1 / S on neighbouring clips (with (4, 4) and S = 8: a tile of four n = 1
frames), a draw, and the out-of-range 0 and S + 3, which the device clamps.
Bars: q_out and res within 1e-6 relative of float64, counts and the statistics' n exact, every stage's loss partials within 1e-5
relative of float64 (the project's vq_loss bar), d_enc and d_cb within 3e-4 of the tensor's max-abs (its gradient bar); two launches
give the same bits.  Outputs lie between guards."""
import numpy as np
import pytest
import torch

from tests import rvq_drop_ref as dr
from tests.test_gpu_rvq_kernels import draw, flat_of, ids, rvq_bwd, rvq_fwd
from tests.test_gpu_vq_kernels import BETA, CANARY, CB_OFF, guarded

pytestmark = pytest.mark.gpu

# (S, Bw, K, B, Le): every value of every axis, each pair of neighbouring axes in several combinations
CASES = [(3, 16, 37, 3, 5), (8, 65, 5, 2, 7), (1, 1, 2, 1, 1), (8, 512, 512, 4, 4), (3, 1, 512, 2, 7), (8, 16, 2, 3, 5), (1, 65, 37, 4, 4),
         (3, 512, 5, 1, 1), (8, 1, 37, 4, 4), (3, 65, 512, 3, 5), (1, 16, 5, 2, 7), (8, 512, 2, 2, 7), (1, 512, 37, 3, 5), (3, 16, 512, 1, 1),
         (8, 65, 2, 4, 4), (3, 16, 37, 5, 300)]


def patterns(S, B, seed=5):
    """name -> (what is uploaded, what the device must make of it)"""
    alt = np.where(np.arange(B) % 2 == 0, 1, S)
    rng = np.random.default_rng(seed)
    out = {"all_S": (np.full(B, S), np.full(B, S)), "all_1": (np.ones(B, dtype=np.int64),) * 2, "alternating": (alt, alt),
           "drawn": (rng.integers(1, S + 1, size=B),) * 2,
           "clamped": (np.where(np.arange(B) % 2 == 0, 0, S + 3), alt)}
    return out


def rvq_fwd_n(enc, cb, S, nstage, with_counts=True):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0] // S
    flat, enc_d = flat_of(cb), torch.from_numpy(enc).cuda()
    n_d = torch.from_numpy(np.asarray(nstage, dtype=np.int32)).cuda()
    q, q_ok = guarded(B * Bw * Le)
    idx, idx_ok = guarded(S * B * Le, torch.int32)
    counts, counts_ok = guarded(S * K, torch.int32, fill=99)             # stale values: the call clears them
    res, res_ok = guarded(S * B * Bw * Le)
    part, part_ok = guarded(S * _lib.VQ_NUM_PARTIALS)
    call("wn_rvq_fwd_n", ptr(enc_d), ptr(flat), CB_OFF, ptr(n_d), ptr(q), ptr(idx), ptr(counts) if with_counts else None, ptr(res), ptr(part),
         S, K, Bw, Le, B, _lib.stream())
    torch.cuda.synchronize()
    assert q_ok() and idx_ok() and counts_ok() and res_ok() and part_ok(), "a guard was overwritten"
    assert not torch.isnan(res).any() and not torch.isnan(part).any() and not torch.isnan(q).any(), "an output was not written"
    assert (idx != -7).all(), "an idx was not written"
    return dict(q=q.cpu().numpy().reshape(B, Bw, Le), idx=idx.cpu().numpy().reshape(S, B, Le).astype(np.int64),
                counts=counts.cpu().numpy().reshape(S, K).astype(np.int64), res=res.cpu().numpy().reshape(S, B, Bw, Le),
                part=part.cpu().numpy().reshape(S, -1), flat=flat, enc_d=enc_d, idx_d=idx, res_d=res, n_d=n_d)


def rvq_bwd_n(f, enc, cb, S, d_q, alias, g_scale=1.0, stats=False, idx_d=None):
    """-> (d_enc, d_c (S K, Bw)[, stat (S, K (Bw + 1))]); the bookkeeping of tests/test_gpu_rvq_kernels.rvq_bwd"""
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0] // S
    total = f["flat"].numel()
    grad, grad_ok = guarded(total, fill=CANARY)
    grad[CB_OFF:CB_OFF + S * K * Bw] = float("nan")
    d_q_d, dq_ok = guarded(B * Bw * Le)
    d_q_d.copy_(torch.from_numpy(d_q.reshape(-1)).cuda())
    d_enc, de_ok = (d_q_d, dq_ok) if alias else guarded(B * Bw * Le)
    stat, stat_ok = guarded(S * K * (Bw + 1))
    head = (ptr(f["enc_d"]), ptr(f["idx_d"] if idx_d is None else idx_d), ptr(f["res_d"]), ptr(f["n_d"]), ptr(d_q_d), ptr(f["flat"]), CB_OFF,
            BETA, g_scale, ptr(d_enc), ptr(grad))
    if stats:
        call("wn_rvq_bwd_stats_n", *head, ptr(stat), S, K, Bw, Le, B, _lib.stream())
    else:
        call("wn_rvq_bwd_n", *head, S, K, Bw, Le, B, _lib.stream())
    torch.cuda.synchronize()
    assert grad_ok() and dq_ok() and de_ok() and stat_ok(), "a guard was overwritten"
    grad = grad.cpu().numpy()
    rest = np.ones(total, dtype=bool)
    rest[CB_OFF:CB_OFF + S * K * Bw] = False
    assert (grad[rest] == CANARY).all(), "flat_grad was written outside the codebook"
    d_c = grad[CB_OFF:CB_OFF + S * K * Bw].reshape(S * K, Bw)
    assert np.isfinite(d_c).all(), "not all S K rows of d_c were written"
    if not alias:
        assert np.array_equal(d_q_d.cpu().numpy(), d_q.reshape(-1)), "d_q was modified"
    out = (d_enc.cpu().numpy().reshape(B, Bw, Le), d_c)
    if stats:
        assert (d_c == 0).all() and not np.signbit(d_c).any(), "the codebook's gradient is not exactly 0 in all S K rows"
        stat = stat.cpu().numpy().reshape(S, -1)
        assert np.isfinite(stat).all(), "not every entry of stat was written"
        out += (stat,)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def within(got, ref, rel):
    return (np.abs(got.astype(np.float64) - ref) <= rel * np.abs(ref)).all()


def check_pattern(case, name, enc, cb, d_q, sent, n):
    S, Bw, K, B, Le = case
    C = B * Le
    ref = dr.forward(enc, cb, S, sent, BETA)
    assert np.array_equal(ref["n"], n)
    f, f2 = rvq_fwd_n(enc, cb, S, sent), rvq_fwd_n(enc, cb, S, sent)
    for k in ("q", "idx", "counts", "res", "part"):
        assert np.array_equal(bits(f[k]), bits(f2[k])), "%s: two launches differ in %s" % (name, k)
    active = np.broadcast_to((np.arange(S)[:, None] < n[None, :])[:, :, None], (S, B, Le))
    assert (f["idx"][~active] == -1).all(), "%s: an inactive entry is not -1" % name
    assert np.array_equal(f["idx"][active], ref["idx"][active]), \
        "%s: idx differs from the float64 argmin in %d active (frame, stage) pairs" % (name, (f["idx"] != ref["idx"])[active].sum())
    assert within(f["q"], ref["q"], 1e-6), "%s: q_out" % name
    assert within(f["res"], ref["res"], 1e-6), "%s: res (active: r_s - q_s; inactive: the carried residual)" % name
    assert np.array_equal(f["counts"], ref["counts"]) and np.array_equal(f["counts"].sum(1), ref["stage_frames"]), "%s: counts" % name
    got = f["part"].astype(np.float64).sum(1)
    print("  %s loss partials %s (float64 %s)" % (name, got, ref["mse"]))
    assert (np.abs(got - ref["mse"]) <= 1e-5 * ref["mse"]).all(), "%s: loss_part (an unused stage's must be exactly 0)" % name
    f3 = rvq_fwd_n(enc, cb, S, sent, with_counts=False)                    # counts is optional
    assert np.array_equal(f3["idx"], f["idx"]) and np.array_equal(bits(f3["part"]), bits(f["part"])) and (f3["counts"] == 99).all()
    # ---- the backward launches, on the device's own codes and residuals
    runs = [rvq_bwd_n(f, enc, cb, S, d_q, alias) for alias in (False, False, True)]
    srun = [rvq_bwd_n(f, enc, cb, S, d_q, alias, stats=True) for alias in (False, True)]
    for r in runs[1:] + srun:
        assert np.array_equal(bits(runs[0][0]), bits(r[0])), "%s: d_enc differs between launches / forms" % name
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])) and np.array_equal(bits(srun[0][2]), bits(srun[1][2])), name
    d_enc, d_c = runs[0]
    stat = srun[0][2].astype(np.float64)
    ref_enc, ref_c = dr.backward(enc, cb, S, sent, f["idx"], d_q, BETA)
    ref_stat = dr.stats(enc, cb, S, sent, f["idx"])
    for got, want, what in ((d_enc, ref_enc, "d_enc"), (d_c, ref_c, "d_cb")):
        err = np.abs(got.astype(np.float64) - want).max()
        print("  %s %s: largest error %.3e of max-abs %.3e" % (name, what, err, np.abs(want).max()))
        assert err <= 3e-4 * np.abs(want).max(), (name, what)
    assert np.array_equal(stat[:, :K], ref["counts"]), "%s: the n of stat" % name
    assert np.array_equal(stat, ref_stat), "%s: the sums of stat (multiples of 1/8: exact)" % name
    unused = (ref["counts"] == 0).reshape(-1)
    assert (d_c[unused] == 0).all(), "%s: an unused code's gradient is not exactly 0" % name
    for s in range(S):
        if not (n > s).any():
            assert (d_c[s * K:(s + 1) * K] == 0).all() and (stat[s] == 0).all() and (f["part"][s] == 0).all(), "%s: stage %d had no frame" % (name, s)
    return f, runs[0], srun[0]


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_every_pattern_against_float64_and_all_active_against_the_plain_entries(case):
    S, Bw, K, B, Le = case
    enc, cb, d_q = draw(case, True, seed=11)
    outs = {}
    for name, (sent, n) in patterns(S, B).items():
        outs[name] = check_pattern(case, name, enc, cb, d_q, sent, np.asarray(n))
    # all S: the bits of wn_rvq_fwd / wn_rvq_bwd / wn_rvq_bwd_stats in every output buffer
    f, (d_enc, d_c), (s_enc, _, stat) = outs["all_S"]
    p = rvq_fwd(enc, cb, S)
    for k in ("q", "idx", "counts", "res", "part"):
        assert np.array_equal(bits(f[k]), bits(p[k])), "all S: %s differs from wn_rvq_fwd's" % k
    p_enc, p_c = rvq_bwd(p, enc, cb, S, d_q, False)
    ps_enc, _, p_stat = rvq_bwd(p, enc, cb, S, d_q, False, stats=True)
    assert np.array_equal(bits(d_enc), bits(p_enc)) and np.array_equal(bits(d_c), bits(p_c)), "all S: wn_rvq_bwd's bits"
    assert np.array_equal(bits(s_enc), bits(ps_enc)) and np.array_equal(bits(stat), bits(p_stat)), "all S: wn_rvq_bwd_stats' bits"
    # 0 and S + 3 are clamped to 1 and S: the alternating pattern's bits
    for a, b in zip(outs["clamped"], outs["alternating"]):
        for k in (("q", "idx", "counts", "res", "part") if isinstance(a, dict) else range(len(a))):
            assert np.array_equal(bits(a[k]), bits(b[k])), "clamped: output %s differs from the alternating pattern's" % (k,)


def test_a_bad_code_gives_nan_in_an_active_stage_only_and_a_scale_reaches_the_loss_gradients():
    case = (3, 64, 24, 4, 4)                                                # C Bw = 1024: every scale a power of two
    S, Bw, K, B, Le = case
    enc, cb, d_q = draw(case, True, seed=31)
    n = np.array([3, 1, 2, 3])
    f = rvq_fwd_n(enc, cb, S, n)
    d_enc, d_c = rvq_bwd_n(f, enc, cb, S, d_q, False, g_scale=4.0)
    ref_enc, ref_c = dr.backward(enc, cb, S, n, f["idx"], d_q, BETA, g=4.0)
    assert np.array_equal(d_enc, ref_enc.astype(np.float32)) and np.array_equal(d_c, ref_c.astype(np.float32))
    d_enc0, d_c0 = rvq_bwd_n(f, enc, cb, S, d_q, False, g_scale=0.0)
    assert np.array_equal(d_enc0, d_q) and (d_c0 == 0).all()
    assert (f["idx"][1:, 1] == -1).all() and (f["idx"][2, 2] == -1).all()
    for wrong, s, b, nan in ((K, 0, 1, True), (-5, 1, 2, True), (1 << 30, 2, 3, True), (K, 1, 1, False), (1 << 30, 2, 2, False)):
        idx = f["idx"].copy()
        idx[s, b, 2] = wrong                                                # compared, never dereferenced; not looked at where inactive
        idx_d = torch.from_numpy(idx.astype(np.int32)).cuda()
        for stats in (False, True):
            out = rvq_bwd_n(f, enc, cb, S, d_q, False, stats=stats, idx_d=idx_d)
            assert np.isnan(out[0][b, :, 2]).all() == nan and np.isfinite(np.delete(out[0], 2, axis=2)).all()
            if not nan:
                assert np.array_equal(out[0], rvq_bwd_n(f, enc, cb, S, d_q, False)[0])


LOOKUP_CASES = [(3, 16, 37, 3, 5), (8, 65, 512, 2, 7), (1, 1, 2, 1, 1), (8, 512, 5, 4, 4)]


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=ids(LOOKUP_CASES))
def test_lookup_with_stage_counts_and_its_flag(case):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    S, Bw, K, B, Le = case
    rng = np.random.default_rng(41)
    cb = rng.standard_normal((S * K, Bw)).astype(np.float32)
    codes = rng.integers(0, K, size=(S, B, Le)).astype(np.int32)
    flat = flat_of(cb)

    def lookup(codes, n, with_flag=True):
        q, q_ok = guarded(B * Bw * Le)
        bad, bad_ok = guarded(1, torch.int32, fill=5)
        codes_d = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
        n_d = torch.from_numpy(np.asarray(n, dtype=np.int32)).cuda()
        call("wn_rvq_lookup_n", ptr(codes_d), ptr(n_d), ptr(flat), CB_OFF, ptr(q), ptr(bad) if with_flag else None, S, K, Bw, Le, B,
             _lib.stream())
        torch.cuda.synchronize()
        assert q_ok() and bad_ok()
        return q.cpu().numpy().reshape(B, Bw, Le), int(bad.item())

    for name, (_, n) in patterns(S, B).items():
        n = np.asarray(n)
        c2 = codes.copy()
        c2[np.arange(S)[:, None] >= n[None, :]] = -1                        # what the forward hands out; not looked at
        want = None
        for s in range(S):                                                  # the fp32 sum in stage order over the active stages
            row = np.where((n > s)[:, None, None], cb[s * K:(s + 1) * K][codes[s]].transpose(0, 2, 1), np.float32(0))
            want = row if want is None else np.where((n > s)[:, None, None], want + row, want)
        q, bad = lookup(c2, n)
        assert bad == 0 and np.array_equal(bits(q), bits(want.astype(np.float32))), name
        # against float64: at most S - 1 roundings, each below 2^-24 of the running sum's magnitude <= sum |rows|
        err = np.abs(q.astype(np.float64) - dr.lookup(cb, S, codes, n))
        assert (err <= S * 2.0 ** -24 * dr.lookup(np.abs(cb), S, codes, n)).all(), name
        assert np.array_equal(bits(lookup(c2, n)[0]), bits(q)), "two launches differ"
        if name == "all_S":                                                 # the bits of wn_rvq_lookup
            p, p_ok = guarded(B * Bw * Le)
            call("wn_rvq_lookup", ptr(torch.from_numpy(codes).cuda()), ptr(flat), CB_OFF, ptr(p), None, S, S, K, Bw, Le, B, _lib.stream())
            torch.cuda.synchronize()
            assert p_ok() and np.array_equal(bits(p.cpu().numpy()), bits(q.reshape(-1)))
    n = np.asarray(patterns(S, B)["alternating"][1])
    q, _ = lookup(codes, n)
    b = B - 1
    for wrong in (K, -1, 1 << 30):                                          # an ACTIVE bad code: NaN frame, flag up, the others untouched
        c2 = codes.copy()
        c2[n[b] - 1, b, Le // 2] = wrong
        q2, bad = lookup(c2, n)
        assert bad == 1 and np.isnan(q2[b, :, Le // 2]).all()
        q2[b, :, Le // 2] = q[b, :, Le // 2]
        assert np.array_equal(q2, q)
        assert np.isnan(lookup(c2, n, with_flag=False)[0][b, :, Le // 2]).all()
    for wrong_n in (0, S + 1, -3, 1 << 30):                                 # a bad n: that clip is NaN, nothing is read through it
        n2 = n.copy()
        n2[b] = wrong_n
        q2, bad = lookup(codes, n2)
        assert bad == 1 and np.isnan(q2[b]).all() and np.array_equal(q2[:b], q[:b])
