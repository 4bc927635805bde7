"""wn_rvq_fwd / wn_rvq_bwd / wn_rvq_bwd_stats / wn_rvq_ema_update / wn_rvq_lookup (music_amd/csrc/wn_vq.hip) alone, through ctypes,
against tests/rvq_ref.py in float64.

  S = 1    every output of the five entries has the bits of the matching wn_vq_* entry.
  grid     inputs are multiples of 1/8: enc in [-2, 2], stage s's rows in [-2, 2] >> min(s, 3), so every residual stays a multiple of 1/8
           below 7 (a planted row below 14), a squared difference is at most 196 x 64 units of 1/64 and a sum of 512 of them stays below
           2^24 units: exact in fp32 in any order.  idx, q, res and counts must EQUAL float64 in every frame and stage; the LAST stage
           holds a frame ON a duplicated row, which must go to the smaller index; the codebooks differ per stage.
  normal   every stage is judged on the DEVICE's own input r_s (enc, then res[s - 1] read back): a frame whose float64 relative margin
           exceeds BAND = 4 (Bw + 2) 2^-24 must get the float64 argmin, every frame's code must lie within BAND of the minimum, res[s]
           must have the bits of numpy's fp32 r_s - c[idx] and q those of the fp32 sum in stage order.
Sums are held to gamma(n) = (n + 2) u / (1 - (n + 2) u) of tests/test_gpu_vq_kernels.py; where 1 / (C Bw) is a power of two, grid
inputs give the gradients exactly.  Outputs lie between guards; flat_grad holds NaN in the codebook's rows and a canary elsewhere."""
import numpy as np
import pytest
import torch

from tests import rvq_ref, vq_ref
from tests import vq_ema_ref as er
from tests.test_gpu_vq_ema_kernels import Device, check_update, draw_stats, guard_block, run_stats
from tests.test_gpu_vq_kernels import BETA, CANARY, CB_OFF, U, gamma, guarded, run_bwd, run_fwd

pytestmark = pytest.mark.gpu

# (S, Bw, K, B, Le): S in {2, 3, 8}; Bw crosses the 64 lanes (1, 12 | 64 | 65, 512); K the 8 waves' split and a workgroup's four codes
# (2 | 24 | 512, 1024); frames 1, 5 (a partly filled tile), 210 (53 tiles; four 64-frame ballots in the backward) and 1500 (375 tiles
# on 256 workgroups: some loop over two)
GRID_CASES = [(2, 12, 24, 5, 300), (2, 1, 2, 1, 1), (3, 12, 24, 1, 5), (8, 64, 512, 3, 70), (2, 65, 1024, 1, 5), (3, 512, 24, 3, 70), (2, 512, 1024, 1, 5),
              (8, 12, 2, 3, 70), (3, 1, 512, 1, 1), (2, 64, 24, 2, 4), (3, 65, 24, 3, 70)]
NORMAL_CASES = [(4, 64, 512, 3, 70), (2, 512, 1024, 1, 32), (3, 12, 24, 1, 5), (8, 65, 24, 3, 70), (2, 1, 24, 5, 300)]
ids = lambda cases: ["s%d_bw%d_k%d_b%d_le%d" % c for c in cases]


def draw(case, grid, seed):
    """enc, cb (S K, Bw), d_q as float32; grid: the last stage's rows 1 and K / 2 (0 and 1 at K = 2) are the residual that reaches it
    in frame (0, 0) - a distance of exactly 0 to both."""
    S, Bw, K, B, Le = case
    rng = np.random.default_rng(seed)
    if not grid:
        enc, d_q = rng.standard_normal((B, Bw, Le)), rng.standard_normal((B, Bw, Le))
        cb = np.concatenate([rng.standard_normal((K, Bw)) * 0.8 ** s for s in range(S)])
        return enc.astype(np.float32), cb.astype(np.float32), d_q.astype(np.float32)
    enc = rng.integers(-16, 17, size=(B, Bw, Le)) / 8.0
    d_q = rng.integers(-16, 17, size=(B, Bw, Le)) / 8.0
    cb = np.concatenate([rng.integers(-(16 >> min(s, 3)), (16 >> min(s, 3)) + 1, size=(K, Bw)) / 8.0 for s in range(S)])
    r = rvq_ref.forward(enc, cb, S)["r"][S - 1][0, :, 0]
    lo, hi = (1, K // 2) if K >= 4 else (0, 1)
    cb[(S - 1) * K + lo] = cb[(S - 1) * K + hi] = r
    return enc.astype(np.float32), cb.astype(np.float32), d_q.astype(np.float32)


def flat_of(cb):
    flat = torch.full((CB_OFF + cb.size + 3,), float("nan"), dtype=torch.float32, device="cuda")
    flat[CB_OFF:CB_OFF + cb.size] = torch.from_numpy(cb.reshape(-1)).cuda()
    return flat


def rvq_fwd(enc, cb, S, with_counts=True):
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0] // S
    flat, enc_d = flat_of(cb), torch.from_numpy(enc).cuda()
    q, q_ok = guarded(B * Bw * Le)
    idx, idx_ok = guarded(S * B * Le, torch.int32)
    counts, counts_ok = guarded(S * K, torch.int32, fill=99)             # stale values: the call clears them
    res, res_ok = guarded(S * B * Bw * Le)
    part, part_ok = guarded(S * _lib.VQ_NUM_PARTIALS)
    call("wn_rvq_fwd", ptr(enc_d), ptr(flat), CB_OFF, ptr(q), ptr(idx), ptr(counts) if with_counts else None, ptr(res), ptr(part), S, K,
         Bw, Le, B, _lib.stream())
    torch.cuda.synchronize()
    assert q_ok() and idx_ok() and counts_ok() and res_ok() and part_ok(), "a guard was overwritten"
    assert not torch.isnan(res).any() and not torch.isnan(part).any() and not torch.isnan(q).any(), "an output was not written"
    return dict(q=q.cpu().numpy().reshape(B, Bw, Le), idx=idx.cpu().numpy().reshape(S, B, Le).astype(np.int64),
                counts=counts.cpu().numpy().reshape(S, K).astype(np.int64), res=res.cpu().numpy().reshape(S, B, Bw, Le),
                part=part.cpu().numpy().reshape(S, -1), flat=flat, enc_d=enc_d, idx_d=idx, res_d=res)


def rvq_bwd(f, enc, cb, S, d_q, alias, g_scale=1.0, stats=False, idx_d=None):
    """-> (d_enc, d_c (S K, Bw)[, stat (S, K (Bw + 1))])"""
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
    head = (ptr(f["enc_d"]), ptr(f["idx_d"] if idx_d is None else idx_d), ptr(f["res_d"]), ptr(d_q_d), ptr(f["flat"]), CB_OFF, BETA, g_scale,
            ptr(d_enc), ptr(grad))
    if stats:
        call("wn_rvq_bwd_stats", *head, ptr(stat), S, K, Bw, Le, B, _lib.stream())
    else:
        call("wn_rvq_bwd", *head, S, K, Bw, Le, B, _lib.stream())
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


def stage_inputs(f, enc):
    """r_s as the device saw it: enc, then what it left in res."""
    return np.concatenate([enc[None], f["res"][:-1]])


def check_grads(f, enc, cb, S, d_q, exact, what):
    """d_enc, d_c and stat against float64 on the DEVICE's codes and residuals; two launches and d_enc = d_q give the same bits."""
    (B, Bw, Le), K = enc.shape, cb.shape[0] // S
    C = B * Le
    runs = [rvq_bwd(f, enc, cb, S, d_q, alias) for alias in (False, False, True)]
    srun = [rvq_bwd(f, enc, cb, S, d_q, alias, stats=True) for alias in (False, True)]
    for r in runs[1:] + srun:
        assert np.array_equal(runs[0][0], r[0]), "%s: d_enc differs between launches / forms" % what
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][1], runs[2][1]) and np.array_equal(srun[0][2], srun[1][2]), what
    d_enc, d_c = runs[0]
    stat = srun[0][2].astype(np.float64)
    ref_enc, _ = rvq_ref.backward(enc, cb, S, f["idx"], d_q, BETA, residuals=f["res"])
    r_in = stage_inputs(f, enc).astype(np.float64)
    ref_c = np.concatenate([vq_ref.backward(r_in[s], cb[s * K:(s + 1) * K], f["idx"][s], None, BETA)[1] for s in range(S)])
    ref_stat = np.stack([er.stats(r_in[s], f["idx"][s], K) for s in range(S)])
    assert (d_c[(f["counts"] == 0).reshape(-1)] == 0).all(), "%s: an unused code's gradient is not exactly 0" % what
    assert np.array_equal(stat[:, :K], f["counts"]), "%s: the counts of stat" % what
    if exact:
        assert np.array_equal(d_enc, ref_enc.astype(np.float32)) and np.array_equal(d_c, ref_c.astype(np.float32)), what
        assert np.array_equal(stat, ref_stat), what
        return
    s2 = 2.0 / (C * Bw)
    b_enc = gamma(S + 1) * (np.abs(d_q.astype(np.float64)) + BETA * s2 * np.abs(f["res"].astype(np.float64)).sum(0))
    b_c, b_s = np.zeros_like(ref_c), np.zeros_like(ref_stat)
    for s in range(S):
        rows = cb[s * K:(s + 1) * K].astype(np.float64)
        frames = r_in[s].transpose(0, 2, 1).reshape(-1, Bw)
        diff, mag = np.zeros((K, Bw)), np.zeros((K, Bw))
        np.add.at(diff, f["idx"][s].reshape(-1), np.abs(rows[f["idx"][s].reshape(-1)] - frames))
        np.add.at(mag, f["idx"][s].reshape(-1), np.abs(frames))
        b_c[s * K:(s + 1) * K] = gamma(f["counts"][s].max() + 1) * s2 * diff
        b_s[s, K:] = ((f["counts"][s].max() + 1) * U * mag).reshape(-1)
    for got, ref, bound, name in ((d_enc, ref_enc, b_enc, "d_enc"), (d_c, ref_c, b_c, "d_c"), (stat, ref_stat, b_s, "stat")):
        err = np.abs(got.astype(np.float64) - ref)
        print("  %s %s: largest error %.3e, largest error / bound %.3f" % (what, name, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (what, name)


def check_mse(f, S, C, Bw, exact, what):
    """every stage's partials against the float64 sum of ITS residual's squares (res[s] = r_s - q_s, bit for bit the device's)"""
    for s in range(S):
        got = f["part"][s].astype(np.float64).sum()
        ref = (f["res"][s].astype(np.float64) ** 2).sum() / (C * Bw)
        print("  %s mse of stage %d: %.9g (float64 %.9g)" % (what, s, got, ref))
        assert got == ref if exact else abs(got - ref) <= gamma(Bw + C + 2) * ref, (what, s, got, ref)


# ------------------------------------------------------------------------------------------------------------------ S = 1
def test_one_stage_has_the_bits_of_the_plain_entries():
    from music_amd import _lib
    from music_amd._lib import call, ptr
    Bw, K, B, Le = 12, 24, 5, 7
    for grid, seed in ((True, 11), (False, 23)):
        enc, cb, d_q = draw((1, Bw, K, B, Le), grid, seed)
        f1, f = run_fwd(enc, cb), rvq_fwd(enc, cb, 1)
        assert np.array_equal(f["q"], f1["q"]) and np.array_equal(f["idx"][0], f1["idx"]) and np.array_equal(f["counts"][0], f1["counts"])
        assert np.array_equal(f["part"][0].view(np.int32), f1["part"].view(np.int32))
        assert np.array_equal(f["res"][0], enc - f1["q"])
        for g in (1.0, 0.5):
            for a, b in zip(rvq_bwd(f, enc, cb, 1, d_q, False, g), run_bwd(f1, enc, cb, d_q, False, g)):
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
        d_enc, _, stat = rvq_bwd(f, enc, cb, 1, d_q, True, stats=True)
        d_enc1, stat1 = run_stats(f1, enc, cb, d_q, True)
        assert np.array_equal(d_enc.view(np.int32), d_enc1.view(np.int32)) and np.array_equal(stat[0].view(np.int32), stat1.view(np.int32))
        # the update: two calls with a restart threshold, on twins
        plain, dev = Device(cb), RvqDevice(cb, 1)
        for stat in draw_stats((Bw, K, B, Le), grid, 41, steps=2):
            want, got = plain.update(stat, 0.9, 1e-5, 0.95), dev.update(stat[None], 0.9, 1e-5, 0.95)
            assert np.array_equal(got["cb"].view(np.int32), want["cb"].view(np.int32))
            assert np.array_equal(got["state"][0].view(np.int32), want["state"].view(np.int32)) and got["info"][0].tolist() == want["info"].tolist()
        assert want["info"][0] > 0
        codes = torch.from_numpy(f1["idx"].astype(np.int32)).cuda()
        outs = []
        for name, extra in (("wn_vq_lookup", ()), ("wn_rvq_lookup", (1, 1))):
            q, q_ok = guarded(B * Bw * Le)
            call(name, ptr(codes), ptr(f["flat"]), CB_OFF, ptr(q), None, *extra, K, Bw, Le, B, _lib.stream())
            torch.cuda.synchronize()
            assert q_ok()
            outs.append(q.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], f1["q"].reshape(-1))


# ------------------------------------------------------------------------------------------------------------------ forward, backward
@pytest.mark.parametrize("case", GRID_CASES, ids=ids(GRID_CASES))
def test_grid_inputs_equal_float64_in_every_frame_and_stage(case):
    S, Bw, K, B, Le = case
    C = B * Le
    enc, cb, d_q = draw(case, True, seed=11)
    assert all((cb[s * K:(s + 1) * K] != cb[:K]).any() for s in range(1, S)), "the stages' codebooks must differ"
    ref = rvq_ref.forward(enc, cb, S, BETA)
    assert vq_ref.margins(ref["dist"][S - 1])[0, 0] == 0, "no tie was planted in the last stage"
    f, f2 = rvq_fwd(enc, cb, S), rvq_fwd(enc, cb, S)
    for k in ("q", "idx", "counts", "res", "part"):
        assert np.array_equal(f[k], f2[k]), "two launches differ in %s" % k
    assert np.array_equal(f["idx"], ref["idx"]), "idx differs in %d (frame, stage) pairs" % (f["idx"] != ref["idx"]).sum()
    # the planted tie went to the smaller index (below it only where a drawn row coincides with the planted one: idx equals float64's)
    assert f["idx"][S - 1, 0, 0] <= (1 if K >= 4 else 0) and ref["dist"][S - 1, 0, 0, f["idx"][S - 1, 0, 0]] == 0
    assert np.array_equal(f["q"], ref["q"].astype(np.float32)) and np.array_equal(f["res"], ref["res"].astype(np.float32))
    assert np.array_equal(f["counts"], ref["counts"]) and (f["counts"].sum(1) == C).all()
    pow2 = (C * Bw) & (C * Bw - 1) == 0
    check_mse(f, S, C, Bw, pow2, "grid")
    check_grads(f, enc, cb, S, d_q, pow2, "grid")
    f3 = rvq_fwd(enc, cb, S, with_counts=False)                           # counts is optional
    assert np.array_equal(f3["idx"], f["idx"]) and np.array_equal(f3["part"], f["part"]) and (f3["counts"] == 99).all()


def inside_band(dist, band):
    return int((vq_ref.margins(dist) <= band).sum())


@pytest.mark.parametrize("case", NORMAL_CASES, ids=ids(NORMAL_CASES))
def test_normal_inputs_stage_by_stage_on_the_devices_own_residuals(case):
    S, Bw, K, B, Le = case
    C = B * Le
    band = 4 * (Bw + 2) * U
    enc, cb, d_q = draw(case, False, seed=23)
    ref = rvq_ref.forward(enc, cb, S, BETA)
    close64 = sum(inside_band(ref["dist"][s], band) for s in range(S))
    print("  float64 chain: %d of %d (frame, stage) pairs inside the band of %.2e" % (close64, S * C, band))
    assert close64 <= 0.05 * S * C, "the float64 side itself has too many pairs inside the band: the draw decides nothing"
    f = rvq_fwd(enc, cb, S)
    r_in = stage_inputs(f, enc)
    close = 0
    q = None
    for s in range(S):
        rows = cb[s * K:(s + 1) * K]
        one = vq_ref.forward(r_in[s], rows, BETA)                         # float64, on the device's own fp32 input of this stage
        clear = vq_ref.margins(one["dist"]) > band
        close += int((~clear).sum())
        assert np.array_equal(f["idx"][s][clear], one["idx"][clear]), "stage %d: a frame outside the band got another code" % s
        chosen = np.take_along_axis(one["dist"], f["idx"][s][..., None], -1)[..., 0]
        assert (chosen <= one["dist"].min(-1) * (1 + band)).all(), "stage %d: a code beyond the band of the minimum" % s
        q_s = rows[f["idx"][s]].transpose(0, 2, 1)
        assert np.array_equal(f["res"][s].view(np.int32), (r_in[s] - q_s).view(np.int32)), "stage %d: res is not fp32 r_s - c[idx]" % s
        q = q_s if q is None else q + q_s
        assert np.array_equal(f["counts"][s], np.bincount(f["idx"][s].reshape(-1), minlength=K))
    print("  device: %d of %d (frame, stage) pairs inside the band" % (close, S * C))
    assert close <= 0.05 * S * C
    assert np.array_equal(f["q"].view(np.int32), q.view(np.int32)), "q is not the fp32 sum of the stages' rows in stage order"
    check_mse(f, S, C, Bw, False, "normal")
    check_grads(f, enc, cb, S, d_q, False, "normal")


def test_an_upstream_scale_reaches_the_loss_gradients_only_and_a_bad_code_gives_nan():
    case = (3, 64, 24, 2, 4)                                                # C Bw = 512: every scale a power of two
    S, Bw, K, B, Le = case
    enc, cb, d_q = draw(case, True, seed=31)
    f = rvq_fwd(enc, cb, S)
    d_enc, d_c = rvq_bwd(f, enc, cb, S, d_q, False, g_scale=4.0)
    ref_enc, ref_c = rvq_ref.backward(enc, cb, S, f["idx"], d_q, BETA, g=4.0)
    assert np.array_equal(d_enc, ref_enc.astype(np.float32)) and np.array_equal(d_c, ref_c.astype(np.float32))
    d_enc0, d_c0 = rvq_bwd(f, enc, cb, S, d_q, False, g_scale=0.0)         # vq_loss left out of the objective
    assert np.array_equal(d_enc0, d_q) and (d_c0 == 0).all()
    for wrong, s in ((K, 0), (-1, 1), (1 << 30, 2)):                         # compared, never dereferenced: that frame's d_enc is NaN
        idx = f["idx"].copy()
        idx[s, 1, 2] = wrong
        idx_d = torch.from_numpy(idx.astype(np.int32)).cuda()
        for stats in (False, True):
            out = rvq_bwd(f, enc, cb, S, d_q, False, stats=stats, idx_d=idx_d)
            assert np.isnan(out[0][1, :, 2]).all() and np.isfinite(np.delete(out[0], 2, axis=2)).all()
            if stats:
                assert out[2][s, :K].sum() == B * Le - 1 and (np.delete(out[2][:, :K].sum(1), s) == B * Le).all()


# ------------------------------------------------------------------------------------------------------------------ the update
class RvqDevice:
    """flat (canary around the S K rows), state (S blocks), work (S blocks) and info [S][2] on the device, between guards."""

    def __init__(self, cb, S):
        from music_amd import _lib
        self.S, self.K, self.Bw = S, cb.shape[0] // S, cb.shape[1]
        self.flat, self.flat_ok = guarded(CB_OFF + cb.size + 3, fill=CANARY)
        self.flat[CB_OFF:CB_OFF + cb.size] = torch.from_numpy(cb.reshape(-1)).cuda()
        self.state, self.state_ok = guarded(S * self.K * (self.Bw + 1))
        self.state.copy_(torch.from_numpy(rvq_ref.initial_state(cb, S).astype(np.float32).reshape(-1)).cuda())
        self.work, self.work_ok = guarded(S * _lib.VQ_EMA_WORK_BYTES // 4)
        self.info, self.info_ok = guarded(2 * S, torch.int32, fill=0)

    def update(self, stat, decay, eps, restart, guard=None, with_info=True):
        from music_amd import _lib
        from music_amd._lib import call, ptr
        stat_d = torch.from_numpy(np.ascontiguousarray(stat, dtype=np.float32)).cuda()
        call("wn_rvq_ema_update", ptr(self.flat), CB_OFF, ptr(stat_d), ptr(self.state), ptr(self.work), ptr(self.info) if with_info else None,
             self.S, self.K, self.Bw, decay, eps, restart, ptr(guard), _lib.stream())
        torch.cuda.synchronize()
        assert self.flat_ok() and self.state_ok() and self.work_ok() and self.info_ok(), "a guard was overwritten"
        return self.read()

    def read(self):
        flat = self.flat.cpu().numpy()
        n = self.S * self.K * self.Bw
        rest = np.ones(flat.size, dtype=bool)
        rest[CB_OFF:CB_OFF + n] = False
        assert (flat[rest] == CANARY).all(), "flat was written outside the codebook"
        return dict(cb=flat[CB_OFF:CB_OFF + n].reshape(self.S * self.K, self.Bw).copy(), state=self.state.cpu().numpy().reshape(self.S, -1),
                    info=self.info.cpu().numpy().reshape(self.S, 2).copy())

    @staticmethod
    def stage(snap, s, K):
        return dict(cb=snap["cb"][s * K:(s + 1) * K], state=snap["state"][s], info=snap["info"][s])


UPDATE_CASES = [(3, 7, 17, 2, 4), (2, 65, 1024, 3, 70), (8, 512, 24, 1, 5)]


@pytest.mark.parametrize("case", UPDATE_CASES, ids=ids(UPDATE_CASES))
def test_updates_with_restarts_decide_per_stage_as_float64_does(case):
    S, Bw, K, B, Le = case
    cb = draw(case, False, 11)[1]
    # a stat per stage and step, the stages' draws differ: a stage that ranks another stage's codes fails
    stats = np.stack([draw_stats((Bw, K, B, Le), True, 41 + s) for s in range(S)], axis=1)          # (steps, S, K (Bw + 1))
    dev, twin = RvqDevice(cb, S), RvqDevice(cb, S)
    restarted = np.zeros(S, dtype=np.int64)
    for step, stat in enumerate(stats):
        before = dev.read()
        after, again = dev.update(stat, 0.5, 0.0, 0.75), twin.update(stat, 0.5, 0.0, 0.75)
        for k in ("cb", "state", "info"):
            assert np.array_equal(after[k], again[k], equal_nan=True), "two runs differ in %s" % k
        for s in range(S):
            ref = check_update(RvqDevice.stage(before, s, K), RvqDevice.stage(after, s, K), stat[s], K, 0.5, 0.0, 0.75,
                               "step %d, stage %d" % (step, s), True)
            restarted[s] += ref["restarted"]
            assert after["info"][s].tolist() == [restarted[s], ref["left"]], "info of stage %d" % s
    assert (restarted > 0).all(), "a stage restarted no code"
    stat = stats[0]
    for g, eps, r in ((0.99, 1e-5, 0.985), (0.9, 1e-5, 0.0)):              # the defaults' decay and smoothing; no restart at 0
        before = dev.read()
        after = dev.update(stat, g, eps, r, with_info=r > 0)
        for s in range(S):
            check_update(RvqDevice.stage(before, s, K), RvqDevice.stage(after, s, K), stat[s], K, g, eps, r, "g = %g, stage %d" % (g, s), False)
    # a skipped guarded step leaves everything bit for bit; a taken one is the unguarded update
    first = dev.read()
    skipped = dev.update(stat, 0.9, 1e-5, 0.95, guard=guard_block(1))
    for k in ("cb", "state", "info"):
        assert np.array_equal(first[k].view(np.int32), skipped[k].view(np.int32)), "a skipped step changed %s" % k
    twin.state.copy_(dev.state), twin.flat.copy_(dev.flat), twin.info.copy_(dev.info)
    taken, want = dev.update(stat, 0.9, 1e-5, 0.95, guard=guard_block(0)), twin.update(stat, 0.9, 1e-5, 0.95)
    for k in ("cb", "state", "info"):
        assert np.array_equal(taken[k], want[k], equal_nan=True), "a taken guarded step differs from the unguarded one in %s" % k


# ------------------------------------------------------------------------------------------------------------------ lookup
LOOKUP_CASES = [(3, 7, 17, 2, 4), (8, 65, 1024, 3, 70)]


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=ids(LOOKUP_CASES))
def test_lookup_of_a_prefix_and_its_out_of_range_flag(case):
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
        codes_d = torch.from_numpy(np.ascontiguousarray(codes[:n])).cuda()
        call("wn_rvq_lookup", ptr(codes_d), ptr(flat), CB_OFF, ptr(q), ptr(bad) if with_flag else None, S, n, K, Bw, Le, B, _lib.stream())
        torch.cuda.synchronize()
        assert q_ok() and bad_ok()
        return q.cpu().numpy().reshape(B, Bw, Le), int(bad.item())

    for n in sorted({1, 2, S - 1, S}):
        want = None
        for s in range(n):                                                  # the fp32 sum in stage order
            row = cb[s * K:(s + 1) * K][codes[s]].transpose(0, 2, 1)
            want = row if want is None else want + row
        q, bad = lookup(codes, n)
        assert bad == 0 and np.array_equal(q.view(np.int32), want.view(np.int32)), "the first %d stages" % n
        assert np.array_equal(lookup(codes, n)[0], q), "two launches differ"
    q, _ = lookup(codes, S)
    for wrong, s in ((K, 0), (-1, S - 1), (1 << 30, 1)):                    # never read: the frame is NaN, the flag is up, the others untouched
        c2 = codes.copy()
        c2[s, B - 1, Le // 2] = wrong
        q2, bad = lookup(c2, S)
        assert bad == 1 and np.isnan(q2[B - 1, :, Le // 2]).all()
        q2[B - 1, :, Le // 2] = q[B - 1, :, Le // 2]
        assert np.array_equal(q2, q)
        assert np.isnan(lookup(c2, S, with_flag=False)[0][B - 1, :, Le // 2]).all()
    if S > 2:                                                               # a bad code in a stage behind the prefix is not looked at
        c2 = codes.copy()
        c2[S - 1, 0, 0] = K
        assert lookup(c2, S - 1)[1] == 0
