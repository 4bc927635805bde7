"""wn_vq_bwd_stats / wn_vq_ema_update (music_amd/csrc/wn_vq.hip) alone, through ctypes, against tests/vq_ema_ref.py in float64.

Stats, on grid inputs (multiples of 1/8 in [-2, 2]; a sum of up to 2^11 of them stays below 2^12 in units of 2^-3: exact in fp32 in
any order): n and s must EQUAL the float64 ones, the codebook's rows of flat_grad are exactly 0, the rest of flat_grad keeps its
canary, d_enc has the bits of wn_vq_bwd on the same inputs (grid and normal, d_enc aliasing d_q or not), two launches agree, and the
stats of two halves of the clips add up to the whole's.

Update, per call against the float64 rule applied to the DEVICE's state before the call and the stat it was given, u = 2^-24:
  N'           3 u relative         (1 - g rounded to fp32, the product g N, the fused multiply-add)
  m'           3 u (|g m| + |(1 - g) s|)
  codebook     (K + 16) u (|g m| + |(1 - g) s|) / Nhat      the K-term sum behind tot, one division, the few roundings around it
  restarted    4 u |s_k / n_k|      one division
With g = 0.5 and the initial state every N' is a dyadic rational, exact in fp32: the dead / donor decisions must EQUAL float64's
(the test asserts first that no float64 N' lies within 1e-6 of the threshold).
Outputs lie between NaN guards; flat holds a canary outside the codebook's rows."""
import numpy as np
import pytest
import torch

from tests import vq_ema_ref as er
from tests.test_gpu_vq_kernels import BETA, CANARY, CB_OFF, draw, guarded, run_bwd, run_fwd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (Bw, K, B, Le): Bw crosses the 64 lanes (1, 7 | 64 | 65, 512), K the four codes of a workgroup and the waves of the ranking
# launch (2 | 17, 64 | 1024), B Le the 64 frames of a ballot (1 .. 16 | 210)
CASES = [(1, 2, 1, 1), (7, 17, 2, 4), (64, 64, 3, 3), (65, 1024, 3, 70), (512, 17, 3, 3), (512, 1024, 2, 4)]
IDS = ["bw%d_k%d_b%d_le%d" % c for c in CASES]


def run_stats(f, enc, cb, d_q, alias, idx_d=None, clips=None):
    """wn_vq_bwd_stats on the forward `f` (tests/test_gpu_vq_kernels.run_fwd) -> (d_enc, stat); clips = (first, count): those clips only."""
    from music_amd import _lib
    from music_amd._lib import call, ptr
    (B, Bw, Le), K = enc.shape, cb.shape[0]
    b0, nb = clips or (0, B)
    total = f["flat"].numel()
    grad, grad_ok = guarded(total, fill=CANARY)
    grad[CB_OFF:CB_OFF + K * Bw] = float("nan")
    stat, stat_ok = guarded(K * (Bw + 1))
    d_q_d, dq_ok = guarded(nb * Bw * Le)
    d_q_d.copy_(torch.from_numpy(np.ascontiguousarray(d_q[b0:b0 + nb]).reshape(-1)).cuda())
    d_enc, de_ok = (d_q_d, dq_ok) if alias else guarded(nb * Bw * Le)
    idx_d = f["idx_d"] if idx_d is None else idx_d
    call("wn_vq_bwd_stats", ptr(f["enc_d"], b0 * Bw * Le), ptr(idx_d, b0 * Le), ptr(d_q_d), ptr(f["flat"]), CB_OFF, BETA, 1.0, ptr(d_enc),
         ptr(grad), ptr(stat), K, Bw, Le, nb, _lib.stream())
    torch.cuda.synchronize()
    assert grad_ok() and stat_ok() and dq_ok() and de_ok(), "a guard was overwritten"
    grad = grad.cpu().numpy()
    rest = np.ones(total, dtype=bool)
    rest[CB_OFF:CB_OFF + K * Bw] = False
    assert (grad[rest] == CANARY).all(), "flat_grad was written outside the codebook"
    rows = grad[CB_OFF:CB_OFF + K * Bw]
    assert (rows == 0).all() and not np.signbit(rows).any(), "the codebook's gradient is not exactly 0 in all K rows"
    stat = stat.cpu().numpy()
    assert np.isfinite(stat).all(), "not every entry of stat was written"
    return d_enc.cpu().numpy().reshape(nb, Bw, Le), stat


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stats_equal_float64_and_d_enc_has_the_bits_of_wn_vq_bwd(case):
    Bw, K, B, Le = case
    for grid, seed in ((True, 11), (False, 23)):
        enc, cb, d_q = draw(case, grid, seed)
        f = run_fwd(enc, cb)
        ref_enc, _ = run_bwd(f, enc, cb, d_q, False)
        runs = [run_stats(f, enc, cb, d_q, alias) for alias in (False, False, True)]
        for d_enc, stat in runs:                                          # = wn_vq_bwd's bits; a second launch and d_enc = d_q: the same
            assert np.array_equal(d_enc, ref_enc), "d_enc differs from wn_vq_bwd's (%s inputs)" % ("grid" if grid else "normal")
            assert np.array_equal(stat, runs[0][1])
        stat = runs[0][1]
        want = er.stats(enc, f["idx"], K)
        n, s = er.split(stat, K)
        assert np.array_equal(n, f["counts"]) and n.sum() == B * Le
        if grid:
            assert np.array_equal(stat.astype(np.float64), want), "grid inputs: n and s must equal float64"
            # the two halves of the clips, added, are the whole (an empty half writes nothing: zeros)
            h = B // 2
            parts = [run_stats(f, enc, cb, d_q, False, clips=(b0, nb))[1] if nb else np.zeros_like(stat) for b0, nb in ((0, h), (h, B - h))]
            assert np.array_equal(parts[0] + parts[1], stat)
        else:
            wn, ws = er.split(want, K)
            frames = np.abs(enc.astype(np.float64)).transpose(0, 2, 1).reshape(-1, Bw)
            mag = np.zeros((K, Bw))
            np.add.at(mag, f["idx"].reshape(-1), frames)
            err = np.abs(s - ws)
            bound = (n.max() + 1) * U * mag
            print("  normal s: largest error %.3e, largest error / bound %.3f" % (err.max(), (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()


def test_a_code_outside_the_codebook_is_compared_and_never_dereferenced():
    case = (7, 17, 2, 4)
    Bw, K, B, Le = case
    enc, cb, d_q = draw(case, True, 31)
    f = run_fwd(enc, cb)
    for wrong in (K, -1, 1 << 30):
        idx = f["idx"].copy()
        idx[1, 2] = wrong
        idx_d = torch.from_numpy(idx.astype(np.int32)).cuda()
        d_enc, stat = run_stats(f, enc, cb, d_q, False, idx_d=idx_d)
        assert np.isnan(d_enc[1, :, 2]).all() and np.isfinite(np.delete(d_enc.reshape(B, Bw, Le), 2, axis=2)).all()
        assert np.array_equal(stat.astype(np.float64), er.stats(enc, idx, K)) and er.split(stat, K)[0].sum() == B * Le - 1


# ---------------------------------------------------------------------------------------------------------------- the update
def guard_block(skip):
    """A wn_guard_state (48 bytes, zeroed) with its skip word set: the upper half of the second 8 bytes."""
    block = torch.zeros(6, dtype=torch.int64, device="cuda")
    block[1] = int(skip) << 32
    return block


class Device:
    """flat (canary around the codebook's rows), state, work and info of one codebook on the device, between guards."""

    def __init__(self, cb, state=None):
        from music_amd import _lib
        K, Bw = cb.shape
        self.K, self.Bw = K, Bw
        self.flat, self.flat_ok = guarded(CB_OFF + K * Bw + 3, fill=CANARY)
        self.flat[CB_OFF:CB_OFF + K * Bw] = torch.from_numpy(cb.reshape(-1)).cuda()
        self.state, self.state_ok = guarded(K * (Bw + 1))
        self.state.copy_(torch.from_numpy((er.initial_state(cb) if state is None else state).astype(np.float32)).cuda())
        self.work, self.work_ok = guarded(_lib.VQ_EMA_WORK_BYTES // 4)
        self.info, self.info_ok = guarded(2, torch.int32, fill=0)

    def update(self, stat, decay, eps, restart, guard=None, with_info=True):
        from music_amd import _lib
        from music_amd._lib import call, ptr
        stat_d = torch.from_numpy(np.asarray(stat, dtype=np.float32)).cuda()
        call("wn_vq_ema_update", ptr(self.flat), CB_OFF, ptr(stat_d), ptr(self.state), ptr(self.work), ptr(self.info) if with_info else None,
             self.K, self.Bw, decay, eps, restart, ptr(guard), _lib.stream())
        torch.cuda.synchronize()
        assert self.flat_ok() and self.state_ok() and self.work_ok() and self.info_ok(), "a guard was overwritten"
        return self.read()

    def read(self):
        flat = self.flat.cpu().numpy()
        rest = np.ones(flat.size, dtype=bool)
        rest[CB_OFF:CB_OFF + self.K * self.Bw] = False
        assert (flat[rest] == CANARY).all(), "flat was written outside the codebook"
        return dict(cb=flat[CB_OFF:CB_OFF + self.K * self.Bw].reshape(self.K, self.Bw).copy(), state=self.state.cpu().numpy(),
                    info=self.info.cpu().numpy().copy())


def draw_stats(case, grid, seed, steps=3):
    """`steps` stat vectors [n | s] as the stats launch gives them for 4 B Le frames whose codes are skewed (a few codes take most
    frames, most codes none: dead codes and donors at every step, ties among the donors), summed here in float64 and rounded to
    fp32 once.  The codes of B Le frames are drawn and used four times over, so every count is a multiple of 4: from the initial
    usage 1 with g = 0.5, N' then takes the fractions .5 | .25, .5 | .125, .25, .5, .625 in steps 1 | 2 | 3 (a restart puts it back
    to 1) and never meets the threshold 0.75 of the test below - a decision ON the threshold is nobody's to check."""
    Bw, K, B, Le = case
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        enc = (rng.integers(-16, 17, size=(4 * B, Bw, Le)) / 8.0) if grid else rng.standard_normal((4 * B, Bw, Le))
        live = rng.permutation(K)[:max(1, min(K, 6))]
        idx = live[np.minimum(rng.geometric(0.4, size=(B, Le)) - 1, len(live) - 1)]
        out.append(er.stats(enc, np.tile(idx, (4, 1)), K).astype(np.float32))
    return out


def check_update(before, after, stat, K, decay, eps, restart, what, exact_decisions):
    """One call: the device's state and codebook behind it against the float64 rule on the device's state in front of it."""
    g, e, r = float(np.float32(decay)), float(np.float32(eps)), float(np.float32(restart))
    ref = er.update(stat, before["state"], K, g, e, r)
    if exact_decisions and r > 0:
        assert (np.abs(ref["N1"] - r) > 1e-6).all(), "a float64 N' lies within 1e-6 of the threshold: the decision is not the test's to make"
    N, m = er.split(after["state"], K)
    Nr, mr = er.split(ref["state"], K)
    hit = ref["donor"] >= 0
    # restarted codes (the pairing itself shows in WHICH rows are batch means: a wrong pairing fails here or below)
    assert (N[hit] == 1.0).all(), what
    mean = ref["cb"][hit]
    err_r = np.abs(after["cb"][hit] - mean)
    assert (err_r <= 4 * U * np.abs(mean)).all(), (what, "restarted rows")
    assert np.array_equal(m[hit], after["cb"][hit].astype(np.float64)), (what, "a restarted code's sums are its new row")
    # every other code: the plain update
    keep = ~hit
    err_N = np.abs(N[keep] - Nr[keep])
    assert (err_N <= 3 * U * Nr[keep]).all(), (what, "N'")
    if exact_decisions:
        assert np.array_equal(N[keep], Nr[keep]), (what, "g = 0.5: N' is exact")
    err_m = np.abs(m[keep] - mr[keep])
    b_m = 3 * U * ref["scale"][keep]
    assert (err_m <= b_m).all(), (what, "m'")
    err_c = np.abs(after["cb"][keep] - ref["cb"][keep])
    b_c = (K + 16) * U * ref["scale"][keep] / ref["nhat"][keep, None]
    assert (err_c <= b_c).all(), (what, "codebook")
    ratio = lambda err, b: float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
    print("  %s: restarted %d, left %d; error / bound: N' %.3f, m' %.3f, codebook %.3f, restarted rows %.3f"
          % (what, ref["restarted"], ref["left"], ratio(err_N, 3 * U * Nr[keep]), ratio(err_m, b_m), ratio(err_c, b_c),
             ratio(err_r, 4 * U * np.abs(mean))))
    return ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_updates_with_restarts_decide_as_float64_does(case):
    Bw, K, B, Le = case
    _, cb, _ = draw(case, True, 11)
    stats = draw_stats(case, True, 41)
    dev, twin = Device(cb), Device(cb)
    restarted = seen_dead = 0
    for step, stat in enumerate(stats):
        before = dev.read()
        after = dev.update(stat, 0.5, 0.0, 0.75)
        again = twin.update(stat, 0.5, 0.0, 0.75)                         # a second run from the same inputs: the same bits
        for k in ("cb", "state", "info"):
            assert np.array_equal(after[k], again[k], equal_nan=True), "two runs differ in %s" % k
        ref = check_update(before, after, stat, K, 0.5, 0.0, 0.75, "step %d" % step, True)
        restarted += ref["restarted"]
        seen_dead += ref["restarted"] + ref["left"]
        assert after["info"].tolist() == [restarted, ref["left"]], "info: restarted so far, dead codes left by this call"
    assert seen_dead > 0, "no code died: the restart was not exercised"
    assert restarted > 0, "no code was restarted"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_restart_at_zero_and_normal_inputs_within_the_bounds(case):
    Bw, K, B, Le = case
    _, cb, _ = draw(case, False, 23)
    stats = draw_stats(case, False, 43)
    dev = Device(cb)
    for step, stat in enumerate(stats):                                   # restart = 0: never, and info stays 0
        before = dev.read()
        after = dev.update(stat, 0.5, 0.0, 0.0)
        ref = check_update(before, after, stat, K, 0.5, 0.0, 0.0, "r = 0, step %d" % step, False)
        assert ref["restarted"] == 0 and after["info"].tolist() == [0, 0]
    dev = Device(cb)
    for step, stat in enumerate(stats):                                   # the defaults' decay and smoothing, a restart threshold between them
        before = dev.read()
        after = dev.update(stat, 0.99, 1e-5, 0.985, with_info=step != 1)  # (info is optional)
        check_update(before, after, stat, K, 0.99, 1e-5, 0.985, "g = 0.99, step %d" % step, False)


def test_a_skipped_step_changes_nothing_and_a_taken_one_is_the_unguarded_update():
    case = (65, 1024, 3, 70)
    Bw, K, B, Le = case
    _, cb, _ = draw(case, False, 23)
    stat = draw_stats(case, False, 47, steps=1)[0]
    dev, plain = Device(cb), Device(cb)
    first = dev.update(stat, 0.9, 1e-5, 0.95)                             # info is no longer 0
    assert first["info"][0] > 0
    skipped = dev.update(stat, 0.9, 1e-5, 0.95, guard=guard_block(1))
    for k in ("cb", "state", "info"):
        assert np.array_equal(first[k].view(np.int32), skipped[k].view(np.int32)), "a skipped step changed %s" % k
    taken = dev.update(stat, 0.9, 1e-5, 0.95, guard=guard_block(0))
    plain.update(stat, 0.9, 1e-5, 0.95)
    want = plain.update(stat, 0.9, 1e-5, 0.95)
    for k in ("cb", "state", "info"):
        assert np.array_equal(taken[k], want[k]), "a taken guarded step differs from the unguarded one in %s" % k
