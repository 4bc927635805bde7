"""Kernel-level tests of the guarded optimizer step (music_amd/csrc/wn_guard.hip, ABI 9) through _lib.call: wn_grad_guard against
float64 numpy on the same float32 inputs, the three guarded updates against torch's optimizers (with clip_grad_norm_ applied
first, with a skipped step omitted)."""
import math

import numpy as np
import pytest
import torch

from music_amd import _lib
from music_amd._lib import call, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 4 * 2.0 ** -24          # float64 accumulation of fewer than 2^31 terms, then ONE rounding to float32
B1, B2 = 0.9, 0.999


class Guard:
    """A zeroed wn_guard_state and its partials on the device."""

    def __init__(self):
        self.state = torch.zeros(6, dtype=torch.int64, device=DEV)
        self.partials = torch.zeros(_lib.GUARD_PARTIALS_BYTES // 8, dtype=torch.int64, device=DEV)

    def run(self, g, n, gscale=1.0, max_norm=0.0, skip=False, b1=B1, b2=B2):
        call("wn_grad_guard", None if g is None else ptr(g), n, gscale, max_norm, 1 if skip else 0, b1, b2, ptr(self.partials),
             ptr(self.state), _lib.stream())
        return self.read()

    def read(self):
        return _lib.GuardState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def raw(self):
        return self.state.cpu().numpy().tobytes(), self.partials.cpu().numpy().tobytes()


def _on_device(values, misalign):
    """float32 numpy -> a device view whose base is 16-byte aligned (misalign 0) or 4 bytes behind such a base (misalign 1)."""
    n = values.size
    buf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[misalign:misalign + n]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 * misalign
    return view


def _ref_norm(values, gscale=1.0):
    return math.sqrt(float(np.sum((values.astype(np.float64) * np.float64(np.float32(gscale))) ** 2)))


def _check_stats(gd, g, values, gscale=1.0):
    n = values.size
    ref = _ref_norm(values, gscale)
    s = gd.run(g, n, gscale)
    print("n %d align %d: norm %.9g ref %.17g rel %.3g" % (n, g.data_ptr() % 16, s.norm, ref, abs(s.norm - ref) / ref))
    assert abs(float(s.norm) - ref) <= REL * ref
    assert (s.nonfinite, s.skip) == (0, 0) and s.coef == 1.0
    first = gd.raw()
    for factor in (0.5, 2.0):
        max_norm = float(np.float32(factor * s.norm))
        c = gd.run(g, n, gscale, max_norm=max_norm)
        want = float(np.float32(min(1.0, max_norm / (float(c.norm) + 1e-6))))
        print("  max_norm %.9g: coef %.9g want %.9g" % (max_norm, c.coef, want))
        assert c.norm == s.norm and abs(float(c.coef) - want) <= REL * want
        assert (c.coef < 1.0) == (want < 1.0)
    # a second run of the first call: bit-equal partials, and the same norm / coef / flags
    again = Guard()
    again.run(g, n, gscale)
    assert again.raw() == first
    return s


@pytest.mark.parametrize("misalign", [0, 1], ids=["aligned16", "base_plus_4"])
@pytest.mark.parametrize("n", [1, 3, 255, 1025, 100003, 256 * 256 * 4 * 2 + 5])
def test_grad_guard_norm_and_coef(n, misalign):
    rng = np.random.default_rng(n + misalign)
    values = (rng.standard_normal(n) * 0.01).astype(np.float32)
    gd = Guard()
    s = _check_stats(gd, _on_device(values, misalign), values)
    assert s.n_taken == 1 and gd.read().n_taken == 3 and gd.read().n_skipped == 0


@pytest.mark.parametrize("value", [1e20, 1e-30], ids=["square_overflows_f32", "square_underflows_f32"])
def test_grad_guard_extreme_magnitudes(value):
    n = 100003
    values = np.full(n, value, dtype=np.float32)
    s = _check_stats(Guard(), _on_device(values, 1), values)
    assert math.isfinite(s.norm) and s.norm > 0


def test_grad_guard_scale_and_counters():
    """gscale enters the norm; bc1 / bc2 follow the device's count of steps taken; an empty gradient is a step of norm 0."""
    n = 1025
    rng = np.random.default_rng(5)
    values = (rng.standard_normal(n) * 0.01).astype(np.float32)
    g = _on_device(values, 1)
    gd = Guard()
    for t in range(1, 4):
        s = gd.run(g, n, gscale=0.25)
        ref = _ref_norm(values, 0.25)
        assert abs(float(s.norm) - ref) <= REL * ref
        assert s.n_taken == t
        b1, b2 = float(np.float32(B1)), float(np.float32(B2))
        assert abs(s.bc1 - (1 - b1 ** t)) <= 2.0 ** -23 * (1 - b1 ** t) and abs(s.bc2 - (1 - b2 ** t)) <= 2.0 ** -23 * (1 - b2 ** t)
    e = Guard().run(None, 0, max_norm=1.0)
    assert (e.norm, e.coef, e.nonfinite, e.skip, e.n_taken, e.n_clipped, e.n_skipped) == (0.0, 1.0, 0, 0, 1, 0, 0)


@pytest.mark.parametrize("flag", [True, False], ids=["skip_nonfinite", "no_flag"])
@pytest.mark.parametrize("where", ["first", "last", "head", "tail"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_grad_guard_nonfinite(value, where, flag):
    n = 100003
    rng = np.random.default_rng(11)
    values = (rng.standard_normal(n) * 0.01).astype(np.float32)
    # base + 4 bytes: elements 0 .. 2 are the scalar head, the body ends at n (no tail), "last" is in the vector body;
    # "tail": a 16-byte aligned base, the last 3 elements are the scalar tail
    g = _on_device(values, 0 if where == "tail" else 1)
    gd = Guard()
    clean = gd.run(g, n, max_norm=1.0, skip=flag)
    assert clean.n_taken == 1 and clean.skip == 0
    g[{"first": 0, "last": n - 1, "head": 1, "tail": n - 2}[where]] = value
    s = gd.run(g, n, max_norm=1.0, skip=flag)
    assert s.nonfinite == 1
    assert math.isnan(s.coef)
    if flag:
        assert s.skip == 1 and s.n_skipped == 1 and s.n_taken == 1
        assert (s.bc1, s.bc2, s.n_clipped) == (clean.bc1, clean.bc2, clean.n_clipped)
    else:
        assert s.skip == 0 and s.n_skipped == 0 and s.n_taken == 2


# ---------------------------------------------------------------------------------------------------------------- guarded updates
N, STEPS, BAR = 100003, 5, 2e-6                           # tests/test_gpu_kernels.py::test_adam_flat_matches_torch: data, constants, bar
TYPICAL_NORM = 0.01 * math.sqrt(N)

OPTS = {
    "adam": (lambda p: torch.optim.Adam([p], lr=1e-3), 0.0),
    "sgd_m0.9": (lambda p: torch.optim.SGD([p], lr=1e-2, momentum=0.9), 0.9),
    "sgd_m0": (lambda p: torch.optim.SGD([p], lr=1e-2, momentum=0.0), 0.0),
    "rmsprop_m0.9": (lambda p: torch.optim.RMSprop([p], lr=1e-3, momentum=0.9), 0.9),
    "rmsprop_m0": (lambda p: torch.optim.RMSprop([p], lr=1e-3, momentum=0.0), 0.0),
}


def _data():
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(N, generator=g)
    grads = [torch.randn(N, generator=g) * 0.01 for _ in range(STEPS)]
    return p0, grads


class Flat:
    """The guarded flat optimizer `kind` on device buffers."""

    def __init__(self, kind, p0, max_norm, skip):
        self.kind, self.mom = kind.split("_")[0], OPTS[kind][1]
        self.p = p0.clone().to(DEV)
        self.a, self.b = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)      # m, v / momentum buffer / square_avg, buffer
        self.gd, self.max_norm, self.skip = Guard(), max_norm, skip

    def step(self, gr):
        g = (gr * 4).to(DEV)                               # gscale 0.25 undoes it, as in test_adam_flat_matches_torch
        adam = self.kind == "adam"
        self.gd.run(g, N, 0.25, self.max_norm, self.skip, B1 if adam else 0.0, B2 if adam else 0.0)
        st, sp = _lib.stream(), ptr(self.gd.state)
        if adam:
            call("wn_adam_flat_guarded", ptr(self.p), ptr(g), ptr(self.a), ptr(self.b), N, 1e-3, B1, B2, 1e-8, 0.25, sp, st)
        elif self.kind == "sgd":
            call("wn_sgd_flat_guarded", ptr(self.p), ptr(g), ptr(self.a) if self.mom else None, N, 1e-2, self.mom, 0.25, sp, st)
        else:
            call("wn_rmsprop_flat_guarded", ptr(self.p), ptr(g), ptr(self.a), ptr(self.b) if self.mom else None, N, 1e-3, 0.99, 1e-8,
                 self.mom, 0.25, sp, st)

    def buffers(self):
        return [self.p.clone(), self.a.clone(), self.b.clone()]


def _torch_run(kind, p0, grads, max_norm=None):
    p_ref = p0.clone().requires_grad_(True)
    opt = OPTS[kind][0](p_ref)
    for gr in grads:
        p_ref.grad = gr.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p_ref], max_norm)
        opt.step()
    return p_ref.detach()


def _err(flat, ref):
    e = (flat.p.cpu() - ref).abs().max().item()
    print("max abs difference to torch: %.3g" % e)
    return e


@pytest.mark.parametrize("kind", list(OPTS))
def test_guarded_update_unclipped_matches_torch(kind):
    p0, grads = _data()
    flat = Flat(kind, p0, 0.0, False)
    for gr in grads:
        flat.step(gr)
    assert _err(flat, _torch_run(kind, p0, grads)) < BAR
    s = flat.gd.read()
    assert (s.n_taken, s.n_clipped, s.n_skipped, s.coef) == (STEPS, 0, 0, 1.0)


@pytest.mark.parametrize("kind", list(OPTS))
def test_guarded_update_clipped_matches_torch_with_clip_grad_norm(kind):
    p0, grads = _data()
    max_norm = 0.5 * TYPICAL_NORM
    flat = Flat(kind, p0, max_norm, True)
    for gr in grads:
        flat.step(gr)
    assert _err(flat, _torch_run(kind, p0, grads, max_norm)) < BAR
    s = flat.gd.read()
    assert (s.n_taken, s.n_clipped, s.n_skipped) == (STEPS, STEPS, 0) and 0.45 < s.coef < 0.55


@pytest.mark.parametrize("kind", list(OPTS))
def test_guarded_update_skips_a_nonfinite_step_bit_for_bit(kind):
    """Step 3 of 5 carries an inf: nothing moves in it, and the run ends where torch ends when step 3 is simply left out - Adam's
    bias correction followed the device's count of steps taken, not the host's count of steps issued."""
    p0, grads = _data()
    grads[2] = grads[2].clone()
    grads[2][N // 3] = float("inf")
    flat = Flat(kind, p0, 0.0, True)
    for k, gr in enumerate(grads):
        before = flat.buffers()
        flat.step(gr)
        if k == 2:
            assert all(torch.equal(a, b) for a, b in zip(before, flat.buffers()))
            assert torch.isfinite(flat.p).all()
    assert _err(flat, _torch_run(kind, p0, grads[:2] + grads[3:])) < BAR
    s = flat.gd.read()
    assert (s.n_taken, s.n_skipped) == (STEPS - 1, 1)


def test_guarded_sgd_first_step_skipped_does_not_seed_the_momentum():
    p0, grads = _data()
    grads[0] = grads[0].clone()
    grads[0][7] = float("nan")
    flat = Flat("sgd_m0.9", p0, 0.0, True)
    flat.a.fill_(123.0)                                    # what a "first step" must overwrite, not accumulate
    for k, gr in enumerate(grads):
        flat.step(gr)
        if k == 0:
            assert torch.equal(flat.p.cpu(), p0) and bool((flat.a == 123.0).all())
    assert _err(flat, _torch_run("sgd_m0.9", p0, grads[1:])) < BAR
