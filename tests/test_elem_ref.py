"""tests/elem_ref.py (the float64 formulas the GPU tests of the elementwise and reduction helpers compare with) against independent
authorities - float64 autograd and torch.optim on float64 parameters - within 1e-12, so that a wrong reference cannot pass a wrong
kernel.  No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elem_ref

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("q", [1, 7, 64, 100, 256])
def test_softmax_and_its_backward_are_autograd(q):
    rng = np.random.default_rng(q)
    x = (rng.standard_normal((13, q)) * 3).astype(np.float32)
    dy = rng.standard_normal((13, q)).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    y = torch.softmax(xt, 1)
    _close(elem_ref.softmax(x), y.detach().numpy())
    y.backward(torch.from_numpy(dy).double())
    _close(elem_ref.softmax_bwd(y.detach().numpy(), dy), xt.grad.numpy())


@pytest.mark.parametrize("q", [1, 7, 65, 256])
def test_fused_ce_is_cross_entropy_of_the_probabilities(q):
    rng = np.random.default_rng(100 + q)
    n = 11
    x = (rng.standard_normal((n, q)) * 3).astype(np.float32)
    x[3] = 1.5                                                          # a row of equal logits
    x[4, 0], x[4, 1:] = 80.0, -80.0
    tgt = rng.integers(0, q, n)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    p = torch.softmax(xt, 1)
    per_row = F.cross_entropy(p, torch.from_numpy(tgt), reduction="none")
    loss = F.cross_entropy(p, torch.from_numpy(tgt))
    loss.backward()
    rp, rl, rmean, rdx = elem_ref.softmax_ce(x, tgt, 1.0 / n)
    _close(rp, p.detach().numpy())
    _close(rl, per_row.detach().numpy())
    _close(rmean, loss.item())
    _close(rdx, xt.grad.numpy())


def test_fused_ce_bad_target_rule():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 9)).astype(np.float32)
    tgt = np.array([0, 9, 3, -1, 1 << 40, 8])
    p, loss, mean, dx = elem_ref.softmax_ce(x, tgt, 1.0 / 6)
    bad = np.array([False, True, False, True, True, False])
    assert np.isnan(loss[bad]).all() and np.isnan(dx[bad]).all() and np.isnan(mean)
    good = np.where(bad, 0, tgt)
    _, l2, _, dx2 = elem_ref.softmax_ce(x, good, 1.0 / 6)
    assert np.array_equal(loss[~bad], l2[~bad]) and np.array_equal(dx[~bad], dx2[~bad]) and np.isfinite(p).all()


def test_gate_and_its_derivatives_are_autograd():
    rng = np.random.default_rng(6)
    f = np.concatenate([rng.standard_normal(40) * 2, [0.0, 15.0, -15.0, 81.0, -81.0, 104.0, -104.0]]).astype(np.float32)
    g = np.concatenate([rng.standard_normal(40) * 2, [0.0, -15.0, 15.0, -81.0, 81.0, -104.0, 104.0]]).astype(np.float32)
    ft, gt = (torch.from_numpy(a).double().requires_grad_(True) for a in (f, g))
    z = torch.tanh(ft) * torch.sigmoid(gt)
    z.sum().backward()
    _close(elem_ref.gate(f, g), z.detach().numpy())
    df, dg = elem_ref.gate_d(f, g)
    assert np.isfinite(df).all() and np.isfinite(dg).all()
    _close(df, ft.grad.numpy())
    _close(dg, gt.grad.numpy())


@pytest.mark.parametrize("mode,le,q,L", [(1, 7, 41, 300), (1, 5, 1000, 37), (1, 3, 700, 1500), (1, 1, 5, 9), (1, 8, 1, 20),
                                         (2, 5, 0, 1), (2, 5, 0, 4), (2, 31, 0, 1103), (2, 64, 0, 64), (2, 100, 0, 250)])
def test_bucket_sums_are_autograd_of_the_expansion(mode, le, q, L):
    rng = np.random.default_rng(le * 1000 + L)
    ix = elem_ref.bucket_index(L, mode, le, q)
    want = np.minimum(np.arange(L) // q, le - 1) if mode == 1 else np.arange(L) % le
    assert np.array_equal(ix, want) and ix.min() >= 0 and ix.max() < le
    tab = rng.standard_normal((2, 3, le)).astype(np.float32)
    w = rng.standard_normal((2, 3, L)).astype(np.float32)
    tt = torch.from_numpy(tab).double().requires_grad_(True)
    ex = tt[:, :, torch.from_numpy(ix)]
    assert np.array_equal(elem_ref.bucket_expand(tab, L, mode, le, q), ex.detach().numpy().astype(np.float32))
    (ex * torch.from_numpy(w).double()).sum().backward()
    _close(elem_ref.bucket_sums(w, mode, le, q), tt.grad.numpy())
    sa, cnt = elem_ref.bucket_abs_sums(w, mode, le, q)
    assert cnt.sum() == L and np.array_equal(cnt, np.bincount(ix, minlength=le))
    _close(sa, elem_ref.bucket_sums(np.abs(w), mode, le, q))
    assert (elem_ref.bucket_sums(w, mode, le, q)[..., cnt == 0] == 0).all()


def test_empty_window_sums_to_zero():
    for mode in (1, 2):
        assert np.array_equal(elem_ref.bucket_sums(np.zeros((2, 3, 0), np.float32), mode, 4, 3), np.zeros((2, 3, 4)))


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for _ in range(4)]


def test_adam_is_torch_optim_adam_over_three_steps():
    n, lr, b1, b2, eps = 50, 1e-3, 0.9, 0.999, 1e-8
    p0, g1, g2, g3 = _inputs(n, 1)
    f32 = lambda v: float(np.float32(v))
    tp = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([tp], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps))
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate((g1, g2, g3), 1):
        tp.grad = torch.from_numpy(g).double() * 0.25
        opt.step()
        # the bias corrections in float64 from the float32 betas: elem_ref takes the float32 value of every scalar, so give it
        # corrections that float32 holds exactly enough for 1e-12 - compare with the unrounded ones through adam_p
        bc1, bc2 = 1 - f32(b1) ** t, 1 - f32(b2) ** t
        _, m, v = elem_ref.adam_step(p, g, m, v, lr, b1, b2, eps, 1.0, 1.0, 0.25)
        p = p - (f32(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + f32(eps))
        _close(p, tp.detach().numpy())
        st = opt.state[tp]
        _close(m, st["exp_avg"].numpy())
        _close(v, st["exp_avg_sq"].numpy())
    # adam_step's own parameter step, with corrections float32 holds exactly
    pa, ma, va = elem_ref.adam_step(p0, g1, m, v, lr, b1, b2, eps, 0.25, 0.0625, 0.25)
    _close(pa, p0 - (f32(lr) / 0.25) * ma / (np.sqrt(va) / 0.25 + f32(eps)))
    _close(elem_ref.adam_p(p0, ma, va, lr, eps, 0.25, 0.0625), pa)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_is_torch_optim_sgd_over_three_steps(momentum):
    n, lr = 50, 1e-2
    f32 = lambda v: float(np.float32(v))
    p0, g1, g2, g3 = _inputs(n, 2)
    tp = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.SGD([tp], lr=f32(lr), momentum=f32(momentum))
    p, buf = p0.astype(np.float64), None
    for t, g in enumerate((g1, g2, g3), 1):
        tp.grad = torch.from_numpy(g).double() * 0.25
        opt.step()
        p, buf = elem_ref.sgd_step(p, g, buf, lr, momentum, 0.25, t == 1)
        _close(p, tp.detach().numpy())
        if momentum:
            _close(buf, opt.state[tp]["momentum_buffer"].numpy())
        else:
            assert buf is None


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_is_torch_optim_rmsprop_over_three_steps(momentum):
    n, lr, alpha, eps = 50, 1e-3, 0.99, 1e-8
    f32 = lambda v: float(np.float32(v))
    p0, g1, g2, g3 = _inputs(n, 3)
    tp = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.RMSprop([tp], lr=f32(lr), alpha=f32(alpha), eps=f32(eps), momentum=f32(momentum))
    p, sq, buf = p0.astype(np.float64), np.zeros(n), (np.zeros(n) if momentum else None)
    for g in (g1, g2, g3):
        tp.grad = torch.from_numpy(g).double() * 0.25
        opt.step()
        p, sq, buf = elem_ref.rmsprop_step(p, g, sq, buf, lr, alpha, eps, momentum, 0.25)
        _close(p, tp.detach().numpy())
        _close(sq, opt.state[tp]["square_avg"].numpy())
        if momentum:
            _close(buf, opt.state[tp]["momentum_buffer"].numpy())
        else:
            assert buf is None


@pytest.mark.parametrize("q,t", [(1, 3), (2, 5), (7, 4), (256, 9)])
def test_onehot_layouts(q, t):
    rng = np.random.default_rng(q + t)
    codes = rng.integers(0, q, (3, t))
    codes[1, 0], codes[2, t - 1], codes[0, 1] = -1, q, np.iinfo(np.int32).min
    proper = elem_ref.onehot(codes, q, False)
    ok = (codes >= 0) & (codes < q)
    want = F.one_hot(torch.from_numpy(np.where(ok, codes, 0)), q).permute(0, 2, 1).numpy().astype(np.float32) * ok[:, None, :]
    assert proper.dtype == np.float32 and np.array_equal(proper, want)
    # scrambled: the (t, q) one-hot of the loader, viewed as (q, t) without moving a float
    scr = elem_ref.onehot(codes, q, True)
    assert np.array_equal(scr, want.transpose(0, 2, 1).reshape(3, q, t))
    assert scr.sum() == ok.sum() == proper.sum()


def test_gather_and_mulaw():
    packed = np.arange(10, dtype=np.float32) + 0.5
    idx = np.array([3, -1, 0, 9, -7, 0])
    assert np.array_equal(elem_ref.gather(packed, idx), np.array([3.5, 0, 0.5, 9.5, 0, 0.5], np.float32))
    thr = np.array([-0.5, 0.0, 0.0, 0.25], np.float32)
    x = np.array([-np.inf, -1, -0.5, np.nextafter(np.float32(-0.5), np.float32(-1)), -0.0, 0.0, 0.1, 0.25, np.inf], np.float32)
    want = [int((thr <= v).sum()) for v in x]
    assert want == [0, 0, 1, 0, 3, 3, 3, 4, 4]
    assert np.array_equal(elem_ref.mulaw_encode(x, thr), want)
    table = np.array([-1, -0.3, 0.0, 0.3, 1], np.float32)
    assert np.array_equal(elem_ref.mulaw_decode([-5, 0, 4, 5, 1 << 30, 2], table), np.array([-1, -1, 1, 1, 1, 0], np.float32))
