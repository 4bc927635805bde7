"""tests/vq_ref.py against torch autograd in float64: the straight-through estimator e + (q - e).detach() with
mse_loss(q, e.detach()) + beta mse_loss(e, q.detach()), the tie rule, unused codes, the perplexity.  No device is touched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vq_ref


def _autograd(enc, cb, w, beta, with_vq_loss=True):
    """loss = sum(w * ste(q)) [+ vq_loss] through torch in float64 -> (idx, q, vq_loss, d_enc, d_cb)"""
    e = torch.tensor(enc, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(cb, dtype=torch.float64, requires_grad=True)
    frames = e.permute(0, 2, 1)                                                   # (B, Le, Bw)
    dist = ((frames[:, :, None, :] - c[None, None]) ** 2).sum(-1)
    idx = dist.argmin(-1)
    q = c[idx].permute(0, 2, 1)
    ste = e + (q - e).detach()
    vq_loss = F.mse_loss(q, e.detach()) + beta * F.mse_loss(e, q.detach())
    loss = (ste * torch.tensor(w, dtype=torch.float64)).sum() + (vq_loss if with_vq_loss else 0.0)
    loss.backward()
    return idx.numpy(), q.detach().numpy(), float(vq_loss.detach()), e.grad.numpy(), (c.grad if c.grad is not None else torch.zeros_like(c)).numpy()


@pytest.mark.parametrize("B,Bw,Le,K,beta", [(1, 1, 1, 2, 0.25), (3, 7, 5, 17, 0.25), (2, 64, 25, 64, 1.5), (3, 65, 3, 5, 0.0)])
def test_forward_and_gradients_equal_autograd(B, Bw, Le, K, beta):
    rng = np.random.default_rng(B * 1000 + Bw)
    enc, cb, w = rng.standard_normal((B, Bw, Le)), rng.standard_normal((K, Bw)), rng.standard_normal((B, Bw, Le))
    idx, q, vq_loss, d_enc, d_cb = _autograd(enc, cb, w, beta)
    f = vq_ref.forward(enc, cb, beta)
    assert np.array_equal(f["idx"], idx) and np.array_equal(f["q"], q)
    assert abs(f["vq_loss"] - vq_loss) <= 1e-13 * max(1.0, abs(vq_loss))
    assert f["counts"].sum() == B * Le and np.array_equal(f["counts"], np.bincount(idx.reshape(-1), minlength=K))
    g_enc, g_cb = vq_ref.backward(enc, cb, f["idx"], w, beta)
    np.testing.assert_allclose(g_enc, d_enc, rtol=0, atol=1e-13 * max(1.0, np.abs(d_enc).max()))
    np.testing.assert_allclose(g_cb, d_cb, rtol=0, atol=1e-13 * max(1.0, np.abs(d_cb).max()))
    # without the vq_loss term: the straight-through path alone - the codebook gets nothing, the encoder d_q unchanged
    _, _, _, d_enc0, d_cb0 = _autograd(enc, cb, w, beta, with_vq_loss=False)
    assert (d_cb0 == 0).all() and np.array_equal(d_enc0, w)
    # an upstream scalar g on vq_loss scales both loss gradients, not d_q
    g2_enc, g2_cb = vq_ref.backward(enc, cb, f["idx"], w, beta, g=3.0)
    np.testing.assert_allclose(g2_enc - w, 3.0 * (g_enc - w), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(g2_cb, 3.0 * g_cb, rtol=1e-12, atol=0)


def test_ties_go_to_the_smallest_index():
    rng = np.random.default_rng(3)
    enc = rng.integers(-16, 17, size=(2, 5, 4)) / 8.0
    cb = rng.integers(-16, 17, size=(9, 5)) / 8.0
    cb[7] = cb[2]                                    # duplicate rows: exact ties
    cb[5] = cb[2]
    cb[0] = enc[0, :, 1]                             # and exact hits at distance 0, doubled behind
    cb[8] = cb[0]
    f = vq_ref.forward(enc, cb)
    assert f["idx"][0, 1] == 0 and not np.isin(f["idx"], (5, 7, 8)).any()
    assert (f["counts"][[5, 7, 8]] == 0).all()
    # every frame: no code in front of the chosen one is as near
    d = f["dist"]
    for b in range(2):
        for l in range(4):
            k = f["idx"][b, l]
            assert (d[b, l, :k] > d[b, l, k]).all() and (d[b, l, k:] >= d[b, l, k]).all()
    assert vq_ref.margins(d)[0, 1] == 0.0            # (a doubled code: no margin)


def test_unused_codes_get_exactly_zero():
    rng = np.random.default_rng(5)
    enc, cb = rng.standard_normal((2, 6, 3)), rng.standard_normal((40, 6))
    f = vq_ref.forward(enc, cb)
    unused = f["counts"] == 0
    assert unused.sum() >= 34
    _, d_cb = vq_ref.backward(enc, cb, f["idx"], rng.standard_normal(enc.shape), 0.25)
    assert (d_cb[unused] == 0).all() and (np.abs(d_cb[~unused]).max(1) > 0).all()


def test_perplexity():
    assert vq_ref.perplexity([4, 0, 0, 0]) == 1.0
    assert abs(vq_ref.perplexity([5, 5, 5, 5, 0]) - 4.0) < 1e-12
    assert abs(vq_ref.perplexity([3, 1]) - np.exp(-(0.75 * np.log(0.75) + 0.25 * np.log(0.25)))) < 1e-12
    f = vq_ref.forward(np.zeros((1, 2, 6)), np.array([[0.0, 0.0], [1.0, 1.0]]))
    assert f["perplexity"] == 1.0 and f["mse"] == 0.0


def test_grid_distances_are_exact_in_float32_in_any_order():
    """What tests/test_gpu_vq_kernels.py builds on: inputs that are multiples of 1/8 in [-2, 2] give squared differences that are
    multiples of 1/64 up to 16, and any partial sum of 512 of them (<= 8192 = 2^13, in units of 2^-6: 19 bits) is exact in fp32."""
    rng = np.random.default_rng(7)
    e = (rng.integers(-16, 17, size=512) / 8.0).astype(np.float32)
    c = (rng.integers(-16, 17, size=(1024, 512)) / 8.0).astype(np.float32)
    d32 = (e[None] - c) ** 2
    assert d32.dtype == np.float32
    fwd, rev = np.cumsum(d32, axis=1, dtype=np.float32)[:, -1], np.cumsum(d32[:, ::-1], axis=1, dtype=np.float32)[:, -1]
    ref = ((e.astype(np.float64)[None] - c.astype(np.float64)) ** 2).sum(1)
    assert np.array_equal(fwd.astype(np.float64), ref) and np.array_equal(rev.astype(np.float64), ref)
    assert 512 * 16 * 64 < 2 ** 24
