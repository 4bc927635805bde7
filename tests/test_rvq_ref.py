"""tests/rvq_ref.py against torch float64 autograd (the straight-through estimator e + (q - e).detach(), the residual passed between
the stages detached, every stage's codebook and commitment term), against tests/vq_ref.py at S = 1 and against tests/vq_ema_ref.py
stage by stage.  No device."""
import numpy as np
import pytest
import torch

from tests import rvq_ref, vq_ema_ref, vq_ref

BETA = 0.25


def draw(S, K, Bw, B, Le, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, Bw, Le)), rng.standard_normal((S * K, Bw)) * 0.7, rng.standard_normal((B, Bw, Le))


@pytest.mark.parametrize("S,g", [(1, 1.0), (2, 1.0), (3, 0.5), (8, 2.0)])
def test_gradients_equal_float64_autograd(S, g):
    K, Bw, B, Le = 9, 5, 2, 7
    enc, cb, d_q = draw(S, K, Bw, B, Le, seed=S)
    f = rvq_ref.forward(enc, cb, S, BETA)
    e = torch.tensor(enc, requires_grad=True)
    c = torch.tensor(cb, requires_grad=True)
    r, q, loss = e, 0.0, 0.0
    for s in range(S):
        rows = c[s * K:(s + 1) * K]
        idx = torch.cdist(r.detach().permute(0, 2, 1), rows.detach()).argmin(-1)
        assert np.array_equal(idx.numpy(), f["idx"][s])
        q_s = rows[idx].permute(0, 2, 1)
        # codebook term + beta x commitment term of this stage on ITS input, which reaches e through the identity r_s = e - sg(...)
        loss = loss + ((q_s - r.detach()) ** 2).mean() + BETA * ((q_s.detach() - r) ** 2).mean()
        q = q + q_s
        r = r - q_s.detach()
    st = e + (q - e).detach()
    assert np.allclose(q.detach().numpy(), f["q"], rtol=0, atol=1e-14)
    assert abs(float(loss.detach()) - f["vq_loss"]) <= 1e-13 * f["vq_loss"]
    ((st * torch.tensor(d_q)).sum() + g * loss).backward()
    d_enc, d_cb = rvq_ref.backward(enc, cb, S, f["idx"], d_q, BETA, g)
    assert np.allclose(d_enc, e.grad.numpy(), rtol=0, atol=1e-13)
    assert np.allclose(d_cb, c.grad.numpy(), rtol=0, atol=1e-13)
    unused = (f["counts"] == 0).reshape(-1)
    assert (d_cb[unused] == 0).all()


def test_commitment_gradient_reaches_e_from_every_stage():
    """r_s = e - sg(q_0 + .. + q_s-1): every stage's commitment term pulls on e, so d_e sums the stages' residuals."""
    S, K = 3, 6
    enc, cb, _ = draw(S, K, 4, 1, 5, seed=5)
    f = rvq_ref.forward(enc, cb, S, BETA)
    d_enc, _ = rvq_ref.backward(enc, cb, S, f["idx"], None, BETA)
    assert np.allclose(d_enc, BETA * 2.0 / enc.size * f["res"].sum(0), rtol=0, atol=1e-15)
    d_dev, _ = rvq_ref.backward(enc, cb, S, f["idx"], None, BETA, residuals=f["res"])
    assert np.array_equal(d_dev, d_enc)


def test_one_stage_is_the_plain_quantiser():
    enc, cb, d_q = draw(1, 17, 7, 3, 4, seed=2)
    f, g = rvq_ref.forward(enc, cb, 1, BETA), vq_ref.forward(enc, cb, BETA)
    assert np.array_equal(f["idx"][0], g["idx"]) and np.array_equal(f["q"], g["q"]) and f["mse"][0] == g["mse"]
    assert f["vq_loss"] == g["vq_loss"] and np.array_equal(f["counts"][0], g["counts"])
    a, b = rvq_ref.backward(enc, cb, 1, f["idx"], d_q, BETA, 1.5), vq_ref.backward(enc, cb, g["idx"], d_q, BETA, 1.5)
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-15) and np.array_equal(a[1], b[1])
    assert np.array_equal(rvq_ref.lookup(cb, 1, f["idx"]), g["q"])
    assert rvq_ref.forward(enc, cb, 1, BETA, ema=True)["vq_loss"] == BETA * g["mse"]


def test_the_chain_and_its_prefix_lookup():
    S, K = 4, 8
    enc, cb, _ = draw(S, K, 6, 2, 5, seed=3)
    f = rvq_ref.forward(enc, cb, S)
    assert np.array_equal(f["r"][0], enc)
    for s in range(S):
        assert np.array_equal(f["res"][s], f["r"][s] - f["stage_q"][s])
        assert np.array_equal(rvq_ref.lookup(cb, S, f["idx"], s + 1), sum(f["stage_q"][1:s + 1], f["stage_q"][0]))
        assert f["mse"][s] == (f["res"][s] ** 2).sum() / enc.size
    assert np.array_equal(rvq_ref.lookup(cb, S, f["idx"]), f["q"])
    assert (np.diff(f["mse"]) <= 0).all()                       # the zero row is not in the codebooks, but these draws do shrink


def test_ema_per_stage_equals_the_plain_reference_on_that_stages_residuals():
    S, K, Bw = 3, 8, 5
    enc, cb, _ = draw(S, K, Bw, 4, 9, seed=4)
    f = rvq_ref.forward(enc, cb, S)
    stat = rvq_ref.stats(enc, cb, S, f["idx"])
    state = rvq_ref.initial_state(cb, S)
    assert stat.shape == state.shape == (S, K * (Bw + 1))
    ups = rvq_ref.update(stat, state, S, K, 0.9, 1e-5, 0.95)
    assert sum(u["restarted"] for u in ups) > 0
    for s in range(S):
        one = vq_ema_ref.stats(f["r"][s], f["idx"][s], K)
        assert np.array_equal(stat[s], one)
        assert np.array_equal(state[s], vq_ema_ref.initial_state(cb[s * K:(s + 1) * K]))
        ref = vq_ema_ref.update(one, state[s], K, 0.9, 1e-5, 0.95)
        for k in ("state", "cb", "donor"):
            assert np.array_equal(ups[s][k], ref[k], equal_nan=True)
        assert (ups[s]["restarted"], ups[s]["left"]) == (ref["restarted"], ref["left"])
