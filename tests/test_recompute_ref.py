"""tests/recompute_ref.py (the float64 formulas the GPU tests of wn_resblock_bwd compare with) against float64 torch autograd of
the gated block - _res_ref of tests/test_gpu_kernels.py plus bias and table terms - so that a wrong reference cannot pass a
wrong kernel.  No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import recompute_ref
from tests.test_gpu_kernels import _res_ref


def _autograd(x, wf, wg, wd, d, t_lo, t_hi, z_lo, dy, dz, bias_f, bias_g, tab, g_row, idx):
    D = wf.shape[0]
    xs = torch.from_numpy(x[:, :, t_lo - d:t_hi]).double()
    twf, twg, twd = (torch.from_numpy(a).double() for a in (wf, wg, wd))
    if bias_f is None and tab is None:
        f, g, z, y = _res_ref(xs, twf.requires_grad_(True), twg.requires_grad_(True), twd, d)
        f0 = g0 = None
    else:
        # the same model with the pre-activations as leaves: f = conv + bias + table, z = tanh f * sigmoid g, y = Wd z + x
        f0 = F.conv1d(xs, twf, dilation=d) + torch.from_numpy(bias_f).double()[None, :D, None]
        g0 = F.conv1d(xs, twg, dilation=d) + torch.from_numpy(bias_g).double()[None, :D, None]
        t = torch.from_numpy(tab).double()
        f0 = f0 + t[:, :D][:, :, torch.from_numpy(idx).long()]
        g0 = g0 + t[:, g_row:g_row + D][:, :, torch.from_numpy(idx).long()]
        f, g = f0.detach().requires_grad_(True), g0.detach().requires_grad_(True)
        z = torch.tanh(f) * torch.sigmoid(g)
        y = F.conv1d(z, twd) + xs[:, :, d:]
    if f0 is None:
        f.retain_grad()
        g.retain_grad()
    loss = 0.0
    if dy is not None:
        loss = loss + (y * torch.from_numpy(dy[:, :, t_lo:t_hi]).double()).sum()
    gz = torch.zeros_like(z)
    if z_lo < t_hi:
        gz[:, :, z_lo - t_lo:] = torch.from_numpy(dz[:, :, z_lo:t_hi]).double()
    loss = loss + (z * gz).sum()
    loss.backward()
    return f.grad.numpy(), g.grad.numpy(), z.detach().numpy()


@pytest.mark.parametrize("B,R,D,d,t_lo,t_hi,z_lo,rule,le,with_dy", [
    (2, 5, 4, 3, 7, 30, 12, 1, 4, True),         # stretch: q = 23 // 4 = 5, the clamp takes the last 3 columns
    (1, 3, 6, 1, 2, 19, 2, 2, 5, True),          # tile: 17 columns over 5 buckets
    (2, 4, 4, 2, 5, 21, 21, 2, 3, True),         # no crop at all (z_lo = t_hi)
    (2, 4, 3, 2, 5, 21, 9, 1, 16, False),        # dy = None
])
def test_recompute_ref_equals_float64_autograd(B, R, D, d, t_lo, t_hi, z_lo, rule, le, with_dy):
    rng = np.random.default_rng(B * 100 + R)
    T = t_hi + 3
    x = rng.standard_normal((B, R, T)).astype(np.float32)
    wf, wg = (rng.standard_normal((D, R, 2)).astype(np.float32) * 0.5 for _ in range(2))
    wd = rng.standard_normal((R, D, 1)).astype(np.float32) * 0.5
    dy = rng.standard_normal((B, R, T)).astype(np.float32) if with_dy else None
    dz = rng.standard_normal((B, D, T)).astype(np.float32)
    bias_f, bias_g = (rng.standard_normal(D + 2).astype(np.float32) for _ in range(2))
    g_row = D + 3
    tab = rng.standard_normal((B, g_row + D, le + 2)).astype(np.float32)
    q = max(1, (t_hi - t_lo) // le)
    idx = recompute_ref.cond_index(t_lo, t_hi, rule, le, q)
    assert idx.min() == 0 and idx.max() == le - 1
    for bias, table in ((True, True), (False, False)):
        kw = dict(bias_f=bias_f, bias_g=bias_g, tab=tab, tab_g_row=g_row, cond_mode=rule, cond_le=le, cond_q=q) if table else {}
        df, dg, z = recompute_ref.recompute_bwd(x, wf, wg, wd, d, t_lo, t_hi, z_lo, dy=dy, dz=dz, **kw)
        rf, rg, rz = _autograd(x, wf, wg, wd, d, t_lo, t_hi, z_lo, dy, dz, bias_f if bias else None, bias_g if bias else None,
                               tab if table else None, g_row, idx)
        for got, ref in ((df, rf), (dg, rg), (z, rz)):
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_cond_index_rules():
    assert recompute_ref.cond_index(10, 21, 1, 3, 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2]
    assert recompute_ref.cond_index(10, 21, 2, 3, 0).tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
