"""tests/wnll_ref.py (the float64 restatement of wn_wstep_nll's rule) held to torch.nn.functional.cross_entropy(ignore_index=,
label_smoothing=, reduction="mean") for the unweighted, unwindowed case, within 1e-12, and to a hand-written weighted sum for weights
and windows.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import win_nll_ref, wnll_ref as ref

TABLE = [(0, 10), (10, 11), (5, 40)]


def _case(B, q, W, seed, ignored=0.3):
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(B, q, W, generator=g, dtype=torch.float64)
    t = torch.randint(0, q, (B, W), generator=g)
    t[torch.rand(B, W, generator=g) < ignored] = -1
    return x, t


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("ignored", [0.0, 0.3])
def test_unweighted_unwindowed_is_torch_cross_entropy(eps, ignored):
    B, q, W = 3, 37, 29
    x, t = _case(B, q, W, 1, ignored)
    xr = x.clone().requires_grad_(True)
    want = F.cross_entropy(xr, t, ignore_index=-1, label_smoothing=eps, reduction="mean")      # (B, C, d1): the class axis is 1
    want.backward()
    f = ref.reference(x, t, ignore_index=-1, smoothing=eps)
    assert abs(f["loss"] - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert float((f["dx"] - xr.grad).abs().max()) <= 1e-12
    assert f["den"][0] == float((t != -1).sum()) and torch.equal(f["skip"], (t == -1).reshape(-1))
    assert (f["dx"][:, :, 0][(t == -1)[:, 0]] == 0).all() and not f["bad"].any()
    xa = x.clone().requires_grad_(True)
    loss = ref.weighted_nll(xa, t, ignore_index=-1, smoothing=eps)
    loss.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach()))) and float((xa.grad - xr.grad).abs().max()) <= 1e-12


def test_no_mask_no_weights_no_smoothing_is_the_windowed_reference():
    B, q, W, pos = 2, 40, 31, [1, 5]
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, q, W, generator=g)
    lo, hi, _ = win_nll_ref.column_windows(TABLE, B, W, q, pos)
    t = (lo + (torch.rand(B, W, generator=g, dtype=torch.float64) * (hi - lo)).long()).clamp(max=q - 1)
    t = torch.minimum(t, hi - 1)
    a = win_nll_ref.reference(x, t, 1.0 / (B * W), TABLE, pos)
    b = ref.reference(x, t, TABLE, pos)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 and float((a["dx"] - b["dx"]).abs().max()) <= 1e-15
    assert torch.equal(a["row_hit"], b["row_hit"]) and float((a["row_nll"] - b["row_nll"]).abs().max()) == 0.0
    assert b["den"] == [float(B * W), 1.0 / (B * W)]


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_weights_and_windows_against_a_hand_written_sum(eps):
    B, q, W, pos = 2, 40, 17, [0, 2]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, q, W, generator=g, dtype=torch.float64)
    lo, hi, _ = win_nll_ref.column_windows(TABLE, B, W, q, pos)
    t = torch.minimum(lo + (torch.rand(B, W, generator=g, dtype=torch.float64) * (hi - lo)).long(), hi - 1)
    w = (2.0 * torch.rand(B, W, generator=g)).float()
    w[0, 3] = w[1, 0] = 0.0
    t[0, 5] = -1
    t[0, 3] = 12345                                                      # (garbage under weight 0: never examined)
    num = den = 0.0
    grad = torch.zeros(B, q, W, dtype=torch.float64)
    for b in range(B):
        for c in range(W):
            wc = 0.0 if int(t[b, c]) == -1 else float(w[b, c])
            if wc == 0.0:
                continue
            a, z = int(lo[b, c]), int(hi[b, c])
            xs = [float(v) for v in x[b, a:z, c]]
            mx = max(xs)
            S = sum(math.exp(v - mx) for v in xs)
            num += wc * (math.log(S) + mx - (1 - eps) * float(x[b, int(t[b, c]), c]) - eps / (z - a) * sum(xs))
            den += wc
            for j, v in enumerate(xs):
                grad[b, a + j, c] = wc * (math.exp(v - mx) / S - (1 - eps) * (a + j == int(t[b, c])) - eps / (z - a))
    f = ref.reference(x, t, TABLE, pos, weight=w, ignore_index=-1, smoothing=eps)
    assert abs(f["loss"] - num / den) <= 1e-12 and abs(f["den"][0] - den) <= 1e-12 and abs(f["den"][1] * den - 1) <= 1e-15
    assert float((f["dx"] - grad / den).abs().max()) <= 1e-14
    assert int(f["skip"].sum()) == 3 and not f["bad"].any()
    assert (f["row_nll"][f["skip"]] == 0).all() and (f["row_hit"][f["skip"]] == 0).all()
    xa = x.clone().requires_grad_(True)
    loss = ref.weighted_nll(xa, t, TABLE, pos, weight=w, ignore_index=-1, smoothing=eps)
    loss.backward()
    assert abs(float(loss.detach()) - num / den) <= 1e-12 and float((xa.grad - grad / den).abs().max()) <= 1e-14


def test_skipped_columns_poison_nothing_and_bad_ones_only_themselves():
    B, q, W = 2, 20, 9
    x, t = _case(B, q, W, 4, 0.0)
    w = torch.ones(B, W)
    w[0, 2] = 0.0
    t[1, 4] = -1
    base = ref.reference(x, t, weight=w, ignore_index=-1, smoothing=0.1)
    x2, t2 = x.clone(), t.clone()
    x2[0, :, 2], x2[1, :, 4], t2[0, 2] = math.nan, math.inf, q + 5
    f = ref.reference(x2, t2, weight=w, ignore_index=-1, smoothing=0.1)
    assert f["loss"] == base["loss"] and torch.equal(f["dx"], base["dx"]) and torch.equal(f["row_nll"], base["row_nll"])
    t2[1, 1] = q                                                         # a counted column with a target outside [0, q)
    f = ref.reference(x2, t2, weight=w, ignore_index=-1)
    assert math.isnan(f["loss"]) and int(f["bad"].sum()) == 1 and f["dx"][1, :, 1].isnan().all()
    assert int(f["dx"].isnan().any(1).sum()) == 1 and f["den"][0] == B * W - 2


def test_nothing_counted_and_poisoned_weights():
    B, q, W = 2, 8, 5
    x, t = _case(B, q, W, 5, 0.0)
    f = ref.reference(x, torch.full((B, W), -1), ignore_index=-1, smoothing=0.2)
    assert f["loss"] == 0.0 and f["den"] == [0.0, 0.0] and (f["dx"] == 0).all() and not torch.signbit(f["dx"]).any()
    assert float(ref.weighted_nll(x, torch.full((B, W), -1), ignore_index=-1)) == 0.0
    for v in (-1.0, math.inf, math.nan):
        w = torch.ones(B, W)
        w[1, 1] = v
        f = ref.reference(x, t, weight=w)
        assert math.isnan(f["loss"]) and all(math.isnan(d) for d in f["den"]) and f["dx"].isnan().all()
        t2 = t.clone()
        t2[1, 1] = -1                                                    # under an ignored target the weight is not looked at
        assert math.isfinite(ref.reference(x, t2, weight=w, ignore_index=-1)["loss"])


def test_smoothing_0_never_forms_the_sum_of_the_logits():
    x, t = _case(1, 6, 3, 6, 0.0)
    x[0, 1, :] = -math.inf
    t[:] = 2
    assert math.isfinite(ref.reference(x, t)["loss"]) and not ref.reference(x, t)["dx"].isnan().any()
    assert ref.reference(x, t, smoothing=0.1)["loss"] == math.inf
