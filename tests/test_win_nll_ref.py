"""tests/win_nll_ref.py - the float64 restatement of the windowed objective's rule that the GPU tests measure the kernels by - against
torch's own cross_entropy and softmax in float64 on the SLICED window of each column, and its edge rules.  No device is touched."""
import math

import torch
import torch.nn.functional as F

from tests import win_nll_ref as ref

TABLE = [(0, 10), (10, 11), (5, 100)]             # unequal, overlapping, one of width 1


def _inputs(B, q, W, windows, pos, seed):
    """logits and targets drawn inside each column's window"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, q, W, generator=g, dtype=torch.float64)
    lo, hi, _ = ref.column_windows(windows, B, W, q, [max(0, p) for p in pos])
    t = lo + (torch.rand(B, W, generator=g, dtype=torch.float64) * (hi - lo)).long().clamp(max=q - 1)
    return x, torch.minimum(t, hi - 1)


def test_every_column_is_torch_on_its_sliced_window():
    B, q, W, pos = 3, 100, 17, [0, 1, 7]
    x, t = _inputs(B, q, W, TABLE, pos, 1)
    x = x.clone().requires_grad_(True)
    inv_n = 1.0 / (B * W)
    r = ref.reference(x.detach(), t, inv_n, TABLE, pos)
    total = 0.0
    for b in range(B):
        for c in range(W):
            lo, hi = TABLE[(pos[b] + c) % len(TABLE)]
            i = b * W + c
            assert (int(r["lo"][i]), int(r["hi"][i])) == (lo, hi)
            z = x[b, lo:hi, c]
            y = int(t[b, c]) - lo
            nll = F.cross_entropy(z[None], torch.tensor([y]))
            total = total + nll
            assert abs(float(nll.detach()) - float(r["row_nll"][i])) < 1e-12
            p = F.softmax(z.detach(), dim=0)
            assert (r["probs"][i, lo:hi] - p).abs().max() < 1e-14
            assert (r["probs"][i, :lo] == 0).all() and (r["probs"][i, hi:] == 0).all()
            assert int(r["arg"][i]) == lo + int(z.argmax()) and int(r["row_hit"][i]) == int(int(z.argmax()) == y)
    loss = total * inv_n
    g, = torch.autograd.grad(loss, x)
    assert abs(float(loss.detach()) - r["loss"]) < 1e-12
    assert (g - r["dx"]).abs().max() < 1e-15
    assert abs(float(ref.windowed_nll(x.detach(), t, TABLE, pos)) - r["loss"]) < 1e-12
    # outside the windows: the bits of +0.0, in dx and in probs
    k = torch.arange(q).view(1, q, 1)
    outside = ~((k >= r["lo"].view(B, 1, W)) & (k < r["hi"].view(B, 1, W)))
    assert (r["dx"][outside].view(torch.int64) == 0).all()
    assert (r["probs"].view(B, W, q).permute(0, 2, 1)[outside].contiguous().view(torch.int64) == 0).all()


def test_values_outside_the_window_influence_nothing():
    B, q, W, pos = 2, 100, 9, [2, 0]
    x, t = _inputs(B, q, W, TABLE, pos, 2)
    base = ref.reference(x, t, 0.25, TABLE, pos)
    k = torch.arange(q).view(1, q, 1)
    outside = ~((k >= base["lo"].view(B, 1, W)) & (k < base["hi"].view(B, 1, W)))
    for v in (float("nan"), float("inf"), 1e30):
        r = ref.reference(torch.where(outside, torch.tensor(v, dtype=torch.float64), x), t, 0.25, TABLE, pos)
        for key in ("probs", "dx", "row_nll", "row_hit", "arg"):
            assert torch.equal(r[key], base[key]), (v, key)
        assert r["loss"] == base["loss"]


def test_a_width_1_window_has_nll_0_and_gradient_0():
    x, _ = _inputs(1, 100, 6, TABLE, [0], 3)
    t = torch.tensor([[0, 10, 5, 0, 10, 5]])
    r = ref.reference(x, t, 1.0, TABLE)
    for c in (1, 4):
        assert float(r["row_nll"][c]) == 0.0 and (r["dx"][0, :, c] == 0).all() and int(r["row_hit"][c]) == 1
        assert float(r["probs"][c, 10]) == 1.0 and float(r["probs"][c].sum()) == 1.0


def test_zero_logits_cost_the_log_of_the_window_width():
    B, q, W = 2, 100, 7
    _, t = _inputs(B, q, W, TABLE, [0, 2], 4)
    r = ref.reference(torch.zeros(B, q, W), t, 1.0, TABLE, [0, 2])
    assert ((r["row_nll"] - (r["hi"] - r["lo"]).double().log()).abs() < 1e-15).all()


def test_a_target_outside_its_window_poisons_its_column_only():
    B, q, W, pos = 2, 100, 8, [0, 1]
    x, t = _inputs(B, q, W, TABLE, pos, 5)
    good = ref.reference(x, t, 0.5, TABLE, pos)
    t2 = t.clone()
    t2[0, 3] = 50               # column 3 of clip 0 is at position 3: window (0, 10); 50 lies in [0, q) and outside
    t2[1, 0] = 4                # clip 1 starts at position 1: window (10, 11)
    t2[1, 5] = -1
    r = ref.reference(x, t2, 0.5, TABLE, pos)
    bad = torch.zeros(B, W, dtype=torch.bool)
    bad[0, 3] = bad[1, 0] = bad[1, 5] = True
    assert torch.equal(r["bad"].view(B, W), bad) and math.isnan(r["loss"])
    assert r["row_nll"].view(B, W)[bad].isnan().all() and not r["row_hit"].view(B, W)[bad].any()
    assert r["dx"].permute(0, 2, 1)[bad].isnan().all()
    keep = ~bad
    assert torch.equal(r["row_nll"].view(B, W)[keep], good["row_nll"].view(B, W)[keep])
    assert torch.equal(r["dx"].permute(0, 2, 1)[keep], good["dx"].permute(0, 2, 1)[keep])
    assert torch.equal(r["probs"], good["probs"])


def test_a_negative_position_poisons_its_clip_and_is_never_an_index():
    B, q, W = 3, 100, 5
    x, t = _inputs(B, q, W, TABLE, [4, 0, 2], 6)
    good = ref.reference(x, t, 1.0, TABLE, [4, 0, 2])
    r = ref.reference(x, t, 1.0, TABLE, [4, -(1 << 40), 2])
    assert torch.equal(r["bad"].view(B, W), torch.tensor([False, True, False]).view(B, 1).expand(B, W))
    assert math.isnan(r["loss"]) and r["row_nll"].view(B, W)[1].isnan().all() and r["dx"][1].isnan().all() and not r["row_hit"].view(B, W)[1].any()
    for b in (0, 2):
        assert torch.equal(r["row_nll"].view(B, W)[b], good["row_nll"].view(B, W)[b]) and torch.equal(r["dx"][b], good["dx"][b])


def test_period_0_and_whole_alphabet_tables_are_the_plain_rule():
    B, q, W = 2, 37, 11
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, q, W, generator=g, dtype=torch.float64)
    t = torch.randint(0, q, (B, W), generator=g)
    z = x.permute(0, 2, 1).reshape(-1, q).clone().requires_grad_(True)
    rows = F.cross_entropy(z, t.reshape(-1), reduction="none")
    loss = rows.sum() / (B * W)
    gz, = torch.autograd.grad(loss, z)
    for windows, pos in ((None, None), ([], None), ([(0, q)] * 3, [5, 9])):
        r = ref.reference(x, t, 1.0 / (B * W), windows, pos)
        assert (r["row_nll"] - rows.detach()).abs().max() < 1e-13 and abs(r["loss"] - float(loss.detach())) < 1e-13
        assert (r["probs"] - F.softmax(z.detach(), dim=1)).abs().max() < 1e-15
        assert (r["dx"] - gz.view(B, W, q).permute(0, 2, 1)).abs().max() < 1e-15
        assert torch.equal(r["arg"], z.detach().argmax(1)) and not r["bad"].any()


def test_positions_add_and_wrap():
    B, q, W = 2, 100, 6
    lo1, hi1, _ = ref.column_windows(TABLE, B, W, q, [1, 2], pos0=(1 << 40) + 3)
    lo2, hi2, _ = ref.column_windows(TABLE, B, W, q, [(1 << 40) + 4, (1 << 40) + 5])
    assert torch.equal(lo1, lo2) and torch.equal(hi1, hi2)
    assert [int(v) for v in lo1[0]] == [TABLE[((1 << 40) + 4 + c) % 3][0] for c in range(W)]
