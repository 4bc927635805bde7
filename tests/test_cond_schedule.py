"""ae_generate.cond_schedule against the oracle's ``condition`` (model1.py:227-247 restated): a "table" whose column e holds
the number e is conditioned onto a zero tensor of every stage's length, so the oracle's output IS the frame index it used
at every column; the schedule's (shift, q, Le) must name the same frame for every column and place the W output positions
at the tail of every stage.  Pure host arithmetic: no device."""
import pytest
import torch

from oracle import wavenet_oracle as wo


def _stage_lengths(k, dil, T):
    """L_{i+1} of every decoder block of the forward (causal layer, then block i consumes (k-1) d_i columns), then W."""
    L, out = T - (k - 1), []
    for d in dil:
        L -= (k - 1) * d
        out.append(L)
    return out + [out[-1]]


def _check(k, dil, T, pool):
    from music_amd import ae_generate as ag
    rf = wo.receptive_field(k, dil)
    W = T - rf + 1
    Le = W // pool
    assert Le >= 1
    lengths = _stage_lengths(k, dil, T)
    assert lengths[-1] == W
    sched = ag.cond_schedule((k, dil), W, Le)
    assert len(sched) == len(dil) + 1
    frames = torch.arange(Le, dtype=torch.float64).view(1, 1, Le)
    stretch = tile = 0
    for L, (shift, q, le) in zip(lengths, sched):
        used = wo.condition(torch.zeros(1, 1, L, dtype=torch.float64), frames)[0, 0].to(torch.int64).tolist()
        assert le == Le and shift == L - W and q >= 0
        assert (q > 0) == (L % Le == 0)
        mine = [(c // q) if q > 0 else (c % Le) for c in range(L)]
        assert mine == used
        # the W output positions are the stage's last W columns
        assert [mine[j + shift] for j in range(W)] == used[-W:]
        stretch += q > 0
        tile += q == 0

    class Geometry:
        filter_width, dilations = k, dil
    assert ag.cond_schedule(Geometry(), W, Le) == sched
    return Le, stretch, tile


def test_one_frame():
    Le, stretch, tile = _check(2, [1, 2, 4, 8, 1, 2], 18 + 40 + 13, 40)
    assert Le == 1 and tile == 0 and stretch == 7          # every length divides by one: all stretch


def test_both_branches_in_one_model():
    # W = 22, Le = 3: stage lengths 45 43 39 31 28 23 22: three divide by 3 (stretch), four do not (tile)
    Le, stretch, tile = _check(2, [1, 2, 4, 8, 3, 5], 46, 6)
    assert Le == 3 and stretch == 3 and tile == 4


def test_filter_width_3():
    Le, stretch, tile = _check(3, [1, 2, 4, 1, 2], wo.receptive_field(3, [1, 2, 4, 1, 2]) + 41, 7)
    assert Le == 6 and stretch >= 1 and tile >= 1


def test_config_4_geometry():
    dil = [2 ** (i % 10) for i in range(30)]
    Le, stretch, tile = _check(2, dil, 16000, 512)
    assert Le == 25 and stretch + tile == 31


def test_bad_arguments():
    from music_amd import ae_generate as ag
    for bad in ((2, [1, 2], 0, 1), (2, [1, 2], 5, 0), (0, [1, 2], 5, 1)):
        with pytest.raises(ValueError):
            ag.cond_schedule((bad[0], bad[1]), bad[2], bad[3])
