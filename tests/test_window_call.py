"""CPU checks of the Python side of position-windowed sampling: fast_generate._decode_call picks wn_win_decode_batch only when windows
are given and nests the argument lists, ``windows=`` / ``window_pos=`` are validated with ValueError before any device work, and
ae_generate.sample_code_stream checks its arguments.  Nothing is launched."""
import ctypes

import pytest
import torch

from tests.test_decode_call import NO_TABLES, P, TABLES, _call


def _call_win(fg, smp, cond, win):
    return fg._decode_call((2, 4, 64, 64, 256, 256), P, P, P, (P, None, P, 4096, None, P, None, P, None),
                           (P, P, P, P, None, P, None), 0, 12, 1, P, 3, 960, smp, (P, 0, 8, 16, 24, 32, 40), cond, win)


@pytest.mark.parametrize("sampling", ["plain", "filtered", "table"])
@pytest.mark.parametrize("cond", [None, NO_TABLES, TABLES], ids=["unconditioned", "cond-origin-no-tables", "cond-origin-tables"])
def test_decode_call_with_windows_picks_the_new_entry_and_begins_with_the_samp_tuple(sampling, cond):
    from music_amd import _lib
    from music_amd import fast_generate as fg
    kw = {"plain": dict(temperature=0.8, top_k=None), "filtered": dict(temperature=0.8, top_k=40),
          "table": dict(temperature=[0.5, 0.8, 1.0], top_k=[0, 40, 5])}[sampling]
    smp = fg._Sampling(3, kw["temperature"], kw["top_k"], None, 7, None, torch.device("cpu"))
    win = fg._Windows(fg.stage_windows(2, 128), 5, 256)
    name, args = _call_win(fg, smp, cond, win.tail(1))
    assert name == "wn_win_decode_batch" and len(args) + 1 == len(_lib.SIGNATURES[name])
    # without windows: today's choice and tuple, whether the argument is left out or None
    old = _call(fg, smp, cond)
    assert _call_win(fg, smp, cond, None) == old
    assert old[0] == ("wn_decode_batch_samp" if sampling != "plain" else "wn_decode_batch_fw" if cond is None else "wn_decode_batch_cond")
    # the tuple begins with the samp tuple of the same launch (a plain launch's: table NULL, filters off)
    filt = smp if sampling != "plain" else fg._Sampling(3, 0.8, 3, None, 7, None, torch.device("cpu"))
    samp = _call(fg, filt, cond)
    assert samp[0] == "wn_decode_batch_samp"
    n_head = len(samp[1]) - 3
    assert args[:n_head] == samp[1][:n_head]
    assert args[n_head:n_head + 3] == (samp[1][n_head:] if sampling != "plain" else (None, 0, 1.0))
    tail = args[n_head + 3:]
    assert len(tail) == 3 and tail[1:] == (2, 6)
    assert list(ctypes.cast(tail[0], ctypes.POINTER(ctypes.c_int32))[:4]) == [0, 128, 128, 256]
    for v, t in zip(args, _lib.SIGNATURES[name]):
        t.from_param(v)


def test_stage_windows_and_the_window_table():
    from music_amd import fast_generate as fg
    assert fg.stage_windows(3, 32) == [(0, 32), (32, 64), (64, 96)]
    assert fg.stage_windows(1, 1024) == [(0, 1024)]
    w = fg._Windows([(0, 4), (4, 6), (1, 3)], 7, 8)
    assert w.at(7) == (4, 6) and w.at(9) == (0, 4)
    assert w.tail()[1:] == (3, 7) and w.tail(1)[1:] == (3, 8)
    assert fg._windows_of(None, 0, 8) is None


@pytest.mark.parametrize("bad", [[], [(0, 1)] * 17, [(0, 9)], [(-1, 4)], [(3, 3)], [(5, 2)], [(0, 4, 5)], 5, [(0, 4), 3]])
def test_windows_are_validated_in_python(bad):
    from music_amd import fast_generate as fg
    with pytest.raises(ValueError, match="window"):
        fg._windows_of(bad, 0, 8)


def test_window_pos_is_validated_in_python():
    from music_amd import fast_generate as fg
    with pytest.raises(ValueError, match="window_pos"):
        fg._windows_of([(0, 4)], -1, 8)
    with pytest.raises(ValueError, match="window_pos"):
        fg._windows_of(None, 3, 8)


class _Net:
    quantization_channels = 8
    receptive_field = 4


def test_windows_need_the_corrected_recurrence():
    """generate_codes / generate_codes_batch refuse windows on the as-written recurrence - and a bad table - before the init forward"""
    from music_amd import fast_generate as fg
    piece = torch.zeros(1, 8, 4)
    for fn in (fg.generate_codes, fg.generate_codes_batch):
        with pytest.raises(ValueError, match="corrected recurrence.*correct_queue=True"):
            fn(_Net(), piece, 6, windows=[(0, 4), (4, 8)])
        with pytest.raises(ValueError, match="0 <= lo < hi <= Q"):
            fn(_Net(), piece, 6, correct_queue=True, windows=[(0, 9)])
        with pytest.raises(ValueError, match="window_pos"):
            fn(_Net(), piece, 6, correct_queue=True, windows=[(0, 8)], window_pos=-2)


def test_first_code_is_the_first_index_argmax_inside_its_window():
    from music_amd import fast_generate as fg
    probs = torch.tensor([[0.5, 0.1, 0.2, 0.2, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.3, 0.7]])
    win = fg._Windows([(0, 2), (2, 4), (4, 6)], 4, 6)          # position 4: pair 1
    assert fg._first_in_window(probs, win).tolist() == [2, 2]
    assert fg._first_in_window(probs, fg._Windows([(0, 2), (2, 4), (4, 6)], 5, 6)).tolist() == [4, 5]


class _Prior(torch.nn.Module):
    quantization_channels = 32
    receptive_field = 6

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_sample_code_stream_checks_its_arguments():
    from music_amd import ae_generate as ag
    prior = _Prior()
    ok = torch.zeros(2, 6, dtype=torch.int64)
    for match, kw in (("alphabet", dict(stages=3, K=16)),
                      ("frame boundary", dict(start_tokens=torch.zeros(2, 7, dtype=torch.int64))),
                      ("frame boundary", dict(start_pos=1)),
                      ("frame boundary", dict(start_pos=-2)),
                      ("start_tokens", dict(start_tokens=torch.zeros(2, 4, dtype=torch.int64))),
                      ("start_tokens", dict(start_tokens=torch.zeros(6, dtype=torch.int64))),
                      ("start_tokens", dict(start_tokens=torch.zeros(2, 6))),
                      ("start_tokens", dict(start_tokens=torch.full((2, 6), 32))),
                      ("start_tokens", dict(start_tokens=torch.full((2, 6), -1))),
                      (">= 1", dict(frames=0)), (">= 1", dict(stages=0))):
        a = dict(prior=prior, stages=2, K=16, frames=3, start_tokens=ok, start_pos=0)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            ag.sample_code_stream(**a)
