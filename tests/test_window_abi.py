"""CPU checks of the position-windowed sampling entries wn_win_decode_batch and wn_win_sample_logits (include/wavenet_hip.h), in the
pattern of tests/test_decode_sample_abi.py: declared, exported and bound with the extended signatures, the ABI still 9, and every
refused argument comes back as -4 with the entry's name and the argument in wn_last_error before anything is launched - so no device
is needed.  Pointers below are never dereferenced (the window table is a host array and IS read)."""
import ctypes
import os
import re

import pytest

from tests.decode_args import P, decode_args
from tests.helpers import ROOT

_KEEP = []


def _lib():
    from music_amd import _lib
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION == 9
    return lib


def _table(pairs):
    if pairs is None:
        return None
    t = (ctypes.c_int32 * max(1, 2 * len(pairs)))(*[v for pr in pairs for v in pr])
    _KEEP.append(t)
    return ctypes.cast(t, ctypes.c_void_p)


def _args(win=((0, 128), (128, 256)), period=None, win_pos0=0, **over):
    """wn_decode_batch_samp's arguments without the stream, the three window arguments, the stream"""
    return decode_args("wn_decode_batch_samp", **{"temperature": 1.0, **over})[:-1] + [
        _table(win), (len(win) if win is not None else 0) if period is None else period, win_pos0, None]


def _refused(lib, what, **kw):
    rc = lib.wn_win_decode_batch(*_args(**kw))
    msg = lib.wn_last_error().decode()
    assert rc == -4 and what in msg, (kw, rc, msg)
    return msg


def _header():
    src = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _names(code, fn):
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % fn, code, flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in decl.split(",")]


def test_the_abi_is_still_9():
    from music_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()[0]).group(1)) == 9
    assert _lib.load().wn_version() == 9
    assert ctypes.sizeof(_lib.Sampling) == 24


def test_entries_are_declared_exported_and_bound_with_the_extended_signatures():
    from music_amd import _lib
    code = _header()[1]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wn_win_decode_batch", "wn_win_sample_logits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(raw, name), name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name]
        assert not name.startswith("wn_decode")
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    for new, old in (("wn_win_decode_batch", "wn_decode_batch_samp"), ("wn_win_sample_logits", "wn_sample_logits")):
        sig = _lib.SIGNATURES[old]
        assert _lib.SIGNATURES[new] == sig[:-1] + [p, i, l] + sig[-1:]
        names, base = _names(code, new), _names(code, old)
        assert names == base[:-1] + ["win_host", "win_period", "win_pos0", "stream"]
    # the existing entries keep their signatures
    assert _lib.SIGNATURES["wn_sample_logits"] == [p, l, i, l, p, ctypes.c_float, l, i, ctypes.c_float, l, p, p, p, p]
    assert len(_lib.SIGNATURES["wn_decode_batch_samp"]) == 52


def test_window_arguments_are_refused_by_name():
    lib = _lib()
    for kw in (dict(), dict(top_k=5, top_p=0.9), dict(samp=P), dict(cond_fg=None, cond_p1=None)):
        for what, bad in (("'win_period'", dict(period=-1)), ("'win_period'", dict(period=17)),
                          ("'win_period'", dict(win=[(0, 1)] * 17)),
                          ("'win_host'", dict(win=None, period=2)),
                          ("'win_host'", dict(win=((0, 128), (-1, 4)))), ("'win_host'", dict(win=((0, 257),))),
                          ("'win_host'", dict(win=((7, 7),))), ("'win_host'", dict(win=((9, 3),))),
                          ("'win_host'", dict(win=((0, 256), (0, 101)), Q=100)),
                          ("'win_pos0'", dict(win_pos0=-1)), ("'win_pos0'", dict(win_pos0=-2 ** 40))):
            msg = _refused(lib, what, **bad, **kw)
            assert msg.startswith("wn_win_decode_batch:"), msg
    assert "pair 1" in _refused(lib, "'win_host'", win=((0, 128), (200, 100)))
    # refused whether or not there is work to do
    _refused(lib, "'win_period'", period=17, n_steps=0)
    _refused(lib, "'win_pos0'", win_pos0=-1, n_utt=0)


def test_everything_the_sampling_entry_refuses():
    lib = _lib()
    for win in (((0, 128), (128, 256)), None):
        kw = dict(win=win)
        _refused(lib, "'top_p'", top_p=float("nan"), **kw)
        _refused(lib, "'top_p'", top_p=-0.25, **kw)
        _refused(lib, "'top_k'", top_k=-1, **kw)
        _refused(lib, "le (columns", le=0, **kw)
        _refused(lib, "c_shift_host", c_shift=None, **kw)
        _refused(lib, "c_q_host", c_q=None, **kw)
        cq = (ctypes.c_int32 * 3)(0, -1, 0)
        _refused(lib, "c_q", c_q=ctypes.cast(cq, ctypes.c_void_p), **kw)
        # windowed decode is corrected recurrence only
        for fw in (1, 2, 3):
            assert "corrected recurrence" in _refused(lib, "push_input", filter_width=fw, push_input=0, **kw)
        _refused(lib, "push_input", push_input=0, cond_fg=None, cond_p1=None, **kw)
        _refused(lib, "filter_width", filter_width=0, **kw)
        for arg in ("note0", "prev0", "note_out", "prev_out", "codes_out", "queues", "w_causal", "w_layers", "w_p1", "w_p2", "sync"):
            _refused(lib, "'%s'" % arg, **dict(kw, **{arg: None}))
        _refused(lib, "'dilations_host'", dil=None, **kw)
        _refused(lib, "quantisation", Q=4096, **kw)
        _refused(lib, "quantisation", Q=0, **kw)
        _refused(lib, "layers", n_layers=65, **kw)
        _refused(lib, "layers", n_layers=0, **kw)
        _refused(lib, "LDS", filter_width=4, R=16384, D=16384, **kw)
    assert _refused(lib, "le (columns", le=0).startswith("wn_win_decode_batch:")


def test_no_work_launches_nothing():
    lib = _lib()
    for kw in (dict(), dict(top_k=3, top_p=0.5), dict(samp=P), dict(win=None), dict(win=[(0, 256)] * 16, win_pos0=2 ** 40)):
        assert lib.wn_win_decode_batch(*_args(n_steps=0, **kw)) == 0
        assert lib.wn_win_decode_batch(*_args(n_utt=0, **kw)) == 0


def _sample(lib, win=((0, 128), (128, 256)), period=None, win_pos0=0, **over):
    a = dict(logits=P, n=4, Q=256, ld=256, samp=None, temperature=1.0, seed=0, top_k=0, top_p=1.0, step0=0, u=None, codes=P,
             probs=None)
    a.update(over)
    rc = lib.wn_win_sample_logits(*a.values(), _table(win), (len(win) if win is not None else 0) if period is None else period,
                                  win_pos0, None)
    return rc, lib.wn_last_error().decode()


def test_windowed_sampler_refusals_and_no_work():
    lib = _lib()
    for what, over in (("'Q'", dict(Q=0)), ("'Q'", dict(Q=1025)), ("'n'", dict(n=-1)), ("'ld'", dict(ld=255)),
                       ("'top_p'", dict(top_p=float("nan"))), ("'top_p'", dict(top_p=-1.0)), ("'top_k'", dict(top_k=-2)),
                       ("'logits'", dict(logits=None)), ("'codes'", dict(codes=None)),
                       ("'win_period'", dict(period=-3)), ("'win_period'", dict(period=17)),
                       ("'win_host'", dict(win=None, period=1)), ("'win_host'", dict(win=((-1, 5),))),
                       ("'win_host'", dict(win=((0, 65),), Q=64, ld=64)), ("'win_host'", dict(win=((0, 4), (4, 4)))),
                       ("'win_pos0'", dict(win_pos0=-1)), ("'win_pos0'", dict(win_pos0=-1, n=0))):
        rc, msg = _sample(lib, **over)
        assert rc == -4 and msg.startswith("wn_win_sample_logits:") and what in msg, (over, rc, msg)
    assert _sample(lib, n=0)[0] == 0
    assert _sample(lib, n=0, win=None)[0] == 0
    assert _sample(lib, n=0, logits=None, codes=None, samp=P, u=P, probs=P, win_pos0=2 ** 40)[0] == 0
    # the entry it extends still reports under its own name
    rc = lib.wn_sample_logits(P, 4, 0, 256, None, 1.0, 0, 0, 1.0, 0, None, P, None, None)
    assert rc == -4 and lib.wn_last_error().decode().startswith("wn_sample_logits:")
