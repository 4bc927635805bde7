"""CPU checks of wn_decode_batch_cond (ABI 7, cached-queue decode with per-utterance conditioning tables): the symbol is
declared, exported and bound, and every refused argument comes back as -4 with a wn_last_error message before anything is
launched, so no device is needed.  Pointers below are never dereferenced."""
import ctypes
import os
import re

from tests.decode_args import decode_args
from tests.helpers import ROOT


def _lib():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 7
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION
    return lib


def _args(lib, **over):
    return decode_args("wn_decode_batch_cond", **over)


def _refused(lib, what, **over):
    rc = lib.wn_decode_batch_cond(*_args(lib, **over))
    msg = lib.wn_last_error().decode()
    assert rc == -4 and "decode" in msg and what in msg, (over, rc, msg)
    return msg


def test_abi_version_is_at_least_7():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 7
    src = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION


def test_symbol_is_declared_exported_and_bound():
    from music_amd import _lib
    src = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+wn_decode_batch_cond\s*\(", src)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wn_decode_batch_cond")
    sig = _lib.SIGNATURES["wn_decode_batch_cond"]
    fw = _lib.SIGNATURES["wn_decode_batch_fw"]
    # the arguments of wn_decode_batch_fw, then cond_fg + stride, cond_p1 + stride, c_shift, c_q, le, pos0, and the stream last
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert sig == fw[:-1] + [p, l, p, l, p, p, i, l] + fw[-1:]
    assert _lib.load().wn_decode_batch_cond.argtypes == sig


def test_table_width_below_one_is_refused():
    lib = _lib()
    _refused(lib, "le (columns", le=0)
    _refused(lib, "le (columns", le=-4)
    _refused(lib, "le (columns", le=0, cond_fg=None, cond_p1=None)


def test_table_without_schedule_is_refused():
    lib = _lib()
    _refused(lib, "c_shift_host", c_shift=None)
    _refused(lib, "c_q_host", c_q=None)
    _refused(lib, "schedule", c_shift=None, cond_p1=None)
    _refused(lib, "schedule", c_q=None, cond_fg=None)
    # without tables no schedule is needed: this one gets as far as decode_k's LDS check
    _refused(lib, "LDS", c_shift=None, c_q=None, cond_fg=None, cond_p1=None, R=16384, D=16384)


def test_negative_stretch_factor_is_refused():
    lib = _lib()
    for pos in range(3):
        cq = (ctypes.c_int32 * 3)(0, 5, 0)
        cq[pos] = -1
        _refused(lib, "c_q", c_q=ctypes.cast(cq, ctypes.c_void_p))


def test_as_written_push_is_refused():
    lib = _lib()
    for fw in (1, 2, 3):
        msg = _refused(lib, "push_input", filter_width=fw, push_input=0)
        assert "corrected recurrence" in msg
    _refused(lib, "push_input", push_input=0, cond_fg=None, cond_p1=None)


def test_everything_the_unconditioned_entry_point_refuses():
    lib = _lib()
    _refused(lib, "filter_width", filter_width=0)
    for arg in ("note0", "prev0", "note_out", "prev_out", "codes_out", "queues", "w_causal", "w_layers", "w_p1", "w_p2", "sync"):
        _refused(lib, "'%s'" % arg, **{arg: None})
    _refused(lib, "'dilations_host'", dil=None)
    _refused(lib, "LDS", filter_width=4, R=16384, D=16384)
    _refused(lib, "quantisation", Q=4096)
    _refused(lib, "quantisation", Q=0)
    _refused(lib, "layers", n_layers=65)
    _refused(lib, "layers", n_layers=0)


def test_no_work_launches_nothing():
    lib = _lib()
    assert lib.wn_decode_batch_cond(*_args(lib, n_steps=0)) == 0
    assert lib.wn_decode_batch_cond(*_args(lib, n_utt=0)) == 0
