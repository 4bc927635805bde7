"""CPU checks of wn_decode_batch_fw (ABI 6, cached-queue decode for any filter width): every refused argument comes back as -4
with a wn_last_error message before anything is launched, so no device is needed.  Pointers below are never dereferenced."""
import ctypes

from tests.decode_args import decode_args


def _lib():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 6
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION
    return lib


def _args(lib, **over):
    return decode_args("wn_decode_batch_fw", **{"filter_width": 3, **over})


def _refused(lib, what, **over):
    rc = lib.wn_decode_batch_fw(*_args(lib, **over))
    msg = lib.wn_last_error().decode()
    assert rc == -4 and what in msg, (over, rc, msg)
    return msg


def test_entry_point_is_bound_with_filter_width_first():
    from music_amd import _lib
    sig = _lib.SIGNATURES["wn_decode_batch_fw"]
    pk = _lib.SIGNATURES["wn_decode_batch_pk"]
    assert sig == [ctypes.c_int] + pk
    _lib_ = _lib.load()
    assert _lib_.wn_decode_batch_fw.argtypes == sig


def test_filter_width_below_one_is_refused():
    lib = _lib()
    _refused(lib, "filter_width", filter_width=0)
    _refused(lib, "filter_width", filter_width=-2)


def test_as_written_push_is_refused_off_filter_width_two():
    lib = _lib()
    for fw in (1, 3, 4, 7):
        msg = _refused(lib, "push_input", filter_width=fw, push_input=0)
        assert "filter_width 2" in msg


def test_null_required_pointers_are_refused():
    lib = _lib()
    for arg in ("note0", "prev0", "note_out", "prev_out", "codes_out", "queues", "w_causal", "w_layers", "w_p1", "w_p2", "sync"):
        _refused(lib, "'%s'" % arg, **{arg: None})
    _refused(lib, "'dilations_host'", dil=None)


def test_layout_that_does_not_fit_is_refused():
    lib = _lib()
    _refused(lib, "LDS", filter_width=4, R=16384, D=16384)          # ~530 KB: beyond the 160 KiB of a CU
    _refused(lib, "quantisation", Q=4096)
    _refused(lib, "quantisation", Q=0)


def test_no_work_needs_no_history_for_filter_width_one():
    lib = _lib()
    # k = 1 keeps no previous input columns: NULL prev0 / prev_out are accepted (no steps: nothing is launched)
    assert lib.wn_decode_batch_fw(*_args(lib, filter_width=1, prev0=None, prev_out=None, n_steps=0)) == 0
    assert lib.wn_decode_batch_fw(*_args(lib, n_utt=0)) == 0
