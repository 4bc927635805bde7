"""CPU checks of wn_decode_batch_fw (ABI 6, cached-queue decode for any filter width): every refused argument comes back as -4
with a wn_last_error message before anything is launched, so no device is needed.  Pointers below are never dereferenced."""
import ctypes

P = 1 << 20            # "some non-NULL address"
_KEEP = []             # the host arrays of the last argument list stay alive


def _lib():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 6
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION
    return lib


def _args(lib, **over):
    dil = (ctypes.c_int32 * 2)(1, 2)
    qoff = (ctypes.c_int64 * 2)(0, 64)
    _KEEP[:] = [dil, qoff]
    a = dict(filter_width=3, n_layers=2, R=32, D=32, S=64, Q=256, dil=ctypes.cast(dil, ctypes.c_void_p),
             qoff=ctypes.cast(qoff, ctypes.c_void_p), queues=P, w_causal=P, b_causal=None, w_layers=P, layer_stride=4096,
             b_layers=None, w_p1=P, b_p1=None, w_p2=P, b_p2=None, note0=P, prev0=P, note_out=P, prev_out=P, forced=None,
             codes_out=P, probs_out=None, step0=0, n_steps=4, push_input=1, sync=P, n_utt=1, queues_ustride=0,
             temperature=0.0, seed=0, pk=None, pk_fg0=0, pk_d0=0, pk_lstride=0, pk_skip=-1, pk_p1=-1, pk_p2=-1, stream=None)
    a.update(over)
    return list(a.values())


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
