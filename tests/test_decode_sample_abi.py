"""CPU checks of the ABI 8 entry points wn_decode_batch_samp (cached-queue decode with top-k / nucleus sampling and a
per-utterance table of sampling settings) and wn_sample_logits (the decoder's sampler on a logits matrix): declared,
exported and bound, and every refused argument comes back as -4 with a wn_last_error message that names it, before anything
is launched - so no device is needed.  Pointers below are never dereferenced."""
import ctypes
import os
import re

from tests.decode_args import P, decode_args
from tests.helpers import ROOT


def _lib():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 8
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION
    return lib


def _args(**over):
    return decode_args("wn_decode_batch_samp", **{"temperature": 1.0, **over})


def _refused(lib, what, **over):
    rc = lib.wn_decode_batch_samp(*_args(**over))
    msg = lib.wn_last_error().decode()
    assert rc == -4 and "decode" in msg and what in msg, (over, rc, msg)
    return msg


def _header():
    src = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_abi_version_is_at_least_8():
    from music_amd import _lib
    assert _lib.ABI_VERSION >= 8
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()[0]).group(1)) == _lib.ABI_VERSION
    assert _lib.load().wn_version() == _lib.ABI_VERSION


def test_symbols_are_declared_exported_and_bound():
    from music_amd import _lib
    code = _header()[1]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wn_decode_batch_samp", "wn_sample_logits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(raw, name), name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name]
    # the arguments of wn_decode_batch_cond, then the wn_sampling table, top_k, top_p, and the stream last
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    cond = _lib.SIGNATURES["wn_decode_batch_cond"]
    assert _lib.SIGNATURES["wn_decode_batch_samp"] == cond[:-1] + [p, i, f] + cond[-1:]
    assert _lib.SIGNATURES["wn_sample_logits"] == [p, l, i, l, p, f, l, i, f, l, p, p, p, p]
    # the declaration's parameter list says the same
    decl = re.search(r"\bint\s+wn_decode_batch_samp\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names[-4:] == ["samp", "top_k", "top_p", "stream"] and len(names) == len(cond) + 3
    decl_c = re.search(r"\bint\s+wn_decode_batch_cond\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl_c.split(",")][:-1] == names[:-4]


def test_sampling_entry_is_24_bytes():
    from music_amd import _lib
    assert ctypes.sizeof(_lib.Sampling) == 24
    S = _lib.Sampling
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("temperature", 0, 4), ("top_p", 4, 4), ("top_k", 8, 4), ("stream", 12, 4), ("seed", 16, 8)]
    m = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*wn_sampling\s*;", _header()[1], flags=re.S)
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    assert fields == [["float", "temperature"], ["float", "top_p"], ["int32_t", "top_k"], ["uint32_t", "stream"], ["uint64_t", "seed"]]


def test_scalar_filters_out_of_range_are_refused():
    lib = _lib()
    _refused(lib, "'top_p'", top_p=float("nan"))
    _refused(lib, "'top_p'", top_p=-0.25)
    _refused(lib, "'top_k'", top_k=-1)
    _refused(lib, "'top_k'", top_k=-1, cond_fg=None, cond_p1=None)
    # with a table the scalars are ignored: such a call gets as far as the next check
    _refused(lib, "le (columns", samp=P, top_p=float("nan"), top_k=-1, le=0)


def test_everything_the_conditioned_entry_point_refuses():
    lib = _lib()
    for kw in (dict(), dict(top_k=5, top_p=0.9), dict(samp=P)):
        _refused(lib, "le (columns", le=0, **kw)
        _refused(lib, "c_shift_host", c_shift=None, **kw)
        _refused(lib, "c_q_host", c_q=None, **kw)
        cq = (ctypes.c_int32 * 3)(0, -1, 0)
        _refused(lib, "c_q", c_q=ctypes.cast(cq, ctypes.c_void_p), **kw)
        for fw in (1, 2, 3):
            assert "corrected recurrence" in _refused(lib, "push_input", filter_width=fw, push_input=0, **kw)
        _refused(lib, "push_input", push_input=0, cond_fg=None, cond_p1=None, **kw)
        _refused(lib, "filter_width", filter_width=0, **kw)
        for arg in ("note0", "prev0", "note_out", "prev_out", "codes_out", "queues", "w_causal", "w_layers", "w_p1", "w_p2", "sync"):
            _refused(lib, "'%s'" % arg, **dict(kw, **{arg: None}))
        _refused(lib, "'dilations_host'", dil=None, **kw)
        _refused(lib, "LDS", filter_width=4, R=16384, D=16384, **kw)
        _refused(lib, "LDS", c_shift=None, c_q=None, cond_fg=None, cond_p1=None, R=16384, D=16384, **kw)
        _refused(lib, "quantisation", Q=4096, **kw)
        _refused(lib, "quantisation", Q=0, **kw)
        _refused(lib, "layers", n_layers=65, **kw)
        _refused(lib, "layers", n_layers=0, **kw)
    # the messages of this entry point carry its own name
    assert _refused(lib, "le (columns", le=0).startswith("wn_decode_batch_samp:")


def test_no_work_launches_nothing():
    lib = _lib()
    for kw in (dict(), dict(top_k=3, top_p=0.5), dict(samp=P)):
        assert lib.wn_decode_batch_samp(*_args(n_steps=0, **kw)) == 0
        assert lib.wn_decode_batch_samp(*_args(n_utt=0, **kw)) == 0


def _sample(lib, **over):
    a = dict(logits=P, n=4, Q=256, ld=256, samp=None, temperature=1.0, seed=0, top_k=0, top_p=1.0, step0=0, u=None, codes=P,
             probs=None, stream=None)
    a.update(over)
    rc = lib.wn_sample_logits(*a.values())
    return rc, lib.wn_last_error().decode()


def test_sample_logits_refusals_and_no_work():
    lib = _lib()
    for what, over in (("'Q'", dict(Q=0)), ("'Q'", dict(Q=1025)), ("'n'", dict(n=-1)), ("'ld'", dict(ld=255)),
                       ("'top_p'", dict(top_p=float("nan"))), ("'top_p'", dict(top_p=-1.0)), ("'top_k'", dict(top_k=-2)),
                       ("'logits'", dict(logits=None)), ("'codes'", dict(codes=None))):
        rc, msg = _sample(lib, **over)
        assert rc == -4 and msg.startswith("wn_sample_logits:") and what in msg, (over, rc, msg)
    assert _sample(lib, n=0)[0] == 0
    assert _sample(lib, n=0, logits=None, codes=None, samp=P, u=P, probs=P)[0] == 0
