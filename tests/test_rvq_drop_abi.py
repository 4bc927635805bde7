"""CPU checks of quantiser dropout's entries wn_rvq_fwd_n, wn_rvq_bwd_n, wn_rvq_bwd_stats_n and wn_rvq_lookup_n (include/wavenet_hip.h,
music_amd/csrc/wn_vq.hip), in the pattern of tests/test_rvq_abi.py: declared, exported, bound with matching arity and types; the ABI
version is still 9; every refusal - a NULL nstage included - returns -4 and names function and argument before anything is launched;
empty calls pass; the limits themselves pass.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

ARGS = {
    "wn_rvq_fwd_n": ("enc", "flat", "cb_off", "nstage", "q_out", "idx", "counts", "res", "loss_part", "S", "K", "bw", "le", "batch", "stream"),
    "wn_rvq_bwd_n": ("enc", "idx", "res", "nstage", "d_q", "flat", "cb_off", "beta", "g_scale", "d_enc", "flat_grad", "S", "K", "bw", "le",
                     "batch", "stream"),
    "wn_rvq_bwd_stats_n": ("enc", "idx", "res", "nstage", "d_q", "flat", "cb_off", "beta", "g_scale", "d_enc", "flat_grad", "stat", "S", "K",
                           "bw", "le", "batch", "stream"),
    "wn_rvq_lookup_n": ("idx", "nstage", "flat", "cb_off", "q_out", "bad", "S", "K", "bw", "le", "batch", "stream"),
}
P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
S, K, BW, LE, B = 3, 32, 16, 25, 2
OK = {
    "wn_rvq_fwd_n": [P, P, 0, P, P, P, P, P, P, S, K, BW, LE, B, None],
    "wn_rvq_bwd_n": [P, P, P, P, P, P, 0, 0.25, 1.0, P, P, S, K, BW, LE, B, None],
    "wn_rvq_bwd_stats_n": [P, P, P, P, P, P, 0, 0.25, 1.0, P, P, P, S, K, BW, LE, B, None],
    "wn_rvq_lookup_n": [P, P, P, 0, P, P, S, K, BW, LE, B, None],
}
REQUIRED = {
    "wn_rvq_fwd_n": ("enc", "flat", "nstage", "q_out", "idx", "res", "loss_part"),
    "wn_rvq_bwd_n": ("enc", "idx", "res", "nstage", "d_q", "flat", "d_enc", "flat_grad"),
    "wn_rvq_bwd_stats_n": ("enc", "idx", "res", "nstage", "d_q", "flat", "d_enc", "flat_grad", "stat"),
    "wn_rvq_lookup_n": ("idx", "nstage", "flat", "q_out"),
}


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name", sorted(ARGS))
def test_entries_are_declared_exported_and_bound(name):
    from music_amd import _lib
    args = ARGS[name]
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(_lib.load(), name)
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == args and len(_lib.SIGNATURES[name]) == len(args) == len(OK[name])
    for a, typ in zip(decl.group(1).split(","), _lib.SIGNATURES[name]):
        want = (ctypes.c_void_p if ("*" in a or "wn_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else
                ctypes.c_float if "float" in a else ctypes.c_int)
        assert typ is want, (name, a)


def test_the_version_is_still_9():
    from music_amd import _lib
    h = _header()
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", h).group(1)) == _lib.ABI_VERSION == _lib.load().wn_version() == 9
    assert int(re.search(r"#define WN_RVQ_MAX_STAGES (\d+)", h).group(1)) == _lib.RVQ_MAX_STAGES == 8


def _bad(lib, fn, arg, **kw):
    a = list(OK[fn])
    for k, v in kw.items():
        a[ARGS[fn].index(k)] = v
    rc = getattr(lib, fn)(*a)
    msg = lib.wn_last_error().decode()
    assert rc == -4 and fn in msg and "'%s'" % arg in msg, (fn, arg, kw, rc, msg)


@pytest.mark.parametrize("fn", sorted(ARGS))
def test_refusals_name_function_and_argument(fn):
    from music_amd import _lib
    lib = _lib.load()
    assert "nstage" in REQUIRED[fn]
    for name in REQUIRED[fn]:
        _bad(lib, fn, name, **{name: None})
    for s in (0, -1, 9):
        _bad(lib, fn, "S", S=s)
    for k in (1, 0, -3, 1025):
        _bad(lib, fn, "K", K=k)
    for bw in (0, -1, 513):
        _bad(lib, fn, "bw", bw=bw)
    _bad(lib, fn, "cb_off", cb_off=-1)
    for le in (0, -2):
        _bad(lib, fn, "le", le=le)
    _bad(lib, fn, "batch", batch=-1)
    _bad(lib, fn, "batch", batch=1 << 20, le=1 << 20)          # more frames than an int counts
    # batch == 0: nothing to do, NULLs allowed ... the shapes are still checked
    a = [None if (isinstance(v, int) and v == P) else v for v in OK[fn]]
    a[ARGS[fn].index("batch")] = 0
    assert getattr(lib, fn)(*a) == 0
    a[ARGS[fn].index("S")] = 9
    assert getattr(lib, fn)(*a) == -4 and "'S'" in lib.wn_last_error().decode()


def test_the_limits_themselves_are_accepted_by_the_checks():
    """S = 1 and 8, K = 2 and 1024, bw = 1 and 512 pass the shape checks: with a NULL pointer the refusal that follows names the
    pointer; counts and bad are optional."""
    from music_amd import _lib
    lib = _lib.load()
    for s, k, bw in ((1, 2, 1), (8, 1024, 512)):
        assert lib.wn_rvq_fwd_n(None, P, 0, P, P, P, None, P, P, s, k, bw, 1, 1, None) == -4 and "'enc'" in lib.wn_last_error().decode()
        assert lib.wn_rvq_fwd_n(P, P, 0, None, P, P, None, P, P, s, k, bw, 1, 1, None) == -4 and "'nstage'" in lib.wn_last_error().decode()
        assert lib.wn_rvq_bwd_n(P, P, P, None, P, P, 0, 0.25, 1.0, P, P, s, k, bw, 1, 1, None) == -4
        assert "'nstage'" in lib.wn_last_error().decode()
        assert lib.wn_rvq_bwd_stats_n(P, P, P, P, P, P, 0, 0.25, 1.0, P, P, None, s, k, bw, 1, 1, None) == -4
        assert "'stat'" in lib.wn_last_error().decode()
        assert lib.wn_rvq_lookup_n(None, P, P, 0, P, None, s, k, bw, 1, 1, None) == -4 and "'idx'" in lib.wn_last_error().decode()
