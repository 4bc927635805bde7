"""CPU checks of the EMA codebook entries wn_vq_bwd_stats and wn_vq_ema_update (include/wavenet_hip.h, music_amd/csrc/wn_vq.hip),
in the pattern of tests/test_vq_abi.py: declared, exported, bound with matching arity and types; the ABI version is still 9 in
header, binding and library; the scratch size agrees; every refusal names function and argument before anything is launched; empty
calls pass; the limits themselves pass.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

STATS_ARGS = ("enc", "idx", "d_q", "flat", "cb_off", "beta", "g_scale", "d_enc", "flat_grad", "stat", "K", "bw", "le", "batch", "stream")
UPDATE_ARGS = ("flat", "cb_off", "stat", "state", "work", "info", "K", "bw", "decay", "eps", "restart", "guard_state", "stream")


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_vq_bwd_stats", STATS_ARGS), ("wn_vq_ema_update", UPDATE_ARGS)])
def test_entries_are_declared_exported_and_bound(name, args):
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == args and len(_lib.SIGNATURES[name]) == len(args)
    for a, typ in zip(decl.group(1).split(","), _lib.SIGNATURES[name]):
        want = (ctypes.c_void_p if ("*" in a or "wn_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else
                ctypes.c_float if "float" in a else ctypes.c_int)
        assert typ is want, (name, a)


def test_the_version_is_still_9_and_the_scratch_size_agrees():
    from music_amd import _lib
    h = _header()
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", h).group(1)) == _lib.ABI_VERSION == _lib.load().wn_version() == 9
    work = int(re.search(r"#define WN_VQ_EMA_WORK_BYTES (\d+)", h).group(1))
    codes = int(re.search(r"#define WN_VQ_MAX_CODES (\d+)", h).group(1))
    assert work == _lib.VQ_EMA_WORK_BYTES and work >= 4 * codes + 12 and work % 4 == 0      # tot, two counters, a donor per code
    assert "wn_vq.hip" in open(os.path.join(ROOT, "music_amd", "csrc", "Makefile")).read()


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
K, BW, LE, B = 32, 16, 25, 2
STATS_OK = [P, P, P, P, 0, 0.25, 1.0, P, P, P, K, BW, LE, B, None]
UPDATE_OK = [P, 0, P, P, P, P, K, BW, 0.99, 1e-5, 0.5, None, None]


def _refuser(fn, names, ok):
    from music_amd import _lib
    lib = _lib.load()

    def bad(arg, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        rc = getattr(lib, fn)(*a)
        msg = lib.wn_last_error().decode()
        assert rc == -4 and fn in msg and "'%s'" % arg in msg, (fn, arg, kw, rc, msg)
    return lib, bad


def test_stats_refusals_name_function_and_argument_and_empty_calls_pass():
    lib, bad = _refuser("wn_vq_bwd_stats", STATS_ARGS, STATS_OK)
    for name in ("enc", "idx", "d_q", "flat", "d_enc", "flat_grad", "stat"):
        bad(name, **{name: None})
    for k in (1, 0, -3, 1025):
        bad("K", K=k)
    for bw in (0, -1, 513):
        bad("bw", bw=bw)
    for le in (0, -2):
        bad("le", le=le)
    bad("batch", batch=-1)
    bad("cb_off", cb_off=-1)
    bad("batch", batch=1 << 20, le=1 << 20)                # more frames than an int counts
    a = [None if (isinstance(v, int) and v == P) else v for v in STATS_OK]
    a[STATS_ARGS.index("batch")] = 0
    assert lib.wn_vq_bwd_stats(*a) == 0                    # batch == 0: nothing to do, NULLs allowed ...
    a[STATS_ARGS.index("K")] = 1
    assert lib.wn_vq_bwd_stats(*a) == -4 and "'K'" in lib.wn_last_error().decode()      # ... the shapes are still checked


def test_update_refusals_name_function_and_argument():
    lib, bad = _refuser("wn_vq_ema_update", UPDATE_ARGS, UPDATE_OK)
    for name in ("flat", "stat", "state", "work"):
        bad(name, **{name: None})
    for k in (1, 0, -3, 1025):
        bad("K", K=k)
    for bw in (0, -1, 513):
        bad("bw", bw=bw)
    bad("cb_off", cb_off=-1)
    for decay in (0.0, 1.0, -0.5, 1.5, float("nan")):
        bad("decay", decay=decay)
    for eps in (-1e-9, float("nan")):
        bad("eps", eps=eps)
    for r in (-0.25, float("nan")):
        bad("restart", restart=r)
    bad("guard_state", guard_state=P + 4)                  # the guard's block is 8-byte aligned


def test_the_limits_themselves_are_accepted_by_the_checks():
    """K = 2 and 1024, bw = 1 and 512 pass the shape checks: with a NULL pointer the refusal that follows names the pointer;
    info and guard_state are optional."""
    from music_amd import _lib
    lib = _lib.load()
    for k, bw in ((2, 1), (1024, 512)):
        assert lib.wn_vq_bwd_stats(None, P, P, P, 0, 0.25, 1.0, P, P, P, k, bw, 1, 1, None) == -4
        assert "'enc'" in lib.wn_last_error().decode()
        assert lib.wn_vq_ema_update(P, 0, P, P, None, None, k, bw, 0.5, 0.0, 0.0, None, None) == -4
        assert "'work'" in lib.wn_last_error().decode()
