"""CPU checks of the vector-quantised bottleneck's entry points wn_vq_fwd, wn_vq_bwd and wn_vq_lookup (include/wavenet_hip.h,
music_amd/csrc/wn_vq.hip): declared, exported, bound with matching arity and types, header, binding and library agree on the ABI
version, every refusal reported with function and argument before anything is launched, empty calls accepted.  No device is
touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

FWD_ARGS = ("enc", "flat", "cb_off", "q_out", "idx", "counts", "loss_part", "K", "bw", "le", "batch", "stream")
BWD_ARGS = ("enc", "idx", "d_q", "flat", "cb_off", "beta", "g_scale", "d_enc", "flat_grad", "K", "bw", "le", "batch", "stream")
LOOKUP_ARGS = ("idx", "flat", "cb_off", "q_out", "bad", "K", "bw", "le", "batch", "stream")


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_vq_fwd", FWD_ARGS), ("wn_vq_bwd", BWD_ARGS), ("wn_vq_lookup", LOOKUP_ARGS)])
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


def test_the_source_is_in_the_makefile_and_the_limits_agree():
    from music_amd import _lib
    assert "wn_vq.hip" in open(os.path.join(ROOT, "music_amd", "csrc", "Makefile")).read()
    h = _header()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, h).group(1))
    assert define("WN_VQ_NUM_PARTIALS") == _lib.VQ_NUM_PARTIALS
    assert define("WN_VQ_MAX_CODES") == _lib.VQ_MAX_CODES == 1024
    assert define("WN_VQ_MAX_WIDTH") == _lib.VQ_MAX_WIDTH == 512
    # the codes must be a sequence the prior's kernels take
    kernels_h = open(os.path.join(ROOT, "music_amd", "csrc", "wn_kernels.h")).read()
    assert define("WN_VQ_MAX_CODES") == int(re.search(r"#define WN_DEC_MAX_Q (\d+)", kernels_h).group(1))


def test_header_binding_and_library_agree_on_the_version():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == _lib.ABI_VERSION == _lib.load().wn_version()


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
K, BW, LE, B = 32, 16, 25, 2
OK = {
    "wn_vq_fwd": (FWD_ARGS, [P, P, 0, P, P, P, P, K, BW, LE, B, None], ("enc", "flat", "q_out", "idx", "loss_part")),
    "wn_vq_bwd": (BWD_ARGS, [P, P, P, P, 0, 0.25, 1.0, P, P, K, BW, LE, B, None], ("enc", "idx", "d_q", "flat", "d_enc", "flat_grad")),
    "wn_vq_lookup": (LOOKUP_ARGS, [P, P, 0, P, P, K, BW, LE, B, None], ("idx", "flat", "q_out")),
}


@pytest.mark.parametrize("fn", sorted(OK))
def test_refusals_name_function_and_argument_and_empty_calls_pass(fn):
    from music_amd import _lib
    lib = _lib.load()
    names, ok, required = OK[fn]

    def bad(arg, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        rc = getattr(lib, fn)(*a)
        msg = lib.wn_last_error().decode()
        assert rc == -4 and fn in msg and "'%s'" % arg in msg, (fn, arg, kw, rc, msg)

    for name in required:                                  # a NULL required pointer with work to do
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
    # batch == 0: nothing to do, NULLs allowed - but the shapes of an empty call are still checked
    a = list(ok)
    a[names.index("batch")] = 0
    for i in range(len(a)):
        if isinstance(a[i], int) and a[i] == P:
            a[i] = None
    assert getattr(lib, fn)(*a) == 0
    a[names.index("K")] = 1
    assert getattr(lib, fn)(*a) == -4 and "'K'" in lib.wn_last_error().decode()


def test_the_limits_themselves_are_accepted_by_the_checks():
    """K = 2 and 1024, bw = 1 and 512 pass the shape checks: with a NULL pointer the refusal that follows names the pointer."""
    from music_amd import _lib
    lib = _lib.load()
    for k, bw in ((2, 1), (1024, 512)):
        assert lib.wn_vq_fwd(None, P, 0, P, P, None, P, k, bw, 1, 1, None) == -4
        assert "'enc'" in lib.wn_last_error().decode()
    # counts and bad are optional: the refusal names the first required pointer behind them
    assert lib.wn_vq_lookup(P, P, 0, None, None, K, BW, LE, B, None) == -4 and "'q_out'" in lib.wn_last_error().decode()
