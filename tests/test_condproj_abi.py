"""CPU checks of the learned conditioning projections' entry points wn_cond_proj_fwd and wn_cond_proj_bwd (include/wavenet_hip.h,
music_amd/csrc/wn_condproj.hip): declared, exported, bound with matching arity, the ABI version unchanged, every refusal reported
with function and argument before anything is launched, empty calls accepted.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

FWD_ARGS = ("enc", "flat", "w_off", "b_off", "stage_stride", "wf_off", "bf_off", "tab", "tab_pair", "enf", "n_stages", "dd", "ch", "sd",
            "bw", "le", "batch", "stream")
BWD_ARGS = ("d_tab", "pair", "d_enf", "enc", "flat", "w_off", "b_off", "stage_stride", "wf_off", "bf_off", "d_enc", "flat_grad",
            "n_stages", "dd", "ch", "sd", "bw", "le", "batch", "stream")


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_cond_proj_fwd", FWD_ARGS), ("wn_cond_proj_bwd", BWD_ARGS)])
def test_entries_are_declared_exported_and_bound(name, args):
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == args and len(_lib.SIGNATURES[name]) == len(args)
    # pointers, 64-bit offsets and ints are bound as such
    for a, typ in zip(decl.group(1).split(","), _lib.SIGNATURES[name]):
        want = ctypes.c_void_p if ("*" in a or "wn_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
        assert typ is want, (name, a)


def test_the_sources_are_in_the_makefile():
    assert "wn_condproj.hip" in open(os.path.join(ROOT, "music_amd", "csrc", "Makefile")).read()


def test_the_version_stays_9():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
N, DD, CH, SD, BW, LE, B = 3, 8, 32, 32, 16, 25, 2
STRIDE = 2 * DD * BW + 2 * DD
OK_FWD = [P, P, 0, 2 * DD * BW, STRIDE, N * STRIDE, N * STRIDE + SD * BW, P, P, P, N, DD, CH, SD, BW, LE, B, None]
OK_BWD = [P, 0, P, P, P, 0, 2 * DD * BW, STRIDE, N * STRIDE, N * STRIDE + SD * BW, P, P, N, DD, CH, SD, BW, LE, B, None]


def _refused(fn, names, ok, arg, **kw):
    from music_amd import _lib
    lib = _lib.load()
    a = list(ok)
    for k, v in kw.items():
        a[names.index(k)] = v
    rc = getattr(lib, fn)(*a)
    msg = lib.wn_last_error().decode()
    assert rc == -4 and fn in msg and "'%s'" % arg in msg, (fn, arg, rc, msg)


@pytest.mark.parametrize("fn,names,ok,required", [
    ("wn_cond_proj_fwd", FWD_ARGS, OK_FWD, ("enc", "flat", "enf")),
    ("wn_cond_proj_bwd", BWD_ARGS, OK_BWD, ("d_tab", "d_enf", "enc", "flat", "d_enc", "flat_grad"))])
def test_refusals_name_function_and_argument_and_empty_calls_pass(fn, names, ok, required):
    from music_amd import _lib
    lib = _lib.load()
    bad = lambda arg, **kw: _refused(fn, names, ok, arg, **kw)
    for name in required:
        bad(name, **{name: None})
    for name in ("n_stages", "dd", "sd", "bw", "le"):
        bad(name, **{name: 0})
    bad("batch", batch=-1)
    bad("ch", ch=48)                                     # not a multiple of 32
    bad("ch", ch=0)
    bad("ch", dd=40)                                     # ch < dd
    for name in ("w_off", "b_off", "wf_off", "bf_off"):
        bad(name, **{name: -1})
    bad("stage_stride", stage_stride=2 * DD * BW - 1)    # the stages' weights would overlap
    bad("stage_stride", bw=BW + 2)                       # (2 dd bw = 288 floats against a stride of 272)
    # batch == 0: nothing to do, NULLs allowed - but the shapes of an empty call are still checked
    a = list(ok)
    a[names.index("batch")] = 0
    for i, n in enumerate(names):
        if isinstance(a[i], int) and a[i] == P:
            a[i] = None
    assert getattr(lib, fn)(*a) == 0
    a[names.index("le")] = 0
    assert getattr(lib, fn)(*a) == -4 and "'le'" in lib.wn_last_error().decode()


def test_pair_tables_want_an_even_batch_and_the_forward_wants_a_table():
    from music_amd import _lib
    lib = _lib.load()
    _refused("wn_cond_proj_fwd", FWD_ARGS, OK_FWD, "batch", batch=3)          # tab_pair given
    _refused("wn_cond_proj_bwd", BWD_ARGS, OK_BWD, "batch", batch=3, pair=1)
    a = list(OK_FWD)
    a[FWD_ARGS.index("tab")] = a[FWD_ARGS.index("tab_pair")] = None
    assert lib.wn_cond_proj_fwd(*a) == -4
    msg = lib.wn_last_error().decode()
    assert "wn_cond_proj_fwd" in msg and "'tab'" in msg and "'tab_pair'" in msg
    # a single stage has no stride to check
    a = list(OK_FWD)
    a[FWD_ARGS.index("n_stages")], a[FWD_ARGS.index("stage_stride")], a[FWD_ARGS.index("enc")] = 1, 0, None
    assert lib.wn_cond_proj_fwd(*a) == -4 and "'enc'" in lib.wn_last_error().decode()
