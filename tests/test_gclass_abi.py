"""CPU checks of the class-conditional WaveNet's table entries wn_gclass_fwd and wn_gclass_bwd (include/wavenet_hip.h,
music_amd/csrc/wn_gcond.hip): declared, exported, bound with matching arity and types, the ABI version unchanged, every refusal - the
cases of wn_gcond_proj_fwd / _bwd that still apply - reported with function and argument before anything is launched, empty calls
accepted.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

TAIL = ("cls", "gw_off", "gstage_stride", "gwf_off", "emb_off", "ge", "n_cls", "stream")
FWD_ARGS = ("flat", "tab", "tab_pair", "enf", "n_stages", "dd", "ch", "sd", "batch") + TAIL
BWD_ARGS = ("d_tab", "pair", "d_enf", "flat", "flat_grad", "n_stages", "dd", "ch", "sd", "batch") + TAIL


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_gclass_fwd", FWD_ARGS), ("wn_gclass_bwd", BWD_ARGS)])
def test_entries_are_declared_exported_and_bound(name, args):
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
    assert decl, "%s is not declared" % name
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    declared = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert tuple(declared) == args and len(_lib.SIGNATURES[name]) == len(args)
    for a, typ in zip(decl.group(1).split(","), _lib.SIGNATURES[name]):
        want = ctypes.c_void_p if ("*" in a or "wn_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
        assert typ is want, (name, a)
    assert "const int32_t* cls" in decl.group(1)


def test_the_version_stays_9_and_the_entries_live_in_wn_gcond():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()
    src = open(os.path.join(ROOT, "music_amd", "csrc", "wn_gcond.hip")).read()
    assert "wn_launch_gclass_fwd" in src and "wn_launch_gclass_bwd" in src


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
N, DD, CH, SD, B, GE, NCLS = 3, 8, 32, 32, 2, 5, 4
NEW_OK = [P, 100, 2 * DD * GE, 100 + N * 2 * DD * GE, 100 + N * 2 * DD * GE + SD * GE, GE, NCLS]
OK_FWD = [P, P, P, P, N, DD, CH, SD, B] + NEW_OK + [None]
OK_BWD = [P, 0, P, P, P, N, DD, CH, SD, B] + NEW_OK + [None]


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
    ("wn_gclass_fwd", FWD_ARGS, OK_FWD, ("flat", "enf", "cls")),
    ("wn_gclass_bwd", BWD_ARGS, OK_BWD, ("d_tab", "d_enf", "flat", "flat_grad", "cls"))])
def test_refusals_name_function_and_argument_and_empty_calls_pass(fn, names, ok, required):
    from music_amd import _lib
    lib = _lib.load()
    bad = lambda arg, **kw: _refused(fn, names, ok, arg, **kw)
    for name in required:
        bad(name, **{name: None})
    for name in ("n_stages", "dd", "sd"):
        bad(name, **{name: 0})
    bad("batch", batch=-1)
    bad("ch", ch=48)
    bad("ch", ch=0)
    bad("ch", dd=40)
    bad("ge", ge=0)
    bad("ge", ge=-3)
    bad("ge", ge=513)
    bad("n_cls", n_cls=0)
    for name in ("gw_off", "gwf_off", "emb_off"):
        bad(name, **{name: -1})
    bad("gstage_stride", gstage_stride=2 * DD * GE - 1)     # the stages' G would overlap
    bad("gstage_stride", gstage_stride=-1)
    # ge = 512, the limit, passes the checks: refused only for the next thing wrong; a single stage has no stride to check
    bad("cls", ge=512, gstage_stride=2 * DD * 512, cls=None)
    bad("cls", n_stages=1, gstage_stride=0, cls=None)
    # batch == 0: nothing to do, NULLs allowed - but the shapes of an empty call are still checked
    a = list(ok)
    a[names.index("batch")] = 0
    for i, n in enumerate(names):
        if isinstance(a[i], int) and a[i] == P:
            a[i] = None
    assert getattr(lib, fn)(*a) == 0
    a[names.index("ge")] = 0
    assert getattr(lib, fn)(*a) == -4 and "'ge'" in lib.wn_last_error().decode()


def test_pair_tables_want_an_even_batch_and_the_forward_a_table():
    from music_amd import _lib
    lib = _lib.load()
    _refused("wn_gclass_fwd", FWD_ARGS, OK_FWD, "batch", batch=3)          # tab_pair given
    _refused("wn_gclass_bwd", BWD_ARGS, OK_BWD, "batch", batch=3, pair=1)
    a = list(OK_FWD)
    a[FWD_ARGS.index("tab")] = a[FWD_ARGS.index("tab_pair")] = None
    assert lib.wn_gclass_fwd(*a) == -4
    msg = lib.wn_last_error().decode()
    assert "wn_gclass_fwd" in msg and "'tab'" in msg and "'tab_pair'" in msg
