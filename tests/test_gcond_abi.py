"""CPU checks of the global class conditioning's entry points wn_gcond_proj_fwd and wn_gcond_proj_bwd (include/wavenet_hip.h,
music_amd/csrc/wn_gcond.hip): declared, exported, bound with matching arity and types, the ABI version unchanged, every refusal -
wn_cond_proj_fwd / _bwd's and the new arguments' - reported with function and argument before anything is launched, empty calls
accepted.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT
from tests.test_condproj_abi import BWD_ARGS as L_BWD_ARGS, FWD_ARGS as L_FWD_ARGS

NEW_ARGS = ("cls", "gw_off", "gstage_stride", "gwf_off", "emb_off", "ge", "n_cls")
FWD_ARGS = L_FWD_ARGS[:-1] + NEW_ARGS + ("stream",)            # the learned entry's arguments, the new ones, the stream last
BWD_ARGS = L_BWD_ARGS[:-1] + NEW_ARGS + ("stream",)


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_gcond_proj_fwd", FWD_ARGS), ("wn_gcond_proj_bwd", BWD_ARGS)])
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


def test_the_existing_entries_are_unchanged_and_the_source_is_in_the_makefile():
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, args in (("wn_cond_proj_fwd", L_FWD_ARGS), ("wn_cond_proj_bwd", L_BWD_ARGS)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
        assert tuple(a.split()[-1].lstrip("*") for a in decl.group(1).split(",")) == args and len(_lib.SIGNATURES[name]) == len(args)
    assert "wn_gcond.hip" in open(os.path.join(ROOT, "music_amd", "csrc", "Makefile")).read()


def test_the_version_stays_9_and_the_limit_is_512():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()
    assert int(re.search(r"#define WN_GCOND_MAX_CHANNELS (\d+)", _header()).group(1)) == 512 == _lib.GCOND_MAX_CHANNELS


P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
N, DD, CH, SD, BW, LE, B, GE, NCLS = 3, 8, 32, 32, 16, 25, 2, 5, 4
STRIDE = 2 * DD * BW + 2 * DD
END = N * STRIDE + SD * BW + SD
NEW_OK = [P, END, 2 * DD * GE, END + N * 2 * DD * GE, END + N * 2 * DD * GE + SD * GE, GE, NCLS]
OK_FWD = [P, P, 0, 2 * DD * BW, STRIDE, N * STRIDE, N * STRIDE + SD * BW, P, P, P, N, DD, CH, SD, BW, LE, B] + NEW_OK + [None]
OK_BWD = [P, 0, P, P, P, 0, 2 * DD * BW, STRIDE, N * STRIDE, N * STRIDE + SD * BW, P, P, N, DD, CH, SD, BW, LE, B] + NEW_OK + [None]


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
    ("wn_gcond_proj_fwd", FWD_ARGS, OK_FWD, ("enc", "flat", "enf", "cls")),
    ("wn_gcond_proj_bwd", BWD_ARGS, OK_BWD, ("d_tab", "d_enf", "enc", "flat", "d_enc", "flat_grad", "cls"))])
def test_refusals_name_function_and_argument_and_empty_calls_pass(fn, names, ok, required):
    from music_amd import _lib
    lib = _lib.load()
    bad = lambda arg, **kw: _refused(fn, names, ok, arg, **kw)
    for name in required:
        bad(name, **{name: None})
    # the learned entry's cases
    for name in ("n_stages", "dd", "sd", "bw", "le"):
        bad(name, **{name: 0})
    bad("batch", batch=-1)
    bad("ch", ch=48)
    bad("ch", ch=0)
    bad("ch", dd=40)
    for name in ("w_off", "b_off", "wf_off", "bf_off"):
        bad(name, **{name: -1})
    bad("stage_stride", stage_stride=2 * DD * BW - 1)
    # the new arguments'
    bad("ge", ge=0)
    bad("ge", ge=-3)
    bad("ge", ge=513)
    bad("n_cls", n_cls=0)
    for name in ("gw_off", "gwf_off", "emb_off"):
        bad(name, **{name: -1})
    bad("gstage_stride", gstage_stride=2 * DD * GE - 1)     # the stages' G would overlap
    bad("gstage_stride", gstage_stride=-1)
    # ge = 512, the limit, passes the checks: refused only for the next thing wrong
    bad("cls", ge=512, gstage_stride=2 * DD * 512, cls=None)
    # batch == 0: nothing to do, NULLs allowed - but the shapes of an empty call are still checked
    a = list(ok)
    a[names.index("batch")] = 0
    for i, n in enumerate(names):
        if isinstance(a[i], int) and a[i] == P:
            a[i] = None
    assert getattr(lib, fn)(*a) == 0
    a[names.index("ge")] = 0
    assert getattr(lib, fn)(*a) == -4 and "'ge'" in lib.wn_last_error().decode()


def test_pair_tables_want_an_even_batch_the_forward_a_table_and_one_stage_no_stride():
    from music_amd import _lib
    lib = _lib.load()
    _refused("wn_gcond_proj_fwd", FWD_ARGS, OK_FWD, "batch", batch=3)          # tab_pair given
    _refused("wn_gcond_proj_bwd", BWD_ARGS, OK_BWD, "batch", batch=3, pair=1)
    a = list(OK_FWD)
    a[FWD_ARGS.index("tab")] = a[FWD_ARGS.index("tab_pair")] = None
    assert lib.wn_gcond_proj_fwd(*a) == -4
    msg = lib.wn_last_error().decode()
    assert "wn_gcond_proj_fwd" in msg and "'tab'" in msg and "'tab_pair'" in msg
    # a single stage has no stride to check
    _refused("wn_gcond_proj_fwd", FWD_ARGS, OK_FWD, "cls", n_stages=1, stage_stride=0, gstage_stride=0, cls=None)
    _refused("wn_gcond_proj_bwd", BWD_ARGS, OK_BWD, "cls", n_stages=1, stage_stride=0, gstage_stride=0, cls=None)
