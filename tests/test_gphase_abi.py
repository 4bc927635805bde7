"""CPU checks of the phase-conditioned WaveNet's table entries wn_phase_tab_fwd and wn_phase_tab_bwd (include/wavenet_hip.h,
music_amd/csrc/wn_phase.hip): declared, exported, bound with matching arity and types, the ABI version unchanged, every refusal
reported with function and argument before anything is launched, empty calls accepted.  No device is touched."""
import ctypes
import os
import re

import pytest

from tests.helpers import ROOT

OFFS = ("pw_off", "pstage_stride", "pwf_off", "pos", "rot")
DIMS = ("n_stages", "dd", "ch", "sd", "period", "batch", "stream")
FWD_ARGS = ("flat",) + OFFS + ("add_tab", "add_pair", "add_enf", "tab", "tab_pair", "enf") + DIMS
BWD_ARGS = ("d_tab", "pair", "d_enf", "flat_grad") + OFFS + ("sum_tab", "sum_enf") + DIMS


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


@pytest.mark.parametrize("name,args", [("wn_phase_tab_fwd", FWD_ARGS), ("wn_phase_tab_bwd", BWD_ARGS)])
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
    assert "const int64_t* pos" in decl.group(1) and "const int32_t* rot" in decl.group(1)


def test_the_version_stays_9_and_the_entries_live_in_wn_phase():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()
    assert int(re.search(r"#define WN_PHASE_MAX_PERIOD (\d+)", _header()).group(1)) == 16 == _lib.PHASE_MAX_PERIOD
    src = open(os.path.join(ROOT, "music_amd", "csrc", "wn_phase.hip")).read()
    assert "wn_launch_phase_tab_fwd" in src and "wn_launch_phase_tab_bwd" in src
    assert "atomic" not in src.lower().replace("no atomics", "")


A = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
N, DD, CH, SD, P, B = 3, 8, 32, 32, 5, 2
OFFS_OK = [100, 2 * DD * P, 100 + N * 2 * DD * P, A, A]
OK_FWD = [A] + OFFS_OK + [None, None, None, A, A, A, N, DD, CH, SD, P, B, None]
OK_BWD = [A, 0, A, A] + OFFS_OK + [None, None, N, DD, CH, SD, P, B, None]


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
    ("wn_phase_tab_fwd", FWD_ARGS, OK_FWD, ("flat", "pos", "rot", "enf")),
    ("wn_phase_tab_bwd", BWD_ARGS, OK_BWD, ("d_tab", "d_enf", "flat_grad", "pos", "rot"))])
def test_refusals_name_function_and_argument_and_empty_calls_pass(fn, names, ok, required):
    from music_amd import _lib
    lib = _lib.load()
    bad = lambda arg, **kw: _refused(fn, names, ok, arg, **kw)
    for name in required:
        bad(name, **{name: None})
    for name in ("n_stages", "dd", "sd"):
        bad(name, **{name: 0})
    bad("batch", batch=-1)
    for period in (0, -1, 17):
        bad("period", period=period)
    bad("ch", ch=48)
    bad("ch", ch=0)
    bad("ch", dd=40)
    for name in ("pw_off", "pwf_off"):
        bad(name, **{name: -1})
    bad("pstage_stride", pstage_stride=2 * DD * P - 1)          # the stages' tables would overlap
    bad("pstage_stride", pstage_stride=-1)
    # period = 16, the limit, and 1 pass the checks: refused only for the next thing wrong; a single stage has no stride to check
    bad("pos", period=16, pstage_stride=2 * DD * 16, pos=None)
    bad("pos", period=1, pos=None)
    bad("pos", n_stages=1, pstage_stride=0, pos=None)
    # batch == 0: nothing to do, NULLs allowed - but the shapes of an empty call are still checked
    a = list(ok)
    a[names.index("batch")] = 0
    for i, n in enumerate(names):
        if isinstance(a[i], int) and a[i] == A:
            a[i] = None
    assert getattr(lib, fn)(*a) == 0
    a[names.index("period")] = 0
    assert getattr(lib, fn)(*a) == -4 and "'period'" in lib.wn_last_error().decode()


def test_pair_tables_want_an_even_batch_the_forward_a_table_and_optional_pointers_come_whole():
    from music_amd import _lib
    lib = _lib.load()
    _refused("wn_phase_tab_fwd", FWD_ARGS, OK_FWD, "batch", batch=3)          # tab_pair given
    _refused("wn_phase_tab_bwd", BWD_ARGS, OK_BWD, "batch", batch=3, pair=1)
    a = list(OK_FWD)
    a[FWD_ARGS.index("tab")] = a[FWD_ARGS.index("tab_pair")] = None
    assert lib.wn_phase_tab_fwd(*a) == -4
    msg = lib.wn_last_error().decode()
    assert "wn_phase_tab_fwd" in msg and "'tab'" in msg and "'tab_pair'" in msg
    # the class term: an addend for every output that is given
    _refused("wn_phase_tab_fwd", FWD_ARGS, OK_FWD, "add_enf", add_tab=A, add_pair=A)
    _refused("wn_phase_tab_fwd", FWD_ARGS, OK_FWD, "add_tab", add_enf=A, add_pair=A)
    _refused("wn_phase_tab_fwd", FWD_ARGS, OK_FWD, "add_pair", add_enf=A, add_tab=A)
    _refused("wn_phase_tab_bwd", BWD_ARGS, OK_BWD, "sum_enf", sum_tab=A)
    _refused("wn_phase_tab_bwd", BWD_ARGS, OK_BWD, "sum_tab", sum_enf=A)
