"""GPU tests of guided pairs in the decode kernels (music_amd/csrc/wn_decode.hip: decode_k<FW, true> and the two choosing sites of
decode_duo_mfma8_k), one wn_cfg_decode_batch launch at a time against tests/cfg_ref.py, the float64 restatement built on
tests/decode_ref.py (run with -m gpu).

The builders, frames and comparisons are those of tests/test_gpu_decode_kernels.py (imported, not copied): explicit weights in the
header's layout, NaN / sentinel frames around every output, slack between the rows' rings, `_route` for the form a launch must run.
The cases (tests/cfg_ref.CASES; tests/test_cfg_ref.py holds their conditions on the CPU): the matrix cores at 64 / 64 / 256 / 256
with 1, 3, 4 and 5 pairs - spare pairs, a full group of eight, a second group holding one pair; the split skip stage (one group) and
the one-workgroup one (two groups; every case again under WN_DEC_KS=1 in a child process) -, 512 skip channels, filter width 3,
biased and unbiased, 32 blocks (the tap-0 table in the hand-off area); decode_k at Q = 100 and Q = 1024 under a 4-pair window table,
filter widths 1, 2, 3 and the Q = 256 fast pick.  Every row has its own rings and tables; row 2j + 1's wn_sampling entry is garbage.

Checked per case: both rows of a pair carry equal codes, probabilities, note_out and prev_out; the pair's probabilities and every
row's rings against the guided reference; frames intact; pair j of the batch is the one-pair launch of rows 2j, 2j + 1 bit for bit
(same form); guidance of all ones gives the even rows of the un-guided launch bit for bit; a second launch gives the same bits.
Bars: decode_ref.bar() on the guided reference's own degraded forms (fp32 kernel 8 e32, matrix cores 4 ex3 + 8 e32) - no new number."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from tests import cfg_ref as cr
from tests import decode_ref as dr
from tests import test_gpu_decode_kernels as tk
from tests.test_gpu_decode_kernels import DEV, FRAME, GAP, NAN, SENT, State, Weights, _bits, _frames_ok, _framed, _inner

ROOT = tk.ROOT
WORST = {}


@functools.lru_cache(maxsize=None)
def inputs(cid):
    return cr.Inputs(cr.CASE[cid])


@functools.lru_cache(maxsize=None)
def refs(cid):
    return inputs(cid).references()


@functools.lru_cache(maxsize=None)
def weights(cid):
    return Weights(inputs(cid).net, cr.CASE[cid]["fam"] == "mf")


def _samp_table(c, rows, sane_odd):
    """wn_sampling entries of `rows`: the conditional member of pair j draws as stream j under the case's temperature; the
    unconditional member's entry is garbage (ignored by a guided launch) unless `sane_odd` (the un-guided comparison launch)"""
    tab = np.zeros(len(rows), dtype=np.dtype([("temperature", "<f4"), ("top_p", "<f4"), ("top_k", "<i4"), ("stream", "<u4"), ("seed", "<u8")]))
    for i, r in enumerate(rows):
        if r % 2 == 0 or sane_odd:
            tab[i] = (c["temp"], 1.0, 0, r // 2, 1234)
        else:
            tab[i] = (5.0, 0.3, 1, 999, 77)
    return torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)


def launch(inp, w, st, capfd, guidance="case", forced="case"):
    """One launch of the case's n steps from state `st` on its rows: wn_cfg_decode_batch with the rows' scales (`guidance`: "case",
    an array of one scale per pair of st.rows, or None - then wn_win_decode_batch, the un-guided launch of the same rows).
    Returns dict(probs [U][n][Q], codes [U][n], note_out, prev_out, form) after the frames, the flags and the slack were checked."""
    c, net = inp.c, inp.net
    k, N, S, Q, n = net.k, net.N, net.S, net.Q, c["n"]
    rows, U = st.rows, len(st.rows)
    assert U % 2 == 0 and all(r % 2 == 0 and rows[i + 1] == r + 1 for i, r in list(enumerate(rows))[0::2]), "whole pairs"
    if forced == "case":
        forced = inp.forced
    forced_t = torch.from_numpy(np.ascontiguousarray(forced[rows])).to(device=DEV, dtype=torch.int32) if forced is not None else None
    probs, codes = _framed(U * n * Q), _framed(U * n, torch.int32, SENT)
    note_out, prev_out = _framed(U * Q), _framed(U * (k - 1) * Q)
    gran = _lib.decode_sync_granules(N, w.Dp, S)
    sync = torch.full((U * gran + 8,), -12345, dtype=torch.int64, device=DEV)
    sync[:U * gran] = 0
    dil = (ctypes.c_int32 * N)(*net.dil)
    qoff = (ctypes.c_int64 * N)(*[int(v) for v in st.q_off[:N]])
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    args = (k, N, w.Rp, w.Dp, S, Q, vp(dil), vp(qoff), ptr(st.rings, FRAME), *w.args(),
            ptr(st.note), ptr(st.prev) if k > 1 else None, ptr(note_out, FRAME), ptr(prev_out, FRAME) if k > 1 else None,
            ptr(forced_t), ptr(codes, FRAME), ptr(probs, FRAME), c["step0"], n, 1, ptr(sync), U, st.ustride, 0.0, 0, *w.chain())
    s = inp.cond
    le, keep, tabs = s["le"], [], []
    for key, width, stages in (("fg", 2 * w.Dp, N), ("p1", S, 1)):          # [U][stages][le][..], NaN between the rows' tables
        src = s[key][rows] if key == "fg" else s[key][rows][:, None]
        full = np.zeros((U, stages, le, width), np.float32)
        if key == "fg":                                                      # rows f then g, each padded to Dp
            full[..., :net.D] = src[..., :net.D]
            full[..., w.Dp:w.Dp + net.D] = src[..., net.D:]
        else:
            full[:] = src
        us = stages * le * width + GAP
        t = torch.full((U, us), NAN, device=DEV)
        t[:, :us - GAP] = torch.from_numpy(full.reshape(U, -1)).to(DEV)
        keep.append(t)
        tabs += [ptr(t), us]
    sh, qs = (ctypes.c_int32 * (N + 1))(*s["shift"]), (ctypes.c_int32 * (N + 1))(*s["q"])
    wh = (ctypes.c_int32 * max(2, 2 * len(c["win"] or [])))(*[v for pr in (c["win"] or []) for v in pr])
    samp = _samp_table(c, rows, sane_odd=guidance is None)
    args += (*tabs, vp(sh), vp(qs), le, s["pos0"], ptr(samp), 0, 1.0, vp(wh) if c["win"] else None, len(c["win"] or []), c["win_pos0"])
    name, gt = "wn_win_decode_batch", None
    if guidance is not None:
        g = inp.guidance[[r // 2 for r in rows[0::2]]] if isinstance(guidance, str) else np.asarray(guidance, np.float32)
        assert g.shape == (U // 2,)
        gt = _framed(U // 2)
        _inner(gt).copy_(torch.from_numpy(g))
        name, args = "wn_cfg_decode_batch", args + (ptr(gt, FRAME),)
    torch.cuda.synchronize()
    capfd.readouterr()
    os.environ["WN_DEC_VERBOSE"] = "1"
    try:
        call(name, *args, _lib.stream())
        torch.cuda.synchronize()
    finally:
        del os.environ["WN_DEC_VERBOSE"]
    m = tk.RAN.search(capfd.readouterr().err)
    assert m, "no WN_DEC_VERBOSE line"
    want = tk._route(dict(c, U=U), n)
    if m.group(1) is not None:
        ran = ("mf", bool(int(m.group(5))), int(m.group(6)), int(m.group(4)), int(m.group(7)), int(m.group(1)))
        assert (int(m.group(2)), int(m.group(3)), int(m.group(8))) == (U, n, 1)
    else:
        ran = ("k",) + want[1:]
        assert (int(m.group(9)), int(m.group(10)), int(m.group(11))) == (U, n, 1)
    assert ran == want and ran[0] == ("mf" if c["fam"] == "mf" else "k"), (c["id"], ran, want)
    assert _frames_ok(probs) and _frames_ok(codes, SENT) and _frames_ok(note_out) and _frames_ok(prev_out) and _frames_ok(st.rings)
    assert gt is None or (_frames_ok(gt) and _bits(_inner(gt).cpu().numpy(), g)), "the guidance table"
    assert bool((sync[U * gran:] == -12345).all()), "the hand-off area's frame"
    assert bool((sync[:U * gran].view(U, gran)[:, -1] == 0).all()), "an error flag is set"
    assert np.isnan(st.ring_host()[:, st.ring_floats:]).all(), "the slack between the rows' rings"
    out = dict(probs=_inner(probs).view(U, n, Q).cpu().numpy(), codes=_inner(codes).view(U, n).cpu().numpy(),
               note_out=_inner(note_out).view(U, Q).cpu().numpy(), prev_out=_inner(prev_out).view(U, k - 1, Q).cpu().numpy(), form=ran)
    assert not np.isnan(out["probs"]).any() and (out["codes"] != SENT).all(), "a row was left unwritten"
    return out


def _share(section, what, err, bar):
    s = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    WORST[(section, what)] = max(WORST.get((section, what), 0.0), s)
    print("  %-22s %-6s error %.3e  bar %.3e  share %.3f" % (section, what, err, bar, s))
    return s


def _pairs_equal(out):
    """both members of every pair carry the pair's code, distribution and input columns"""
    assert np.array_equal(out["codes"][0::2], out["codes"][1::2]), "the members' codes_out rows differ"
    assert _bits(out["probs"][0::2], out["probs"][1::2]), "the members' probs_out rows differ"
    assert np.array_equal(out["note_out"][0::2], out["note_out"][1::2]) and np.array_equal(out["prev_out"][0::2], out["prev_out"][1::2])


@pytest.mark.parametrize("cid", cr.IDS)
def test_launch(cid, capfd):
    c, inp, w = cr.CASE[cid], inputs(cid), weights(cid)
    n, U = c["n"], c["U"]
    rows = list(range(U))
    st = State(inp, w)
    out = launch(inp, w, st, capfd)
    fam = out["form"][0]
    sec = tk._section(out["form"])
    print("%s: %s" % (cid, tk._form_name(out["form"])))
    _pairs_equal(out)
    ref, err = refs(cid)
    if c["free"]:       # the kernel ran on its own codes: they are the float64 roll-out's (its margins: tests/test_cfg_ref.py)
        assert np.array_equal(out["codes"][0::2], ref["codes"]), (out["codes"][0::2], ref["codes"])
    tk.check_exact(c, dict(probs=out["probs"][0::2], codes=out["codes"][0::2]))
    e = dr.prob_err(out["probs"][0::2].astype(np.float64), ref["probs"])
    assert _share(sec, "probs", e, dr.bar(err["probs"], fam)) <= 1.0, cid
    tk.check_rings(c, inp, w, st, ref, err, fam, n, rows, sec)          # every member's rings
    assert np.array_equal(out["note_out"], ref["note_out"]) and np.array_equal(out["prev_out"], ref["prev_out"])
    # a second launch from the same state
    st2 = State(inp, w)
    out2 = launch(inp, w, st2, capfd)
    assert _bits(out["probs"], out2["probs"]) and np.array_equal(out["codes"], out2["codes"])
    assert _bits(st.ring_host()[:, :st.ring_floats], st2.ring_host()[:, :st.ring_floats])
    # pair j of the batch = the one-pair launch of its two rows (where both run the same form)
    j = (U // 2) - 1
    if tk._route(dict(c, U=2), n) == out["form"] or fam == "k":
        st1 = State(inp, w, rows=[2 * j, 2 * j + 1])
        one = launch(inp, w, st1, capfd)
        assert one["form"] == out["form"]
        assert _bits(out["probs"][2 * j:2 * j + 2], one["probs"]) and np.array_equal(out["codes"][2 * j:2 * j + 2], one["codes"])
        assert _bits(st.ring_host()[2 * j:2 * j + 2, :st.ring_floats], st1.ring_host()[:, :st.ring_floats])
        assert np.array_equal(out["note_out"][2 * j:2 * j + 2], one["note_out"])
    else:
        assert U > 8 and out["form"][4] == 1, "only the two-group case changes its form with the pair count"
    # guidance of all ones = the even rows of the un-guided launch of the same rows, bit for bit
    st3, st4 = State(inp, w), State(inp, w)
    ones = launch(inp, w, st3, capfd, guidance=np.ones(U // 2, np.float32))
    plain = launch(inp, w, st4, capfd, guidance=None)
    assert ones["form"] == plain["form"]
    _pairs_equal(ones)
    assert _bits(ones["probs"][0::2], plain["probs"][0::2]) and np.array_equal(ones["codes"][0::2], plain["codes"][0::2])
    assert _bits(st3.ring_host()[0::2, :st.ring_floats], st4.ring_host()[0::2, :st.ring_floats])
    assert np.array_equal(ones["note_out"][0::2], plain["note_out"][0::2])
    # ... and the case's own scales are not that launch: pairs with s != 1 moved by more than the bar
    for jj, s in enumerate(inp.guidance):
        d = dr.prob_err(out["probs"][2 * jj:2 * jj + 1].astype(np.float64), np.maximum(ones["probs"][2 * jj:2 * jj + 1].astype(np.float64), 1e-300))
        assert (d > 10 * dr.bar(err["probs"], fam)) if s != 1.0 else True, (jj, s, d)


def test_one_workgroup_skip_stage_in_a_child():
    """WN_DEC_KS is read once per process: this module's matrix-core cases again in a fresh child under WN_DEC_KS=1 - the
    one-workgroup choosing site with spare pairs and at 512 skip channels.  Every case asserts its instantiation there as here."""
    e = dict(os.environ, WN_DEC_KS="1")
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_launch and mf_"], cwd=ROOT, env=e, timeout=300, capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])


def test_zz_print_worst_shares():
    """the worst observed share of its bar per section (DESIGN.md records them)"""
    for (sec, what), s in sorted(WORST.items()):
        print("worst share  %-28s %-6s %.3f" % (sec, what, s))
