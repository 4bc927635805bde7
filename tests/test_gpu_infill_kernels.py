"""GPU tests of partially forced decode in the decode kernels (music_amd/csrc/wn_decode.hip: decode_k<FW, CFG> and the chain's
feedback site of decode_duo_mfma8_k), one launch at a time (run with -m gpu).  The rule under test (include/wavenet_hip.h, wn_decode):
forced[u][s] >= 0 - the input column after step s of utterance u is that code; < 0 - it is the code the launch chose at step s.

The builders, NaN / sentinel frames, `_route` and the comparisons are those of tests/test_gpu_decode_kernels.py and
tests/test_gpu_cfg_decode_kernels.py (imported, not copied); the bars are decode_ref.bar() on the reference's own degraded forms -
there is no new number.  The float64 reference follows that module's free-running pattern: it is fed
`where(mask >= 0, mask, the kernel's own codes)`, so no top-2 margin is needed and every step is still checked by check_exact,
check_probs and check_rings.

Masks (tests/infill_ref.make_mask): a stage prefix (p % 4 < 2), alternating steps, a forced prompt of 3 steps then free, free except
the last step, and per-row masks that differ inside one group of eight (a row forced at step s next to a row free at step s).

Shapes, the smallest that reach every site: the matrix cores at 64 / 64 / 256 / 256, dilations [1, 2, 4], 8 steps with 1, 3 and 9
utterances (a partly filled group whose spare columns mirror the last row; a second group) - the split skip stage here and the
one-workgroup one again under WN_DEC_KS=1 in a child process, as the CFG module does -, 512 skip channels, filter width 3 (the s_src
history), biases, a temperature (the uniform numbers do not move with the mask), one case under WN_DEC_T0=0 in a child, one split
launch (5 + 3 steps, the second half on decode_k's 64-wide rings) on the carried state; guided pairs: 1 and 3.  decode_k: Q = 100 and
Q = 1024 under a 4-pair window table, filter widths 1, 2, 3, the Q = 256 fast pick, one guided pair.

Identities, bit for bit within one kernel form, per case and mask M:
  - the launch under M equals the fully forced launch fed M's resolved stream - probabilities, codes, rings, note_out, prev_out (THE
    test of the rule, no tolerance);
  - a second launch gives the same bits;
and per case: all -1 equals forced = NULL; row u (pair j) of the batch equals the single-row (one-pair) launch."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cfg_ref as cr
from tests import decode_ref as dr
from tests import infill_ref as ir
from tests import test_gpu_cfg_decode_kernels as ck
from tests import test_gpu_decode_kernels as tk
from tests.test_gpu_decode_kernels import State, Weights, _bits

ROOT = tk.ROOT
DIL, N8 = [1, 2, 4], 8
Q4 = cr.Q4
CASES = [
    # ---- decode_duo_mfma8_k
    tk.C("mf_u1_plain", "mf", 2, DIL, 64, 64, 256, 256, 1, N8, step0=3),
    tk.C("mf_u3_plain", "mf", 2, DIL, 64, 64, 256, 256, 3, N8, step0=2 ** 33 + 5),
    tk.C("mf_u9_win_temp", "mf", 2, DIL, 64, 64, 256, 256, 9, N8, step0=1, temp=0.8, win=[(0, 128), (128, 256), (40, 41)], win_pos0=1),
    tk.C("mf_u3_s512", "mf", 2, DIL, 64, 64, 512, 256, 3, N8, step0=7),
    tk.C("mf_u3_fw3", "mf", 3, DIL, 64, 64, 256, 256, 3, N8, step0=4),
    tk.C("mf_u9_fw3_bias", "mf", 3, DIL, 64, 64, 256, 256, 9, N8, step0=6, bias=True),
    tk.C("mf_u3_bias", "mf", 2, DIL, 64, 64, 256, 256, 3, N8, step0=5, bias=True),
    tk.C("mf_u3_split_5_3", "mf", 2, DIL, 64, 64, 256, 256, 3, N8, step0=9, split=(5, 3)),
    cr.C("cfg_mf_p1", "mf", 2, DIL, 64, 64, 256, 256, 1, N8, step0=3),
    cr.C("cfg_mf_p3_bias_win", "mf", 2, DIL, 64, 64, 256, 256, 3, N8, step0=2, bias=True, win=[(0, 128), (128, 256)], win_pos0=1),
    # ---- decode_k
    tk.C("k_q100_win", "k", 2, [1, 2, 3], 24, 40, 48, 100, 2, N8, step0=7, bias=True, win=Q4(100), win_pos0=2),
    tk.C("k_q1024_fw3_win", "k", 3, [1, 2], 32, 32, 64, 1024, 2, N8, step0=5, win=Q4(1024), win_pos0=1),
    tk.C("k_fw1_q100_temp", "k", 1, [1, 1], 16, 16, 32, 100, 2, N8, bias=True, temp=0.7),
    tk.C("k_q256_fast_pick", "k", 2, DIL, 32, 32, 64, 256, 3, N8, step0=11),
    cr.C("cfg_k_q256_p1", "k", 2, DIL, 32, 32, 64, 256, 1, N8, step0=11),
]
IDS = [c["id"] for c in CASES]
CASE = dict(zip(IDS, CASES))
GUIDED = {c["id"] for c in CASES if c["id"].startswith("cfg_")}
WORST = {}


@functools.lru_cache(maxsize=None)
def inputs(cid):
    return (cr.Inputs if cid in GUIDED else tk.Inputs)(CASE[cid])


@functools.lru_cache(maxsize=None)
def weights(cid):
    return Weights(inputs(cid).net, CASE[cid]["fam"] == "mf")


@functools.lru_cache(maxsize=None)
def stream(cid):
    """the codes the masks keep: inside every step's window, equal for the two rows of a guided pair"""
    c = CASE[cid]
    rng = np.random.default_rng(zlib.crc32(("stream " + cid).encode()))
    rows = c["U"] // 2 if cid in GUIDED else c["U"]
    s = ir.in_window_stream(rng, rows, c["n"], c["Q"], c["win"], c["win_pos0"])
    return np.repeat(s, 2, 0) if cid in GUIDED else s


def mask_of(cid, kind):
    return (ir.pair_mask if cid in GUIDED else ir.make_mask)(kind, stream(cid))


def fed_with(inp, forced, U=None):
    """the case's inputs with another `forced` (None: the NULL pointer), optionally as a launch of U rows"""
    out = type(inp).__new__(type(inp))
    out.__dict__.update(inp.__dict__)
    out.forced = None if forced is None else np.ascontiguousarray(forced, dtype=np.int32)
    if U is not None:
        out.c = dict(inp.c, U=U)
    return out


def run(cid, forced, capfd, rows=None, steps=None):
    """the case's steps from its start state under `forced` ([U][n] over ALL rows, or None), as one launch or as the launches
    `steps` on the carried state -> (the launches' outputs, the state)"""
    c, w = CASE[cid], weights(cid)
    inp = fed_with(inputs(cid), forced, None if rows is None else len(rows))
    st = State(inp, w, rows=rows)
    outs = []
    for n in steps or [c["n"]]:
        outs.append(ck.launch(inp, w, st, capfd) if cid in GUIDED else tk.launch(inp, w, st, n, capfd))
    return outs, st


def _rings(st):
    return st.ring_host()[:, :st.ring_floats]


def same_bits(a, sa, b, sb, what):
    for x, y in zip(a, b):
        assert x["form"] == y["form"], what
        assert _bits(x["probs"], y["probs"]), (what, "probs")
        assert np.array_equal(x["codes"], y["codes"]), (what, "codes")
        assert np.array_equal(x["note_out"], y["note_out"]) and np.array_equal(x["prev_out"], y["prev_out"]), (what, "note_out / prev_out")
    assert _bits(_rings(sa), _rings(sb)), (what, "rings")


def _share(section, what, err, bar):
    s = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    WORST[(section, what)] = max(WORST.get((section, what), 0.0), s)
    print("  %-24s %-6s error %.3e  bar %.3e  share %.3f" % (section, what, err, bar, s))
    return s


def against_float64(cid, outs, st, fed):
    """every step of the launches against the float64 reference fed `fed`: exact conditions, probabilities, rings, input columns"""
    c, inp, w = CASE[cid], inputs(cid), weights(cid)
    rows, guided = list(range(c["U"])), cid in GUIDED
    ref, err = fed_with(inp, fed).references()
    s0, seen_mf = 0, False
    for o in outs:
        n = o["probs"].shape[1]
        sec = tk._section(o["form"])
        # (a half on the fp32 kernel behind a matrix-core half inherits that half's state: the matrix-core bar)
        seen_mf = seen_mf or o["form"][0] == "mf"
        fam = "mf" if seen_mf else "k"
        if guided:
            assert np.array_equal(o["codes"][0::2], o["codes"][1::2]) and _bits(o["probs"][0::2], o["probs"][1::2])
            tk.check_exact(c, dict(probs=o["probs"][0::2], codes=o["codes"][0::2]), s0)
            e = dr.prob_err(o["probs"][0::2].astype(np.float64), ref["probs"][:, s0:s0 + n])
            assert _share(sec, "probs", e, dr.bar(err["probs"], fam)) <= 1.0, cid
        else:
            tk.check_exact(c, o, s0)
            tk.check_probs(c, o, ref, err, fam, rows, slice(s0, s0 + n), sec)
        s0 += n
    tk.check_rings(c, inp, w, st, ref, err, "mf" if seen_mf else "k", c["n"], rows, tk._section(outs[-1]["form"]))
    assert np.array_equal(outs[-1]["note_out"], ref["note_out"]) and np.array_equal(outs[-1]["prev_out"], ref["prev_out"])


def _codes(outs):
    return np.concatenate([o["codes"] for o in outs], 1)


@pytest.mark.parametrize("cid", IDS)
def test_masks(cid, capfd):
    c = CASE[cid]
    steps = list(c["split"]) if c["split"] else None
    print("%s" % cid)
    for kind in ir.MASKS:
        mask = mask_of(cid, kind)
        assert (mask >= 0).any() and (mask < 0).any()
        outs, st = run(cid, mask, capfd, steps=steps)
        print(" %s: %s" % (kind, ", ".join(tk._form_name(o["form"]) for o in outs)))
        fed = ir.resolve(mask, _codes(outs))
        assert np.array_equal(fed[mask >= 0], mask[mask >= 0])
        # THE rule: the launch under the mask IS the fully forced launch on the resolved stream
        full, st_full = run(cid, fed, capfd, steps=steps)
        same_bits(outs, st, full, st_full, (cid, kind, "masked against fully forced"))
        against_float64(cid, outs, st, fed)
        # a second launch
        again, st_again = run(cid, mask, capfd, steps=steps)
        same_bits(outs, st, again, st_again, (cid, kind, "second launch"))
        # the mask matters: the kept codes differ from the launch's own somewhere (one kept code per row may agree by chance)
        assert kind == "last_only" or (fed != _codes(outs)).any(), (cid, kind)


@pytest.mark.parametrize("cid", IDS)
def test_all_free_is_the_null_pointer(cid, capfd):
    c = CASE[cid]
    steps = list(c["split"]) if c["split"] else None
    free, st_free = run(cid, None, capfd, steps=steps)
    for v in (-1, -(2 ** 31)):
        m, st_m = run(cid, np.full((c["U"], c["n"]), v, np.int64), capfd, steps=steps)
        same_bits(free, st_free, m, st_m, (cid, "all", v))
    # ... and it is not the masked launch: the free run's codes are fed back, every step against float64
    against_float64(cid, free, st_free, _codes(free))


def _row_cases():
    """the cases of more than one row (pair) whose single-row launch runs the same form in THIS process: two groups of eight choose
    the one-workgroup skip stage and one row the split one, so those are compared under WN_DEC_KS=1 in the child"""
    out = []
    for i in IDS:
        c, one = CASE[i], 2 if i in GUIDED else 1
        if c["U"] > one and not c["split"] and tk._route(dict(c, U=one)) == tk._route(c):
            out.append(i)
    return out


@pytest.mark.parametrize("cid", _row_cases())
def test_batch_row_equals_single_launch(cid, capfd):
    """row u (guided: pair j) of a batch under per-row masks = the launch of that row (pair) alone, bit for bit"""
    c = CASE[cid]
    g = cid in GUIDED
    # (a sampled launch keys its uniform numbers by the row's index in the launch: row 0 is stream 0 in both)
    rows = [c["U"] - 2, c["U"] - 1] if g else [0 if c["temp"] > 0 else 1]
    mask = mask_of(cid, "per_row")
    outs, st = run(cid, mask, capfd)
    one, st1 = run(cid, mask, capfd, rows=rows)
    assert one[0]["form"] == outs[0]["form"]
    assert _bits(outs[0]["probs"][rows], one[0]["probs"]) and np.array_equal(outs[0]["codes"][rows], one[0]["codes"])
    assert _bits(_rings(st)[rows], _rings(st1)) and np.array_equal(outs[0]["note_out"][rows], one[0]["note_out"])
    assert np.array_equal(outs[0]["prev_out"][rows], one[0]["prev_out"])


def test_cases_reach_the_sites():
    """the forms the table reaches in this process and in the children (restated dispatch: tests/test_gpu_decode_kernels._route)"""
    here = {cid: tk._route(CASE[cid], t0_env=1, ks_env=-1) for cid in IDS}
    mf = {cid: f for cid, f in here.items() if f[0] == "mf"}
    assert {cid for cid in IDS if CASE[cid]["fam"] == "mf"} == set(mf)
    assert {f[4] for f in mf.values()} == {1, 4, 8} and {f[5] for f in mf.values()} == {2, 3} and {f[1] for f in mf.values()} == {False, True}
    assert all(f[2] == 1 for f in mf.values())
    assert tk._route(CASE["mf_u3_split_5_3"], 3)[0] == "k" and tk._route(CASE["mf_u3_split_5_3"], 5)[0] == "mf"
    assert all(tk._route(CASE[cid], t0_env=1, ks_env=1)[4] == 1 for cid in mf)
    assert tk._route(CASE["mf_u3_plain"], t0_env=0, ks_env=-1)[:3] == ("mf", False, 0)
    k = [f for f in here.values() if f[0] == "k"]
    assert any(f[1] == 2 and f[2] for f in k) and any(f[1] == 2 and not f[2] for f in k) and any(f[1] == 0 for f in k)
    assert {CASE[cid]["k"] for cid, f in here.items() if f[0] == "k"} == {1, 2, 3}


def _child(env, select):
    e = dict(os.environ, **env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", select], cwd=ROOT, env=e, timeout=300, capture_output=True, text=True)
    print(env, r.stdout[-600:])
    assert r.returncode == 0, (env, r.stdout[-3000:], r.stderr[-1000:])


def test_one_workgroup_skip_stage_in_a_child():
    """WN_DEC_KS is read once per process: the matrix-core cases again under WN_DEC_KS=1 - the one-workgroup skip stage with spare
    columns and at 512 skip channels, and the row identity of the two-group cases"""
    _child({"WN_DEC_KS": "1"}, "(test_masks or test_batch_row) and mf_")


def test_no_tap0_ahead_in_a_child():
    """WN_DEC_T0=0: the chain without the sample-ahead pass (load_queues in front of the feedback site)"""
    _child({"WN_DEC_T0": "0"}, "(test_masks or test_all_free) and mf_u3_plain")


def test_zz_print_worst_shares():
    for (sec, what), s in sorted(WORST.items()):
        print("worst share  %-28s %-6s %.3f" % (sec, what, s))
