"""CPU checks of classifier-free guidance: tests/cfg_ref.py against itself and the references it is built on, class_dropout.draw_null,
the conditions the GPU tests' cases rest on, and the refusals of wn_cfg_decode_batch / wn_cfg_sample_logits in the pattern of
tests/test_window_abi.py (declared, exported, bound, ABI still 9; refused arguments come back as -4 with the entry's name before
anything is launched - no device is needed, pointers are never dereferenced)."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import cfg_ref as cr
from tests import class_cond_ref as ref
from tests import decode_ref as dr
from tests.decode_args import P, decode_args
from tests.helpers import ROOT

_KEEP = []


# ================================================================================================ class_dropout.draw_null
def test_draw_null_is_a_pure_function_of_the_global_clip():
    from music_amd import class_dropout as cd, vq_dropout
    a = cd.draw_null(7, 12, 0, 64, 0.3)
    assert a.dtype == np.bool_ and a.shape == (64,)
    assert np.array_equal(a, cd.draw_null(7, 12, 0, 64, 0.3))
    # any shard split of the global batch draws the same clips
    for cuts in ([32], [1, 2, 40], [8, 16, 24, 32, 40, 48, 56], list(range(1, 64))):
        edges = [0] + cuts + [64]
        parts = [cd.draw_null(7, 12, lo, hi - lo, 0.3) for lo, hi in zip(edges[:-1], edges[1:])]
        assert np.array_equal(np.concatenate(parts), a), cuts
    # another step, another seed: other draws; p = 0 and p = 1 are certain; an empty batch is empty
    assert not np.array_equal(a, cd.draw_null(7, 13, 0, 64, 0.3)) and not np.array_equal(a, cd.draw_null(8, 12, 0, 64, 0.3))
    assert not cd.draw_null(1, 2, 3, 100, 0.0).any() and cd.draw_null(1, 2, 3, 100, 1.0).all()
    assert cd.draw_null(1, 2, 3, 0, 0.5).shape == (0,)
    # a larger p drops a superset (one uniform per clip, compared with p)
    assert (cd.draw_null(7, 12, 0, 64, 0.6) | ~a).all()
    # its own domain: not the clips quantiser dropout draws for under the same seed, step and p
    st = vq_dropout.draw_stages(7, 12, 0, 4096, 4, 0.3) < 4
    mine = cd.draw_null(7, 12, 0, 4096, 0.3)
    assert abs(float(np.corrcoef(st, mine)[0, 1])) < 0.1
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=True), dict(B=-1), dict(step=-1), dict(first_clip=-2)):
        kw = dict(seed=0, step=0, first_clip=0, B=4, p=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            cd.draw_null(**kw)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_draw_null_drops_a_share_p(p):
    """n = 20000 clips over 50 steps: the count lies within 5 standard deviations of the binomial's mean (a fair draw fails this
    once in 1.7 million), and so does every step's own count of 400"""
    from music_amd import class_dropout as cd
    steps, B = 50, 400
    draws = np.stack([cd.draw_null(3, t, 0, B, p) for t in range(steps)])
    n = steps * B
    assert abs(draws.sum() - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert (np.abs(draws.sum(1) - B * p) <= 5 * math.sqrt(B * p * (1 - p))).all()
    assert (np.abs(draws.sum(0) - steps * p) <= 5 * math.sqrt(steps * p * (1 - p)) + 1).all()       # per clip index, over the steps


def test_apply_and_options():
    from music_amd import class_dropout as cd
    cls = [3, 1, 4, 1, 5, 2, 6, 5]
    drop = cd.draw_null(9, 4, 16, 8, 0.5)
    want = [0 if d else c for c, d in zip(cls, drop)]
    assert cd.apply(cls, 0, 9, 4, 16, 0.5) == want and cls == [3, 1, 4, 1, 5, 2, 6, 5]
    t = torch.tensor(cls, dtype=torch.int32)
    got = cd.apply(t, 0, 9, 4, 16, 0.5)
    assert got.dtype == torch.int32 and got.tolist() == want and t.tolist() == cls
    assert cd.apply(cls, 0, 9, 4, 16, 0.0) == cls and cd.apply(cls, 7, 9, 4, 16, 1.0) == [7] * 8
    assert cd.options({}, None) is None and cd.options({}, 3) is None
    assert cd.options({"class_dropout": 0.25}, 3) == (0.25, 0) and cd.options({"class_dropout": 1, "class_dropout_seed": 5}, 0) == (1.0, 5)
    for bad, null in (({"class_dropout": 0.2}, None), ({"class_dropout": 1.5}, 2), ({"class_dropout": "x"}, 2), ({"class_dropout": True}, 2),
                      ({"class_dropout_seed": 4}, 2), ({"class_dropout": 0.5, "class_dropout_seed": 1.5}, 2)):
        with pytest.raises(ValueError):
            cd.options(bad, null)


def test_null_class_is_a_model_argument_without_parameters():
    from music_amd.model import wavenet
    cfg = dict(ref.DECODE_CASES["fp32"]["cfg"])
    torch.manual_seed(0)
    a = wavenet(**cfg)
    torch.manual_seed(0)
    b = wavenet(null_class=2, **cfg)
    assert a.null_class is None and b.null_class == 2
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    b.load_state_dict(sa)                                   # checkpoints load both ways
    a.load_state_dict(sb)
    for bad in (3, -1, True, 1.0):
        with pytest.raises(ValueError, match="null_class"):
            wavenet(null_class=bad, **cfg)
    plain = {k: v for k, v in cfg.items() if not k.startswith("global")}
    with pytest.raises(ValueError, match="null_class"):
        wavenet(null_class=0, **plain)


# ================================================================================================ the reference against itself
def test_combine_is_the_rule():
    rng = np.random.default_rng(0)
    lc, lu = rng.standard_normal((5, 9)), rng.standard_normal((5, 9))
    s = np.array([0.0, 1.0, 1.5, 3.0, -0.5])
    g = cr.combine(lc, lu, s)
    assert np.allclose(g[0], lu[0], rtol=0, atol=1e-15)
    assert np.array_equal(g[1], lc[1])
    assert np.allclose(g, s[:, None] * lc - (s[:, None] - 1) * lu, rtol=0, atol=1e-14)
    assert cr.amp(s) == 5.0 and cr.amp([1.0]) == 1.0 and cr.amp([-0.5]) == 2.0


@functools.lru_cache(maxsize=None)
def _case_refs(cid):
    inp = cr.Inputs(cr.CASE[cid])
    return inp, inp.references()


@pytest.mark.parametrize("cid", ["mf_p1_free", "k_q100_p4_win", "k_fw1_q100_p2"])
def test_guided_ref_at_scale_one_is_decode_ref_on_the_conditional_rows(cid):
    """s = 1 everywhere: the pairs' distributions, codes and the conditional members' rings are decode_ref's for those rows alone,
    fed the same codes - and at s = 0 the unconditional members'"""
    c = cr.CASE[cid]
    inp = cr.Inputs(c)
    n, U = c["n"], c["U"]
    for s, member in ((1.0, 0), (0.0, 1)):
        g = cr.guided_ref(inp.net, inp.rings, inp.note0, inp.prev0, n, [s] * (U // 2), **inp.kw())
        fed = np.repeat(g["codes"], 2, 0) if inp.forced is None else inp.forced
        rows = slice(member, U, 2)
        cond = dict(inp.cond, fg=inp.cond["fg"][rows], p1=inp.cond["p1"][rows])
        o = dr.decode_ref(inp.net, [r[rows] for r in inp.rings], inp.note0[rows], inp.prev0[rows] if c["k"] > 1 else None, n,
                          step0=c["step0"], forced=fed[rows], cond=cond, temperature=c["temp"], windows=c["win"], win_pos0=c["win_pos0"])
        assert np.abs(g["probs"] - o["probs"]).max() < 1e-12 and np.array_equal(g["codes"], o["codes"])
        assert all(np.abs(a[rows] - b).max() < 1e-12 for a, b in zip(g["rings"], o["rings"]) if b.size)    # (a BLAS sums per batch shape)
        assert np.array_equal(g["note_out"][0::2], g["note_out"][1::2]) and np.array_equal(g["prev_out"][0::2], g["prev_out"][1::2])


@pytest.mark.parametrize("cid", cr.IDS)
def test_launch_cases_rest_on_their_conditions(cid):
    """what tests/test_gpu_cfg_decode_kernels.py assumes of a case, from the references alone: free-running cases keep a float64
    top-2 margin of g above 1e-4 (|s| + |s - 1|) at every step, the guided distribution differs from the conditional member's
    wherever s != 1, no reference probability is under 1e-30, and the loss of the f16 lo halves is several bars away"""
    c = cr.CASE[cid]
    inp, (r, err) = _case_refs(cid)
    fam = c["fam"]
    assert c["U"] % 2 == 0 and c["cond"] is not None and c["push"] == 1
    if c["free"]:
        need = 1e-4 * cr.amp(inp.guidance)
        print("  %s: smallest top-2 margin of g %.3e (needs %.1e)" % (cid, r["margin"], need))
        assert c["temp"] <= 0 and r["margin"] > need
    assert r["probs"][r["probs"] > 0].min() > 1e-30           # (nothing near float32's subnormals: relative errors stay meaningful)
    plain = cr.guided_ref(inp.net, inp.rings, inp.note0, inp.prev0, c["n"], [1.0] * (c["U"] // 2),
                          **inp.kw(np.repeat(r["codes"], 2, 0) if inp.forced is None else None))
    bar = dr.bar(err["probs"], fam)
    for j, s in enumerate(inp.guidance):
        d = dr.prob_err(r["probs"][j:j + 1], plain["probs"][j:j + 1])
        assert (d == 0) if s == 1.0 else (d > 100 * bar), (j, s, d, bar)
    if fam == "mf":
        assert err["probs"]["ex1"] > 8 * bar, (err["probs"], bar)


# ================================================================================================ the model-level cases
@pytest.mark.parametrize("name", sorted(ref.DECODE_CASES))
def test_model_cases_keep_their_margin(name):
    """the greedy guided roll-outs of tests/test_gpu_cfg_decode.py: every utterance's float64 top-2 margin of g stays above
    1e-4 (|s| + |s - 1|), plain and under the stage windows - so a decoder inside the project's bar picks the same codes"""
    case = cr.model_case(name)
    cfg = case["cfg"]
    assert cfg["null_class"] not in case["classes"]
    net = ref.build(cfg, case["seed"])
    Q, U = cfg["quantization_channels"], len(case["classes"])
    seeds = ref.seed_codes(U, net.receptive_field, Q, case["seed"])
    params = {k: v.detach() for k, v in net.state_dict().items()}
    for win in (None, [(0, Q // 2), (Q // 2, Q)]):
        codes, margin = cr.guided_rollout(params, cfg["dilations"], seeds, case["classes"], cfg["null_class"], case["guidance"],
                                          case["steps"], Q, cfg["filter_width"], windows=win, pos0=0)
        need = np.array([1e-4 * cr.amp([s]) for s in case["guidance"]])
        print("  %s %s: margins %s need %s" % (name, "windowed" if win else "plain", margin, need))
        assert (margin > need).all()
    # guidance changes what is generated: some utterance with s != 1 leaves the conditional roll-out
    plain, _ = ref.greedy_rollout(params, cfg["dilations"], seeds, torch.tensor(case["classes"]), case["steps"], Q, cfg["filter_width"])
    codes, _ = cr.guided_rollout(params, cfg["dilations"], seeds, case["classes"], cfg["null_class"], case["guidance"], case["steps"], Q,
                                 cfg["filter_width"])
    for u, s in enumerate(case["guidance"]):
        if s == 1.0:
            assert torch.equal(codes[u], plain[u])
    assert not torch.equal(codes, plain)


# ================================================================================================ the entries on the CPU
def _lib():
    from music_amd import _lib
    lib = _lib.load()
    assert lib.wn_version() == _lib.ABI_VERSION == 9
    return lib


def _table(pairs):
    if pairs is None:
        return None
    t = (ctypes.c_int32 * max(1, 2 * len(pairs)))(*[v for pr in pairs for v in pr])
    _KEEP.append(t)
    return ctypes.cast(t, ctypes.c_void_p)


def _args(win=((0, 128), (128, 256)), period=None, win_pos0=0, guidance=P, **over):
    """wn_decode_batch_samp's arguments without the stream, the three window arguments, guidance, the stream"""
    return decode_args("wn_decode_batch_samp", **{"temperature": 1.0, "n_utt": 2, **over})[:-1] + [
        _table(win), (len(win) if win is not None else 0) if period is None else period, win_pos0, guidance, None]


def _refused(lib, what, **kw):
    rc = lib.wn_cfg_decode_batch(*_args(**kw))
    msg = lib.wn_last_error().decode()
    assert rc == -4 and what in msg, (kw, rc, msg)
    return msg


def _header():
    src = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _names(code, fn):
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % fn, code, flags=re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in decl.split(",")]


def test_entries_are_declared_exported_and_bound_and_the_abi_is_still_9():
    from music_amd import _lib
    src, code = _header()
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    p = ctypes.c_void_p
    for name in ("wn_cfg_decode_batch", "wn_cfg_sample_logits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code) and hasattr(raw, name), name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name]
        assert not name.startswith("wn_decode")
    sig = _lib.SIGNATURES["wn_win_decode_batch"]
    assert _lib.SIGNATURES["wn_cfg_decode_batch"] == sig[:-1] + [p] + sig[-1:]
    assert _names(code, "wn_cfg_decode_batch") == _names(code, "wn_win_decode_batch")[:-1] + ["guidance", "stream"]
    sig = _lib.SIGNATURES["wn_win_sample_logits"]
    assert _lib.SIGNATURES["wn_cfg_sample_logits"] == sig[:-1] + [p, p] + sig[-1:]
    base = _names(code, "wn_win_sample_logits")
    assert _names(code, "wn_cfg_sample_logits") == ["logits_c"] + base[1:-1] + ["logits_u", "guidance", "stream"]
    # the entries they extend keep their signatures
    assert len(_lib.SIGNATURES["wn_win_decode_batch"]) == 55 and len(_lib.SIGNATURES["wn_win_sample_logits"]) == 17
    assert "CLASSIFIER-FREE GUIDANCE" in src and "g_i = l_c,i + (s - 1) (l_c,i - l_u,i)" in src


def test_guidance_is_refused_by_name():
    lib = _lib()
    for kw in (dict(), dict(top_k=5, top_p=0.9), dict(samp=P), dict(win=None)):
        for n_utt in (1, 3, 7, 1023):
            msg = _refused(lib, "'n_utt'", n_utt=n_utt, **kw)
            assert msg.startswith("wn_cfg_decode_batch:") and "'guidance'" in msg and "even" in msg
        msg = _refused(lib, "'guidance'", cond_fg=None, cond_p1=None, **kw)
        assert msg.startswith("wn_cfg_decode_batch:") and "'cond_fg'" in msg
    # refused whether or not there is work to do; one table is enough
    _refused(lib, "'n_utt'", n_utt=3, n_steps=0)
    _refused(lib, "'guidance'", cond_fg=None, cond_p1=None, n_steps=0)
    assert lib.wn_cfg_decode_batch(*_args(n_steps=0, cond_fg=None)) == 0
    assert lib.wn_cfg_decode_batch(*_args(n_steps=0, cond_p1=None)) == 0
    assert lib.wn_cfg_decode_batch(*_args(n_utt=0)) == 0 and lib.wn_cfg_decode_batch(*_args(n_steps=0)) == 0
    # without a table the entry is wn_win_decode_batch: odd counts and unconditioned launches are its business
    assert lib.wn_cfg_decode_batch(*_args(guidance=None, n_utt=3, n_steps=0)) == 0
    assert lib.wn_cfg_decode_batch(*_args(guidance=None, n_utt=1, n_steps=0, cond_fg=None, cond_p1=None)) == 0


def test_everything_the_windowed_entry_refuses():
    lib = _lib()
    for guidance in (P, None):
        kw = dict(guidance=guidance)
        for what, bad in (("'win_period'", dict(period=-1)), ("'win_period'", dict(period=17)), ("'win_host'", dict(win=None, period=2)),
                          ("'win_host'", dict(win=((0, 128), (-1, 4)))), ("'win_host'", dict(win=((0, 257),))),
                          ("'win_host'", dict(win=((9, 3),))), ("'win_pos0'", dict(win_pos0=-1)),
                          ("'top_p'", dict(top_p=float("nan"))), ("'top_p'", dict(top_p=-0.25)), ("'top_k'", dict(top_k=-1)),
                          ("le (columns", dict(le=0)), ("c_shift_host", dict(c_shift=None)), ("c_q_host", dict(c_q=None)),
                          ("filter_width", dict(filter_width=0)), ("quantisation", dict(Q=4096)), ("quantisation", dict(Q=0)),
                          ("layers", dict(n_layers=65)), ("layers", dict(n_layers=0)), ("'dilations_host'", dict(dil=None)),
                          ("LDS", dict(filter_width=4, R=16384, D=16384))):
            _refused(lib, what, **bad, **kw)
        for fw in (1, 2, 3):
            assert "corrected recurrence" in _refused(lib, "push_input", filter_width=fw, push_input=0, **kw)
        for arg in ("note0", "prev0", "note_out", "prev_out", "codes_out", "queues", "w_causal", "w_layers", "w_p1", "w_p2", "sync"):
            _refused(lib, "'%s'" % arg, **dict(kw, **{arg: None}))
        assert _refused(lib, "le (columns", le=0, **kw).startswith("wn_cfg_decode_batch:")


def _sample(lib, win=((0, 128), (128, 256)), period=None, win_pos0=0, logits_u=P, guidance=P, **over):
    a = dict(logits=P, n=4, Q=256, ld=256, samp=None, temperature=1.0, seed=0, top_k=0, top_p=1.0, step0=0, u=None, codes=P,
             probs=None)
    a.update(over)
    rc = lib.wn_cfg_sample_logits(*a.values(), _table(win), (len(win) if win is not None else 0) if period is None else period,
                                  win_pos0, logits_u, guidance, None)
    return rc, lib.wn_last_error().decode()


def test_guided_sampler_refusals_and_no_work():
    lib = _lib()
    for guidance in (P, None):
        for what, over in (("'Q'", dict(Q=0)), ("'Q'", dict(Q=1025)), ("'n'", dict(n=-1)), ("'ld'", dict(ld=255)),
                           ("'top_p'", dict(top_p=float("nan"))), ("'top_p'", dict(top_p=-1.0)), ("'top_k'", dict(top_k=-2)),
                           ("'logits'", dict(logits=None)), ("'codes'", dict(codes=None)),
                           ("'win_period'", dict(period=-3)), ("'win_period'", dict(period=17)),
                           ("'win_host'", dict(win=None, period=1)), ("'win_host'", dict(win=((-1, 5),))),
                           ("'win_host'", dict(win=((0, 4), (4, 4)))), ("'win_pos0'", dict(win_pos0=-1)), ("'win_pos0'", dict(win_pos0=-1, n=0))):
            rc, msg = _sample(lib, guidance=guidance, **over)
            assert rc == -4 and msg.startswith("wn_cfg_sample_logits:") and what in msg, (over, rc, msg)
    rc, msg = _sample(lib, logits_u=None)
    assert rc == -4 and msg.startswith("wn_cfg_sample_logits:") and "'logits_u'" in msg, (rc, msg)
    assert _sample(lib, n=0)[0] == 0 and _sample(lib, n=0, win=None, logits_u=None, guidance=None)[0] == 0
    # the entry it extends still reports under its own name
    rc = lib.wn_win_sample_logits(P, 4, 0, 256, None, 1.0, 0, 0, 1.0, 0, None, P, None, None, 0, 0, None)
    assert rc == -4 and lib.wn_last_error().decode().startswith("wn_win_sample_logits:")


# ================================================================================================ the Python side, no device
def test_decode_call_picks_the_guided_entry_only_with_a_table():
    from music_amd import _lib, fast_generate as fg

    class Smp:
        plain, temperature, seed = True, 0.0, 0

        def tail(self):
            return (None, 0, 1.0)
    base = ((2, 3, 64, 64, 256, 256), 1, 2, 3, (0,) * 9, (0,) * 7, 0, 4, 1, 5, 2, 0, Smp(), (None, 0, 0, 0, -1, -1, -1))
    cond = (1, 2, 3, 4, 5, 6, 1, 0)
    for win in (None, (7, 2, 5)):
        name, args = fg._decode_call(*base, cond, win, 99)
        assert name == "wn_cfg_decode_batch" and len(args) + 1 == len(_lib.SIGNATURES[name]) and args[-1] == 99
        assert args[-4:-1] == (win if win is not None else (None, 0, 0))
        plain, pargs = fg._decode_call(*base, cond, win)
        assert plain == ("wn_win_decode_batch" if win else "wn_decode_batch_cond")
        assert args[:len(pargs)] == pargs


def test_guidance_argument_is_checked_before_any_launch():
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    cfg = dict(ref.DECODE_CASES["fp32"]["cfg"])
    with_null, without = wavenet(null_class=2, **cfg), wavenet(**cfg)
    plain = wavenet(**{k: v for k, v in cfg.items() if not k.startswith("global")})
    assert fg._guidance_of(with_null, None, 3, False, None) is None
    assert fg._guidance_of(with_null, 1.5, 3, True, [0, 1, 0]) == [1.5] * 3
    assert fg._guidance_of(with_null, torch.tensor([0.0, 1.0, -2.0]), 3, True, [0, 1, 0]) == [0.0, 1.0, -2.0]
    with pytest.raises(ValueError, match="null_class"):
        fg._guidance_of(without, 1.5, 3, True, [0, 1, 0])
    with pytest.raises(ValueError, match="corrected recurrence"):
        fg._guidance_of(with_null, 1.5, 3, False, [0, 1, 0])
    with pytest.raises(ValueError, match="global_classes"):
        fg._guidance_of(plain, 1.5, 3, True, None)
    with pytest.raises(ValueError, match="global_classes"):
        fg._guidance_of(with_null, 1.5, 3, True, None)
    for bad in ([1.0, 2.0], float("nan"), float("inf"), "2", [1.0, None, 2.0], True):
        with pytest.raises(ValueError, match="guidance"):
            fg._guidance_of(with_null, bad, 3, True, [0, 1, 0])
