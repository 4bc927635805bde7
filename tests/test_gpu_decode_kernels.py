"""GPU tests of the decode kernels (music_amd/csrc/wn_decode.hip), one launch at a time, against float64 (run with -m gpu).

The rules of tests/test_gpu_fwd_kernels.py and tests/test_gpu_block_kernels.py, for decode_k<2>, decode_k<0> and every launch
form of decode_duo_mfma8_k<BIAS, T0, S, KS, KT>:
  - the test builds the decode-layout float32 weight buffer and (matrix-core cases) the packed fragments ITSELF, from explicit
    matrices, by the layout text of include/wavenet_hip.h (pack_index + wn_pack_weights as the other kernel tests), and launches ONE
    entry through _lib.call; test_decode_pack_builds_the_same_buffers holds fast_generate._DecodePack to the same bytes;
  - every utterance of a launch has its own random rings, one-hot note0 / prev0, forced codes and conditioning tables, and is
    compared with ITS float64 reference (tests/decode_ref.py, written from the header alone);
  - the rings (queues_ustride leaves slack between the utterances), note_out, prev_out, probs_out, codes_out and the hand-off
    area lie between NaN / sentinel frames that must survive; the blocks of the weight buffer are layer_stride apart with NaN
    between them, the sections of the buffer and the utterances' conditioning tables are separated by NaN, table columns the
    schedule never reaches are NaN; ring slots the launch's steps do not reach keep their bits; padded channels stay exactly 0.
    (note0 / prev0 / note_out / prev_out / forced / codes_out / probs_out have the fixed per-utterance strides of the header.)
  - exact, no case excused: codes_out[s] is the first-index argmax of the kernel's own probs_out[s] inside the step's window
    (greedy launches); probabilities outside the window are exact zeros; note_out / prev_out are the one-hot columns of the
    reference; every error-flag word is 0; a repeated launch from the same state gives the same bits; a row of a batch equals
    the single-utterance launch in the same form;
  - against float64: probabilities as RELATIVE error |p / p64 - 1| over all entries, rings in units of max(1, max |ref|).
  - every case asserts the instantiation it ran, from the launcher's own WN_DEC_VERBOSE line (read per launch) and `_route`,
    this module's restatement of wn_launch_decode's dispatch; test_cases_reach_every_form lists the forms the table reaches.

Bars: none is a new constant.  Per case and compared tensor decode_ref supplies e32 = |ref32 - ref64| and ex3 = |refx3 - ref64|
on the comparison's scale: fp32 kernels 8 e32, matrix-core kernels 4 ex3 + 8 e32 (decode_ref.bar).  tests/test_decode_ref.py
proves for every case, from the references alone, that the loss of the f16 lo halves (refx1) is at least 16 bars away, that no
reference probability is under 1e-6 and no logit over 8.
Observed worst share of its bar on an MI355X (test_zz_print_worst_shares prints them): decode_k probabilities 0.58, rings 0.18;
matrix-core forms probabilities 0.14 - 0.19, rings 0.08 - 0.15.

Cases are teacher-forced except one free-running greedy case per kernel family, whose reference is fed the kernel's own
emitted codes - every step is still checked.  WN_DEC_T0 / WN_DEC_KS are cached per process: test_cached_switches_in_children
runs this module's matrix-core cases in fresh child processes, one after another, under WN_DEC_T0=0, WN_DEC_KS=1 and
WN_DEC_KS=8 (this process serves T0 1 / 2, KS 4 at one pair, KS 1 at 256 skip channels with 9 or more utterances, KS 8 at 512)."""
import ctypes
import functools
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from music_amd import _lib
from music_amd._lib import call, ptr
from tests import decode_ref as dr

DEV = "cuda"
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0_ENV = int(os.environ.get("WN_DEC_T0", "1"))          # what wn_launch_decode caches on its first call
KS_ENV = int(os.environ.get("WN_DEC_KS", "-1"))
FRAME = 64                                               # floats of NaN in front of and behind every output buffer
GAP = 16                                                 # floats of NaN between the sections of the weight buffer
SENT = -77                                               # codes_out frame


# ================================================================================================ the case table
def C(id, fam, k, dil, R, D, S, Q, U, n, step0=0, push=1, bias=False, cond=None, temp=0.0, win=None, free=False, split=None,
      win_pos0=0):
    """fam 'k': the fp32 kernel's own shapes (no pk); fam 'mf': a matrix-core state (rings, weights and tables padded to 64
    channels, pk handed over) - which a launch of fewer than four steps, or a switched-off form, still runs on decode_k.
    cond: dict(shift, q, le, pos0, fg=bool, p1=bool); split: (n1, n2) - the n = n1 + n2 steps also as two launches."""
    return dict(id=id, fam=fam, k=k, dil=list(dil), R=R, D=D, S=S, Q=Q, U=U, n=n, step0=step0, push=push, bias=bias, cond=cond,
                temp=temp, win=win, free=free, split=split, win_pos0=win_pos0)


BIG = 2 ** 33 + 11                                       # a ring position past 2^32 that is no multiple of any L below
CASES = [
    # ---- decode_k: dec_matvec edges, both instantiations with Q = 256 and Q != 256
    # R = 8: 64 lanes share one output, K below the lane group; rings [1, 2, 4] wrap more than once, L = 32 is partly overwritten
    C("k_r8_wrap_partial_bigstep", "k", 2, [1, 2, 4, 32], 8, 16, 64, 256, 3, 20, step0=BIG, bias=True),
    # nothing divides the thread count; the as-written recurrence (push_input = 0)
    C("k_r24_d40_s48_q100_aswritten", "k", 2, [1, 2, 3], 24, 40, 48, 100, 2, 16, step0=7, push=0),
    # any-width instantiation at Q = 256, conditioned: priming columns (pos0 < 0), a stretch schedule past le - 1, tile wrapping
    C("k_fw3_q256_cond_win", "k", 3, [1, 2, 4], 32, 32, 64, 256, 2, 20, step0=1000003, bias=True,
      cond=dict(shift=[5, 3, 1, 0], q=[4, 0, 2, 3], le=5, pos0=-7, fg=True, p1=True), win=[(0, 100), (100, 256), (31, 32)], win_pos0=2),
    # k = 1: no rings, prev0 NULL (the probabilities carry the comparison); Q = 1: every probability is 1 (the rings carry it)
    C("k_fw1_q100_no_rings", "k", 1, [1, 1], 16, 16, 32, 100, 2, 12, bias=True),
    C("k_q1", "k", 2, [1, 2], 16, 16, 32, 1, 2, 12, step0=3, bias=True),
    # more than 64 KB of dynamic LDS; S = 1100 outputs > 1024 threads (a second pass of the row loop); Q = 1024
    C("k_fw12_s1100_q1024_raised_lds", "k", 12, [1, 2], 64, 64, 1100, 1024, 2, 12, step0=5),
    C("k_free_running", "k", 2, [1, 2, 4], 32, 32, 64, 256, 3, 24, free=True),
    C("k_temperature_q100", "k", 2, [1, 2], 32, 32, 64, 100, 2, 12, temp=0.7, bias=True),
    C("k_fw4_q100_split_launch", "k", 4, [1, 3], 24, 40, 48, 100, 2, 12, step0=13, split=(5, 7)),
    # ---- decode_duo_mfma8_k
    C("mf_k2_s256_u1_wrap_partial_bigstep", "mf", 2, [1, 2, 4, 32], 64, 64, 256, 256, 1, 20, step0=BIG),
    C("mf_k2_s256_u9_pad32_bias_aswritten", "mf", 2, [1, 2, 4], 32, 32, 256, 256, 9, 12, step0=5, push=0, bias=True),
    C("mf_k2_s512_u8_32blocks_4steps", "mf", 2, [1, 2] * 16, 64, 64, 512, 256, 8, 4, step0=3),
    C("mf_k3_s256_u17_bias_win", "mf", 3, [1, 2, 4], 64, 64, 256, 256, 17, 12, step0=BIG, bias=True,
      win=[(0, 128), (128, 256)], win_pos0=1),
    C("mf_k4_s512_u2", "mf", 4, [1, 2, 4, 8], 64, 64, 512, 256, 2, 16, step0=17),
    C("mf_k3_s256_u1_32blocks_bias", "mf", 3, [1, 2] * 16, 64, 64, 256, 256, 1, 6, step0=9, bias=True),
    C("mf_k4_s256_u9_32blocks_cond", "mf", 4, [1, 2] * 16, 32, 32, 256, 256, 9, 6, step0=2,
      cond=dict(shift=[(3 * i) % 7 for i in range(33)], q=[(i % 3) * 2 for i in range(33)], le=4, pos0=-2, fg=True, p1=True)),
    C("mf_k2_s512_u3_cond_stretch_tile", "mf", 2, [1, 2, 4], 64, 64, 512, 256, 3, 20, step0=11,
      cond=dict(shift=[5, 3, 1, 0], q=[4, 0, 2, 3], le=5, pos0=-7, fg=True, p1=True)),
    C("mf_k2_s256_u2_cond_fg_only", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 2, 12, bias=True,
      cond=dict(shift=[2, 1, 0, 0], q=[0, 3, 0, 1], le=3, pos0=0, fg=True, p1=False)),
    C("mf_k3_s256_u2_cond_p1_only_le1", "mf", 3, [1, 2, 4], 64, 64, 256, 256, 2, 12,
      cond=dict(shift=[0, 0, 0, 4], q=[0, 0, 0, 0], le=1, pos0=3, fg=False, p1=True)),
    C("mf_free_running", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 8, 16, free=True),
    # a matrix-core state, 3 steps: decode_k on the 64-wide padded rings; its state carried into a 5-step matrix-core launch
    C("mf_fallback_3_steps_then_5", "mf", 2, [1, 2, 4], 32, 32, 256, 256, 2, 8, step0=6, bias=True, split=(3, 5)),
    C("mf_k3_split_launch", "mf", 3, [1, 2, 4], 64, 64, 256, 256, 3, 12, step0=4, split=(5, 7)),
]
IDS = [c["id"] for c in CASES]
CASE = dict(zip(IDS, CASES))


# ================================================================================================ wn_launch_decode's dispatch, restated
def _t0_fits_lds(n_layers):
    return 4 * (16 * 256 + 16 * 64) + 2 * (8 * 136 * (3 + 4)) + n_layers * 256 * 16 + 1024 <= 160 * 1024


def _route(c, n_steps=None, t0_env=None, ks_env=None):
    """The kernel instantiation wn_launch_decode runs for a launch of case `c` (sync always holds wn_decode_sync_granules words
    per utterance here): ('mf', BIAS, T0, S, KS, KT) or ('k', FW template value, Q == 256, dynamic LDS above 64 KB)."""
    t0_env = T0_ENV if t0_env is None else t0_env
    ks_env = KS_ENV if ks_env is None else ks_env
    n = c["n"] if n_steps is None else n_steps
    k, N, S, Q, U = c["k"], len(c["dil"]), c["S"], c["Q"], c["U"]
    cond = c["cond"] is not None
    R = D = 64
    if c["fam"] == "mf":
        mf_taps = k == 2 or (k in (3, 4) and t0_env != 0)
        cond_ok = not cond or t0_env != 0
        if mf_taps and cond_ok and n >= 4 and S in (256, 512) and Q == 256:
            t0 = 0 if not t0_env else (1 if _t0_fits_lds(N) else 2)
            pairs, ks_full = (U + 7) // 8, S // 64
            fits = pairs * (1 + ks_full) <= 224
            want = ks_env > 1 or (ks_env < 0 and (S == 512 or pairs <= 1))
            return ("mf", bool(c["bias"] or cond), t0, S, ks_full if (fits and want) else 1, k)
    else:
        R, D = c["R"], c["D"]
    lds = 4 * ((k + 1) * Q + (k + 1) * R + 3 * D + 2 * S + 64)
    return ("k", 2 if k == 2 else 0, Q == 256, lds > 64 * 1024)


def _launches(c):
    """the step counts this module launches case `c` with"""
    return [c["n"]] + (list(c["split"]) if c["split"] else [])


def forms_reached(t0_env=1, ks_env=-1):
    """{instantiation: [case ids]} over the table under the given switches, plus the conditioned cases' forms"""
    out, cond = {}, set()
    for c in CASES:
        for n in _launches(c):
            f = _route(c, n, t0_env, ks_env)
            out.setdefault(f, []).append(c["id"])
            if c["cond"] is not None:
                cond.add(f)
    return out, cond


def check_forms():
    """Every form the issue names is reached: in this process (default switches) or in the children of
    test_cached_switches_in_children (WN_DEC_T0=0, WN_DEC_KS=1, WN_DEC_KS=8).  Returns the listing."""
    dflt, dcond = forms_reached()
    t0off, _ = forms_reached(t0_env=0)
    ks1, _ = forms_reached(ks_env=1)
    ks8, _ = forms_reached(ks_env=8)
    every = set(dflt) | set(t0off) | set(ks1) | set(ks8)
    kf = [f for f in dflt if f[0] == "k"]
    for fw in (2, 0):
        assert any(f[1] == fw and f[2] for f in kf) and any(f[1] == fw and not f[2] for f in kf), ("decode_k", fw)
    assert any(f[3] for f in kf), "decode_k raised-LDS branch"
    # a matrix-core state of fewer than four steps on decode_k with 64-wide rings
    assert _route(CASE["mf_fallback_3_steps_then_5"], 3)[0] == "k" and _route(CASE["mf_fallback_3_steps_then_5"], 5)[0] == "mf"
    mf = [f for f in every if f[0] == "mf"]
    here = [f for f in dflt if f[0] == "mf"]
    for t0, kt in [(0, 2), (1, 2), (2, 2), (1, 3), (2, 3), (1, 4), (2, 4)]:
        assert any(f[2] == t0 and f[5] == kt for f in mf), ("T0, KT", t0, kt)
        if t0:
            assert any(f[2] == t0 and f[5] == kt for f in here), ("T0, KT in this process", t0, kt)
    for s, ks in [(256, 1), (256, 4), (512, 1), (512, 8)]:
        assert any(f[3] == s and f[4] == ks for f in mf), ("S, KS", s, ks)
    for f in [(256, 1), (256, 4), (512, 8)]:
        assert any(g[3] == f[0] and g[4] == f[1] for g in here), ("S, KS in this process", f)
    assert any(f[3] == 512 and f[4] == 1 for f in ks1 if f[0] == "mf")
    for t0 in (0, 1, 2):
        for b in (False, True):
            assert any(f[1] == b and f[2] == t0 for f in mf), ("BIAS, T0", b, t0)
    assert any(f[1] and f[4] > 1 for f in here), "BIAS with KS > 1"
    mfc = [f for f in dcond if f[0] == "mf"]
    assert any(f[2] == 1 for f in mfc) and any(f[2] == 2 for f in mfc) and any(f[4] > 1 for f in mfc), "conditioned forms"
    lines = []
    for name, d in (("default", dflt), ("WN_DEC_T0=0", t0off), ("WN_DEC_KS=1", ks1), ("WN_DEC_KS=8", ks8)):
        for f in sorted(d, key=str):
            if name == "default" or f not in dflt:
                lines.append("%-12s %s: %s" % (name, _form_name(f), ", ".join(sorted(set(d[f])))))
    return lines


def _form_name(f):
    if f[0] == "k":
        return "decode_k<%d> Q %s 256%s" % (f[1], "==" if f[2] else "!=", ", raised LDS limit" if f[3] else "")
    return "decode_duo_mfma8_k<BIAS %d, T0 %d, S %d, KS %d, KT %d>" % (int(f[1]), f[2], f[3], f[4], f[5])


def test_cases_reach_every_form():
    for ln in check_forms():
        print(ln)


# ================================================================================================ inputs and references (CPU)
class Inputs:
    """The float32 arrays one case's launch reads, per utterance distinct, and what decode_ref takes."""

    def __init__(self, c):
        seed = zlib.crc32(c["id"].encode())
        rng = np.random.default_rng(seed)
        k, Q, U, n = c["k"], c["Q"], c["U"], c["n"]
        self.c = c
        self.net = net = dr.Net(k, c["dil"], c["R"], c["D"], c["S"], Q, bias=c["bias"], seed=seed + 1)
        self.rings = net.rings(U, seed + 2)
        eye = np.eye(Q, dtype=np.float32)
        self.note0 = eye[rng.integers(0, Q, U)]
        self.prev0 = eye[rng.integers(0, Q, (U, k - 1))] if k > 1 else None
        self.forced = None if c["free"] else rng.integers(0, Q, (U, n)).astype(np.int32)
        self.cond = None
        if c["cond"] is not None:
            s = c["cond"]
            N, le = net.N, s["le"]
            self.cond = dict(shift=s["shift"], q=s["q"], le=le, pos0=s["pos0"],
                             fg=(rng.standard_normal((U, N, le, 2 * net.D)) * 0.5).astype(np.float32) if s["fg"] else None,
                             p1=(rng.standard_normal((U, le, net.S)) * 0.5).astype(np.float32) if s["p1"] else None)

    def kw(self, forced=None):
        c = self.c
        return dict(step0=c["step0"], push_input=c["push"], forced=self.forced if forced is None else forced, cond=self.cond,
                    temperature=c["temp"], windows=c["win"], win_pos0=c["win_pos0"])

    def references(self, forced=None):
        return dr.references(self.net, self.rings, self.note0, self.prev0, self.c["n"], **self.kw(forced))

    def touched(self, stage):
        """table columns stage `stage` reads over the launch"""
        s = self.cond
        return sorted({dr.cond_index(s["pos0"] + t + s["shift"][stage], s["q"][stage], s["le"]) for t in range(self.c["n"])})


@functools.lru_cache(maxsize=None)
def inputs(cid):
    return Inputs(CASE[cid])


@functools.lru_cache(maxsize=None)
def refs(cid):
    """(float64 reference, degraded-form distances) of a case; a free-running case's reference runs on ITS OWN codes here (the
    CPU conditions) - the GPU test feeds it the kernel's"""
    inp = inputs(cid)
    if not CASE[cid]["free"]:
        return inp.references()
    codes = dr.decode_ref(inp.net, inp.rings, inp.note0, inp.prev0, CASE[cid]["n"], **inp.kw())["codes"]
    return inp.references(forced=codes)


# ================================================================================================ device buffers
def _framed(n, dtype=torch.float32, fill=NAN):
    return torch.full((FRAME + n + FRAME,), fill, dtype=dtype, device=DEV)


def _inner(t):
    return t[FRAME:t.numel() - FRAME]


def _frames_ok(t, fill=NAN):
    fr = torch.cat([t[:FRAME], t[t.numel() - FRAME:]])
    return bool(torch.isnan(fr).all()) if fill != fill else bool((fr == fill).all())


def _packed(wmat, chained=False):
    """[M][K] float32 -> f16 hi / lo fragments as wn_pack_weights writes them (tests/test_gpu_kernels._packed)"""
    from music_amd.engine import pack_index
    m, k = wmat.shape
    flat = torch.from_numpy(np.ascontiguousarray(wmat, dtype=np.float32).reshape(-1)).to(DEV)
    idx = torch.from_numpy(pack_index(np.arange(m * k, dtype=np.int64).reshape(m, k), chained)).to(DEV)
    out = torch.zeros(idx.numel() * 2, dtype=torch.int16, device=DEV)
    call("wn_pack_weights", ptr(flat), ptr(idx), ptr(out), idx.numel(), _lib.F16X3, _lib.stream())
    return out


def _pad(m, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:m.shape[0], :m.shape[1]] = m
    return out


class Weights:
    """The decode layout of include/wavenet_hip.h from a Net's explicit matrices: w_causal [Rp][kQ] (tap 0 q | .. | tap k-1 q);
    per block, layer_stride floats apart, Wfg [2Dp][kRp] (rows f then g; tap k-1 r | .. | tap 0 r), Wd [Rp][Dp], Ws [S][Dp];
    w_p1 [S][S]; w_p2 [Q][S]; biases bc [Rp], per block [bf Dp | bg Dp | bd Rp | bs S], b1 [S], b2 [Q].  Rp = Dp = 64 on the
    matrix-core path (zero rows and columns beyond R / D), else R / D.  NaN between the sections and behind every block.
    pk (matrix-core): per block fg [2 x 64][64 k] in natural k order (tap 0 first) then d [64][64] chained, then skip
    [S][N x 64], p1, p2."""

    def __init__(self, net, mf):
        k, N, R, D, S, Q = net.k, net.N, net.R, net.D, net.S, net.Q
        Rp, Dp = (64, 64) if mf else (R, D)
        self.Rp, self.Dp = Rp, Dp
        sec, self.off, o = [], {}, GAP

        def add(name, a):
            nonlocal o
            self.off[name] = o
            sec.append((o, np.ascontiguousarray(a, np.float32).reshape(-1)))
            o += a.size + GAP
        add("causal", _pad(np.concatenate([net.wc[j] for j in range(k)], 1), Rp, k * Q))
        self.block = 2 * Dp * k * Rp + Rp * Dp + S * Dp
        self.layer_stride = self.block + GAP
        blocks = np.full((N, self.layer_stride), NAN, np.float32)
        order = range(k - 1, -1, -1)
        for l in range(N):
            fg = np.concatenate([np.concatenate([_pad(net.wf[l][j], Dp, Rp) for j in order], 1),
                                 np.concatenate([_pad(net.wg[l][j], Dp, Rp) for j in order], 1)], 0)
            blocks[l, :self.block] = np.concatenate([fg.reshape(-1), _pad(net.wd[l], Rp, Dp).reshape(-1), _pad(net.ws[l], S, Dp).reshape(-1)])
        add("layers", blocks)
        add("p1", net.p1)
        add("p2", net.p2)
        if net.bias:
            pv = lambda v, n: _pad(v[None, :], 1, n)[0]
            add("bc", pv(net.bc, Rp))
            add("bl", np.stack([np.concatenate([pv(net.bf[l], Dp), pv(net.bg[l], Dp), pv(net.bd[l], Rp), net.bs[l]]) for l in range(N)]))
            add("b1", net.b1)
            add("b2", net.b2)
        host = np.full(o, NAN, np.float32)
        for at, a in sec:
            host[at:at + a.size] = a
        self.host = host
        self.buf = torch.from_numpy(host).to(DEV)
        self.pk, self.pk_off = None, None
        if mf:
            parts, offs, at = [], {}, 0
            for l in range(N):
                fgn = np.concatenate([np.concatenate([_pad(net.wf[l][j], 64, 64) for j in range(k)], 1),
                                      np.concatenate([_pad(net.wg[l][j], 64, 64) for j in range(k)], 1)], 0)
                for name, m, ch in (("fg%d" % l, fgn, False), ("d%d" % l, _pad(net.wd[l], 64, 64), True)):
                    offs[name] = at
                    parts.append(_packed(m, ch))
                    at += parts[-1].numel()
            for name, m in (("skip", np.concatenate([_pad(net.ws[l], S, 64) for l in range(N)], 1)), ("p1", net.p1), ("p2", net.p2)):
                offs[name] = at
                parts.append(_packed(m))
                at += parts[-1].numel()
            self.pk, self.pk_off = torch.cat(parts), offs
            self.pk_stride = offs["fg1"] - offs["fg0"] if N > 1 else 0

    def args(self):
        p = lambda n: ptr(self.buf, self.off[n]) if n in self.off else None
        return (p("causal"), p("bc"), p("layers"), self.layer_stride, p("bl"), p("p1"), p("b1"), p("p2"), p("b2"))

    def chain(self):
        if self.pk is None:
            return None, 0, 0, 0, -1, -1, -1
        o = self.pk_off
        return ptr(self.pk), o["fg0"], o["d0"], self.pk_stride, o["skip"], o["p1"], o["p2"]


@functools.lru_cache(maxsize=None)
def weights(cid):
    return Weights(inputs(cid).net, CASE[cid]["fam"] == "mf")


RAN = re.compile(r"\[wn_decode\] (?:matrix-core, 8 utterances per pair: filter width (\d+), (\d+) utterances, (\d+) steps, (\d+) skip "
                 r"channels, biases (\d), tap-0 ahead (\d), skip parts (\d+), conditioned (\d)|generic fp32 kernel: (\d+) utterances, "
                 r"(\d+) steps, conditioned (\d))")


class State:
    """the device state of U utterances between launches: framed rings with slack between the utterances, note / prev columns"""

    def __init__(self, inp, w, rows=None):
        c, net = inp.c, inp.net
        self.rows = rows = list(range(c["U"])) if rows is None else rows
        Rp = w.Rp
        self.q_off = np.cumsum([0] + [(net.k - 1) * d * Rp for d in net.dil]).astype(np.int64)
        self.ring_floats = int(self.q_off[-1])
        self.ustride = self.ring_floats + 32
        host = np.full((len(rows), self.ustride), NAN, np.float32)
        for i, d in enumerate(net.dil):
            L = (net.k - 1) * d
            col = np.zeros((len(rows), L, Rp), np.float32)
            col[:, :, :net.R] = inp.rings[i][rows]
            host[:, self.q_off[i]:self.q_off[i + 1]] = col.reshape(len(rows), -1)
        self.rings0 = host
        self.rings = _framed(host.size)
        _inner(self.rings).copy_(torch.from_numpy(host.reshape(-1)))
        self.note = torch.from_numpy(inp.note0[rows]).to(DEV).contiguous()
        self.prev = torch.from_numpy(inp.prev0[rows]).to(DEV).contiguous() if net.k > 1 else None
        self.done = 0

    def ring_host(self):
        return _inner(self.rings).cpu().numpy().reshape(len(self.rows), self.ustride)


def launch(inp, w, st, n, capfd, forced="case"):
    """One launch of n steps from state `st` (advanced in place), through the narrowest entry that takes the case's arguments.
    Returns dict(probs [U][n][Q], codes [U][n], note_out, prev_out, form) - after the frames, the flags and the slack were checked."""
    c, net = inp.c, inp.net
    k, N, S, Q = net.k, net.N, net.S, net.Q
    rows, U, s0 = st.rows, len(st.rows), st.done
    if forced == "case":
        forced = inp.forced
    forced_t = torch.from_numpy(np.ascontiguousarray(forced[rows][:, s0:s0 + n])).to(device=DEV, dtype=torch.int32) if forced is not None else None
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
            ptr(forced_t), ptr(codes, FRAME), ptr(probs, FRAME), c["step0"] + s0, n, c["push"], ptr(sync), U, st.ustride,
            float(c["temp"]), 1234, *w.chain())
    name = "wn_decode_batch_fw"
    keep = []
    if inp.cond is not None or c["win"]:
        name = "wn_decode_batch_cond"
        cargs = (None, 0, None, 0, None, None, 1, 0)
        if inp.cond is not None:
            s = inp.cond
            le = s["le"]
            tabs = []
            for key, width, real, stages in (("fg", 2 * w.Dp, net.D, N), ("p1", S, None, 1)):
                if s[key] is None:
                    tabs += [None, 0]
                    continue
                src = s[key][rows] if key == "fg" else s[key][rows][:, None]                 # [U][stages][le][..]
                full = np.zeros((U, stages, le, width), np.float32)
                if key == "fg":                                                              # rows f then g, each padded to Dp
                    full[..., :real] = src[..., :real]
                    full[..., w.Dp:w.Dp + real] = src[..., real:]
                else:
                    full[:] = src
                for i in range(stages):                                                      # columns the schedule never reaches
                    dead = [j for j in range(le) if j not in inp.touched(i if key == "fg" else N)]
                    full[:, i, dead] = NAN
                us = stages * le * width + GAP
                t = torch.full((U, us), NAN, device=DEV)
                t[:, :us - GAP] = torch.from_numpy(full.reshape(U, -1)).to(DEV)
                keep.append(t)
                tabs += [ptr(t), us]
            sh, qs = (ctypes.c_int32 * (N + 1))(*s["shift"]), (ctypes.c_int32 * (N + 1))(*s["q"])
            keep += [sh, qs]
            cargs = (*tabs, vp(sh), vp(qs), le, s["pos0"] + s0)
        args += cargs
        if c["win"]:
            name = "wn_win_decode_batch"
            wh = (ctypes.c_int32 * (2 * len(c["win"])))(*[v for pr in c["win"] for v in pr])
            keep.append(wh)
            args += (None, 0, 1.0, vp(wh), len(c["win"]), c["win_pos0"] + s0)
    torch.cuda.synchronize()
    capfd.readouterr()
    os.environ["WN_DEC_VERBOSE"] = "1"
    try:
        call(name, *args, _lib.stream())
        torch.cuda.synchronize()
    finally:
        del os.environ["WN_DEC_VERBOSE"]
    m = RAN.search(capfd.readouterr().err)
    assert m, "no WN_DEC_VERBOSE line"
    want = _route(c, n)
    if m.group(1) is not None:
        ran = ("mf", bool(int(m.group(5))), int(m.group(6)), int(m.group(4)), int(m.group(7)), int(m.group(1)))
        assert (int(m.group(2)), int(m.group(3)), int(m.group(8))) == (U, n, int(inp.cond is not None))
    else:
        ran = ("k",) + want[1:]
        assert (int(m.group(9)), int(m.group(10)), int(m.group(11))) == (U, n, int(inp.cond is not None))
    assert ran == want, "case %s ran %s, its id and _route say %s" % (c["id"], _form_name(ran) if ran[0] == "mf" else ran, _form_name(want))
    # frames and flags
    assert _frames_ok(probs) and _frames_ok(codes, SENT) and _frames_ok(note_out) and _frames_ok(prev_out) and _frames_ok(st.rings)
    assert bool((sync[U * gran:] == -12345).all()), "the hand-off area's frame"
    assert bool((sync[:U * gran].view(U, gran)[:, -1] == 0).all()), "an error flag is set"
    rh = st.ring_host()
    assert np.isnan(rh[:, st.ring_floats:]).all(), "the slack between the utterances' rings"
    out = dict(probs=_inner(probs).view(U, n, Q).cpu().numpy(), codes=_inner(codes).view(U, n).cpu().numpy(),
               note_out=_inner(note_out).view(U, Q).cpu().numpy(), prev_out=_inner(prev_out).view(U, k - 1, Q).cpu().numpy(), form=ran)
    assert not np.isnan(out["probs"]).any() and (out["codes"] != SENT).all()
    st.note = _inner(note_out).view(U, Q).clone()
    st.prev = _inner(prev_out).view(U, k - 1, Q).clone() if k > 1 else None
    st.done += n
    return out


# ================================================================================================ the comparisons
WORST = {}


def _share(section, what, err, bar):
    s = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    WORST[(section, what)] = max(WORST.get((section, what), 0.0), s)
    print("  %-10s %-6s error %.3e  bar %.3e  share %.3f" % (section, what, err, bar, s))
    return s


def check_exact(c, out, s0=0):
    """what needs no reference: the greedy code is the first-index argmax of the kernel's own probabilities inside the window,
    and nothing lies outside it"""
    U, n, Q = out["probs"].shape
    for s in range(n):
        lo, hi = c["win"][(c["win_pos0"] + s0 + s) % len(c["win"])] if c["win"] else (0, Q)
        p = out["probs"][:, s]
        assert (p[:, :lo] == 0).all() and (p[:, hi:] == 0).all(), "probabilities outside the window"
        code = out["codes"][:, s]
        assert (code >= lo).all() and (code < hi).all()
        if c["temp"] <= 0:
            assert (code == lo + np.argmax(p[:, lo:hi], 1)).all(), ("step", s, "code is not the first-index argmax of probs_out")


def check_rings(c, inp, w, st, ref, err, fam, n_done, rows, section):
    """rings after n_done steps from the case's start: reached slots against the reference, the others bit for bit as they
    were, padded channels exactly 0"""
    net = inp.net
    got = st.ring_host()
    rings_got = []
    for i, d in enumerate(net.dil):
        L = (net.k - 1) * d
        a = got[:, st.q_off[i]:st.q_off[i + 1]].reshape(len(rows), L, w.Rp)
        a0 = st.rings0[:, st.q_off[i]:st.q_off[i + 1]].reshape(len(rows), L, w.Rp)
        reached = sorted({(c["step0"] + s) % L for s in range(n_done)}) if L else []
        rest = [j for j in range(L) if j not in reached]
        assert np.array_equal(a[:, rest].view(np.int32), a0[:, rest].view(np.int32)), "a ring slot the launch did not reach changed"
        assert (a[:, :, net.R:] == 0).all(), "padded channels of a ring column"
        assert np.array_equal(np.asarray(ref["rings"][i])[rows][:, rest], a0[:, rest, :net.R].astype(np.float64))
        rings_got.append(a[:, :, :net.R])
    e = dr.ring_err(rings_got, [np.asarray(r)[rows] for r in ref["rings"]])
    assert _share(section, "rings", e, dr.bar(err["rings"], fam)) <= 1.0, c["id"]


def check_probs(c, out, ref, err, fam, rows, steps, section):
    e = dr.prob_err(out["probs"].astype(np.float64), ref["probs"][rows][:, steps])
    assert _share(section, "probs", e, dr.bar(err["probs"], fam)) <= 1.0, c["id"]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _section(form):
    return "decode_k" if form[0] == "k" else "mfma T0=%d KS=%d KT=%d" % (form[2], form[4], form[5])


@pytest.mark.parametrize("cid", IDS)
def test_launch(cid, capfd):
    """One launch of the case against its float64 reference, every check of the module docstring; a second launch from the same
    state gives the same bits.  Cases with `split`: the same steps as two launches on the carried state, both halves against the
    one reference run and against the single launch."""
    c, inp, w = CASE[cid], inputs(cid), weights(cid)
    n, rows = c["n"], list(range(c["U"]))
    st = State(inp, w)
    out = launch(inp, w, st, n, capfd)
    fam = out["form"][0]
    if c["free"]:                                   # the reference follows the kernel's own codes: every step is still checked
        assert c["temp"] <= 0 and inp.forced is None
        ref, err = inp.references(forced=out["codes"])
    else:
        ref, err = refs(cid)
    sec = _section(out["form"])
    print("%s: %s" % (cid, _form_name(out["form"])))
    check_exact(c, out)
    check_probs(c, out, ref, err, fam, rows, slice(0, n), sec)
    check_rings(c, inp, w, st, ref, err, fam, n, rows, sec)
    assert np.array_equal(out["note_out"], ref["note_out"]) and np.array_equal(out["prev_out"], ref["prev_out"])
    # a repeated launch
    st2 = State(inp, w)
    out2 = launch(inp, w, st2, n, capfd)
    assert _bits(out["probs"], out2["probs"]) and np.array_equal(out["codes"], out2["codes"]) and _bits(st.ring_host()[:, :st.ring_floats], st2.ring_host()[:, :st.ring_floats])
    if c["split"]:
        n1, n2 = c["split"]
        st3 = State(inp, w)
        a = launch(inp, w, st3, n1, capfd)
        b = launch(inp, w, st3, n2, capfd)
        for o, s0, steps in ((a, 0, slice(0, n1)), (b, n1, slice(n1, n))):
            f = o["form"][0]
            check_exact(c, o, s0)
            # (a half on the fp32 kernel answers to the fp32 bar; the state it inherits from a matrix-core half to that half's)
            check_probs(c, o, ref, err, "mf" if "mf" in (a["form"][0], f) and s0 else f, rows, steps, _section(o["form"]) + " split")
        check_rings(c, inp, w, st3, ref, err, "mf" if "mf" in (a["form"][0], b["form"][0]) else "k", n, rows, _section(b["form"]) + " split")
        assert np.array_equal(b["note_out"], ref["note_out"]) and np.array_equal(b["prev_out"], ref["prev_out"])
        two = np.concatenate([a["probs"], b["probs"]], 1)
        e = dr.prob_err(two.astype(np.float64), out["probs"].astype(np.float64))
        print("  one launch against two: probabilities %.3e relative, same bits: %s" % (e, _bits(two, out["probs"])))
        assert e <= dr.bar(err["probs"], "mf" if "mf" in (a["form"][0], b["form"][0], fam) else "k")
        if a["form"] == b["form"] == out["form"]:       # within one form: the same sums in the same order
            assert _bits(two, out["probs"]) and _bits(st.ring_host()[:, :st.ring_floats], st3.ring_host()[:, :st.ring_floats])
            assert np.array_equal(np.concatenate([a["codes"], b["codes"]], 1), out["codes"])


@pytest.mark.parametrize("cid,row", [("k_r8_wrap_partial_bigstep", 1), ("mf_k2_s512_u3_cond_stretch_tile", 1), ("mf_k3_split_launch", 2)])
def test_batch_row_equals_single_launch(cid, row, capfd):
    """row u of a batch = the single-utterance launch of that utterance, bit for bit (both launches in the same form)"""
    c, inp, w = CASE[cid], inputs(cid), weights(cid)
    st = State(inp, w)
    out = launch(inp, w, st, c["n"], capfd)
    one = dict(c, U=1)
    assert _route(one) == _route(c)
    inp1 = Inputs.__new__(Inputs)
    inp1.__dict__.update(inp.__dict__)
    inp1.c = one
    st1 = State(inp, w, rows=[row])
    out1 = launch(inp1, w, st1, c["n"], capfd)
    assert out1["form"] == out["form"]
    assert _bits(out["probs"][row], out1["probs"][0]) and np.array_equal(out["codes"][row], out1["codes"][0])
    assert _bits(st.ring_host()[row, :st.ring_floats], st1.ring_host()[0, :st.ring_floats])
    assert np.array_equal(out["note_out"][row], out1["note_out"][0])


def test_temperature_scales_the_logits(capfd):
    """probs_out of a launch with a temperature is softmax(logits / T): against the reference's logits / T (the case's bar), and
    NOT the plain softmax raised or rescaled afterwards - the distance to softmax(logits) is far over the bar"""
    cid = "k_temperature_q100"
    c, inp, w = CASE[cid], inputs(cid), weights(cid)
    ref, err = refs(cid)
    out = launch(inp, w, State(inp, w), c["n"], capfd)
    lg = ref["logits"]
    want = np.exp(lg / c["temp"] - (lg / c["temp"]).max(2, keepdims=True))
    want /= want.sum(2, keepdims=True)
    assert np.abs(want - ref["probs"]).max() < 1e-15
    plain = np.exp(lg - lg.max(2, keepdims=True))
    plain /= plain.sum(2, keepdims=True)
    b = dr.bar(err["probs"], "k")
    assert dr.prob_err(out["probs"].astype(np.float64), want) <= b
    assert dr.prob_err(out["probs"].astype(np.float64), plain) > 1000 * b


# ================================================================================================ _DecodePack builds the same buffers
@pytest.mark.parametrize("R,bias", [(32, False), (32, True), (64, False), (64, True)], ids=["32-padded", "32-padded-bias", "64", "64-bias"])
def test_decode_pack_builds_the_same_buffers(R, bias):
    """fast_generate._DecodePack of a model.wavenet holding the same matrices: the same float32 sections, offsets relative to each
    other, strides and fragment bits as this module's own builder (which follows the header's layout text)."""
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    dil, S, Q, k = [1, 2, 4], 256, 256, 2
    net = dr.Net(k, dil, R, R, S, Q, bias=bias, seed=900 + R + bias)
    m = wavenet(filter_width=k, dilations=dil, dilation_channels=R, residual_channels=R, skip_channels=S, quantization_channels=Q,
                use_bias=bias)
    sd = {"causal_layer.weight": np.stack(list(net.wc), 2), "post_process_1.weight": net.p1[:, :, None], "post_process_2.weight": net.p2[:, :, None]}
    for l in range(len(dil)):
        for j, a in enumerate((np.stack(list(net.wf[l]), 2), np.stack(list(net.wg[l]), 2), net.wd[l][:, :, None], net.ws[l][:, :, None])):
            sd["dilation_layer_stack.%d.weight" % (4 * l + j)] = a
    if bias:
        sd.update({"causal_layer.bias": net.bc, "post_process_1.bias": net.b1, "post_process_2.bias": net.b2})
        for l in range(len(dil)):
            for j, a in enumerate((net.bf[l], net.bg[l], net.bd[l], net.bs[l])):
                sd["dilation_layer_stack.%d.bias" % (4 * l + j)] = a
    m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(a)) for n, a in sd.items()})
    m = m.cuda()
    eng = m._engine_for(torch.device("cuda", torch.cuda.current_device()))
    assert fg._mfma_decode(eng)
    pack = fg._pack_for(m, eng)
    pack.refresh()
    torch.cuda.synchronize()
    w = Weights(net, True)
    assert (pack.Rp, pack.Dp, pack.layer_stride) == (64, 64, w.block)
    got = pack.buf.cpu().numpy()
    N = len(dil)
    sections = [("causal", pack.o_causal, 64 * k * Q), ("p1", pack.o_p1, S * S), ("p2", pack.o_p2, Q * S)]
    if bias:
        sections += [("bc", pack.ob_causal, 64), ("bl", pack.ob_layers, N * (3 * 64 + S)), ("b1", pack.ob_p1, S), ("b2", pack.ob_p2, Q)]
    else:
        assert pack.o_bias is None
    for name, o, size in sections:
        assert _bits(got[o:o + size], w.host[w.off[name]:w.off[name] + size]), name
    for l in range(N):
        o, mine = pack.o_layers + l * pack.layer_stride, w.off["layers"] + l * w.layer_stride
        assert _bits(got[o:o + w.block], w.host[mine:mine + w.block]), ("block", l)
    ch, mine = pack.chain(), w.chain()
    assert ch[1:] == mine[1:], "fragment offsets"
    assert torch.equal(pack.pk, w.pk), "fragment bits"


# ================================================================================================ the cached switches
def test_cached_switches_in_children():
    """WN_DEC_T0 and WN_DEC_KS are read once per process: this module's matrix-core cases again in fresh child processes, one after
    another - T0 = 0 (filter widths 3 / 4 and conditioned launches then run decode_k on the 64-wide rings), the one-workgroup
    skip stage at 512 skip channels, the split form wherever it fits.  Every case asserts its instantiation there as here."""
    for env in ({"WN_DEC_T0": "0"}, {"WN_DEC_KS": "1"}, {"WN_DEC_KS": "8"}):
        e = dict(os.environ, **env)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                            "-k", "test_launch and mf_"], cwd=ROOT, env=e, timeout=300, capture_output=True, text=True)
        print(env, r.stdout[-400:])
        assert r.returncode == 0, (env, r.stdout[-3000:], r.stderr[-1000:])


def test_zz_print_worst_shares():
    """the worst observed share of its bar per section (DESIGN.md records them)"""
    for (sec, what), s in sorted(WORST.items()):
        print("worst share  %-28s %-6s %.3f" % (sec, what, s))
