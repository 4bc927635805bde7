"""Float64 restatement of classifier-free guidance in the decoder (include/wavenet_hip.h, wn_cfg_decode_batch / wn_cfg_sample_logits),
the case tables of its GPU tests and the conditions tests/test_cfg_ref.py holds them to on the CPU.  Not a test module.

The rule: the rows of a launch are pairs - row 2j the conditional member, row 2j + 1 the unconditional one, scale s_j.  Each member
runs tests/decode_ref.py's recurrence on its own rings and tables; per step
    g = l_c + (s - 1) (l_c - l_u)
is windowed, tempered and picked from ONCE, and the one code is the next input of both members.  Launch level: `guided_ref` steps
decode_ref one sample at a time (so the recurrence is decode_ref's own, in each of its arithmetic modes).  Model level:
`guided_rollout` on class_cond_ref.logits, one full forward per member and step."""
import zlib

import numpy as np

from tests import decode_ref as dr


def combine(lc, lu, s):
    """g of the rule, float64; s broadcasts over the rows"""
    lc, lu = np.asarray(lc, dtype=np.float64), np.asarray(lu, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64).reshape((-1,) + (1,) * (lc.ndim - 1))
    return lc + (s - 1.0) * (lc - lu)


def amp(s):
    """|s| + |s - 1|: what the rule multiplies an error of the two logit rows by (g = s l_c - (s - 1) l_u)"""
    return float(np.max(np.abs(s) + np.abs(np.asarray(s, dtype=np.float64) - 1.0)))


def top2_margin(g, lo, hi):
    """smallest gap between the largest and the second largest entry of the rows of g inside [lo, hi) (inf for one entry)"""
    w = np.sort(np.asarray(g)[..., lo:hi], axis=-1)
    return float("inf") if hi - lo < 2 else float((w[..., -1] - w[..., -2]).min())


def guided_ref(net, rings, note0, prev0, n_steps, guidance, step0=0, forced=None, cond=None, temperature=0.0, windows=None,
               win_pos0=0, mode="64"):
    """n_steps for U = 2 P rows (P pairs).  Arguments as decode_ref's (corrected recurrence); note0 / prev0 / forced hold equal rows
    for the two members of a pair; guidance [P].  Returns dict(probs [P][n][Q] - the distribution of g -, g, logits [U][n][Q],
    codes [P][n], margin - the smallest top-2 gap of g inside its window over all steps and pairs -, rings, note_out [U][Q],
    prev_out [U][k-1][Q])."""
    k, Q = net.k, net.Q
    U = note0.shape[0]
    assert U % 2 == 0 and len(guidance) == U // 2
    P = U // 2
    s_ = np.asarray(guidance, dtype=np.float64)
    rings = [np.asarray(r, dtype=np.float64).copy() for r in rings]
    note = np.asarray(note0, dtype=np.float64).copy()
    prev = np.asarray(prev0, dtype=np.float64).copy() if k > 1 else None
    probs, gs, logits = np.zeros((P, n_steps, Q)), np.zeros((P, n_steps, Q)), np.zeros((U, n_steps, Q))
    codes, margin = np.zeros((P, n_steps), dtype=np.int64), float("inf")
    for s in range(n_steps):
        c_s = None if cond is None else dict(cond, pos0=cond["pos0"] + s)
        o = dr.decode_ref(net, rings, note, prev, 1, step0=step0 + s, push_input=1, cond=c_s, mode=mode)
        rings = o["rings"]
        lg = o["logits"][:, 0]
        g = combine(lg[0::2], lg[1::2], s_)
        if mode != "64":
            g = g.astype(np.float32).astype(np.float64)              # (a stored intermediate of the degraded forms)
        lo, hi = windows[(win_pos0 + s) % len(windows)] if windows else (0, Q)
        lw = g[:, lo:hi] / (temperature if temperature > 0 else 1.0)
        e = np.exp(lw - lw.max(1, keepdims=True))
        probs[:, s, lo:hi] = e / e.sum(1, keepdims=True)
        gs[:, s], logits[:, s] = g, lg
        codes[:, s] = lo + np.argmax(g[:, lo:hi], 1)
        margin = min(margin, top2_margin(g, lo, hi))
        nextc = np.asarray(forced)[0::2, s] if forced is not None else codes[:, s]
        if k > 1:
            prev = np.concatenate([prev[:, 1:], note[:, None]], 1)
        note = np.zeros((U, Q))
        note[np.arange(U), np.repeat(nextc, 2)] = 1.0
    return dict(probs=probs, g=gs, logits=logits, codes=codes, margin=margin, rings=rings, note_out=note,
                prev_out=prev if k > 1 else np.zeros((U, 0, Q)))


def references(net, rings, note0, prev0, n_steps, guidance, forced=None, **kw):
    """(float64 guided reference, the degraded forms' distances from it) as decode_ref.references: the degraded forms are fed the
    float64 reference's inputs (its own codes when the case runs free), so the distances are those of the arithmetic alone"""
    ref = guided_ref(net, rings, note0, prev0, n_steps, guidance, forced=forced, mode="64", **kw)
    fed = forced if forced is not None else np.repeat(ref["codes"], 2, 0)
    err = {"probs": {}, "rings": {}}
    for m in ("32", "x3", "x1"):
        o = guided_ref(net, rings, note0, prev0, n_steps, guidance, forced=fed, mode=m, **kw)
        err["probs"]["e" + m] = dr.prob_err(o["probs"], ref["probs"])
        err["rings"]["e" + m] = dr.ring_err(o["rings"], ref["rings"])
    return ref, err


# ---------------------------------------------------------------------------------------------- launch-level cases
SCALES = [1.5, 0.0, 3.0, -0.5, 1.0]          # pair j of a case runs under SCALES[j % 5]


def C(id, fam, k, dil, R, D, S, Q, pairs, n, step0=0, bias=False, temp=0.0, win=None, win_pos0=0, free=False, le=3):
    """fam 'mf': a matrix-core state (64 / 64 / S / 256, pk handed over); 'k': the fp32 kernel's own shapes.  Every case is
    conditioned (guidance needs tables): both tables, le columns under the tile rule, shifted per stage."""
    return dict(id=id, fam=fam, k=k, dil=list(dil), R=R, D=D, S=S, Q=Q, U=2 * pairs, n=n, step0=step0, push=1, bias=bias, temp=temp,
                win=win, win_pos0=win_pos0, free=free, split=None,
                cond=dict(shift=[(2 * i + 1) % 4 for i in range(len(dil) + 1)], q=[0] * (len(dil) + 1), le=le, pos0=1, fg=True, p1=True))


Q4 = lambda Q: [(0, Q // 4), (Q // 4, Q // 2), (Q // 2, Q - 3), (Q - 3, Q)]       # a 4-pair window table, unequal widths
CASES = [
    # ---- decode_duo_mfma8_k at 64 / 64 / 256 / 256, dilations [1, 2, 4], 6 steps: 1, 3, 4 and 5 pairs = spare pairs, a full group, a
    # second group that holds one pair (two groups: the one-workgroup skip stage; one group: the split one)
    C("mf_p1_free", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 1, 6, step0=3, free=True),
    C("mf_p3_bias", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 3, 6, step0=2 ** 33 + 5, bias=True),
    C("mf_p4_win", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 4, 6, win=[(0, 128), (128, 256), (40, 41)], win_pos0=1),
    C("mf_p5_ks1_free", "mf", 2, [1, 2, 4], 64, 64, 256, 256, 5, 6, step0=1, bias=True, free=True),
    C("mf_p3_s512", "mf", 2, [1, 2, 4], 64, 64, 512, 256, 3, 6, step0=7),
    C("mf_p3_fw3_bias_temp", "mf", 3, [1, 2, 4], 64, 64, 256, 256, 3, 6, step0=4, bias=True, temp=0.8),
    # more than 31 blocks: the tap-0 table sits in the first row's hand-off area
    C("mf_p2_32blocks", "mf", 2, [1, 2] * 16, 64, 64, 256, 256, 2, 6, step0=9),
    # ---- decode_k: two members per workgroup; Q = 100 and Q = 1024 under a 4-pair window table, filter widths 1, 2, 3, the
    # Q = 256 two-tap fast pick
    C("k_q100_p4_win", "k", 2, [1, 2, 3], 24, 40, 48, 100, 4, 8, step0=7, bias=True, win=Q4(100), win_pos0=2),
    C("k_q1024_fw3_p2_win_free", "k", 3, [1, 2], 32, 32, 64, 1024, 2, 8, step0=5, win=Q4(1024), win_pos0=1, free=True),
    C("k_fw1_q100_p2", "k", 1, [1, 1], 16, 16, 32, 100, 2, 8, bias=True),
    C("k_q256_p3_free", "k", 2, [1, 2, 4], 32, 32, 64, 256, 3, 8, step0=11, free=True),
]
IDS = [c["id"] for c in CASES]
CASE = dict(zip(IDS, CASES))


class Inputs:
    """The float32 arrays one case's launch reads (the attributes tests/test_gpu_decode_kernels.State takes): per row its own rings
    and conditioning tables; the members of a pair share note0, prev0 and the forced codes."""

    def __init__(self, c):
        seed = zlib.crc32(c["id"].encode())
        rng = np.random.default_rng(seed)
        k, Q, U, n = c["k"], c["Q"], c["U"], c["n"]
        P = U // 2
        self.c = c
        self.net = net = dr.Net(k, c["dil"], c["R"], c["D"], c["S"], Q, bias=c["bias"], seed=seed + 1)
        self.rings = net.rings(U, seed + 2)
        eye = np.eye(Q, dtype=np.float32)
        two = lambda a: np.repeat(a, 2, 0)
        self.note0 = two(eye[rng.integers(0, Q, P)])
        self.prev0 = two(eye[rng.integers(0, Q, (P, k - 1))]) if k > 1 else None
        self.forced = None if c["free"] else two(rng.integers(0, Q, (P, n)).astype(np.int32))
        self.guidance = np.array([SCALES[j % len(SCALES)] for j in range(P)], np.float32)
        s = c["cond"]
        self.cond = dict(shift=s["shift"], q=s["q"], le=s["le"], pos0=s["pos0"],
                         fg=(rng.standard_normal((U, net.N, s["le"], 2 * net.D)) * 0.5).astype(np.float32),
                         p1=(rng.standard_normal((U, s["le"], net.S)) * 0.5).astype(np.float32))

    def kw(self, forced=None):
        c = self.c
        return dict(step0=c["step0"], forced=self.forced if forced is None else forced, cond=self.cond, temperature=c["temp"],
                    windows=c["win"], win_pos0=c["win_pos0"])

    def references(self, forced=None):
        return references(self.net, self.rings, self.note0, self.prev0, self.c["n"], self.guidance, **self.kw(forced))


# ---------------------------------------------------------------------------------------------- model-level cases
# tests/class_cond_ref.DECODE_CASES with the last class as the model's null_class and a scale per utterance
MODEL_GUIDANCE = {"mfma": [1.5, 3.0, 0.0], "fp32": [2.0, -0.5, 1.0]}


def model_case(name):
    from tests import class_cond_ref as ref
    case = ref.DECODE_CASES[name]
    cfg = dict(case["cfg"], null_class=case["cfg"]["global_classes"] - 1)
    classes = [c if c != cfg["null_class"] else 0 for c in case["classes"]]
    return dict(cfg=cfg, seed=case["seed"], classes=classes, steps=case["steps"], guidance=MODEL_GUIDANCE[name])


def guided_rollout(params, dilations, seed_codes, classes, null_class, guidance, n_steps, Q, filter_width=2, windows=None, pos0=0):
    """Free-running guided argmax decode in float64, two full forwards per step (as `classes`, as null_class) over ONE history:
    seed_codes (U, rf) int64 -> (codes (U, n_steps), the smallest top-2 margin of g met, per utterance)."""
    import torch
    import torch.nn.functional as F
    from tests import class_cond_ref as ref
    p64 = {k: v.detach().double() for k, v in params.items()}
    rf = ref.receptive_field(filter_width, dilations)
    U = seed_codes.size(0)
    hist, out, margin = seed_codes.clone(), [], np.full(U, np.inf)
    cls, null = torch.as_tensor(classes), torch.full((U,), int(null_class))
    for n in range(n_steps):
        x = F.one_hot(hist[:, -rf:], Q).permute(0, 2, 1).double()
        lc = ref.logits(p64, dilations, x, cls, filter_width)[:, :, -1].numpy()
        lu = ref.logits(p64, dilations, x, null, filter_width)[:, :, -1].numpy()
        g = combine(lc, lu, guidance)
        lo, hi = windows[(pos0 + n) % len(windows)] if windows is not None else (0, Q)
        margin = np.minimum(margin, [top2_margin(g[u], lo, hi) for u in range(U)])
        code = torch.from_numpy(lo + np.argmax(g[:, lo:hi], 1))
        out.append(code)
        hist = torch.cat([hist, code[:, None]], 1)
    return torch.stack(out, 1), margin
