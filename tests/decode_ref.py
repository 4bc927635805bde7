"""Float64 restatement of the cached-queue decoder, wn_win_decode_batch, as include/wavenet_hip.h documents it - written from
the header alone, plain numpy, no device.  tests/test_decode_ref.py holds it to the oracle (fast_predict_next, wavenet_forward,
autoencoder_decode); tests/test_gpu_decode_kernels.py holds the decode kernels to it, one launch at a time.

The recurrence, per utterance and step s of a launch (global step g = step0 + s, output position pos0 + s):
  causal layer   x_0 = Wc [prev_0 .. prev_{k-2} | note] (+ bc)                 w_causal [R][kQ], k = tap 0 q | .. | tap k-1 q
  block i        [f; g] = Wfg_i [x_i | tap k-2 | .. | tap 0] (+ bf, bg) (+ cond_fg column)
                 tap j = ring_i[(g + j d_i) mod L_i], L_i = (k-1) d_i
                 z = tanh f * sigmoid g;  x_{i+1} = Wd_i z (+ bd) + x_i;  skip += Ws_i z (+ bs)
                 ring_i[g mod L_i] = x_i (push_input = 1) or x_{i+1} (push_input = 0, k = 2 only)
  post           h = relu(W1 relu(skip) (+ b1) (+ cond_p1 column));  logits = W2 h (+ b2)
  window         (lo, hi) = pair (win_pos0 + s) mod period, or (0, Q)
  probabilities  softmax(logits[lo:hi] / T) inside the window (T = 1 when greedy), exact 0 outside
  code           lo + first-index argmax inside the window (greedy); the next input is forced[s] if given, else the code
  table column   c = pos0 + s + c_shift[i]:  0 if c < 0;  min(c // c_q[i], le - 1) if c_q[i] > 0;  c mod le if c_q[i] == 0

Three degraded forms of the same function size the tests' bars and prove their sensitivity (never a kernel's output); in all
three every stored intermediate is rounded to float32 -
  "32": the float32 restatement - every product and every sum of a matrix-vector product in float32 too (the bar it sizes,
        8 e32, stands for "the same float32 work in another summation order");
  "x3": float64 on rounded operands: weights and vectors split hi = f16(x), lo = f16(x - hi), products hi.hi + hi.lo + lo.hi
        (what the matrix-core design accepts);
  "x1": the same with the hi halves only (a decoder that lost its lo planes).
The causal layer is a gather of float32 weights by one-hot columns in every kernel form: the split forms leave it exact."""
import numpy as np

MODES = ("64", "32", "x3", "x1")


def _r32(v):
    return v.astype(np.float32).astype(np.float64)


def _f16(v):
    return v.astype(np.float16).astype(np.float64)


def _split(v):
    h = _f16(v)
    return h, _f16(v - h)


class Net:
    """The weights of one decoder as explicit float32 matrices (what the decode layout is built from):
    wc [k][R][Q] (tap j, 0 = oldest), wf / wg [N][k][D][R], wd [N][R][D], ws [N][S][D], p1 [S][S], p2 [Q][S];
    biases (None, or all of them): bc [R], bf / bg [N][D], bd [N][R], bs [N][S], b1 [S], b2 [Q]."""

    def __init__(self, k, dil, R, D, S, Q, bias=False, seed=0, deep_gain=None):
        rng = np.random.default_rng(seed)
        N = len(dil)
        self.k, self.dil, self.R, self.D, self.S, self.Q, self.N = k, list(dil), R, D, S, Q, N
        # f / g and dense at unit gain, skip at unit gain (deep stacks: the gains of the products that ADD UP over the blocks
        # shrink with the depth, so the residual stream and the skip sum keep the statistics of an 8-block net)
        dg = min(1.0, np.sqrt(8.0 / N)) if deep_gain is None else deep_gain
        n = lambda *sh, s: (rng.standard_normal(sh) * s).astype(np.float32)
        self.wc = n(k, R, Q, s=0.7 / np.sqrt(k))
        self.wf = n(N, k, D, R, s=1.0 / np.sqrt(k * R))
        self.wg = n(N, k, D, R, s=1.0 / np.sqrt(k * R))
        self.wd = n(N, R, D, s=dg / np.sqrt(D))
        self.ws = n(N, S, D, s=dg / np.sqrt(D))
        self.p1 = n(S, S, s=1.4 / np.sqrt(S))
        self.p2 = n(Q, S, s=1.4 / np.sqrt(S))
        self.bias = bias
        if bias:
            self.bc, self.bf, self.bg, self.bd = n(R, s=0.2), n(N, D, s=0.2), n(N, D, s=0.2), n(N, R, s=0.2)
            self.bs, self.b1, self.b2 = n(N, S, s=0.1), n(S, s=0.2), n(Q, s=0.3)

    def rings(self, U, seed):
        """unit-variance initial rings of U utterances: a list of [U][L_i][R] float32"""
        rng = np.random.default_rng(seed)
        return [rng.standard_normal((U, (self.k - 1) * d, self.R)).astype(np.float32) for d in self.dil]


def cond_index(c, q, le):
    """the table column of stage position c (include/wavenet_hip.h, wn_decode_batch_cond)"""
    if c < 0:
        return 0
    if q > 0:
        return min(c // q, le - 1)
    return c % le


class _Arith:
    def __init__(self, mode):
        assert mode in MODES
        self.mode, self._w = mode, {}

    def t(self, v):
        return v if self.mode == "64" else _r32(v)

    def mv(self, W, x, exact=False):
        """x [U][K] times W [M][K] (float64 arrays holding float32 values) -> [U][M]"""
        if self.mode == "64" or (exact and self.mode != "32"):
            return x @ W.T
        if self.mode == "32":                      # float32 products, float32 sums (numpy's pairwise order: the same on every host)
            return (x.astype(np.float32)[:, None, :] * W.astype(np.float32)[None]).sum(-1, dtype=np.float32).astype(np.float64)
        sp = self._w.get(id(W))
        if sp is None:
            sp = self._w[id(W)] = tuple(np.ascontiguousarray(a.T) for a in _split(W))
        wh, wl = sp
        xh, xl = _split(x)
        if self.mode == "x1":
            return xh @ wh
        return xh @ wh + xl @ wh + xh @ wl


def decode_ref(net, rings, note0, prev0, n_steps, step0=0, push_input=1, forced=None, cond=None, temperature=0.0, windows=None,
               win_pos0=0, mode="64"):
    """n_steps of the recurrence for U utterances side by side.  rings: list of [U][L_i][R]; note0 [U][Q]; prev0 [U][k-1][Q]
    (None when k = 1); forced [U][n_steps] or None; cond: None or dict(fg=[U][N][le][2D] | None, p1=[U][le][S] | None,
    shift=[N+1], q=[N+1], le=, pos0=); windows: list of (lo, hi) or None.  Inputs are the float32 arrays the kernel reads.
    Returns dict(probs [U][n][Q], logits [U][n][Q], codes [U][n], rings (list, as given), note_out [U][Q], prev_out [U][k-1][Q])."""
    ar = _Arith(mode)
    k, N, R, D, S, Q = net.k, net.N, net.R, net.D, net.S, net.Q
    assert push_input or k == 2
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    U = note0.shape[0]
    rings = [f8(r).copy() for r in rings]
    note = f8(note0).copy()
    prev = f8(prev0).copy() if k > 1 else np.zeros((U, 0, Q))
    Wc = f8(np.concatenate([net.wc[j] for j in range(k)], 1))                                       # [R][kQ]: tap 0 | .. | tap k-1
    order = list(range(k - 1, -1, -1))                                                              # tap k-1 (current) | .. | tap 0
    Wfg = [f8(np.concatenate([np.concatenate([net.wf[l][j] for j in order], 1),
                              np.concatenate([net.wg[l][j] for j in order], 1)], 0)) for l in range(N)]
    Wd, Ws, P1, P2 = [f8(a) for a in net.wd], [f8(a) for a in net.ws], f8(net.p1), f8(net.p2)
    b = net.bias
    probs, logits, codes = np.zeros((U, n_steps, Q)), np.zeros((U, n_steps, Q)), np.zeros((U, n_steps), dtype=np.int64)
    for s in range(n_steps):
        g = step0 + s
        cur = ar.mv(Wc, np.concatenate([prev.reshape(U, -1), note], 1), exact=True)
        cur = ar.t(cur + f8(net.bc) if b else cur)
        skip = np.zeros((U, S))
        for l, d in enumerate(net.dil):
            L = (k - 1) * d
            taps = [rings[l][:, (g + j * d) % L] for j in range(k - 1)]
            fg = ar.mv(Wfg[l], np.concatenate([cur] + taps[::-1], 1))
            if b:
                fg = fg + np.concatenate([f8(net.bf[l]), f8(net.bg[l])])
            if cond is not None and cond.get("fg") is not None:
                fg = fg + f8(cond["fg"][:, l, cond_index(cond["pos0"] + s + cond["shift"][l], cond["q"][l], cond["le"])])
            fg = ar.t(fg)
            z = ar.t(np.tanh(fg[:, :D]) / (1.0 + np.exp(-fg[:, D:])))
            nxt = ar.mv(Wd[l], z) + cur
            sk = skip + ar.mv(Ws[l], z)
            if b:
                nxt, sk = nxt + f8(net.bd[l]), sk + f8(net.bs[l])
            nxt, skip = ar.t(nxt), ar.t(sk)
            if L:
                rings[l][:, g % L] = cur if push_input else nxt
            cur = nxt
        h1 = ar.mv(P1, np.maximum(skip, 0.0))
        if b:
            h1 = h1 + f8(net.b1)
        if cond is not None and cond.get("p1") is not None:
            h1 = h1 + f8(cond["p1"][:, cond_index(cond["pos0"] + s + cond["shift"][N], cond["q"][N], cond["le"])])
        h1 = ar.t(np.maximum(h1, 0.0))
        lg = ar.mv(P2, h1)
        lg = ar.t(lg + f8(net.b2) if b else lg)
        lo, hi = windows[(win_pos0 + s) % len(windows)] if windows else (0, Q)
        lw = lg[:, lo:hi] / (temperature if temperature > 0 else 1.0)
        e = np.exp(lw - lw.max(1, keepdims=True))
        probs[:, s, lo:hi] = e / e.sum(1, keepdims=True)
        logits[:, s] = lg
        codes[:, s] = lo + np.argmax(probs[:, s, lo:hi], 1)
        nextc = np.asarray(forced)[:, s] if forced is not None else codes[:, s]
        if k > 1:
            prev = np.concatenate([prev[:, 1:], note[:, None]], 1)
        note = np.zeros((U, Q))
        note[np.arange(U), nextc] = 1.0
    return dict(probs=probs, logits=logits, codes=codes, rings=rings, note_out=note, prev_out=prev)


def prob_err(p, p64):
    """max |p / p64 - 1| over the entries the reference gives a probability (outside a window both are exact zeros)"""
    m = p64 > 0
    return float(np.abs(p[m] / p64[m] - 1.0).max())


def ring_err(rings, rings64):
    """max |ring - ring64| over all rings, in units of max(1, max |ring64|)"""
    sc = max([1.0] + [float(np.abs(r).max()) for r in rings64 if r.size])
    return max([0.0] + [float(np.abs(np.asarray(a, dtype=np.float64) - r).max()) for a, r in zip(rings, rings64) if r.size]) / sc


def references(net, *args, **kw):
    """The float64 reference and the degraded forms' distances from it, on the scales of the comparisons:
    (ref64, {"probs": {"e32", "ex3", "ex1"}, "rings": {..}})"""
    ref = decode_ref(net, *args, mode="64", **kw)
    err = {"probs": {}, "rings": {}}
    for m in ("32", "x3", "x1"):
        o = decode_ref(net, *args, mode=m, **kw)
        err["probs"]["e" + m] = prob_err(o["probs"], ref["probs"])
        err["rings"]["e" + m] = ring_err(o["rings"], ref["rings"])
    return ref, err


def bar(err, family):
    """fp32 kernels: 8 e32 (the same float32 work in another summation order, a few ulp of tanhf / expf); matrix-core kernels:
    4 ex3 + 8 e32 (the operand rounding the design accepts, plus float32 accumulation)"""
    return 8 * err["e32"] if family == "k" else 4 * err["ex3"] + 8 * err["e32"]
