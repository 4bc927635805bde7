"""tests/decode_ref.py held to the oracle, on the CPU: the cached-queue recurrence in float64 against fast_predict_next (filter
width 2, both recurrences), against wavenet_forward over the whole window (filter widths 1, 2, 3, 4) and, conditioned, against
autoencoder_decode - all within 1e-12; and, for every case of tests/test_gpu_decode_kernels.py's table, the three conditions
that make its bars meaningful, from the references alone."""
import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as wo
from tests import decode_ref as dr
from tests import test_gpu_decode_kernels as gk

TOL = 1e-12


def _params(net):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    p = {"causal_layer.weight": t(np.stack(list(net.wc), 2)), "post_process_1.weight": t(net.p1[:, :, None]),
         "post_process_2.weight": t(net.p2[:, :, None])}
    for l in range(net.N):
        for j, a in enumerate((np.stack(list(net.wf[l]), 2), np.stack(list(net.wg[l]), 2), net.wd[l][:, :, None], net.ws[l][:, :, None])):
            p["dilation_layer_stack.%d.weight" % (4 * l + j)] = t(a)
    if net.bias:
        p.update({"causal_layer.bias": t(net.bc), "post_process_1.bias": t(net.b1), "post_process_2.bias": t(net.b2)})
        for l in range(net.N):
            for j, a in enumerate((net.bf[l], net.bg[l], net.bd[l], net.bs[l])):
                p["dilation_layer_stack.%d.bias" % (4 * l + j)] = t(a)
    return p


def _onehot(codes, Q):
    return np.eye(Q, dtype=np.float32)[np.asarray(codes)]


def _ring_from_queue(q, step0):
    """time-ordered columns [L][R] (oldest first) -> ring slots at global step step0 (slot g mod L is the oldest)"""
    return np.roll(q, step0 % len(q), 0) if len(q) else q


def _queue_from_ring(r, g):
    return np.roll(r, -(g % len(r)), 0) if len(r) else r


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("correct", [False, True], ids=["as_written", "corrected"])
def test_against_fast_predict_next(correct, bias):
    """filter width 2, both recurrences: every step's probabilities and the queues the oracle's incremental path leaves"""
    dil, R, D, S, Q, n, step0 = [1, 2, 4, 3], 6, 5, 7, 9, 11, 2 ** 33 + 5
    net = dr.Net(2, dil, R, D, S, Q, bias=bias, seed=3)
    params = _params(net)
    rng = np.random.default_rng(1)
    queue = {"causal_layer": torch.from_numpy(_onehot(rng.integers(0, Q, 1), Q).T.copy()).double().view(1, Q, 1)}
    rings = []
    for i, d in enumerate(dil):
        q = rng.standard_normal((d, R)).astype(np.float32)
        queue["block_%d" % (i + 1)] = torch.from_numpy(q.T.copy()).double().view(1, R, d)
        rings.append(_ring_from_queue(q, step0)[None])
    codes = rng.integers(0, Q, n + 1)
    prev0 = queue["causal_layer"].numpy()[:, :, 0][None].astype(np.float32)                  # [1][1][Q]
    out = dr.decode_ref(net, rings, _onehot(codes[:1], Q), prev0, n, step0=step0, push_input=int(correct),
                        forced=codes[None, 1:])
    for s in range(n):
        note = torch.from_numpy(_onehot(codes[s:s + 1], Q).T.copy()).double().view(1, Q, 1)
        pred, queue, probs = wo.fast_predict_next(params, dil, note, queue, quantization_channels=Q, correct_queue=correct, return_probs=True)
        assert np.abs(out["probs"][0, s] - probs.numpy()).max() < TOL
        assert out["codes"][0, s] == int(pred)
    for i, d in enumerate(dil):
        assert np.abs(_queue_from_ring(out["rings"][i][0], step0 + n).T - queue["block_%d" % (i + 1)][0].numpy()).max() < TOL
    assert np.array_equal(out["prev_out"][0, 0], _onehot(codes[n - 1:n], Q)[0]) and np.array_equal(out["note_out"][0], _onehot(codes[n:], Q)[0])


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_against_wavenet_forward(k, bias):
    """the corrected recurrence over a teacher-forced window equals the full forward: probabilities at every position, and the
    rings are the last (k-1) d columns of every block's input"""
    dil, R, D, S, Q, n, step0 = [1, 2, 4, 3], 6, 5, 7, 9, 13, 1000003
    net = dr.Net(k, dil, R, D, S, Q, bias=bias, seed=10 + k)
    params = _params(net)
    rf = wo.receptive_field(k, dil)
    rng = np.random.default_rng(2)
    codes = rng.integers(0, Q, rf + n + 1)
    x = torch.from_numpy(_onehot(codes[:rf + n], Q).T.copy()).double().view(1, Q, rf + n)
    inter = {}
    wo.wavenet_forward(params, dil, x, filter_width=k, quantization_channels=Q, intermediates=inter)
    p_ref = torch.softmax(inter["pre_softmax"][0], 0).t().numpy()                              # (n + 1, Q): input ending at rf - 1 + w

    def rings_at(done):
        """the rings after `done` decode steps: block i's input up to time rf - 1 + done"""
        out = []
        for i, d in enumerate(dil):
            xs = inter["x"][i][0].numpy().T                                                     # [time][R], last row = time rf + n - 1
            end = len(xs) - n + done
            out.append(_ring_from_queue(xs[end - (k - 1) * d:end], step0 + done))
        return out
    rings = [r[None] for r in rings_at(0)]
    prev0 = _onehot(codes[rf - (k - 1):rf], Q)[None] if k > 1 else None
    out = dr.decode_ref(net, rings, _onehot(codes[rf:rf + 1], Q), prev0, n, step0=step0, forced=codes[None, rf + 1:rf + n + 1])
    assert np.abs(out["probs"][0] - p_ref[1:]).max() < TOL
    assert np.abs(out["logits"][0] - inter["pre_softmax"][0].numpy().T[1:]).max() < 1e-11
    for got, want in zip(out["rings"], rings_at(n)):
        assert got.shape[1:] == want.shape and (want.size == 0 or np.abs(got[0] - want).max() < TOL)
    if k > 1:
        assert np.array_equal(out["prev_out"][0], _onehot(codes[rf + n - (k - 1):rf + n], Q))


def test_conditioned_against_autoencoder_decode():
    """the per-utterance schedule (stretch where a stage's length divides by Le, tile elsewhere; stage column = position + L_stage - W)
    and the [f | g] table order against the autoencoder's decoder over the whole clip"""
    k, dil, R, D, S, Q, bw = 2, [1, 2, 4, 1], 6, 5, 7, 9, 3
    net = dr.Net(k, dil, R, D, S, Q, bias=True, seed=21)
    rf = wo.receptive_field(k, dil)
    n, le = 15, 4
    T = rf + n                                                  # W = n + 1 output positions
    rng = np.random.default_rng(4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    params = {"de_causal_layer.weight": t(np.stack(list(net.wc), 2)), "de_causal_layer.bias": t(net.bc),
              "connection_1.weight": t(net.p1[:, :, None]), "connection_1.bias": t(net.b1),
              "connection_2.weight": t(net.p2[:, :, None]), "connection_2.bias": t(net.b2)}
    for l in range(net.N):
        # the reference's filter_gate conv: gate = first half of the channels, filter = second half
        params["de_dilation_layer_stack.%d.weight" % (3 * l)] = t(np.concatenate([np.stack(list(net.wg[l]), 2), np.stack(list(net.wf[l]), 2)], 0))
        params["de_dilation_layer_stack.%d.bias" % (3 * l)] = t(np.concatenate([net.bg[l], net.bf[l]]))
        params["de_dilation_layer_stack.%d.weight" % (3 * l + 1)] = t(net.wd[l][:, :, None])
        params["de_dilation_layer_stack.%d.bias" % (3 * l + 1)] = t(net.bd[l])
        params["de_dilation_layer_stack.%d.weight" % (3 * l + 2)] = t(net.ws[l][:, :, None])
        params["de_dilation_layer_stack.%d.bias" % (3 * l + 2)] = t(net.bs[l])
    enc = t(rng.standard_normal((1, bw, le)).astype(np.float32))
    cond = [(t(rng.standard_normal((2 * D if i < net.N else S, bw, 1)).astype(np.float32)),
             t(rng.standard_normal(2 * D if i < net.N else S).astype(np.float32))) for i in range(net.N + 1)]
    codes = rng.integers(0, Q, T + 1)
    x = t(_onehot(codes[:T], Q).T).view(1, Q, T)
    inter = {}
    W = T - rf + 1
    wo.autoencoder_decode(params, dil, x, enc, W, cond, q=Q, intermediates=inter)
    # (the oracle's own output is the reference's chunk softmax over the channels-first buffer: the per-position logits are
    #  connection_2 of the conditioned, rectified connection_1 output it hands out)
    lg = torch.nn.functional.conv1d(torch.relu(inter["de_conn"]), params["connection_2.weight"], params["connection_2.bias"])
    p_ref = torch.softmax(lg[0], 0).t().numpy()
    # the tables in the decode layout and the schedule
    lens = [T - (k - 1) * (1 + sum(dil[:i + 1])) for i in range(net.N)] + [W]
    shift = [L - W for L in lens]
    qs = [L // le if L % le == 0 else 0 for L in lens]
    assert any(qs) and not all(qs)                              # both branches of _conditon
    en = [torch.nn.functional.conv1d(enc, w_, b_)[0].numpy() for w_, b_ in cond]                # [C][le]
    fg = np.stack([np.concatenate([e[D:], e[:D]], 0).T for e in en[:net.N]])[None].astype(np.float64)      # [1][N][le][f | g]
    p1 = en[net.N].T[None].astype(np.float64)
    # the recurrence starts from an all-zero state at sample 0 and is forced through the clip: the forward has no output before
    # position rf - 1 (pos0 = -(rf - 1): those steps are priming steps and are not compared), and from there on nothing the
    # zero state touched is inside any stage's receptive field
    start = rf - 1
    rings0 = [np.zeros((1, (k - 1) * d, R)) for d in dil]
    prev0 = np.zeros((1, k - 1, Q), np.float32)
    c = dict(fg=fg, p1=p1, shift=shift, q=qs, le=le, pos0=-start)
    out = dr.decode_ref(net, rings0, _onehot(codes[:1], Q), prev0, T, step0=0, forced=codes[None, 1:T + 1], cond=c)
    # step s consumes input sample s: output position s - (rf - 1)
    assert np.abs(out["probs"][0, start:] - p_ref).max() < TOL


# ================================================================================================ the GPU table's conditions
def test_gpu_table_reaches_every_form():
    for ln in gk.check_forms():
        print(ln)


@pytest.mark.parametrize("cid", gk.IDS)
def test_gpu_case_conditions(cid):
    """From the references alone: the loss of the f16 lo halves is at least 16 bars away on the rings and on the relative
    probabilities; every reference probability (inside its window) is at least 1e-6; no logit is above 8."""
    c = gk.CASE[cid]
    ref, err = gk.refs(cid)
    fams = sorted({gk._route(c, n, t0, ks)[0] for n in gk._launches(c) for t0, ks in ((1, -1), (0, -1), (1, 1), (1, 8))})
    p = ref["probs"]
    pmin, lmax = float(p[p > 0].min()), float(np.abs(ref["logits"]).max())
    print("%s: min p %.2e, max |logit| %.2f" % (cid, pmin, lmax))
    for what in ("probs", "rings"):
        e = err[what]
        if (what == "probs" and c["Q"] == 1) or (what == "rings" and c["k"] == 1):
            # constant by construction (one probability of 1; no rings): compared exactly, the case's other tensor carries the condition
            assert e["e32"] == e["ex3"] == e["ex1"] == 0
            continue
        for fam in fams:
            b = dr.bar(e, fam)
            print("  %-5s %-2s e32 %.2e ex3 %.2e ex1 %.2e  bar %.2e  ex1 / bar %.0f" % (what, fam, e["e32"], e["ex3"], e["ex1"], b, e["ex1"] / b if b else 0))
            assert e["ex1"] >= 16 * b, (cid, what, fam)
    inside = np.zeros(p.shape, bool)
    for s in range(c["n"]):
        lo, hi = c["win"][(c["win_pos0"] + s) % len(c["win"])] if c["win"] else (0, c["Q"])
        inside[:, s, lo:hi] = True
    assert (p[inside] >= 1e-6).all() and (p[~inside] == 0).all()
    assert lmax <= 8
