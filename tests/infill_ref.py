"""Float64 restatement of partially forced decode (include/wavenet_hip.h, wn_decode: "PARTIALLY FORCED DECODE"), the masks of its GPU
tests and what both test levels share.  Not a test module.

The rule, per utterance u and step s of a launch: mask[u][s] >= 0 - the input column after step s is that code; mask[u][s] < 0 - it
is the code the launch chose at step s.  Nothing else depends on the mask: the codes and probabilities reported are the model's own
at every step.

`masked_ref` steps tests/decode_ref.decode_ref one sample at a time, the way tests/cfg_ref.guided_ref does - so the recurrence is
decode_ref's own, in each of its arithmetic modes -, asks it for the step's code and feeds the RESOLVED code on: that step's `forced`.
`masked_guided_ref` steps cfg_ref.guided_ref the same way for (conditional, unconditional) pairs of rows.  decode_ref.py itself is not
touched.  tests/test_infill_ref.py holds both to decode_ref / guided_ref: with no negative entry they are the fully forced run, with
all -1 the free run, bit for bit.

The GPU tests need no top-2 margin: their reference is fed `resolve(mask, the kernel's own codes)`, a stream without a negative entry,
for which the masked recurrence IS decode_ref(forced=) - every step is still checked against float64."""
import numpy as np

from tests import cfg_ref as cr
from tests import decode_ref as dr


def resolve(mask, codes):
    """the fed stream: the mask's code where it holds one, else the launch's own"""
    mask, codes = np.asarray(mask), np.asarray(codes)
    return np.where(mask >= 0, mask, codes).astype(np.int64)


def _onehot(codes, Q):
    note = np.zeros((len(codes), Q))
    note[np.arange(len(codes)), codes] = 1.0
    return note


def masked_ref(net, rings, note0, prev0, n_steps, mask, step0=0, push_input=1, cond=None, temperature=0.0, windows=None, win_pos0=0,
               mode="64"):
    """n_steps of the masked recurrence for U utterances.  Arguments as decode_ref's, `mask` [U][n_steps] integers in place of
    `forced` (None: every step free).  Returns decode_ref's dict and `fed` [U][n_steps], the stream that was fed."""
    k, Q = net.k, net.Q
    U = note0.shape[0]
    mask = np.full((U, n_steps), -1, np.int64) if mask is None else np.asarray(mask)
    assert mask.shape == (U, n_steps)
    rings = [np.asarray(r, dtype=np.float64).copy() for r in rings]
    note = np.asarray(note0, dtype=np.float64).copy()
    prev = np.asarray(prev0, dtype=np.float64).copy() if k > 1 else None
    probs, logits = np.zeros((U, n_steps, Q)), np.zeros((U, n_steps, Q))
    codes, fed = np.zeros((U, n_steps), dtype=np.int64), np.zeros((U, n_steps), dtype=np.int64)
    for s in range(n_steps):
        c_s = None if cond is None else dict(cond, pos0=cond["pos0"] + s)
        o = dr.decode_ref(net, rings, note, prev, 1, step0=step0 + s, push_input=push_input, cond=c_s, temperature=temperature,
                          windows=windows, win_pos0=win_pos0 + s, mode=mode)
        rings = o["rings"]
        probs[:, s], logits[:, s], codes[:, s] = o["probs"][:, 0], o["logits"][:, 0], o["codes"][:, 0]
        fed[:, s] = resolve(mask[:, s], codes[:, s])                 # this step's `forced`
        if k > 1:
            prev = np.concatenate([prev[:, 1:], note[:, None]], 1)
        note = _onehot(fed[:, s], Q)
    return dict(probs=probs, logits=logits, codes=codes, fed=fed, rings=rings, note_out=note,
                prev_out=prev if k > 1 else np.zeros((U, 0, Q)))


def masked_guided_ref(net, rings, note0, prev0, n_steps, guidance, mask, step0=0, cond=None, temperature=0.0, windows=None, win_pos0=0,
                      mode="64"):
    """The same for U = 2 P rows under guidance [P]: `mask` [U][n_steps] holds equal rows for the two members of a pair (row 2j's
    is read).  Returns guided_ref's dict (probs, g, codes per PAIR) and `fed` [P][n_steps]."""
    k, Q = net.k, net.Q
    U = note0.shape[0]
    P = U // 2
    mask = np.full((U, n_steps), -1, np.int64) if mask is None else np.asarray(mask)
    assert mask.shape == (U, n_steps) and np.array_equal(mask[0::2], mask[1::2])
    rings = [np.asarray(r, dtype=np.float64).copy() for r in rings]
    note = np.asarray(note0, dtype=np.float64).copy()
    prev = np.asarray(prev0, dtype=np.float64).copy() if k > 1 else None
    probs, gs, logits = np.zeros((P, n_steps, Q)), np.zeros((P, n_steps, Q)), np.zeros((U, n_steps, Q))
    codes, fed, margin = np.zeros((P, n_steps), dtype=np.int64), np.zeros((P, n_steps), dtype=np.int64), float("inf")
    for s in range(n_steps):
        c_s = None if cond is None else dict(cond, pos0=cond["pos0"] + s)
        o = cr.guided_ref(net, rings, note, prev, 1, guidance, step0=step0 + s, cond=c_s, temperature=temperature, windows=windows,
                          win_pos0=win_pos0 + s, mode=mode)
        rings = o["rings"]
        probs[:, s], gs[:, s], logits[:, s], codes[:, s] = o["probs"][:, 0], o["g"][:, 0], o["logits"][:, 0], o["codes"][:, 0]
        margin = min(margin, o["margin"])
        fed[:, s] = resolve(mask[0::2, s], codes[:, s])
        if k > 1:
            prev = np.concatenate([prev[:, 1:], note[:, None]], 1)
        note = _onehot(np.repeat(fed[:, s], 2), Q)
    return dict(probs=probs, g=gs, logits=logits, codes=codes, fed=fed, margin=margin, rings=rings, note_out=note,
                prev_out=prev if k > 1 else np.zeros((U, 0, Q)))


# ---------------------------------------------------------------------------------------------- the masks of the GPU tests
MASKS = ("stage_prefix", "alternate", "prompt3", "last_only", "per_row")


def make_mask(kind, stream, lo=None, hi=None):
    """A mask [U][n] over `stream` [U][n], a stream of valid codes (inside every step's window where the case has one): the kept
    entries are the stream's, the others -1.
      stage_prefix: steps with s % 4 < 2 are kept (the first 2 of 4 stages of a frame-major token stream);
      alternate:    every other step is kept, starting with a kept one;
      prompt3:      a forced prompt of 3 steps, then free;
      last_only:    free except the last step;
      per_row:      every row its own pattern, so that inside one group of eight a row forced at step s sits next to a row free at
                    step s: row u keeps step s when (s + u) % 3 == 0."""
    stream = np.asarray(stream)
    U, n = stream.shape
    s, u = np.arange(n)[None, :], np.arange(U)[:, None]
    keep = {"stage_prefix": (s % 4 < 2) & (u >= 0), "alternate": (s % 2 == 0) & (u >= 0), "prompt3": (s < 3) & (u >= 0),
            "last_only": (s == n - 1) & (u >= 0), "per_row": (s + u) % 3 == 0}[kind]
    return np.where(keep, stream, -1).astype(np.int32)


def pair_mask(kind, stream):
    """the same for guided rows: pair j's pattern on both of its rows (`stream` [2 P][n] holds equal rows per pair)"""
    m = make_mask(kind, np.asarray(stream)[0::2])
    return np.repeat(m, 2, 0)


def in_window_stream(rng, U, n, Q, windows, win_pos0):
    """[U][n] random codes, step s inside pair (win_pos0 + s) % len(windows) of the table (None: the whole alphabet)"""
    out = np.zeros((U, n), np.int32)
    for s in range(n):
        lo, hi = windows[(win_pos0 + s) % len(windows)] if windows else (0, Q)
        out[:, s] = rng.integers(lo, hi, U)
    return out
