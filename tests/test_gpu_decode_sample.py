"""Top-k / nucleus sampling in the decoder (ABI 8: wn_sample_logits, wn_decode_batch_samp) against tests/sampling_ref.py, the
float64 restatement of the rule in include/wavenet_hip.h.

Bars.  Kept sets are decided on the logits and must be EXACT; the only excuse is a top-p boundary: a candidate threshold whose
float64 head mass lies within 1e-5 of top_p may round to either side, at most 2 % of a case's rows (the seeded rows are
counted on the CPU in tests/test_sampling_ref.py).  Probabilities: 1e-6 absolute (fp32 exp and two roundings of the
normalisation on values <= 1).  An entry the rule keeps may come back as an exact zero only where fp32 cannot hold it
(float64 probability below 1e-30: exp underflow).  Draws: the code is the inverse CDF of the RETURNED distribution for the
restated uniform number, within the +-1e-5 band tests/test_gpu_parity.py uses for the plain sampled decode.
At decode level the logits are not returned, so the expected kept set comes from the PLAIN run's probabilities of the same
teacher-forced steps: distinct logits can round to one probability, hence {p > v} <= support <= {p >= v} at a boundary value v.
Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sampling_ref as sr
from tests.helpers import ROOT

P_TOL = 1e-6
BAND = 1e-5
TINY = 1e-30


# ------------------------------------------------------------------------------------------------ (a) the sampler alone
def _check_rows(rows, T, top_k, top_p, u, codes, probs):
    """every row of one wn_sample_logits launch against the rule; returns the number of excused rows"""
    excused = 0
    for i in range(rows.shape[0]):
        k = top_k[i] if np.ndim(top_k) else top_k
        p = top_p[i] if np.ndim(top_p) else top_p
        ref = sr.sample_row(rows[i], T[i], k, p)
        sup = probs[i] > 0
        l64 = rows[i].astype(np.float64)
        e = np.exp((l64 - l64.max()) / (T[i] if T[i] > 0 else 1.0))
        which = None
        for j, cand in enumerate(ref.alt):                  # the rule's set first, then what a boundary row may round to
            full = np.where(cand, e, 0.0)
            full = full / full.sum()
            if not (sup & ~cand).any() and (full[cand & ~sup] < TINY).all():
                which, r = j, full
                break
        assert which is not None, ("kept set", i, k, p, np.nonzero(sup)[0][:12], np.nonzero(ref.N)[0][:12])
        excused += which > 0
        assert np.abs(probs[i] - r).max() < P_TOL, (i, k, p, np.abs(probs[i] - r).max())
        c = int(codes[i])
        kept = ref.alt[which]
        assert 0 <= c < rows.shape[1] and kept[c], ("code outside the kept set", i, k, p, c, float(u[i]))
        if T[i] > 0:
            cdf = np.cumsum(probs[i].astype(np.float64))
            lo = cdf[c - 1] if c > 0 else 0.0
            assert lo - BAND <= u[i] < cdf[c] + BAND or (u[i] >= cdf[-1] - BAND and c == np.nonzero(kept)[0][-1]), (i, c, float(u[i]), lo, cdf[c])
        else:
            assert c == int(np.argmax(rows[i]))
    return excused


@pytest.mark.parametrize("Q", sr.QS)
def test_sampler_follows_the_rule(Q):
    """wn_sample_logits on 200 seeded rows per case (random at four scales, exact ties on and around the k boundary, -inf
    entries, one dominating logit), every top_k x top_p of the issue in the scalar form, u = 0, 0.5, 1 - 2^-24 and random:
    kept set exact, probabilities within 1e-6, code = inverse CDF of the returned row and always inside the kept set."""
    from music_amd import fast_generate as fg
    rows, u = sr.make_rows(Q)
    T = sr.temperatures(sr.ROWS)
    x = torch.from_numpy(rows).cuda()
    worst = 0
    plain = {}
    for k in sr.top_ks(Q):
        for p in sr.TOP_P:
            codes, probs = fg.sample_logits(x, temperature=T.tolist(), top_k=k, top_p=p, u=u, want_probs=True)
            codes, probs = codes.cpu().numpy(), probs.cpu().numpy()
            n = _check_rows(rows, T, k, p, u, codes, probs)
            assert n <= sr.EXCUSED_CAP * sr.ROWS, (k, p, n)
            worst = max(worst, n)
            if p == 1.0 and (k <= 0 or k >= Q):
                plain[k] = (codes, probs)
    # filters off, however it is said: the plain temperature path, bit for bit
    c0, p0 = plain[0]
    for k, (c, pr) in plain.items():
        assert np.array_equal(c, c0) and np.array_equal(pr.view(np.int32), p0.view(np.int32)), k
    # top_k = 1 with top_p = 1e-6: the argmax (the first index when u = 0 or the maximum is unique; always one of the maxima)
    for uu in (u, np.zeros_like(u)):
        codes = fg.sample_logits(x, temperature=T.tolist(), top_k=1, top_p=1e-6, u=uu).cpu().numpy()
        for i in range(sr.ROWS):
            m = rows[i] == rows[i].max()
            assert m[codes[i]], i
            if m.sum() == 1 or uu[i] == 0:
                assert codes[i] == int(np.argmax(rows[i])), i
    print("Q = %d: %d x %d cases of %d rows, at most %d rows excused per case" % (Q, len(sr.top_ks(Q)), len(sr.TOP_P), sr.ROWS, worst))


@pytest.mark.parametrize("Q", [1, 65, 256, 1000])
def test_sampler_per_row_tables_and_generated_uniforms(Q):
    """A per-row table with mixed greedy and sampled rows, distinct filters, seeds and streams: every row follows ITS entry,
    with the uniform number restated on the CPU (splitmix64 of (seed, step0 + row, stream)); a strided logits matrix."""
    from music_amd import fast_generate as fg
    rows, _ = sr.make_rows(Q, seed=5)
    rng = np.random.default_rng(Q)
    n = sr.ROWS
    T = sr.temperatures(n, 1)
    T[rng.random(n) < 0.25] = 0.0                                     # greedy rows
    ks = rng.choice(sr.top_ks(Q), size=n)
    ps = rng.choice([1.0, 0.9, 0.5, 0.05], size=n)
    seeds = [int(v) for v in rng.integers(0, 2 ** 63, size=n)]
    streams = [int(v) for v in rng.integers(0, 2 ** 32, size=n)]
    step0 = 2 ** 33 + 11
    wide = torch.zeros(n, Q + 3).cuda()
    wide[:, :Q] = torch.from_numpy(rows).cuda()
    codes, probs = fg.sample_logits(wide[:, :Q], temperature=T.tolist(), top_k=ks.tolist(), top_p=ps.tolist(), seed=seeds, step0=step0,
                                    streams=streams, want_probs=True)
    u = np.array([sr.uniform(seeds[i], step0 + i, streams[i]) for i in range(n)])
    excused = _check_rows(rows, T, ks, ps, u, codes.cpu().numpy(), probs.cpu().numpy())
    assert excused <= sr.EXCUSED_CAP * n, excused
    # the scalar form draws row i as step step0 + i of stream 0
    c2, p2 = fg.sample_logits(wide[:, :Q], temperature=0.8, top_k=3, top_p=0.7, seed=9, step0=4, want_probs=True)
    u2 = np.array([sr.uniform(9, 4 + i, 0) for i in range(n)])
    assert _check_rows(rows, np.full(n, 0.8, np.float32), 3, 0.7, u2, c2.cpu().numpy(), p2.cpu().numpy()) <= sr.EXCUSED_CAP * n
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(ValueError):
            fg.sample_logits(wide[:, :Q], **bad)


# ------------------------------------------------------------------------------------------------ decode level
def _model(S=256, Q=256, k=2, R=64, D=64, dil=(1, 2, 4, 8, 16), bias=False, seed=41):
    from music_amd.model import wavenet
    torch.manual_seed(seed)
    net = wavenet(filter_width=k, dilations=list(dil), dilation_channels=D, residual_channels=R, skip_channels=S,
                  quantization_channels=Q, use_bias=bias)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)                                                # so that the distribution is not flat
    return net.cuda()


def _state(net, U, n, seed=42):
    """random queues, one-hot input columns and forced codes for U utterances"""
    from music_amd import fast_generate as fg
    dev = torch.device("cuda", 0)
    eng = net._engine_for(dev)
    rng = np.random.default_rng(seed)
    rw, K1, Q = fg._ring_width(eng), fg._taps(eng), eng.Q
    rings = torch.from_numpy(rng.standard_normal((U, max(1, sum(K1 * d * rw for d in eng.dil)))).astype(np.float32)).to(dev)
    prev = torch.zeros(U, K1, Q, device=dev)
    note = torch.zeros(U, Q, device=dev)
    for uu in range(U):
        for j in range(K1):
            prev[uu, j, int(rng.integers(0, Q))] = 1.0
        note[uu, int(rng.integers(0, Q))] = 1.0
    forced = torch.from_numpy(rng.integers(0, Q, size=(U, n)).astype(np.int32))
    return eng, rings, prev, note, forced


def _run(net, st, n, forced=True, step0=3, **kw):
    from music_amd import fast_generate as fg
    eng, rings, prev, note, f = st
    r = rings.clone()
    codes, probs, note_out, prev_out = fg.decode_batch_cond(net, r, prev.clone(), note.clone(), n, step0=step0, forced=f if forced is True else forced,
                                                            want_probs=True, **kw)
    return codes.cpu().numpy(), probs.cpu().numpy(), note_out.cpu(), prev_out.cpu(), r.cpu()


def _bounds(p, top_k, top_p):
    """(must, may, near): the kept set of the rule applied to a plain run's fp32 probabilities p (one step).  Distinct logits
    may share a probability, so entries AT a boundary value may or may not be kept; near: a head mass within BAND of top_p."""
    Q = p.size
    p = p.astype(np.float64)
    must, may, near = np.ones(Q, bool), np.ones(Q, bool), False
    if 0 < top_k < Q:
        v = np.sort(p)[Q - top_k]
        must, may = p > v, p >= v
    if 0.0 < top_p < 1.0:
        outs = []
        for K in ([must, may] if (must != may).any() and must.any() else [may]):
            pk = np.where(K, p, 0.0)
            pk = pk / pk.sum()
            order = np.argsort(-pk, kind="stable")
            cs = np.cumsum(pk[order])
            vals = pk[order]
            last = np.nonzero(np.append(vals[1:] != vals[:-1], True))[0]
            mass = cs[last]
            near = near or bool((np.abs(mass - top_p) < BAND).any())
            j = np.nonzero(mass >= top_p)[0]
            tau = vals[last[j[0]]] if j.size else 0.0
            outs.append((K & (pk > tau), K & (pk >= tau) & (pk > 0)))
        must = np.logical_and.reduce([o[0] for o in outs]) & must
        may = np.logical_or.reduce([o[1] for o in outs])
    return must, may, near


def _check_decode(p_plain, p_trunc, codes, T, top_k, top_p, seed, step0, stream, what):
    """one utterance's truncated run against its plain run at the same temperature (teacher-forced, same codes fed)"""
    n, Q = p_plain.shape
    excused = 0
    for t in range(n):
        must, may, near = _bounds(p_plain[t], top_k, top_p)
        sup = p_trunc[t] > 0
        ok = not (must & ~sup & (p_plain[t] > TINY)).any() and not (sup & ~may).any()
        if not ok and near:
            excused += 1
            continue
        assert ok, (what, t, np.nonzero(sup)[0], np.nonzero(must)[0], np.nonzero(may)[0])
        ref = np.where(sup, p_plain[t].astype(np.float64), 0.0)
        ref /= ref.sum()
        assert np.abs(p_trunc[t] - ref).max() < P_TOL, (what, t, np.abs(p_trunc[t] - ref).max())
        u = sr.uniform(seed, step0 + t, stream)
        cdf = np.cumsum(p_trunc[t].astype(np.float64))
        c = int(codes[t])
        lo = cdf[c - 1] if c > 0 else 0.0
        assert sup[c] and lo - BAND <= u < cdf[c] + BAND, (what, t, c, u, lo, cdf[c])
    assert excused <= sr.EXCUSED_CAP * n, (what, excused)
    return excused


SETTINGS = [(1.0, 5, 1.0), (0.8, 0, 0.9), (1.3, 40, 0.5), (1.0, 1, 1e-6), (0.7, 255, 0.97)]


def _forced_forms(net, n, settings=SETTINGS, Q=256, step0=3):
    st = _state(net, 1, n)
    for T, k, p in settings:
        cp, pp, _, _, _ = _run(net, st, n, step0=step0, temperature=T, seed=17)
        ct, pt, _, _, _ = _run(net, st, n, step0=step0, temperature=T, seed=17, top_k=k, top_p=p)
        assert np.abs(pp.sum(2) - 1).max() < 1e-5 and np.abs(pt.sum(2) - 1).max() < 1e-5
        ex = _check_decode(pp[0], pt[0], ct[0], T, k, p, 17, step0, 0, (T, k, p))
        kept = (pt[0] > 0).sum(1)
        print("T %.1f top_k %d top_p %g: %d steps, kept %d..%d entries, %d excused" % (T, k, p, n, kept.min(), kept.max(), ex))
        if 0 < k < Q and p >= 1.0:
            assert kept.min() >= k and kept.max() <= k + 2
        if k == 1:
            assert (ct[0] == pp[0].argmax(1)).all()
    return True


def test_matrix_core_decode_truncates_like_the_rule():
    """64 / 64 / 256 / 256, dilations 1..16, 300 teacher-forced steps, plain at T and truncated with the same forced codes."""
    from music_amd import fast_generate as fg
    net = _model()
    assert fg._mfma_decode(net._engine_for(torch.device("cuda", 0)))
    _forced_forms(net, 300)


def test_filters_off_through_the_new_entry_point_is_the_old_one_bit_for_bit():
    """wn_decode_batch_samp with the filters off - in its scalar form (top_k = Q says "off") and through a table - against
    wn_decode_batch_cond: codes, probability bits, handed-back columns and queues, forced and free-running, sampled and greedy."""
    net = _model(bias=True)
    n, U = 60, 3
    st = _state(net, U, n)
    for forced in (True, None):
        for T in (0.9, None):
            old = _run(net, st, n, forced=forced, temperature=T, seed=23)
            scalar = _run(net, st, n, forced=forced, temperature=T, seed=23, top_k=256)
            table = _run(net, st, n, forced=forced, temperature=[T or 0.0] * U, seed=[23] * U)
            for new in (scalar, table):
                assert np.array_equal(old[0], new[0]) and np.array_equal(old[1].view(np.int32), new[1].view(np.int32))
                assert torch.equal(old[2], new[2]) and torch.equal(old[3], new[3]) and torch.equal(old[4], new[4])
    assert len(np.unique(old[0])) > 1


def _table_rows(U):
    from music_amd import fast_generate as fg
    net = _model()
    n = 48
    eng, rings, prev, note, forced = _state(net, U, n, seed=50 + U)
    rings[1], prev[1], note[1] = rings[0], prev[0], note[0]           # rows 0 and 1: same state, same settings, other seed
    rng = np.random.default_rng(U)
    T = [float(v) for v in rng.choice([0.0, 0.6, 1.0, 1.4], size=U)]
    K = [int(v) for v in rng.choice([0, 1, 3, 40, 300], size=U)]
    Pn = [float(v) for v in rng.choice([1.0, 0.95, 0.6], size=U)]
    S = [int(v) for v in rng.integers(0, 2 ** 62, size=U)]
    T[0] = T[1] = 1.0
    K[0] = K[1] = 40
    Pn[0] = Pn[1] = 0.95
    T[2] = 0.0
    st = (eng, rings, prev, note, forced)
    full = _run(net, st, n, forced=None, temperature=T, top_k=K, top_p=Pn, seed=S)
    assert not np.array_equal(full[0][0], full[0][1])
    for uu in range(U):
        one = (eng, rings[uu:uu + 1], prev[uu:uu + 1], note[uu:uu + 1], None)
        if T[uu] > 0:
            single = _run(net, one, n, forced=None, temperature=[T[uu]], top_k=[K[uu]], top_p=[Pn[uu]], seed=[S[uu]], streams=[uu])
        else:
            single = _run(net, one, n, forced=None)
        assert np.array_equal(full[0][uu], single[0][0]), uu
        assert np.array_equal(full[1][uu].view(np.int32), single[1][0].view(np.int32)), uu
        assert torch.equal(full[4][uu], single[4][0]) and torch.equal(full[2][uu], single[2][0]), uu
        if T[uu] > 0 and (0 < K[uu] < 256 or Pn[uu] < 1):
            kept = (full[1][uu] > 0).sum(1)
            assert kept.max() < 256
            if 0 < K[uu] < 256:
                assert kept.max() <= K[uu] + 2


@pytest.mark.parametrize("U,ks", [(24, "1"), (9, "1"), (9, "4")])
def test_every_row_of_a_table_is_its_own_single_launch(U, ks):
    """U = 24 (eight per workgroup pair) and 9 (spare columns mirror the last utterance): rows with distinct (T, top_k, top_p,
    seed), some greedy; row u equals the single-utterance launch with that row's entry and streams=[u] exactly, greedy rows the
    greedy launch, and two rows with the same settings and state but different seeds differ.
    Left to its defaults the library runs ONE pair's skip stage split over four workgroups and several pairs' in one workgroup
    each (decode); the two forms add the post-processing products up in different orders, so a batch and a single
    launch are only comparable bit for bit in the SAME form: WN_DEC_KS (read once per process, hence the child process) holds
    it fixed - the one-workgroup form at both sizes, the split form at U = 9."""
    e = dict(os.environ, WN_DEC_KS=ks, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from tests.test_gpu_decode_sample import _table_rows; _table_rows(%d)" % U
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, check=True, timeout=600)


def test_fp32_kernel_general_plan():
    """the fp32 kernel: a general-plan model with Q = 100 and filter width 3"""
    from music_amd import fast_generate as fg
    net = _model(S=48, Q=100, k=3, R=24, D=20, dil=(1, 2, 4, 1), bias=True)
    assert not fg._mfma_decode(net._engine_for(torch.device("cuda", 0)))
    _forced_forms(net, 120, settings=[(1.0, 5, 1.0), (0.8, 0, 0.9), (1.2, 30, 0.5), (1.0, 99, 0.99)], Q=100)


def test_split_skip_stage():
    """512 skip channels: the skip stage split over eight workgroups, part 0 chooses"""
    from music_amd import fast_generate as fg
    net = _model(S=512)
    assert fg._mfma_decode(net._engine_for(torch.device("cuda", 0)))
    _forced_forms(net, 120, settings=SETTINGS[:3])


def _child_fp32():
    from music_amd import fast_generate as fg
    net = _model()
    assert not fg._mfma_decode(net._engine_for(torch.device("cuda", 0)))
    _forced_forms(net, 120, settings=SETTINGS[:3])


def test_fp32_kernel_at_the_matrix_core_shape():
    """WN_DEC_MFMA=0 (a process-wide switch: child process): decode_k with its compile-time 256-entry sampler"""
    e = dict(os.environ, WN_DEC_MFMA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from tests.test_gpu_decode_sample import _child_fp32; _child_fp32()"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, check=True, timeout=600)


def test_conditioned_resynthesis_with_per_clip_settings():
    """ae_generate.resynthesize on two clips with their own tables AND their own sampling settings (teacher-forced): each clip's
    truncated run against its plain run at its temperature, drawn from its own stream."""
    from music_amd import ae_generate as ag
    from tests.test_gpu_decode_cond import _build
    net, params, cfg, x, cond = _build("batch3")
    x = x[:2].contiguous()
    T, K, Pn, S = [0.9, 1.2], [5, 0], [1.0, 0.8], [3, 4]
    _, pp, _ = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True, temperature=T, seed=S)
    ct, pt, _ = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True, temperature=T, seed=S, top_k=K, top_p=Pn)
    rf = net.receptive_field
    pp, pt, ct = pp.cpu().numpy(), pt.cpu().numpy(), ct.cpu().numpy()
    for b in range(2):
        _check_decode(pp[b], pt[b], ct[b], T[b], K[b], Pn[b], S[b], rf - 1, b, "clip %d" % b)
    assert (pt[0] > 0).sum(1).max() <= 7 and (pt[1] > 0).sum(1).max() < 256


def test_free_running_top_k_stays_in_the_top_k():
    """200 free-running steps with top_k = 4: every generated code lies in the top 4 of a teacher-forced plain replay of the
    same codes from the same state; the run is not the greedy one and repeats for its seed."""
    net = _model()
    n = 200
    st = _state(net, 1, n, seed=77)
    run = _run(net, st, n, forced=None, temperature=1.0, seed=5, top_k=4)
    again = _run(net, st, n, forced=None, temperature=1.0, seed=5, top_k=4)
    greedy = _run(net, st, n, forced=None)
    assert np.array_equal(run[0], again[0]) and not np.array_equal(run[0], greedy[0])
    replay = _run(net, st, n, forced=torch.from_numpy(run[0].astype(np.int32)), temperature=1.0, seed=5)
    for t in range(n):
        p = replay[1][0, t]
        assert p[run[0][0, t]] >= np.sort(p)[-4], t
    assert len(np.unique(run[0])) > 4
