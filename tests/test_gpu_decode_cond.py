"""Cached-queue decode with per-utterance conditioning tables (ABI 7, wn_decode_batch_cond; ae_generate.resynthesize): encode a
clip, regenerate it from an encoding of ANY number of pooled frames.

The reference is the float64 oracle's forward (oracle.autoencoder_forward: encoder, ``_conditon`` on every decoder block and
on the post-processing stage, same parameters and conditioning projections).  A decode step's probabilities are the softmax
over the Q channels of ONE output column, so they are compared with the softmax over the channel axis of the oracle's
pre-softmax (connection_2 applied to relu of the oracle's ``de_conn`` intermediate, in float64) - the reference's own chunk
softmax mixes channels and positions and has no per-sample counterpart; tests/test_gpu_decode_taps.py compares the
unconditioned decoder the same way.  Bar: 1e-3 on probabilities (README "parity").  Matrix-core against fp32 kernel: 1e-4, the
bar tests/test_gpu_decode_taps.py uses for that comparison.  The other kernel forms (WN_DEC_MFMA=0, WN_DEC_KS=1) are process-wide
switches of the library, so they run in a child process.  Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import wavenet_oracle as wo
from tests.helpers import ROOT

PROB_TOL = 1e-3          # README "parity"
KERNEL_TOL = 1e-4        # matrix-core vs fp32 kernel (tests/test_gpu_decode_taps.py)
ROLL_GAP = 1e-2          # ten times PROB_TOL: a legitimate deviation cannot flip an argmax


def _cfg(k, dil, en, bw, pool, de, bias):
    return dict(filter_width=k, quantization_channel=256, dilations=dil, en_residual_channel=en[0], en_dilation_channel=en[1],
                en_bottleneck_width=bw, en_pool_kernel_size=pool, de_residual_channel=de[0], de_dilation_channel=de[1],
                de_skip_channel=de[2], use_bias=bias)


TINY = [1, 2, 4, 8, 16, 1, 2, 4, 8]                     # receptive field 48
# name -> (config, clips, samples per clip, model seed, gain, gain of connection_2, matrix-core kernel expected)
CASES = {
    "tiny_le1": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), False), 1, 47 + 20, 11, 2.0, 4.0, True),
    "tiny_le1_bias": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), True), 1, 47 + 20, 12, 2.0, 4.0, True),
    "tiny_le3": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), False), 1, 47 + 50, 13, 2.0, 4.0, True),
    "tiny_le3_bias": (_cfg(2, TINY, (24, 20), 6, 16, (48, 40, 256), True), 1, 47 + 50, 14, 2.0, 4.0, True),
    "tiny_le5": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), False), 1, 47 + 85, 15, 2.0, 4.0, True),
    "tiny_le5_bias": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), True), 1, 47 + 85, 16, 2.0, 4.0, True),
    # W = 22, Le = 3: stage lengths 45 43 39 31 28 23 22 - three stretch, four tile
    "mixed": (_cfg(2, [1, 2, 4, 8, 3, 5], (32, 32), 8, 6, (64, 64, 256), True), 1, 46, 17, 2.0, 4.0, True),
    "batch3": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), True), 3, 47 + 50, 18, 2.0, 4.0, True),
    "k3_fp32": (_cfg(3, [1, 2, 4, 1, 2], (24, 20), 6, 7, (40, 36, 72), True), 2, 22 + 41, 19, 2.0, 4.0, False),
    "k3_matrix_core": (_cfg(3, [1, 2, 4, 1, 2], (24, 20), 6, 7, (40, 36, 256), False), 2, 22 + 41, 20, 2.0, 4.0, True),
    "s512": (_cfg(2, [1, 2, 4, 8, 16, 32] * 2, (32, 32), 16, 32, (32, 32, 512), False), 2, 127 + 100, 21, 2.2, 2.0, True),
    # the free-running roll-outs (seeds chosen on the CPU from the oracle's side, see ROLL below)
    "roll1": (_cfg(2, TINY, (24, 20), 6, 16, (64, 64, 256), True), 1, 47 + 220, 213, 2.0, 12.0, True),
    "roll3": (_cfg(2, TINY, (24, 20), 6, 16, (48, 40, 256), False), 3, 47 + 60, 239, 2.0, 20.0, True),
    "config4": (_cfg(2, [2 ** (i % 10) for i in range(30)], (64, 64), 64, 512, (64, 64, 256), False), 1, 16000, 6, 1.6, 12.0, True),
}


def _build(name, device=True):
    """(net on the device, float64 parameters, config, clips (B, Q, T) one-hot, conditioning projections)"""
    from music_amd.model1 import wavenet_autoencoder
    cfg, B, T, seed, gain, gain2, _ = CASES[name]
    torch.manual_seed(seed)
    net = wavenet_autoencoder(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gain)
        net.connection_2.weight.mul_(gain2)
    params = {k: v.detach().clone().double() for k, v in net.state_dict().items()}
    codes = np.random.default_rng(seed + 1000).integers(0, 256, size=(B, T))
    x = torch.zeros(B, 256, T)
    for b in range(B):
        x[b, torch.from_numpy(codes[b]), torch.arange(T)] = 1.0
    torch.manual_seed(seed + 2000)
    cond = net._draw_conditioning()
    return (net.cuda() if device else net), params, cfg, x, cond


def _rows(params, r1):
    """per-position probabilities (B, W, Q) from the oracle's ``de_conn``"""
    b2 = params.get("connection_2.bias")
    return torch.softmax(F.conv1d(F.relu(r1), params["connection_2.weight"], b2), 1).transpose(1, 2)


def _oracle(params, cfg, x, cond):
    inter = {}
    c64 = [(w.double(), b.double()) for w, b in cond]
    with torch.no_grad():
        _, enc = wo.autoencoder_forward(params, cfg["dilations"], x.double(), cfg["en_pool_kernel_size"], c64,
                                        filter_width=cfg["filter_width"], q=256, intermediates=inter)
        return _rows(params, inter["de_conn"]), enc


def _margin(p):
    top = torch.topk(p, 2).values
    return float(top[0] - top[1])


def _child(name, tmp_path, **env):
    """teacher-forced probabilities and codes of case `name` from a child process with the given switches"""
    out = os.path.join(str(tmp_path), "%s_%s.npz" % (name, "_".join("%s%s" % kv for kv in sorted(env.items()))))
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    code = "from tests.test_gpu_decode_cond import _child_main; _child_main(%r, %r)" % (name, out)
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, check=True, timeout=600)
    d = np.load(out)
    return torch.from_numpy(d["probs"]), torch.from_numpy(d["codes"]), int(d["mfma"])


def _child_main(name, out):
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    net, params, cfg, x, cond = _build(name)
    codes, probs, enc = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True)
    wnet, _ = ag.conditioned_decoder(net, cond)
    mfma = fg._mfma_decode(wnet._engine_for(torch.device("cuda", 0)))
    np.savez(out, probs=probs.cpu().numpy(), codes=codes.cpu().numpy(), mfma=int(mfma))


def _kernel_form(net, cond):
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    wnet, _ = ag.conditioned_decoder(net, cond)
    return fg._mfma_decode(wnet._engine_for(torch.device("cuda", 0)))


def _check_forced(name, probs, codes, p_ref):
    B, W, Q = p_ref.shape
    assert tuple(probs.shape) == (B, W, Q) and tuple(codes.shape) == (B, W)
    err = (probs.double().cpu() - p_ref).abs().max().item()
    print("%s: teacher-forced probability error %.2e over %d x %d positions, largest oracle probability %.3f"
          % (name, err, B, W, float(p_ref.max())))
    assert err < PROB_TOL, err
    assert abs(probs.sum(2).double().cpu() - 1).max().item() < 1e-4
    codes = codes.cpu()
    checked = 0
    for b in range(B):
        for j in range(W):
            if _margin(p_ref[b, j]) > 2 * PROB_TOL:
                assert int(codes[b, j]) == int(p_ref[b, j].argmax()), (b, j)
                checked += 1
    assert checked >= max(1, B * W // 8), checked
    return err


@pytest.mark.parametrize("name", [c for c in CASES if not c.startswith("roll")])
def test_teacher_forced_probabilities_match_the_float64_forward(name):
    """resynthesize(teacher_forced=True) on every clip of the case: each output position's probabilities equal the float64
    forward's within 1e-3 (every clip of a batch against ITS OWN encoding: the tables are per utterance), the encoding is the
    oracle's, and wherever the oracle's top two are more than 2e-3 apart the code is the oracle's argmax.
    Observed on an MI355X: see DESIGN.md (decode, "conditioned")."""
    from music_amd import ae_generate as ag
    torch.set_num_threads(8)
    net, params, cfg, x, cond = _build(name)
    codes, probs, enc = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True)
    assert _kernel_form(net, cond) == CASES[name][6]
    p_ref, enc_ref = _oracle(params, cfg, x, cond)
    W = x.size(2) - net.receptive_field + 1
    assert tuple(enc.shape) == tuple(enc_ref.shape) and enc.size(2) == W // cfg["en_pool_kernel_size"]
    assert (enc.double().cpu() - enc_ref).abs().max().item() < 1e-3 * max(1.0, enc_ref.abs().max().item())
    sched = ag.cond_schedule(net, W, enc.size(2))
    if name in ("mixed", "config4"):
        assert any(q > 0 for _, q, _ in sched) and any(q == 0 for _, q, _ in sched)
    _check_forced(name, probs, codes, p_ref)
    if x.size(0) > 1:
        # the clips differ, and so do their conditioning tables: clip 0's probabilities are not clip 1's
        assert (p_ref[0] - p_ref[1]).abs().max().item() > 10 * PROB_TOL


def test_s512_one_workgroup_form(tmp_path):
    """512 skip channels with the skip / post-processing stage in ONE workgroup (WN_DEC_KS=1; the default at this batch is the
    split form, which the parametrised case runs) against the float64 forward."""
    torch.set_num_threads(8)
    net, params, cfg, x, cond = _build("s512")
    probs, codes, mfma = _child("s512", tmp_path, WN_DEC_KS="1")
    assert mfma == 1
    p_ref, _ = _oracle(params, cfg, x, cond)
    _check_forced("s512 (one skip workgroup)", probs, codes, p_ref)


@pytest.mark.parametrize("name", ["tiny_le3_bias", "mixed", "batch3", "k3_matrix_core", "s512"])
def test_matrix_core_kernel_agrees_with_the_fp32_kernel(name, tmp_path):
    """The same case on the matrix-core kernel (this process) and on the fp32 kernel (child process, WN_DEC_MFMA=0):
    probabilities within 1e-4, the same codes wherever the top two are further apart than that."""
    from music_amd import ae_generate as ag
    net, params, cfg, x, cond = _build(name)
    cm, pm, _ = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True)
    assert _kernel_form(net, cond)
    pf, cf, mfma = _child(name, tmp_path, WN_DEC_MFMA="0")
    assert mfma == 0
    pm, cm = pm.cpu(), cm.cpu()
    err = (pm - pf).abs().max().item()
    print("%s: matrix-core vs fp32 kernel, largest probability difference %.2e" % (name, err))
    assert err < KERNEL_TOL, err
    for b in range(pf.size(0)):
        for j in range(pf.size(1)):
            if _margin(pf[b, j]) > KERNEL_TOL:
                assert int(cm[b, j]) == int(cf[b, j]), (b, j)


def _identity_once(S):
    from music_amd import fast_generate as fg
    from music_amd.model import wavenet
    torch.manual_seed(31)
    net = wavenet(filter_width=2, dilations=[1, 2, 4, 8, 16, 1, 2], dilation_channels=64, residual_channels=64, skip_channels=S,
                  quantization_channels=256, use_bias=True)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    net = net.cuda()
    dev = torch.device("cuda", 0)
    eng = net._engine_for(dev)
    rng = np.random.default_rng(32)
    n = 90
    rw = fg._ring_width(eng)
    rings = torch.from_numpy(rng.standard_normal(sum(d * rw for d in eng.dil)).astype(np.float32)).to(dev)
    prev = torch.zeros(256, device=dev)
    prev[7] = 1.0
    note = torch.zeros(256, device=dev)
    note[200] = 1.0
    forced = torch.from_numpy(rng.integers(0, 256, size=n).astype(np.int32))
    out = []
    for use_forced in (True, False):
        st = fg.DecodeState(eng, rings.clone(), prev.clone(), 5)
        c0, p0, n0 = fg._decode(net, st, note.clone(), n, forced=forced if use_forced else None, want_probs=True, correct_queue=True)
        r1 = rings.clone().view(1, -1)
        c1, p1, n1, v1 = fg.decode_batch_cond(net, r1, prev.clone().view(1, 1, 256), note.clone().view(1, 256), n, step0=5, pos0=-3,
                                              forced=forced.view(1, n) if use_forced else None, want_probs=True)
        assert torch.equal(c0, c1[0]) and torch.equal(p0.view(torch.int32), p1[0].view(torch.int32))
        assert torch.equal(n0, n1[0]) and torch.equal(st.prev.view(-1), v1.view(-1)) and torch.equal(st.rings, r1[0])
        out.append(fg._mfma_decode(eng))
    return out[0]


def test_null_tables_are_the_unconditioned_decoder_bit_for_bit(tmp_path):
    """wn_decode_batch_cond with NULL tables against wn_decode_batch_fw from the same state (random queues, biases, forced and
    free-running): identical codes, probability bits, handed-back input columns and queues - on the matrix-core kernel here,
    on the fp32 kernel both through a shape it alone serves and in a child process with WN_DEC_MFMA=0."""
    assert _identity_once(256) is True
    assert _identity_once(96) is False
    e = dict(os.environ, WN_DEC_MFMA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from tests.test_gpu_decode_cond import _identity_once; assert _identity_once(256) is False"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, check=True, timeout=600)


def test_one_frame_agrees_with_generate_cached():
    """Le = 1: the conditioning is constant, so resynthesize must agree with the decoder that folds it into the biases
    (cached_decoder / generate_cached).  The clip ends with its own first receptive field, so generate_cached (which starts
    from the LAST receptive field of its start piece) continues the same context under the same encoding: teacher-forced
    probabilities through the cached decoder within 1e-3 (not bit-equal: the bias is added in a different place), and the
    free-running codes equal generate_cached's up to the first position whose top two are closer than 2e-3."""
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    net, params, cfg, x, cond = _build("tiny_le1")
    rf = net.receptive_field
    x[:, :, -rf:] = x[:, :, :rf]
    W = x.size(2) - rf + 1
    n = W
    got, wnet, enc = ag.generate_cached(net, x, n, cond=cond)
    codes, probs, enc2 = ag.resynthesize(net, x, cond=cond, want_probs=True)
    assert enc2.size(2) == 1 and torch.equal(enc.cpu(), enc2.cpu())
    got, codes, pc = got.cpu().tolist(), codes[0].cpu().tolist(), probs[0].cpu()
    agreed = 0
    for j in range(n):
        if _margin(pc[j]) <= 2 * PROB_TOL:
            break
        assert got[j] == codes[j], (j, got[j], codes[j])
        agreed += 1
    print("one frame: %d of %d free-running codes equal generate_cached's before the first near-tie" % (agreed, n))
    assert agreed >= 10
    # teacher-forced through both decoders
    _, pt, _ = ag.resynthesize(net, x, cond=cond, teacher_forced=True, want_probs=True)
    cin = x[0].argmax(0)
    pred, st = fg.predict_next(wnet, x[:, :, :rf].cuda(), None)
    nxt = torch.cat([cin[rf + 1:], torch.zeros(1, dtype=cin.dtype)]).to(torch.int32)
    _, pw, _ = fg._decode(wnet, st, x[0, :, rf].contiguous().cuda(), W - 1, forced=nxt, want_probs=True, correct_queue=True)
    err = (pt[0, 1:] - pw).abs().max().item()
    print("one frame: resynthesize vs cached decoder, largest probability difference %.2e" % err)
    assert err < PROB_TOL, err
    if _margin(pt[0, 0].cpu()) > 2 * PROB_TOL:
        assert int(pred[0]) == int(pt[0, 0].argmax())


# (case, model seed override) whose float64 roll-out keeps its top two at least ROLL_GAP apart at every step: found on the CPU
# by running _oracle_rollout over seeds (the oracle's side only; nothing of the code under test enters the choice)
ROLL = [("roll1", 220), ("roll3", 60)]


def _oracle_rollout(params, cfg, x, cond, n):
    """greedy roll-out of the float64 decoder under the clip's encoding: the first receptive field is the clip's, every later
    sample the argmax of the previous position (the forward over the whole length, so the schedule is the whole clip's)"""
    k, dil = cfg["filter_width"], cfg["dilations"]
    rf = wo.receptive_field(k, dil)
    B, Q, T = x.shape
    W = T - rf + 1
    c64 = [(w.double(), b.double()) for w, b in cond]
    codes, gaps = [], []
    with torch.no_grad():
        enc = wo.autoencoder_encode(params, dil, x.double(), cfg["en_pool_kernel_size"])
        for b in range(B):
            xb = x[b:b + 1].double().clone()
            xb[:, :, rf:] = 0.0
            row = []
            for j in range(n):
                inter = {}
                wo.autoencoder_decode(params, dil, xb, enc[b:b + 1], W, c64, 256, intermediates=inter)
                p = _rows(params, inter["de_conn"])[0, j]
                gaps.append(_margin(p))
                c = int(p.argmax())
                row.append(c)
                if rf + j < T:
                    xb[0, c, rf + j] = 1.0
            codes.append(row)
    return codes, min(gaps)


@pytest.mark.parametrize("name,n", ROLL, ids=[r[0] for r in ROLL])
def test_free_running_codes_equal_the_float64_roll_out(name, n):
    """Greedy resynthesis over n positions (220 for the single clip: at least 200) equals the float64 oracle's roll-out code for
    code.  The oracle's top two stay at least 1e-2 apart at every rolled-out step (asserted here, from the oracle's side): ten
    times the probability bar, so no legitimate deviation can flip an argmax and no position is excused."""
    from music_amd import ae_generate as ag
    torch.set_num_threads(8)
    net, params, cfg, x, cond = _build(name)
    rf = net.receptive_field
    W = x.size(2) - rf + 1
    assert n == W
    want, gap = _oracle_rollout(params, cfg, x, cond, n)
    print("%s: smallest top-two gap of the oracle's roll-out %.3e over %d x %d steps" % (name, gap, x.size(0), n))
    assert gap >= ROLL_GAP, gap
    got, _, _ = ag.resynthesize(net, x, cond=cond)
    assert tuple(got.shape) == (x.size(0), W)
    for b in range(x.size(0)):
        assert got[b, :n].cpu().tolist() == want[b], b


def test_sampling_repeats_for_a_seed_and_the_error_flags_stay_zero():
    """With a temperature the same seed gives the same codes twice and another seed different ones; rows of a batch differ.
    Every launch above and here checks the error flag word of every utterance (decode_batch_cond raises WavenetHipError on a
    non-zero one); here the words are also read back directly from a launch of the entry point."""
    from music_amd import ae_generate as ag
    from music_amd import fast_generate as fg
    net, params, cfg, x, cond = _build("batch3")
    a, _, _ = ag.resynthesize(net, x, cond=cond, temperature=0.9, seed=5)
    b, _, _ = ag.resynthesize(net, x, cond=cond, temperature=0.9, seed=5)
    c, _, _ = ag.resynthesize(net, x, cond=cond, temperature=0.9, seed=6)
    g, _, _ = ag.resynthesize(net, x, cond=cond)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, g)
    assert not torch.equal(a[0], a[1]) and int(a.min()) >= 0 and int(a.max()) < 256
    assert fg.last_error_flags is not None and fg.last_error_flags.numel() == 3 and int(fg.last_error_flags.abs().max()) == 0
