"""Generation with a vq bottleneck (music_amd/ae_generate.py: encode_codes, decode_codes, the part they share with resynthesize;
tools/vq_codes_dataset.py): codes out of clips, clips out of codes, and the whole loop at toy size - encode a corpus to codes,
train a prior on the codes for a step, sample new codes, decode them to audio codes.  Run with -m gpu."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import ROOT
from tests.test_gpu_cond_learned import W, _build
from tests.test_gpu_vq_model import K, build_cpu


@functools.lru_cache(maxsize=None)
def _vq():
    """the long_encoding case of tests/test_gpu_vq_model.py (pool 8: 40 frames per clip), on the device, and its batch"""
    net, cfg, B, x, _ = build_cpu("long_encoding")
    return net.cuda(), cfg, B, x.cuda()


def test_encode_codes_is_the_forwards_assignment():
    from music_amd.ae_generate import encode_codes
    net, cfg, B, x = _vq()
    with torch.no_grad():
        net(x)
    want = net.vq_codes.clone()
    codes = encode_codes(net, x)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (B, W // cfg["en_pool_kernel_size"]) and torch.equal(codes, want)
    assert int(codes.min()) >= 0 and int(codes.max()) < K and codes.unique().numel() >= 3
    cont, _, _ = _build("fast64")
    with pytest.raises(ValueError, match="vq"):
        encode_codes(cont, x)


def test_decode_codes_reproduces_teacher_forced_resynthesis_bit_for_bit():
    from music_amd.ae_generate import decode_codes, encode_codes, resynthesize
    net, cfg, B, x = _vq()
    rf = net.receptive_field
    r_codes, r_probs, r_enc = resynthesize(net, x, teacher_forced=True, want_probs=True)
    assert torch.equal(net.vq_codes, encode_codes(net, x))                         # resynthesize exposes the codes; it decodes from q
    assert torch.equal(r_enc, net.vq_codebook.weight.detach()[net.vq_codes].permute(0, 2, 1))
    clip = x.argmax(1)                                                             # (B, rf - 1 + W)
    codes, probs = decode_codes(net, encode_codes(net, x), W, start=clip[:, :rf - 1], teacher_forced=clip, want_probs=True)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (B, W) and tuple(probs.shape) == (B, W, 256)
    assert torch.equal(codes, r_codes) and torch.equal(probs, r_probs)
    codes2, _ = decode_codes(net, encode_codes(net, x), W, teacher_forced=clip)    # start defaults to the clip's first rf - 1
    assert torch.equal(codes2, r_codes)


def test_resynthesis_of_a_continuous_model_goes_through_the_shared_path_unchanged():
    from music_amd import ae_generate
    net, cfg, B = _build("fast64")
    x = _vq()[3]
    rf = net.receptive_field
    for kw in (dict(teacher_forced=True), dict(teacher_forced=False), dict(teacher_forced=False, temperature=0.8, seed=5, top_k=40)):
        codes, probs, enc = ae_generate.resynthesize(net, x, want_probs=True, **kw)
        assert net.vq_codes is None and tuple(enc.shape) == (B, 16, W // 40)
        clip = x.argmax(1).to(torch.int32)
        forced = torch.cat([clip[:, rf:], torch.zeros(B, 1, dtype=torch.int32, device=x.device)], 1) if kw["teacher_forced"] else None
        samp = {k: v for k, v in kw.items() if k != "teacher_forced"}
        c2, p2 = ae_generate._decode_from_encoding(net, enc, net.conditioning_projections(), W, x[:, :, 0].contiguous(), clip[:, 1:rf],
                                                   forced, want_probs=True, **samp)
        assert torch.equal(codes, c2.to(torch.int64)) and torch.equal(probs, p2)


def test_free_running_decode_from_codes():
    from music_amd.ae_generate import decode_codes, encode_codes
    net, cfg, B, x = _vq()
    rf = net.receptive_field
    z = encode_codes(net, x)
    a, _ = decode_codes(net, z, W, temperature=1.0, seed=3)                        # start=None: primed with the mid code
    b, _ = decode_codes(net, z, W, temperature=1.0, seed=3)
    c, _ = decode_codes(net, z, W, temperature=1.0, seed=4)
    assert a.dtype == torch.int64 and tuple(a.shape) == (B, W) and int(a.min()) >= 0 and int(a.max()) < 256
    assert torch.equal(a, b) and not torch.equal(a, c)
    g1, _ = decode_codes(net, z, W)                                                # greedy
    g2, _ = decode_codes(net, z, W)
    assert torch.equal(g1, g2)
    s1, p1 = decode_codes(net, z, W, start=x.argmax(1)[:, :rf - 1], want_probs=True)   # a given start: the rf-th sample is the model's own
    assert tuple(s1.shape) == (B, W) and tuple(p1.shape) == (B, W, 256) and bool(torch.isfinite(p1).all())
    other, _ = decode_codes(net, z.flip(0), W)                                     # the codes matter
    assert not torch.equal(other, g1)
    # refusals: a code outside [0, K), a start of the wrong length, audio codes outside [0, Q)
    bad = z.clone()
    bad[0, 1] = K
    with pytest.raises(ValueError, match="outside"):
        decode_codes(net, bad, W)
    with pytest.raises(ValueError, match="start"):
        decode_codes(net, z, W, start=torch.zeros(B, rf, dtype=torch.int64))
    with pytest.raises(ValueError, match="teacher_forced"):
        decode_codes(net, z, W, teacher_forced=torch.full((B, rf - 1 + W), 256))


def test_corpus_to_codes_to_prior_to_audio_codes(tmp_path):
    """Two tiny pieces -> tools/vq_codes_dataset.encode_pieces -> a pickle audio_dataset reads -> one nll step of
    wavenet(quantization_channels=K) on the canonical one-hot -> generate_codes -> decode_codes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vq_codes_dataset
    from music_amd import fast_generate as fg
    from music_amd import objective
    from music_amd.ae_generate import decode_codes, encode_codes
    from music_amd.faster_audio_data import audio_data_loader, onehot_device
    from music_amd.model import wavenet
    net, cfg, B, x = _vq()
    rf, pool = net.receptive_field, cfg["en_pool_kernel_size"]
    rng = np.random.default_rng(0)
    pieces = [rng.integers(0, 256, size=rf - 1 + 70 * pool + 3).astype(np.int32), rng.integers(0, 256, size=rf - 1 + 41 * pool).astype(np.int32),
              rng.integers(0, 256, size=rf - 2).astype(np.int32)]
    seqs = vq_codes_dataset.encode_pieces(net, pieces, frames=32, batch=2, one_hot="canonical")
    assert [s.dtype for s in seqs] == [np.int32] * 3 and [s.shape for s in seqs] == [(70,), (41,), (0,)]
    assert all(s.min() >= 0 and s.max() < K for s in seqs[:2])
    # the windows' codes are the whole piece's
    whole = encode_codes(net, onehot_device(torch.from_numpy(pieces[0][None]).cuda(), 256, False))[0].cpu().numpy()
    assert np.array_equal(seqs[0], whole)
    path = str(tmp_path / "codes.pkl")
    with open(path, "wb") as f:
        pickle.dump([s for s in seqs if s.size], f)
    torch.manual_seed(0)
    prior = wavenet(2, [1, 2, 4], 32, 32, 32, K, False).cuda()
    win = 16
    loader = audio_data_loader(batch_size=2, shuffle=False, num_workers=0, pin_memory=False, one_hot="canonical", audio_path=path,
                               receptive_field=prior.receptive_field, window_length=win, cuda_available=True, quantization_channels=K)
    batch = next(iter(loader))
    piece, target = batch["audio_piece"], batch["audio_target"].view(-1)
    assert tuple(piece.shape) == (2, K, prior.receptive_field + win - 1)
    opt = torch.optim.Adam(prior.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in prior.parameters()]
    loss = objective.nll_loss(prior, piece, target)
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss)) and 0.5 * np.log(K) < float(loss.detach()) < 2.0 * np.log(K)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, prior.parameters()))
    start = torch.zeros(1, K, prior.receptive_field, device="cuda")
    start[:, K // 2, :] = 1.0
    n_new = 40
    new = fg.generate_codes(prior, start, n_new, correct_queue=True, temperature=1.0, seed=1)
    assert new.dtype == torch.int64 and tuple(new.shape) == (n_new,) and int(new.min()) >= 0 and int(new.max()) < K
    audio, _ = decode_codes(net, new[None], n_new * pool, temperature=1.0, seed=2)
    assert audio.dtype == torch.int64 and tuple(audio.shape) == (1, n_new * pool) and int(audio.min()) >= 0 and int(audio.max()) < 256
