"""Generation with a residual vq bottleneck of three stages (music_amd/ae_generate.py: encode_codes, decode_codes,
split_code_stream; tools/vq_codes_dataset.py): (B, S, Le) codes out of clips, clips out of codes - all stages and a prefix of them -
and the round trip through the interleaved token stream a prior is trained on.  Run with -m gpu."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import ROOT
from tests.test_gpu_cond_learned import W
from tests.test_gpu_rvq_model import K, S, build_cpu


@functools.lru_cache(maxsize=None)
def _rvq():
    """the long_encoding case of tests/test_gpu_rvq_model.py (pool 8: 40 frames per clip), on the device, and its batch"""
    net, cfg, B, x, _ = build_cpu("long_encoding")
    return net.cuda(), cfg, B, x.cuda()


def test_decode_codes_reproduces_teacher_forced_resynthesis_bit_for_bit():
    from music_amd.ae_generate import decode_codes, encode_codes, resynthesize
    net, cfg, B, x = _rvq()
    rf, Le = net.receptive_field, W // cfg["en_pool_kernel_size"]
    with torch.no_grad():
        net(x)
    want = net.vq_codes.clone()
    codes = encode_codes(net, x)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (B, S, Le) and torch.equal(codes, want)
    assert int(codes.min()) >= 0 and int(codes.max()) < K and all(codes[:, s].unique().numel() >= 3 for s in range(S))
    r_codes, r_probs, r_enc = resynthesize(net, x, teacher_forced=True, want_probs=True)
    assert torch.equal(net.vq_codes, codes)                                        # resynthesize exposes the codes; it decodes from q
    clip = x.argmax(1)                                                             # (B, rf - 1 + W)
    out, probs = decode_codes(net, codes, W, start=clip[:, :rf - 1], teacher_forced=clip, want_probs=True)
    assert out.dtype == torch.int64 and tuple(out.shape) == (B, W) and tuple(probs.shape) == (B, W, 256)
    assert torch.equal(out, r_codes) and torch.equal(probs, r_probs)
    eng = net._engine_for(x.device)
    assert torch.equal(eng.vq_lookup(codes), r_enc)                                # the lookup from codes alone: the forward's q, bit for bit


def test_a_prefix_of_the_stages_decodes_and_is_the_coarser_code():
    from music_amd.ae_generate import decode_codes, encode_codes
    net, cfg, B, x = _rvq()
    clip = x.argmax(1)
    with torch.no_grad():
        net(x)                                                                     # (leaves e in net.last_encoding_pre)
    codes = encode_codes(net, x)
    eng = net._engine_for(x.device)
    full, p_full = decode_codes(net, codes, W, teacher_forced=clip, want_probs=True)
    cb = net.vq_codebook.weight.detach()
    err = []
    for n in range(1, S + 1):
        out, probs = decode_codes(net, codes[:, :n], W, teacher_forced=clip, want_probs=True)
        assert tuple(out.shape) == (B, W) and bool(torch.isfinite(probs).all())
        assert torch.equal(probs, p_full) == (n == S), "a prefix of %d stages" % n
        q = eng.vq_lookup(codes[:, :n])
        want = None
        for s in range(n):                                                         # the partial sum in stage order
            row = cb[s * K:(s + 1) * K][codes[:, s]].permute(0, 2, 1)
            want = row if want is None else want + row
        assert torch.equal(q, want)
        err.append(float(((q - net.last_encoding_pre) ** 2).mean()))
    print("  mse of q against e with 1 .. %d stages: %s" % (S, ["%.4g" % e for e in err]))
    assert err[0] > err[-1]                                                        # more stages: nearer to e
    for bad in (codes[:, 0], codes[:, :0], torch.cat([codes, codes[:, :1]], 1)):   # (B, Le), no stage, S + 1 stages
        with pytest.raises(ValueError, match="codes must be"):
            decode_codes(net, bad, W)
    wrong = codes.clone()
    wrong[0, 1, 3] = K                                                             # stage 1's range is [0, K) too: K is stage 2's token, not a code
    with pytest.raises(ValueError, match="outside"):
        decode_codes(net, wrong, W)


def test_the_interleaved_token_stream_round_trips_to_the_same_codes():
    from music_amd.ae_generate import encode_codes, split_code_stream
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import vq_codes_dataset as tool
    finally:
        sys.path.pop(0)
    net, cfg, B, x = _rvq()
    codes = encode_codes(net, x)                                                   # (B, S, Le)
    Le = codes.shape[2]
    pieces = [row.cpu().numpy().astype(np.int16) for row in x.argmax(1)]           # the clips as pieces of mu-law codes
    tokens = tool.encode_pieces(net, pieces, frames=16, batch=2, one_hot="canonical")
    assert len(tokens) == B and all(t.dtype == np.int32 and t.shape == (Le * S,) for t in tokens)
    stream = torch.from_numpy(np.stack(tokens))
    assert int(stream.min()) >= 0 and int(stream.max()) < S * K                    # the prior's alphabet
    assert torch.equal(stream.view(B, Le, S)[:, :, 1] // K, torch.ones(B, Le, dtype=torch.int32))      # frame-major: l0s0, l0s1, ..
    back = split_code_stream(stream, S, K)
    assert torch.equal(back.to(codes.device), codes)
    with pytest.raises(ValueError, match="multiple"):
        split_code_stream(stream[:, :-1], S, K)
    with pytest.raises(ValueError, match="tokens"):
        tool.check_alphabet(3, 512)
