"""Counterpart of the reference's ``wavenet_autoencoder/generate.py``: naive generation by a full
forward per generated sample (generate.py:13-65).  The reference version cannot run as shipped (``librosa`` used
without import :65, the start tensor instead of the predicted int appended :48, ``.cuda()`` hard-wired :53); the
algorithm is kept, the output is written with scipy.  It is a harness, not a kernel.

As written, the window update ``input_wav[:,-net.receptive_field-511:]`` (generate.py:55) slices dimension 1 - the
256 CHANNELS - so it is a no-op and the window GROWS by one sample per step (the pooled encoding gains a frame
every ``pool`` steps and the ``_conditon`` branches change with it; cost O(T^2)).  ``generate`` reproduces that by
default, like ``fast_generate`` reproduces the as-written queue recurrence; ``sliding_window=True`` is the evident
intent (the last ``receptive_field + 511`` samples along TIME plus the new one, O(T * rf)) and NOT the reference's
behaviour.  Both are pinned by tests/golden/g9_ae_harness.json (outputs of the reference's own ``predict_next``).

``generate_cached`` / ``cached_decoder`` are the SURVEY 8f3 replacement: encoder ONCE on the start window,
conditioning projections drawn ONCE, then the persistent cached-queue decode kernel (wn_decode).  That is a
different algorithm from the reference's, not a faster form of it: the reference re-encodes the sliding window
and re-draws its 31 random projections for every generated sample (generate.py:13-19, model1.py:178-217).
With a time-constant encoding (one pooled frame: the reference's window of receptive_field + 512 samples and
pool 512 give exactly one) the conditioning is a constant per-channel bias, so the conditioned decoder IS a
plain WaveNet with effective biases, and the existing decode kernel runs it unchanged.

``resynthesize`` is the same idea for an encoding of ANY number of pooled frames (encode a clip, regenerate audio from the
encoding): the projections of the encoding become per-clip TABLES with one column per frame, and the conditioned decode
kernel (``wn_decode_batch_cond``) adds, at every step, the column the reference's ``_conditon`` (model1.py:227-247) would
have added at that position of the forward over the whole clip - ``cond_schedule`` says which."""
import json
import math
import os

import numpy as np
import torch

try:
    from .audio_func import mu_law_decode
    from .model1 import wavenet_autoencoder
    from .train import load_model
except ImportError:
    from music_amd.audio_func import mu_law_decode
    from music_amd.model1 import wavenet_autoencoder
    from music_amd.train import load_model


def predict_next(net, input_wav, quantization_channel=256, temperature=None, top_k=None, top_p=None, seed=0, step=0, classes=None):
    """generate.py:13-19 — argmax over the last chunk-row of the forward output.  ``temperature`` > 0: the code is drawn by
    the decoder's sampler (``fast_generate.sample_logits`` on the log of that row: the softmax only shifts the logits) as
    step ``step`` of ``seed``, truncated by ``top_k`` / ``top_p``.  ``classes``: the clip's class, for a model with global class conditioning."""
    with torch.no_grad():
        out = (net(input_wav) if classes is None else net(input_wav, classes)).view(-1, quantization_channel)
    if temperature is not None and temperature > 0:
        try:
            from . import fast_generate as fg
        except ImportError:
            from music_amd import fast_generate as fg
        return int(fg.sample_logits(torch.log(out[-1:, :].float()), temperature, top_k, top_p, seed=seed, step0=step)[0])
    return int(torch.topk(out[-1, :].view(-1), 1)[1])


def _decoder_wavenet(net, proj=None):
    """The autoencoder's decoder as a ``music_amd.model.wavenet`` on the device: filter / gate = second / first half of
    ``filter_gate`` (model1.py:188-190), the autoencoder's own biases (zeros without ``use_bias``) plus, if given, the N + 1
    constant conditioning vectors ``proj`` (reference row order, gate rows first)."""
    try:
        from .model import wavenet
    except ImportError:
        from music_amd.model import wavenet
    N, Dd = len(net.dilations), net.de_dilation_channel
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    zeros = lambda n: torch.zeros(n)
    bias = lambda name, n: sd[name + ".bias"] if net.use_bias else zeros(n)
    out = {"causal_layer.weight": sd["de_causal_layer.weight"],
           "causal_layer.bias": bias("de_causal_layer", net.de_residual_channel)}
    for i in range(N):
        fg, dn, sk = ("de_dilation_layer_stack.%d" % (3 * i + k) for k in range(3))
        w, b = sd[fg + ".weight"], bias(fg, 2 * Dd)
        if proj is not None:
            b = b + proj[i]
        out["dilation_layer_stack.%d.weight" % (4 * i)], out["dilation_layer_stack.%d.bias" % (4 * i)] = w[Dd:], b[Dd:]
        out["dilation_layer_stack.%d.weight" % (4 * i + 1)], out["dilation_layer_stack.%d.bias" % (4 * i + 1)] = w[:Dd], b[:Dd]
        out["dilation_layer_stack.%d.weight" % (4 * i + 2)] = sd[dn + ".weight"]
        out["dilation_layer_stack.%d.bias" % (4 * i + 2)] = bias(dn, net.de_residual_channel)
        out["dilation_layer_stack.%d.weight" % (4 * i + 3)] = sd[sk + ".weight"]
        out["dilation_layer_stack.%d.bias" % (4 * i + 3)] = bias(sk, net.de_skip_channel)
    out["post_process_1.weight"] = sd["connection_1.weight"]
    out["post_process_1.bias"] = bias("connection_1", net.de_skip_channel) + (proj[N] if proj is not None else 0)
    out["post_process_2.weight"] = sd["connection_2.weight"]
    out["post_process_2.bias"] = bias("connection_2", net.quantization_channel)
    wnet = wavenet(filter_width=net.filter_width, dilations=list(net.dilations), dilation_channels=Dd,
                   residual_channels=net.de_residual_channel, skip_channels=net.de_skip_channel,
                   quantization_channels=net.quantization_channel, use_bias=True)
    wnet.load_state_dict({k: v.contiguous() for k, v in out.items()})
    return wnet.cuda()


def global_term(net, B, classes=None, global_vectors=None, what="decode"):
    """The clip-level input of a decode: None for a model without global class conditioning (both arguments are refused there),
    else the (B, E) float32 vectors on the model's device - the embedding rows of ``classes`` (B integers in [0, global_classes))
    or ``global_vectors`` as given (a row may mix two embedding rows: timbre morphing).  Exactly one of the two is wanted."""
    n = getattr(net, "global_classes", 0)
    if not n:
        if classes is not None or global_vectors is not None:
            raise ValueError("music_amd.ae_generate.%s: the model has no global class conditioning (global_classes is 0): classes "
                             "and global_vectors must be None" % what)
        return None
    if (classes is None) == (global_vectors is None):
        raise ValueError("music_amd.ae_generate.%s: global_classes = %d: pass classes (one integer per clip) or global_vectors "
                         "((B, %d) floats), never both" % (what, n, net.global_channels))
    dev = net.global_embedding.weight.device
    if classes is not None:
        cls = torch.as_tensor(classes)
        if cls.dim() != 1 or cls.numel() != B or cls.is_floating_point():
            raise ValueError("music_amd.ae_generate.%s: classes must be %d integers, one per clip" % (what, B))
        return net.global_vectors(cls).float()
    gv = torch.as_tensor(global_vectors)
    if gv.dim() != 2 or tuple(gv.shape) != (B, net.global_channels) or not gv.is_floating_point():
        raise ValueError("music_amd.ae_generate.%s: global_vectors must be (%d, %d) floats, got %s %s"
                         % (what, B, net.global_channels, gv.dtype, tuple(gv.shape)))
    return gv.detach().to(device=dev, dtype=torch.float32)


def cached_decoder(net, encoding, cond, gvec=None):
    """The autoencoder's conditioned decoder (model1.py:158-225) for ONE pooled frame of encoding
    ``(1, bottleneck, 1)`` and fixed conditioning projections ``cond`` (N+1 (weight (C, bottleneck, 1), bias (C,))
    pairs, gate rows first, the last one for the post-processing stage) as a ``music_amd.model.wavenet``:
    filter / gate = second / first half of ``filter_gate`` (model1.py:188-190), conditioning folded into the
    biases.  Its forward and its cached-queue decoder (``fast_generate``) then reproduce the decoder exactly.
    ``gvec`` (1, E): the clip's global vector (``global_term``), folded in as G_i gvec."""
    if encoding.dim() != 3 or encoding.size(0) != 1 or encoding.size(2) != 1:
        raise ValueError("cached_decoder needs a single pooled frame of encoding, got %s" % (tuple(encoding.shape),))
    enc = encoding.detach().float().cpu()[0, :, 0]
    proj = [w.detach().float().cpu()[:, :, 0] @ enc + b.detach().float().cpu() for w, b in cond]
    if gvec is not None:
        proj = [p + g.float().cpu() @ gvec.detach().float().cpu()[0] for p, g in zip(proj, net.global_projections())]
    return _decoder_wavenet(net, proj)


def cond_schedule(net_or_geometry, W, Le):
    """The conditioning schedule of a forward with ``W`` output rows and ``Le`` pooled frames: per stage i = 0..N (the N
    decoder blocks, then the post-processing stage) the triple ``(shift_i, q_i, Le)``.  Block i's output in that forward has
    L_{i+1} columns (L_N = W; the post-processing stage W) and ``_conditon`` (model1.py:227-247) adds frame
    ``c // (L_{i+1} / Le)`` at its column c when Le divides L_{i+1} (stretch: q_i = L_{i+1} / Le > 0), frame ``c % Le``
    otherwise (tile: q_i = 0).  Output position j is column j + shift_i, shift_i = L_{i+1} - W.  The schedule depends on W as
    the reference's forward does.  ``net_or_geometry``: anything with ``filter_width`` and ``dilations``, or that pair.
    Pure host arithmetic."""
    if isinstance(net_or_geometry, (tuple, list)):
        k, dil = net_or_geometry
    else:
        k, dil = net_or_geometry.filter_width, net_or_geometry.dilations
    k, dil, W, Le = int(k), [int(d) for d in dil], int(W), int(Le)
    if k < 1 or W < 1 or Le < 1:
        raise ValueError("cond_schedule: filter_width, W and Le must be >= 1")
    out = []
    for i in range(len(dil) + 1):
        L = W + (k - 1) * sum(dil[i + 1:]) if i < len(dil) else W         # L_{i+1}: what the blocks behind block i still consume
        out.append((L - W, L // Le if L % Le == 0 else 0, Le))
    return out


def conditioned_decoder(net, cond):
    """The autoencoder's decoder as a ``music_amd.model.wavenet`` with the autoencoder's OWN biases only (no conditioning
    folded in), and the N + 1 conditioning projections ``cond`` as device matrices in the decode layout:
    ``[(weight (C, bottleneck), bias (C,))]`` with the blocks' rows ordered filter first, gate second (the reference draws
    them gate first, model1.py:188-190), the last pair for the post-processing stage.  A table column is
    ``weight @ encoding[:, frame] + bias``."""
    Dd = net.de_dilation_channel
    wnet = _decoder_wavenet(net)
    dev = next(wnet.parameters()).device
    N = len(net.dilations)
    proj = []
    for i, (w, b) in enumerate(cond):
        w, b = w.detach().float()[:, :, 0], b.detach().float()
        if i < N:
            w, b = torch.cat([w[Dd:], w[:Dd]]), torch.cat([b[Dd:], b[:Dd]])
        proj.append((w.contiguous().to(dev), b.contiguous().to(dev)))
    return wnet, proj


def _decode_from_encoding(net, enc, cond, W, first, prime, forced, free_step=False, want_probs=False, temperature=None, seed=0,
                          top_k=None, top_p=None, streams=None, gvec=None):
    """What ``resynthesize`` and ``decode_codes`` share: from an encoding ``enc`` (B, Bw, Le) on the device and the conditioning
    projections ``cond``, build the per-clip tables and the schedule of a forward with ``W`` output rows, prime the queues from
    zero with the input samples ``first`` (B,) then ``prime`` (B, n) - teacher-forced steps at output positions -(rf - 1) .. -
    and decode the W output positions in one persistent conditioned launch, fed ``forced`` (B, W) or its own codes.
    ``free_step``: ``prime`` holds rf - 2 samples only and the sample in front of output position 0 is the model's own.
    ``gvec`` (B, E): the clips' global vectors (``global_term``) - every column of clip b's tables gains G_i gvec[b].
    Returns (codes int32 (B, W), probabilities (B, W, Q) or None)."""
    try:
        from . import fast_generate as fg
    except ImportError:
        from music_amd import fast_generate as fg
    dev = enc.device
    B, Le = enc.size(0), enc.size(2)
    rf = net.receptive_field
    wnet, proj = conditioned_decoder(net, cond)
    deng = wnet._engine_for(dev)
    N, Dd, Dp = len(net.dilations), net.de_dilation_channel, fg._pack_for(wnet, deng).Dp
    # tables: column e of stage i = proj_i(enc[:, e]); blocks [B][N][Le][f Dp | g Dp] (zero rows beyond Dd), post-processing [B][Le][S]
    cw = torch.stack([p[0] for p in proj[:N]])                        # (N, 2 Dd, Bw), rows [f | g]
    cb = torch.stack([p[1] for p in proj[:N]])
    en = torch.einsum("nck,bkl->bnlc", cw, enc) + cb[None, :, None, :]
    cond_fg = torch.zeros(B, N, Le, 2 * Dp, dtype=torch.float32, device=dev)
    cond_fg[..., :Dd] = en[..., :Dd]
    cond_fg[..., Dp:Dp + Dd] = en[..., Dd:]
    cond_p1 = (torch.einsum("ck,bkl->blc", proj[N][0], enc) + proj[N][1]).contiguous()
    if gvec is not None:
        # the per-clip term, constant over the frames: G_i gvec[b], the blocks' rows filter first like proj's
        G = [g.float().to(dev) for g in net.global_projections()]
        gfg = torch.einsum("nce,be->bnc", torch.stack([torch.cat([g[Dd:], g[:Dd]]) for g in G[:N]]), gvec.to(dev))
        cond_fg[..., :Dd] += gfg[:, :, None, :Dd]
        cond_fg[..., Dp:Dp + Dd] += gfg[:, :, None, Dd:]
        cond_p1 += (gvec.to(dev) @ G[N].t())[:, None, :]
    sched = cond_schedule(net, W, Le)
    rings, prev = fg.zero_state(deng, B)
    note = first
    tabs = dict(cond_fg=cond_fg, cond_p1=cond_p1, schedule=sched)
    n = prime.size(1)
    if n > 0:
        # priming: step s takes sample s and is forced to continue with sample s + 1
        _, _, note, prev = fg.decode_batch_cond(wnet, rings, prev, note, n, step0=0, pos0=-(rf - 1), forced=prime, **tabs)
    if free_step:
        _, _, note, prev = fg.decode_batch_cond(wnet, rings, prev, note, 1, step0=n, pos0=n - (rf - 1), temperature=temperature, seed=seed,
                                                top_k=top_k, top_p=top_p, streams=streams, **tabs)
    codes, probs, _, _ = fg.decode_batch_cond(wnet, rings, prev, note, W, step0=rf - 1, pos0=0, forced=forced,
                                              want_probs=want_probs, temperature=temperature, seed=seed, top_k=top_k, top_p=top_p,
                                              streams=streams, **tabs)
    return codes, probs


def _region_mask(regions, B, W, teacher_forced=False):
    """``regions=`` of ``resynthesize`` -> None, or the (B, W) bool mask of the output positions inside a region.  Pure host work."""
    if regions is None:
        return None
    if teacher_forced:
        raise ValueError("resynthesize: regions= says where the clip's samples are fed: pass it without teacher_forced")
    is_pair = lambda r: isinstance(r, (tuple, list)) and len(r) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in r)
    if not isinstance(regions, (tuple, list)):
        raise ValueError("resynthesize: regions must be a list of (a, b) ranges, or one such list per clip")
    per_clip = [list(regions)] * B if all(is_pair(r) for r in regions) else list(regions)
    if len(per_clip) != B or not all(isinstance(rs, (tuple, list)) and all(is_pair(r) for r in rs) for rs in per_clip):
        raise ValueError("resynthesize: regions must be a list of (a, b) ranges, or one such list per clip (%d clips)" % B)
    mask = torch.zeros(B, W, dtype=torch.bool)
    for b, rs in enumerate(per_clip):
        for a, e in rs:
            if not 0 <= a <= e <= W:
                raise ValueError("resynthesize: region (%d, %d) of clip %d lies outside the %d output positions (0 <= a <= b <= %d)"
                                 % (a, e, b, W, W))
            mask[b, int(a):int(e)] = True
    return mask


def resynthesize(net, clips, cond=None, teacher_forced=False, want_probs=False, temperature=None, seed=0, top_k=None, top_p=None,
                 streams=None, classes=None, global_vectors=None, stages=None, regions=None):
    """Encode ``clips`` (B, Q, T) one-hot, T >= receptive_field with at least one pooled frame, and regenerate them from the
    encoding with the cached-queue decoder: the encoder runs ONCE, the conditioning projections are drawn ONCE (or taken
    from ``cond``), the per-clip tables (one column per pooled frame and stage) are built on the device, the queues are
    primed by teacher-forced decode steps over the first receptive_field - 1 samples from zero queues (output positions
    -(rf - 1) .. -1: their conditioning columns clamp to frame 0 and nothing of them reaches a valid position), and the
    W = T - rf + 1 output positions are decoded in one persistent launch, every clip with its own tables.
    ``teacher_forced``: the clip's own codes are fed (the probabilities are then the forward's, row for row); otherwise the
    model's own codes are fed back after the clip's first receptive_field samples.  ``temperature``: sample instead of
    argmax, reproducibly for ``seed``; ``top_k`` / ``top_p`` truncate the distribution first; each of the four may be one value per clip
    (``streams``: the clips' random-number stream ids, default their index).  Returns (codes int64 (B, W), probabilities (B, W, Q) or None, encodings (B, Bw, Le)).
    With a vq bottleneck the encoding is the quantised one, and ``net.vq_codes`` (B, Le; (B, S, Le) with ``vq_stages`` = S > 1) / ``net.last_encoding_pre`` hold the
    frames' codes and the encoding in front of the quantiser.
    A model with global class conditioning wants ``classes`` (one integer per clip) or ``global_vectors`` ((B, E) floats, e.g. a
    mix of two rows of ``net.global_vectors``), never both: the clips are decoded AS that class - their own for a reconstruction,
    another for a conversion (the encoder takes no class).
    ``stages`` (a residual vq bottleneck): None, an int n or one int per clip in [1, vq_stages] - every clip is quantised with its
    first n stages (wn_rvq_fwd_n) and decoded from that coarser encoding; ``net.vq_codes`` then holds -1 in the absent stages.
    ``regions``: None, or a list of ``(a, b)`` ranges of output positions, 0 <= a <= b <= W - shared by all clips, or one such list per
    clip - to regenerate while the rest of the clip is kept (the decoder sees the whole clip's encoding either way): inside a region
    the model's own codes are fed, outside it the clip's samples, as teacher forcing, in the ONE conditioned launch over the W
    positions behind the unchanged priming (a negative ``forced`` entry frees its step: include/wavenet_hip.h, wn_decode).  The codes
    returned are then the composed stream - the clip's samples outside the regions (the model's at position W - 1, which no sample
    of the clip follows), the model's inside - and the probabilities are the model's at every position.  ``[(0, W)]`` is the free
    run, ``[]`` feeds what ``teacher_forced=True`` feeds; not together with ``teacher_forced``."""
    if clips.dim() != 3 or clips.size(1) != net.quantization_channel:
        raise ValueError("resynthesize: clips must be (B, %d, T)" % net.quantization_channel)
    x = clips.detach().cuda().float().contiguous()
    B, Q, T = x.shape
    rf = net.receptive_field
    W = T - rf + 1
    if W < 1:
        raise ValueError("wave sample not long enough")
    inside = _region_mask(regions, B, W, teacher_forced)             # (B, W) bool on the host, or None
    eng_cond = net.engine_cond(cond)                                  # (learned conditioning: None, and a given `cond` is refused)
    cond = eng_cond if eng_cond is not None else net.conditioning_projections()
    gvec = global_term(net, B, classes, global_vectors, "resynthesize")
    eng = net._engine_for(x.device)
    with torch.no_grad():
        # (raises when the clip pools to no frame; with a global term the encoder alone runs: the decoder's class is the caller's)
        _, enc, ws = eng.forward(x, eng_cond, want_probs=False, encode_only=gvec is not None, **({} if stages is None else {"stages": stages}))
    enc = net.last_encoding = enc.clone()
    if eng.vq:
        net.vq_codes, net.last_encoding_pre = eng.vq_codes_of(ws), ws["enc_pre"]
    codes_in = x.argmax(1).to(torch.int32)                            # (B, T)
    forced = None
    if teacher_forced or inside is not None:
        forced = torch.cat([codes_in[:, rf:], torch.zeros(B, 1, dtype=torch.int32, device=x.device)], 1)
    if inside is not None:
        inside = inside.to(x.device)
        forced = torch.where(inside, torch.full_like(forced, -1), forced)
    codes, probs = _decode_from_encoding(net, enc, cond, W, x[:, :, 0].contiguous(), codes_in[:, 1:rf], forced, want_probs=want_probs,
                                         temperature=temperature, seed=seed, top_k=top_k, top_p=top_p, streams=streams, gvec=gvec)
    codes = codes.to(torch.int64)
    if inside is not None:
        inside[:, W - 1] = True                                       # (no sample of the clip follows the last position)
        codes = torch.where(inside, codes, forced.to(torch.int64))
    return codes, probs, enc


def _vq_engine(net, what):
    if getattr(net, "bottleneck", "continuous") != "vq":
        raise ValueError('music_amd.ae_generate.%s needs a model with bottleneck="vq"' % what)
    return net._engine_for(next(net.parameters()).device)


def encode_codes(net, clips, stages=None):
    """The codes of ``clips`` (B, Q, T) one-hot under a vq model: (B, Le) int64, Le = (T - rf + 1) // pool frames per clip;
    (B, S, Le) with ``vq_stages`` = S > 1, stage s in [:, s].  Runs the encoder, the pool and the quantiser (wn_vq_fwd / wn_rvq_fwd) only.
    ``stages``: None, an int n or one int per clip in [1, S] - the codes of the first n stages, still (B, S, Le), with -1 in the absent
    stages (wn_rvq_fwd_n); ``decode_codes`` takes them as they are."""
    eng = _vq_engine(net, "encode_codes")
    if clips.dim() != 3 or clips.size(1) != net.quantization_channel:
        raise ValueError("encode_codes: clips must be (B, %d, T)" % net.quantization_channel)
    if clips.size(2) - net.receptive_field + 1 < 1:
        raise ValueError("wave sample not long enough")
    x = clips.detach().to(eng.device).float().contiguous()
    with torch.no_grad():
        _, _, ws = eng.forward(x, None, want_probs=False, encode_only=True, **({} if stages is None else {"stages": stages}))
    return eng.vq_codes_of(ws)


def decode_codes(net, codes, W, start=None, teacher_forced=None, want_probs=False, temperature=None, top_k=None, top_p=None, seed=0,
                 streams=None, classes=None, global_vectors=None):
    """Audio codes from bottleneck codes: ``codes`` (B, Le) integers in [0, K) are looked up in the codebook (wn_vq_lookup; a code
    out of range raises) and the encoding is decoded as ``resynthesize`` decodes one - the same tables, schedule
    (``cond_schedule(net, W, Le)``), priming and persistent conditioned launch - into ``W`` samples per clip.
    The rf = receptive_field samples in front of output position 0: ``start`` (B, rf - 1) codes are the first rf - 1 of them and
    the last is the model's own continuation; ``start=None`` primes with the mid code Q / 2 throughout, as
    ``fast_generate.generate`` does.  ``teacher_forced``: the codes (B, rf - 1 + W) of whole clips - they are fed instead of the
    model's own (the probabilities are then those of a forward over the clip whose encoding these codes are), ``start``
    defaults to their first rf - 1.  ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` / ``streams``: as in ``resynthesize``,
    and so are ``classes`` / ``global_vectors`` (the same codes as another class: the conversion of VQ-VAE).
    With ``vq_stages`` = S > 1: ``codes`` (B, n, Le), 1 <= n <= S, the first n stages' codes; the encoding is the sum of their rows in
    stage order (wn_rvq_lookup) - all S give the encoding the forward decoded, a prefix the coarser code.  Codes with -1 in a clip's
    absent stages (``encode_codes(..., stages=)``) give every clip the sum of ITS stages' rows (wn_rvq_lookup_n); a clip's -1 entries
    must form a stage suffix, identical over its frames, and never include stage 0 (ValueError otherwise, before any launch).
    Returns (codes int64 (B, W), probabilities (B, W, Q) or None)."""
    eng = _vq_engine(net, "decode_codes")
    dev = eng.device
    Q, rf, W = net.quantization_channel, net.receptive_field, int(W)
    if eng.vq_S > 1:
        if codes.dim() != 3 or not 1 <= codes.size(1) <= eng.vq_S or W < 1:
            raise ValueError("decode_codes: vq_stages = %d: codes must be (B, n, Le) with 1 <= n <= %d, and W >= 1" % (eng.vq_S, eng.vq_S))
    elif codes.dim() != 2 or W < 1:
        raise ValueError("decode_codes: codes must be (B, Le) and W >= 1")
    B = codes.size(0)
    gvec = global_term(net, B, classes, global_vectors, "decode_codes")
    enc = eng.vq_lookup(codes)
    as_codes = lambda t, n, what: _checked_codes(t, B, n, Q, dev, what)
    forced = last = None
    if teacher_forced is not None:
        tf = as_codes(teacher_forced, rf - 1 + W, "teacher_forced")
        start = tf[:, :rf - 1] if start is None else start
        last = tf[:, rf - 1:rf]
        forced = torch.cat([tf[:, rf:], torch.zeros(B, 1, dtype=torch.int32, device=dev)], 1)
    if start is None:
        start = torch.full((B, rf - 1), Q // 2, dtype=torch.int32, device=dev)
        last = start[:, :1]
    start = as_codes(start, rf - 1, "start")
    seq = start if last is None else torch.cat([start, last], 1)
    first = torch.zeros(B, Q, dtype=torch.float32, device=dev)
    first.scatter_(1, seq[:, :1].to(torch.int64), 1.0)
    out, probs = _decode_from_encoding(net, enc, net.conditioning_projections(), W, first, seq[:, 1:].contiguous(), forced,
                                       free_step=last is None, want_probs=want_probs, temperature=temperature, seed=seed, top_k=top_k,
                                       top_p=top_p, streams=streams, gvec=gvec)
    return out.to(torch.int64), probs


def rate_distortion(net, clips, classes=None):
    """What every prefix of the stages costs and gives on ``clips`` (B, Q, T) canonical one-hot, as ``resynthesize`` takes them: for
    n = 1 .. S one forward in eval mode over the first T - 1 samples with ``stages=n``, scored against the clips' own next samples
    (output column w predicts sample rf + w).  Returns a list of S dicts:
    ``stages`` n, ``bits_per_frame`` n log2 K, ``mse`` (the encoding's error against e: the last active stage's) and ``nll``
    (nats per sample, the mean over the clips of ``objective.score``).  The model's mode is restored.  On a chain whose codebooks were
    not fitted the mse may GROW with n: a stage refines a frame only where one of its rows is nearer to the residual than 0 is."""
    eng = _vq_engine(net, "rate_distortion")
    if clips.dim() != 3 or clips.size(1) != net.quantization_channel:
        raise ValueError("rate_distortion: clips must be (B, %d, T)" % net.quantization_channel)
    try:
        from . import objective
    except ImportError:
        from music_amd import objective
    if clips.size(2) - net.receptive_field < 1:
        raise ValueError("wave sample not long enough")
    full = clips.detach().to(eng.device).float()
    x = full[:, :, :-1].contiguous()
    target = full[:, :, net.receptive_field:].argmax(1)                # (B, T - rf)
    was_training = net.training
    net.eval()
    rows = []
    try:
        for n in range(1, eng.vq_S + 1):
            s = objective.score(net, x, target, classes=classes, stages=n if eng.vq_S > 1 else None)
            st = eng.last_vq
            mse = st.stage_mse[n - 1] if eng.vq_S > 1 else st.mse
            rows.append({"stages": n, "bits_per_frame": n * math.log2(eng.vq_K), "mse": float(mse), "nll": float(s["nll"].mean())})
    finally:
        net.train(was_training)
    return rows


LAYOUTS = ("interleaved", "phase")


def _layout(layout, what):
    if layout not in LAYOUTS:
        raise ValueError('%s: layout must be "interleaved" (token = stage * K + code) or "phase" (token = code), not %r' % (what, layout))
    return layout == "phase"


def _phase_prior(prior, stages, K, what):
    """True for a phase-conditioned prior over the K-ary stream of `stages` stages (phase_period == stages, quantization_channels ==
    K), False for a prior over the interleaved S K alphabet; any other combination of phase_period and alphabet is refused by name"""
    P, Q = int(getattr(prior, "phase_period", 0) or 0), int(prior.quantization_channels)
    if not P:
        return False
    if P != stages or Q != K:
        raise ValueError("%s: the prior has phase_period = %d and quantization_channels = %d; a phase-conditioned prior of %d stages "
                         "x %d codes needs phase_period = %d and quantization_channels = %d" % (what, P, Q, stages, K, stages, K))
    return True


def split_code_stream(tokens, stages, K, layout="interleaved"):
    """The interleaved token stream of tools/vq_codes_dataset.py back into codes: ``tokens`` (B, Le * stages) or (Le * stages,)
    integers, frame-major (l0s0, l0s1, .., l1s0, ..) with token = s * K + code, -> (B, stages, Le) int64 codes in [0, K), what
    ``decode_codes`` takes.  Raises on a length that is no multiple of ``stages`` and on a token outside its position's stage range.
    A prior over the S K alphabet sampled freely may emit one; ``sample_code_stream`` samples it under the decoder's position
    windows (``fast_generate.stage_windows``), which keep every token inside its position's range, so its streams always split.
    ``layout="phase"`` (tools/vq_codes_dataset.py --layout phase, a phase-conditioned prior): the tokens ARE the codes, frame-major,
    every one in [0, K)."""
    t = torch.as_tensor(tokens)
    stages, K = int(stages), int(K)
    phase = _layout(layout, "split_code_stream")
    if stages < 1 or K < 1:
        raise ValueError("split_code_stream: stages and K must be >= 1")
    if t.is_floating_point() or t.dim() not in (1, 2):
        raise ValueError("split_code_stream: tokens must be integers, (B, Le * stages) or (Le * stages,)")
    t = t.reshape(1, -1) if t.dim() == 1 else t
    if t.size(1) % stages:
        raise ValueError("split_code_stream: %d tokens per clip are not a multiple of %d stages" % (t.size(1), stages))
    t = t.to(torch.int64).reshape(t.size(0), -1, stages)                              # (B, Le, S)
    codes = t if phase else t - torch.arange(stages, dtype=torch.int64, device=t.device) * K
    wrong = (codes < 0) | (codes >= K)
    if bool(wrong.any()):
        b, l, s = (int(v) for v in wrong.nonzero()[0])
        raise ValueError("split_code_stream: token %d of clip %d at frame %d, stage %d lies outside that stage's range [%d, %d)"
                         % ((int(t[b, l, s]), b, l, s) + ((0, K) if phase else (s * K, (s + 1) * K))))
    return codes.permute(0, 2, 1).contiguous()


def join_code_stream(codes, K, layout="interleaved"):
    """The inverse of ``split_code_stream``: ``codes`` (B, S, Le) integers in [0, K) -> (B, Le * S) int64 tokens, frame-major (l0s0,
    l0s1, .., l1s0, ..) with token = s * K + code.  A -1 (an absent stage of ``encode_codes(..., stages=n)``, a code still to be
    sampled) stays -1.  ``split_code_stream(join_code_stream(c, K), S, K) == c`` on complete codes.  Raises on anything else.
    ``layout="phase"``: token = code (``split_code_stream``)."""
    c = torch.as_tensor(codes)
    K = int(K)
    phase = _layout(layout, "join_code_stream")
    if K < 1:
        raise ValueError("join_code_stream: K must be >= 1")
    if c.is_floating_point() or c.dtype == torch.bool or c.dim() != 3:
        raise ValueError("join_code_stream: codes must be (B, stages, Le) integers")
    c = c.to(torch.int64)
    wrong = (c < -1) | (c >= K)
    if bool(wrong.any()):
        b, s, l = (int(v) for v in wrong.nonzero()[0])
        raise ValueError("join_code_stream: code %d of clip %d at frame %d, stage %d lies outside [0, %d) (-1: no code)"
                         % (int(c[b, s, l]), b, l, s, K))
    tok = c if phase else c + (torch.arange(c.size(1), dtype=torch.int64, device=c.device) * K)[None, :, None]
    return torch.where(c >= 0, tok, c).permute(0, 2, 1).reshape(c.size(0), -1).contiguous()


def sample_code_stream(prior, stages, K, frames, start_tokens, start_pos=0, temperature=None, top_k=None, top_p=None, seed=0,
                       streams=None, classes=None, guidance=None, keep_codes=None):
    """New bottleneck codes from a prior over the interleaved token stream (a ``wavenet`` with ``quantization_channels`` >= stages
    * K trained on tools/vq_codes_dataset.py's output): ``start_tokens`` (U, n0 >= receptive_field) are tokens of a real stream
    whose first token sits at stream position ``start_pos``; their last receptive_field tokens (canonical one-hot) prime the
    prior, and ``frames * stages`` tokens are generated in ONE ``fast_generate.generate_codes_batch`` launch (corrected
    recurrence) under ``stage_windows(stages, K)``: the token at stream position p is drawn among stage p mod stages' K tokens
    only, renormalised there, so no token can leave its range.  ``(start_pos + n0) % stages`` must be 0: generation starts on a
    frame boundary.  ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` / ``streams``: as in ``generate_codes_batch``.
    ``classes``: one class per stream for a class-conditional prior (required there, refused elsewhere): stream u is drawn as
    class classes[u], under the same stage windows.  ``guidance``: None, a scale or one per stream - classifier-free guidance
    of a prior with ``null_class`` (``fast_generate.generate_codes_batch``): the guided logits are windowed like the plain ones.
    ``keep_codes``: (U, stages, frames) integers, a code in [0, K) where the caller has one and -1 where one is to be sampled - the
    format of ``encode_codes(..., stages=n)``, sliced to the frames generated here.  The kept codes are fed to the prior at their
    positions and the others drawn GIVEN them, in the same one launch (``generate_codes_batch(keep=)``: coarse-to-fine when the kept
    codes are a stage prefix; single frames, everything or nothing are as welcome); the result holds the caller's codes where given.
    A kept code outside [0, K) is refused before any launch.
    A phase-conditioned prior (``phase_period == stages`` and ``quantization_channels == K``, trained on the tool's ``--layout phase``
    stream) is detected: its tokens are the codes themselves, every logit is legal, so it runs without a window table and is told the
    stage by ``phase_pos = start_pos + n0``; everything else is as above.  Any other (phase_period, alphabet) is refused by name.
    Returns ``split_code_stream`` of the generated tokens: (U, stages, frames) int64 codes in [0, K), what ``decode_codes`` takes."""
    try:
        from . import fast_generate as fg
    except ImportError:
        from music_amd import fast_generate as fg
    stages, K, frames, start_pos = int(stages), int(K), int(frames), int(start_pos)
    rf, Q = prior.receptive_field, prior.quantization_channels
    if stages < 1 or K < 1 or frames < 1:
        raise ValueError("sample_code_stream: stages, K and frames must be >= 1")
    phase = _phase_prior(prior, stages, K, "sample_code_stream")
    if not phase and stages * K > Q:
        raise ValueError("sample_code_stream: %d stages x %d codes = %d tokens, the prior's alphabet holds %d" % (stages, K, stages * K, Q))
    t = torch.as_tensor(start_tokens)
    if t.is_floating_point() or t.dim() != 2 or t.size(1) < rf:
        raise ValueError("sample_code_stream: start_tokens must be (U, n0 >= %d) integer tokens" % rf)
    if start_pos < 0 or (start_pos + t.size(1)) % stages:
        raise ValueError("sample_code_stream: generation must start on a frame boundary: start_pos + n0 = %d + %d is no multiple of "
                         "%d stages (start_pos >= 0)" % (start_pos, t.size(1), stages))
    if int(t.min()) < 0 or int(t.max()) >= Q:
        raise ValueError("sample_code_stream: start_tokens must hold tokens in [0, %d)" % Q)
    keep = {}
    if keep_codes is not None:
        kc = torch.as_tensor(keep_codes)
        if kc.is_floating_point() or kc.dtype == torch.bool or tuple(kc.shape) != (t.size(0), stages, frames):
            raise ValueError("sample_code_stream: keep_codes must be (%d, %d, %d) integers (a code in [0, %d), or -1: to be sampled)"
                             % (t.size(0), stages, frames, K))
        try:
            keep["keep"] = join_code_stream(kc, K, "phase" if phase else "interleaved")
        except ValueError as e:
            raise ValueError("sample_code_stream: keep_codes: %s" % e) from None
    dev = next(prior.parameters()).device
    x = torch.nn.functional.one_hot(t[:, -rf:].to(device=dev, dtype=torch.int64), Q).transpose(1, 2).float().contiguous()
    where = dict(phase_pos=start_pos + t.size(1)) if phase else dict(windows=fg.stage_windows(stages, K), window_pos=start_pos + t.size(1))
    tokens = fg.generate_codes_batch(prior, x, frames * stages, correct_queue=True, temperature=temperature, seed=seed, top_k=top_k,
                                     top_p=top_p, streams=streams, classes=classes, guidance=guidance, **where, **keep)
    return split_code_stream(tokens, stages, K, "phase" if phase else "interleaved")


def prior_score(prior, tokens, stages, K, start_pos=0, classes=None, weights=None, ignore_index=None, label_smoothing=0.0):
    """Held-out figures of a prior on token streams ``tokens`` (U, n > receptive_field) whose first token sits at stream position
    ``start_pos``, under the windows ``sample_code_stream`` draws with: ``objective.score`` of every token behind the first
    receptive_field ones - per-stream "nll", "bits" (per token, of the distribution that is sampled) and "accuracy".  ``classes``: one
    class per stream for a class-conditional prior.  A phase-conditioned prior (``sample_code_stream``) is scored without windows,
    under ``phase_pos = start_pos + receptive_field``.  ``weights`` ((U, n - receptive_field), one per scored token) /
    ``ignore_index`` / ``label_smoothing``: ``objective.score``'s - the figures become weighted means over the tokens that count (a
    dropped stage's -1 under ``ignore_index=-1`` does not), with "tokens", their sum of weights per stream."""
    try:
        from . import fast_generate as fg, objective
    except ImportError:
        from music_amd import fast_generate as fg, objective
    rf = prior.receptive_field
    t = torch.as_tensor(tokens)
    if t.is_floating_point() or t.dim() != 2 or t.size(1) <= rf:
        raise ValueError("prior_score: tokens must be (U, n > %d) integer tokens" % rf)
    t = t.to(next(prior.parameters()).device)
    if int(start_pos) < 0:
        raise ValueError("prior_score: start_pos must be >= 0")
    wnll = dict(weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing)
    if _phase_prior(prior, int(stages), int(K), "prior_score"):
        return objective.score(prior, t[:, :-1].to(torch.int32), t[:, rf:].to(torch.int64), classes=classes, phase_pos=int(start_pos) + rf,
                               **wnll)
    return objective.score(prior, t[:, :-1].to(torch.int32), t[:, rf:].to(torch.int64), classes=classes, **wnll,
                           windows=fg.stage_windows(int(stages), int(K)), window_pos=int(start_pos) + rf)


def _checked_codes(t, B, n, Q, dev, what):
    t = torch.as_tensor(t)
    if t.dim() != 2 or tuple(t.shape) != (B, n):
        raise ValueError("decode_codes: %s must be (%d, %d) codes, got %s" % (what, B, n, tuple(t.shape)))
    if t.is_floating_point() or int(t.min()) < 0 or int(t.max()) >= Q:
        raise ValueError("decode_codes: %s must hold integer codes in [0, %d)" % (what, Q))
    return t.to(device=dev, dtype=torch.int32).contiguous()


def generate_cached(net, start_piece, note_num, cond=None, temperature=None, seed=0, top_k=None, top_p=None, classes=None,
                    global_vectors=None):
    """encode ``start_piece`` (1, Q, >= receptive_field) once, draw the conditioning projections once
    (or take ``cond``), then generate ``note_num`` codes with the persistent cached-queue decoder (corrected queue
    recurrence).  Returns (codes int64 on the device, the wavenet-form decoder, the encoding).
    ``classes`` ([c]) / ``global_vectors`` ((1, E)): the class to generate as, for a model with global class conditioning."""
    try:
        from . import fast_generate as fg
    except ImportError:
        from music_amd import fast_generate as fg
    if cond is not None:
        net.engine_cond(cond)                                # (learned conditioning: a given `cond` is refused, as in resynthesize)
    gvec = global_term(net, start_piece.size(0), classes, global_vectors, "generate_cached")
    with torch.no_grad():
        if gvec is None:
            net(start_piece.cuda())                          # sets net.last_encoding (model1.py:256-268)
        else:                                                # (the encoder alone: it takes no class)
            x = start_piece.detach().cuda().float().contiguous()
            net.last_encoding = net._engine_for(x.device).forward(x, None, want_probs=False, encode_only=True)[1].clone()
    enc = net.last_encoding
    if enc.size(2) != 1:
        raise ValueError("the start piece pools to %d frames; the cached decoder needs exactly one "
                         "(receptive_field + pool .. receptive_field + 2*pool - 1 samples)" % enc.size(2))
    if cond is None:
        cond = net.conditioning_projections()
    wnet = cached_decoder(net, enc, cond) if gvec is None else cached_decoder(net, enc, cond, gvec)
    codes = fg.generate_codes(wnet, start_piece[:, :, -wnet.receptive_field:].cuda(), note_num, correct_queue=True,
                              temperature=temperature, seed=seed, top_k=top_k, top_p=top_p)
    return codes, wnet, enc


def generate_codes_naive(net, start_piece, note_num, sliding_window=False, window=None, seed=None, temperature=None, top_k=None,
                         top_p=None, classes=None):
    """The loop of generate.py:44-55: one full forward (encoder + conditioned decoder, fresh random conditioning
    projections) per generated code.  ``sliding_window`` False = as written (growing window), True = the last
    ``window - 1`` samples + the new one (``window`` defaults to receptive_field + 512).  ``seed``: torch.manual_seed(seed + i)
    before step i (the projections are drawn from the global RNG), for reproducible runs and the golden tests.
    ``temperature`` / ``top_k`` / ``top_p``: draw each code with the decoder's sampler instead of the argmax (``predict_next``).
    ``classes`` ([c]): the clip's class, for a model with global class conditioning (every step is the model's own forward)."""
    win = window if window is not None else net.receptive_field + 512
    input_wav = start_piece.cuda()
    generated = []
    for i in range(note_num):
        if seed is not None:
            torch.manual_seed(int(seed) + i)
        code = predict_next(net, input_wav, net.quantization_channel, temperature=temperature, top_k=top_k, top_p=top_p,
                            seed=seed or 0, step=i, **({} if classes is None else {"classes": classes}))
        generated.append(code)
        note = torch.zeros(1, net.quantization_channel, 1, device=input_wav.device)
        note[0, code, 0] = 1.0
        keep = input_wav[:, :, -(win - 1):] if sliding_window else input_wav
        input_wav = torch.cat((keep, note), 2)
    return generated


def generate(model_path, model_name, generate_path, generate_name, start_piece=None, sr=16000, duration=10,
             sliding_window=False, seed=None, temperature=None, top_k=None, top_p=None, classes=None, global_vectors=None):
    """``classes`` ([c]) for a model with global class conditioning: the class to generate as.  ``global_vectors`` is refused here -
    this loop runs the model's own forward, which takes class ids; ``generate_cached`` / ``resynthesize`` / ``decode_codes`` decode
    from a vector."""
    if global_vectors is not None:
        raise ValueError("music_amd.ae_generate.generate runs the model's own forward per code, which takes classes; decode from "
                         "global_vectors with generate_cached, resynthesize or decode_codes")
    if os.path.exists(generate_path) is False:
        os.makedirs(generate_path)
    with open('./params/model_params.json') as f:
        model_params = json.load(f)
    net = wavenet_autoencoder(**model_params)
    net = load_model(net, model_path, model_name)
    if net is None:
        raise FileNotFoundError(model_path + model_name)
    net = net.cuda()
    if start_piece is None:
        start_piece = torch.zeros(1, 256, net.receptive_field + 512)
        start_piece[:, 128, :] = 1.0
    generated = generate_codes_naive(net, start_piece, int(duration * sr), sliding_window=sliding_window,
                                     window=start_piece.size(2), seed=seed, temperature=temperature, top_k=top_k, top_p=top_p,
                                     classes=classes)
    audio = mu_law_decode(torch.tensor(generated, dtype=torch.int64), net.quantization_channel).cpu().numpy()
    from scipy.io import wavfile
    wavfile.write(generate_path + generate_name, sr, audio.astype(np.float32))
    return generated
