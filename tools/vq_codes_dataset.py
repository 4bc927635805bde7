#!/usr/bin/env python
"""Encode a corpus with a vq autoencoder: mu-law pickle in, bottleneck-code pickle out - the training set of a prior over the codes.

    python tools/vq_codes_dataset.py --model-params params/model_params.json --checkpoint restore/wavenet_autoencoder9.model \\
        --audio data/train.pkl --out data/train_codes.pkl

Input: the loader's own format (music_amd/faster_audio_data.py), a pickled list of 1-D integer arrays, one per PIECE of audio.
Output: the same format, a pickled list of 1-D int32 arrays: THE CODES OF ONE PIECE ARE ONE ARRAY, frame l of a piece being the
code of its pooled frame l (samples rf - 1 + l * pool .. + pool of the piece; the first rf - 1 samples only feed the encoder), in
the order of the input; a piece too short for one frame gives an empty array (and is left out with --drop-empty).  `audio_dataset`
+ `wavenet(quantization_channels=K)` with `"objective": "nll"` and `"one_hot": "canonical"` then train the prior unchanged:
dataset_params.json takes "quantization_channels": K and this file as "audio_path".  Sampled codes go back to audio through
music_amd.ae_generate.decode_codes.

The checkpoint is read under its EMA shadow when `<checkpoint minus .model>.ema` exists (--no-ema: the raw weights).  A piece is
encoded in windows of --frames pooled frames (rf - 1 samples of overlap, so every frame sees what it sees in the whole piece),
--batch windows per forward; only the encoder, the pool and the quantiser run (music_amd.ae_generate.encode_codes).

A model with "vq_stages": S > 1 gives S codes per frame.  A piece is still ONE array, frame-major - l0s0, l0s1, .., l1s0, .. - of
TOKENS s * K + code, so the prior's alphabet ("quantization_channels") is S * K and a position's stage is readable from its
token; S * K > 1024, the decoder's sampler limit, is refused.  music_amd.ae_generate.split_code_stream turns a sampled stream back
into the (B, S, Le) codes that decode_codes takes; music_amd.ae_generate.sample_code_stream samples the prior under the decoder's
position windows, so a token never leaves its position's stage range and the stream always splits.  Train that prior on the
distribution it is sampled from: `"nll_windows": {"stages": S, "codes": K}` beside `"objective": "nll"` in train_params.json and
`"token_positions": true` in dataset_params.json (music_amd/objective.py: the softmax, the loss and the validation figures of a
position are taken over its stage's K tokens only; the loss starts at ln K, not ln(S K)).  Every array written here starts at a
frame boundary, so position 0 of an item is stage 0 - what the loader's 'audio_pos' counts from; sampling with sample_code_stream is
unchanged.

--layout phase writes the K-ary stream instead: the same frame-major order, every token the CODE itself, so the prior's alphabet
stays K whatever S is, and the refusal becomes K > 1024.  Such a stream is for a phase-conditioned prior - `wavenet(...,
quantization_channels=K, phase_period=S)` with `"token_positions": true` in dataset_params.json - which is told the stage of a
position, p mod S, as conditioning (music_amd/model.py); split_code_stream / join_code_stream take `layout="phase"` for it, and
sample_code_stream / prior_score detect such a prior.  --labels is unchanged.

--labels (the source corpus' "labels_path": a JSON list of integers, one per piece of --audio) with --labels-out writes the labels
of the token pickle's items - every item the label of the piece it was encoded from, the pieces --drop-empty leaves out left out
here too - as the "labels_path" of a class-conditional prior (`wavenet(..., global_classes=n, global_channels=E)`)."""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def encode_pieces(net, pieces, frames=32, batch=8, one_hot="scrambled", layout="interleaved"):
    """pieces: list of 1-D integer arrays of mu-law codes -> list of 1-D int32 arrays, the bottleneck codes of every piece (one
    array per piece, empty where a piece pools to no frame).  `one_hot`: the layout the autoencoder was trained on (the loader's
    default is "scrambled").  `layout`: "interleaved" (token = s * K + code) or "phase" (token = code)."""
    from music_amd import faster_audio_data
    from music_amd.ae_generate import encode_codes
    if one_hot not in ("scrambled", "canonical"):
        raise ValueError('one_hot must be "scrambled" or "canonical", not %r' % (one_hot,))
    Q, rf, pool = net.quantization_channel, net.receptive_field, net.en_pool_kernel_size
    S, K = getattr(net, "vq_stages", 1), net.vq_num_codes
    check_alphabet(S, K, layout)
    dev = next(net.parameters()).device
    out = []
    for piece in pieces:
        piece = np.asarray(piece)
        if piece.ndim != 1:
            raise ValueError("a piece is a 1-D array of codes, got shape %s" % (piece.shape,))
        if piece.size and (int(piece.min()) < 0 or int(piece.max()) >= Q):
            raise ValueError("a piece holds codes outside [0, %d)" % Q)
        n_frames = max(0, (piece.size - rf + 1) // pool)
        codes = np.empty((n_frames, S), dtype=np.int32)            # tokens: s * K + code, frame-major
        # windows of `frames` frames (the last one shorter), full ones `batch` at a time
        starts = list(range(0, n_frames, frames))
        full = [f0 for f0 in starts if f0 + frames <= n_frames]
        groups = [full[i:i + batch] for i in range(0, len(full), batch)] + [[f0] for f0 in starts if f0 + frames > n_frames]
        for group in groups:
            nf = min(frames, n_frames - group[0])
            win = np.stack([piece[f0 * pool:f0 * pool + rf - 1 + nf * pool] for f0 in group]).astype(np.int32)
            x = faster_audio_data.onehot_device(torch.from_numpy(win).to(dev), Q, one_hot == "scrambled")
            got = encode_codes(net, x).cpu().numpy().astype(np.int32).reshape(len(group), S, -1)
            assert got.shape == (len(group), S, nf)
            for row, f0 in zip(got, group):
                codes[f0:f0 + nf] = row.T + (np.arange(S, dtype=np.int32) * K if layout == "interleaved" else 0)
        out.append(codes.reshape(-1))
    return out


def item_labels(labels, codes, drop_empty=False):
    """The labels of the token pickle's items: labels[i] of source piece i for every item written (with drop_empty: the pieces
    whose code array is empty are left out, as main() leaves them out of the pickle)."""
    labels = list(labels)
    if len(labels) != len(codes):
        raise ValueError("%d labels for %d pieces of audio: the labels file names one class per piece" % (len(labels), len(codes)))
    for v in labels:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("a label is an integer >= 0, got %r" % (v,))
    return [int(v) for v, c in zip(labels, codes) if not drop_empty or np.asarray(c).size]


def check_alphabet(stages, K, layout="interleaved"):
    """The prior's alphabet is stages * K tokens (layout "phase": K, the stage being conditioning); the decoder's samplers take at
    most 1024."""
    from music_amd import _lib
    if layout not in ("interleaved", "phase"):
        raise ValueError('layout must be "interleaved" or "phase", not %r' % (layout,))
    if layout == "phase":
        if K > _lib.VQ_MAX_CODES:
            raise ValueError('"vq_codes" = %d: a prior over the code stream would need more than the %d classes the decoder\'s samplers '
                             "take - use a smaller codebook" % (K, _lib.VQ_MAX_CODES))
        return
    if stages * K > _lib.VQ_MAX_CODES:
        raise ValueError('"vq_stages" x "vq_codes" = %d x %d = %d tokens: a prior over the interleaved stream would need more than the '
                         "%d classes the decoder's samplers take - use fewer stages, a smaller codebook, or --layout phase (a "
                         "phase-conditioned prior over the K-ary stream)" % (stages, K, stages * K, _lib.VQ_MAX_CODES))


def load_vq_model(model_params, checkpoint, use_ema=True):
    """The vq autoencoder of `model_params` (dict) on the device with `checkpoint`'s weights - its EMA shadow's, where the .ema file
    lies next to it and use_ema is on.  Returns (net, the file read)."""
    from music_amd.ae_train import load_model
    from music_amd.model1 import wavenet_autoencoder
    net = wavenet_autoencoder(**model_params)
    if net.bottleneck != "vq":
        raise ValueError('model_params.json: this tool needs "bottleneck": "vq"')
    ema_path = checkpoint[:-len(".model")] + ".ema" if checkpoint.endswith(".model") else None
    path = ema_path if (use_ema and ema_path and os.path.exists(ema_path)) else checkpoint
    if load_model(net, os.path.dirname(path) + os.sep if os.path.dirname(path) else "", os.path.basename(path)) is None:
        raise FileNotFoundError(path)
    return net.cuda(), path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model-params", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--audio", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--one-hot", default="scrambled", choices=("scrambled", "canonical"))
    ap.add_argument("--no-ema", action="store_true")
    ap.add_argument("--drop-empty", action="store_true")
    ap.add_argument("--layout", default="interleaved", choices=("interleaved", "phase"),
                    help="interleaved: token = stage * K + code (alphabet S K); phase: token = code (alphabet K, for a prior with phase_period = S)")
    ap.add_argument("--labels", help='the "labels_path" of --audio: a JSON list of integers, one per piece')
    ap.add_argument("--labels-out", help="where the labels of the items of --out go (needs --labels)")
    args = ap.parse_args(argv)
    if bool(args.labels) != bool(args.labels_out):
        ap.error("--labels and --labels-out go together")
    with open(args.model_params) as f:
        net, read = load_vq_model(json.load(f), args.checkpoint, not args.no_ema)
    with open(args.audio, "rb") as f:
        pieces = pickle.load(f)
    codes = encode_pieces(net, pieces, args.frames, args.batch, args.one_hot, args.layout)
    if args.labels:
        with open(args.labels) as f:
            out_labels = item_labels(json.load(f), codes, args.drop_empty)
        with open(args.labels_out, "w") as f:
            json.dump(out_labels, f)
    if args.drop_empty:
        codes = [c for c in codes if c.size]
    with open(args.out, "wb") as f:
        pickle.dump(codes, f)
    used = np.unique(np.concatenate(codes)).size if codes and sum(c.size for c in codes) else 0
    print("%s: %d pieces, %d codes, %d of %d codebook rows in use (weights: %s)"
          % (args.out, len(codes), sum(c.size for c in codes), used, net.vq_codebook.num_embeddings, read))


if __name__ == "__main__":
    main()
