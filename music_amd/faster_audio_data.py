"""Counterpart of the reference's ``wavenet/faster_audio_data.py``.

Same names and arguments (``audio_dataset``, ``audio_data_loader``, ``one_hot_encode``), same piece
chopping including the tail re-append quirk (faster_audio_data.py:24-40) and the same
"scrambled" one-hot layout (faster_audio_data.py:62-83) — but MI355X-first: the dataset
keeps the int32 codes, a batch crosses PCIe as B x T int32 (128 KB at 8 x 16000) instead of
B x 256 x T float32 (131 MB), and the one-hot is written directly in HBM by ``wn_onehot``.
``num_workers`` is accepted and ignored (there is no per-item CPU work left to parallelise).
"""
import json
import pickle

import torch
from torch.utils.data import DataLoader, Dataset

try:
    from . import _lib
except ImportError:
    from music_amd import _lib


class audio_dataset(Dataset):

    def __init__(self, audio_path, receptive_field, window_length, cuda_available=False,
                 quantization_channels=256, labels_path=None, n_classes=None, token_positions=False):
        """labels_path (the optional key "labels_path" of dataset_params.json): a JSON list of integers, one class per item of the
        audio pickle (global class conditioning of the autoencoder); every piece then carries 'audio_class', the label of the item
        it was cut from.  n_classes: the model's global_classes - a label outside [0, n_classes) raises here.
        token_positions (the optional key "token_positions" of dataset_params.json): every piece also carries 'audio_pos', the offset
        of its FIRST TARGET sample within the pickle item it was cut from - the stream position the windowed objective needs
        (music_amd/objective.py, "nll_windows"; an item of tools/vq_codes_dataset.py starts at a frame boundary, position 0 = stage 0)."""
        self.token_positions = bool(token_positions)
        self.audio_path = audio_path
        self.labels_path = labels_path
        self.receptive_field = receptive_field
        self.window_length = window_length
        self.cuda_available = cuda_available
        self.quantization_channels = quantization_channels
        with open(self.audio_path, 'rb') as f:
            data = pickle.load(f)
        self.data = self._make_data_pieces(data, self._load_labels(len(data), n_classes))

    def _load_labels(self, n_items, n_classes):
        if self.labels_path is None:
            return None
        with open(self.labels_path) as f:
            labels = json.load(f)
        if not isinstance(labels, list) or any(isinstance(v, bool) or not isinstance(v, int) for v in labels):
            raise ValueError("labels_path %s: a JSON list of integers is wanted" % self.labels_path)
        if len(labels) != n_items:
            raise ValueError("labels_path %s: %d labels for %d items of %s" % (self.labels_path, len(labels), n_items, self.audio_path))
        hi = n_classes if n_classes is not None else float("inf")
        bad = [v for v in labels if not 0 <= v < hi]
        if bad:
            raise ValueError("labels_path %s: label %d lies outside [0, %s) (global_classes)"
                             % (self.labels_path, bad[0], n_classes if n_classes is not None else "inf"))
        return labels

    def _make_data_pieces(self, data, labels=None):
        """faster_audio_data.py:24-40.  A remainder longer than rf but shorter than rf+window
        advances by rf and appends the PREVIOUS piece/target again (the reference's `else` branch
        assigns nothing new); a first item that short raises NameError, as the reference does."""
        rf, win = self.receptive_field, self.window_length
        pieces = []
        piece = target = label = pos = None
        for n, item in enumerate(data):
            item = torch.from_numpy(item)
            consumed = 0                         # samples of this item cut off so far
            while len(item) > rf:
                if len(item) >= rf + win:
                    piece = item[:rf + win - 1]
                    target = item[rf:rf + win].long()
                    label = labels[n] if labels is not None else None
                    pos = consumed + rf          # where target[0] sits in the item
                    item = item[win:]
                    consumed += win
                else:
                    item = item[rf:]
                    consumed += rf
                if target is None:
                    raise NameError("name 'target' is not defined")
                # (a re-appended piece keeps the label of the item its samples came from - the previous item's, where a short item
                # repeats that one's last piece - and, with token_positions, the position of the piece it repeats)
                pieces.append({'audio_piece': piece, 'audio_target': target} if labels is None else
                              {'audio_piece': piece, 'audio_target': target, 'audio_class': label})
                if self.token_positions:
                    pieces[-1]['audio_pos'] = pos
        return pieces

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        # integer codes only; the one-hot is built on the device per batch (see _collate)
        return self.data[idx]


def onehot_device(codes, quantization_channels=256, scrambled=True):
    """int (B,T) codes -> float32 (B,Q,T) one-hot in HBM.  scrambled=True is the loader's layout."""
    if not torch.cuda.is_available():
        raise RuntimeError("music_amd.faster_audio_data builds the one-hot on an MI355X only; there is no CPU path")
    c = codes.to(device="cuda", dtype=torch.int32, non_blocking=True).contiguous()
    b, t = c.shape
    out = torch.empty(b, quantization_channels, t, dtype=torch.float32, device="cuda")
    _lib.call("wn_onehot", _lib.ptr(c), _lib.ptr(out), b, quantization_channels, t, 1 if scrambled else 0, _lib.stream())
    # the codes ride along with the tensor: the engine forms the causal layer's weight gradient from them (a scatter)
    # as long as the tensor has not been modified since (music_amd/engine.py: forward_logits)
    out._wn_codes = (c, bool(scrambled), out._version, c._version)
    return out


def one_hot_encode(sample_piece, cuda_available=False, quantization_channels=256):
    """faster_audio_data.py:62-83 for ONE item: dict -> dict with a (Q,T) float32 tensor (on the
    device) in the reference's reshape-not-transpose layout."""
    piece, target = sample_piece['audio_piece'], sample_piece['audio_target']
    return {"audio_piece": onehot_device(piece[None], quantization_channels)[0], "audio_target": target}


def shard_bounds(n_items, rank, world):
    """DataParallel's scatter (torch.chunk): chunks of ceil(n/world) items in rank order, the last
    non-empty chunk takes the remainder and trailing ranks may get nothing.  Returns [lo, hi)."""
    c = -(-n_items // world)
    lo = min(rank * c, n_items)
    return lo, min(lo + c, n_items)


class _Stager:
    """Host -> device for the loader's two small integer tensors without stalling the launch stream: the batch is gathered
    into one of three rotating PINNED buffers and copied on a copy stream; the caller's stream only waits for that copy's
    event.  (A `.cuda()` of pageable memory is a synchronous copy queued BEHIND the previous step's kernels: the host then sits
    out the whole step before it can prepare the next one - 6.1 instead of 4.5 ms per step through train.py at 8 x 16000.)"""

    def __init__(self):
        self.bufs, self.k, self.stream = {}, 0, None

    def to_device(self, parts, dtype):
        """parts: list of equally long 1-D CPU tensors -> (len(parts), n) tensor of `dtype` on the device"""
        n = parts[0].numel()
        key = (len(parts), n, dtype)
        ring = self.bufs.get(key)
        if ring is None:
            ring = self.bufs[key] = [[torch.empty(len(parts), n, dtype=dtype).pin_memory(), None] for _ in range(3)]
        slot = ring[self.k % 3]
        self.k += 1
        pin, ev = slot
        if ev is not None:
            ev.synchronize()                     # the copy that last read this buffer has left it
        pn = pin.numpy()
        for i, t in enumerate(parts):            # plain memcpys (numpy): no OpenMP region
            pn[i] = t.numpy()
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        main = torch.cuda.current_stream()
        with torch.cuda.stream(self.stream):
            dev = pin.to("cuda", non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        slot[1] = ev
        main.wait_event(ev)
        dev.record_stream(main)
        return dev


ONE_HOT_LAYOUTS = ("scrambled", "canonical")


class _Collate:
    def __init__(self, q, shard=None, scrambled=True):
        self.q = q
        self.shard = shard
        self.scrambled = bool(scrambled)
        self.stager = _Stager()

    def __call__(self, items):
        scale = 1.0
        if self.shard is not None:
            # DataParallel's scatter: contiguous chunk r of the global batch goes to replica r.  On the ragged last
            # batch of an epoch the chunks differ in size (a rank may get none): "dp_scale" = n_local * world / n_global
            # is the weight that turns `mean over ranks of (scale_r * local-mean gradient)` back into DataParallel's
            # global-batch mean; a rank with no items gets audio_piece = None and must still join the all-reduce.
            r, w = self.shard
            lo, hi = shard_bounds(len(items), r, w)
            scale = (hi - lo) * w / float(len(items))
            items = items[lo:hi]
        if not items:
            return {"audio_piece": None, "audio_target": None, "dp_scale": 0.0}
        same = len({it['audio_piece'].numel() for it in items}) == 1 and len({it['audio_target'].numel() for it in items}) == 1
        if same and torch.cuda.is_available():
            codes = self.stager.to_device([it['audio_piece'].to(torch.int32) for it in items], torch.int32)
            target = self.stager.to_device([it['audio_target'] for it in items], torch.int64)
            if "audio_pos" in items[0]:
                pos = self.stager.to_device([torch.tensor([it['audio_pos']], dtype=torch.int64) for it in items], torch.int64).view(-1)
        else:                                    # (torch.stack raises on ragged items, as in the reference; no device: onehot_device raises)
            codes = torch.stack([it['audio_piece'] for it in items]).to(torch.int32)
            target = torch.stack([it['audio_target'] for it in items])
            target = target.cuda(non_blocking=True) if torch.cuda.is_available() else target
            if "audio_pos" in items[0]:
                pos = torch.tensor([it['audio_pos'] for it in items], dtype=torch.int64)
                pos = pos.cuda(non_blocking=True) if torch.cuda.is_available() else pos
        batch = {"audio_piece": onehot_device(codes, self.q, scrambled=self.scrambled), "audio_target": target}
        if "audio_pos" in items[0]:                  # (token_positions: the clips' stream positions, staged like the targets)
            batch["audio_pos"] = pos
        if "audio_class" in items[0]:                # (labels_path: this shard's classes, on the host - the engine checks and copies them)
            batch["audio_class"] = torch.tensor([it["audio_class"] for it in items], dtype=torch.int64)
        if self.shard is not None:
            batch["dp_scale"] = scale
            batch["first_clip"] = lo             # this shard's first clip in the global batch (quantiser dropout draws per GLOBAL clip)
        return batch


def audio_data_loader(batch_size, shuffle, num_workers, pin_memory, shard=None, one_hot="scrambled", **kwargs):
    """faster_audio_data.py:51-59.  Yields {"audio_piece": float32 (B,256,T) on the device,
    "audio_target": int64 (B,win) on the device}.  Shuffling is torch's own RandomSampler, i.e. the
    same permutation stream as the reference under the same seed.  ``shard=(rank, world)`` (set by
    train.py under torchrun) makes this process build only its contiguous chunk of every global
    batch; all ranks must share the torch seed so they draw the same permutation.  ``one_hot`` (the optional key "one_hot" of
    dataset_params.json): "scrambled" is the reference's reshape-not-transpose layout, "canonical" the true one-hot
    x[b][code[t]][t] = 1 - what a model trained on the true likelihood (music_amd/objective.py) and the decoder see.
    With ``labels_path`` (audio_dataset) a batch also has "audio_class": int64 (B,) on the HOST, the classes of this process's clips;
    with ``token_positions`` "audio_pos": int64 (B,) on the device, the offset of each clip's first target within its item."""
    if one_hot not in ONE_HOT_LAYOUTS:
        raise ValueError("one_hot must be one of %s, not %r" % (", ".join(ONE_HOT_LAYOUTS), one_hot))
    audioDataset = audio_dataset(**kwargs)
    print("{} pieces in total".format(len(audioDataset)))
    return DataLoader(audioDataset, batch_size=batch_size, shuffle=shuffle, num_workers=0,
                      pin_memory=False, collate_fn=_Collate(audioDataset.quantization_channels, shard, scrambled=one_hot == "scrambled"))
