"""CPU checks of the label channel of music_amd/faster_audio_data.py (the "labels_path" key of dataset_params.json): every piece
carries the label of the item it was cut from - the reference's re-appended pieces included -, the collate hands this rank's shard
on as "audio_class", bad label files are refused at load, and with the key unset pieces and batches are the parent's.  No device
is touched (the one-hot of a batch is stubbed: it is the device's work)."""
import json
import pickle

import numpy as np
import pytest
import torch

RF, WIN = 5, 8


def _files(tmp_path, lengths, labels):
    rng = np.random.default_rng(3)
    items = [rng.integers(0, 256, size=n).astype(np.int64) for n in lengths]
    audio = tmp_path / "audio.pkl"
    with open(audio, "wb") as f:
        pickle.dump(items, f)
    path = None
    if labels is not None:
        path = tmp_path / "labels.json"
        path.write_text(json.dumps(labels))
    return items, str(audio), None if path is None else str(path)


def _dataset(audio, labels=None, **kw):
    from music_amd.faster_audio_data import audio_dataset
    return audio_dataset(audio, RF, WIN, labels_path=labels, **kw)


# item 0: two whole pieces, then a remainder of 7 > rf: its last piece is appended AGAIN (the reference's quirk);
# item 1: shorter than rf + win but longer than rf: it appends item 0's last piece once more, and nothing of its own;
# item 2: one piece and a remainder <= rf; item 3: too short for anything
LENGTHS, LABELS = [2 * WIN + 7, RF + 3, RF + WIN, RF], [2, 0, 1, 2]


def test_pieces_inherit_the_label_of_the_item_they_were_cut_from(tmp_path):
    items, audio, labels = _files(tmp_path, LENGTHS, LABELS)
    plain, ds = _dataset(audio), _dataset(audio, labels, n_classes=3)
    assert len(ds) == len(plain) == 5
    # the pieces are the parent's, in its order
    for a, b in zip(plain.data, ds.data):
        assert torch.equal(a["audio_piece"], b["audio_piece"]) and torch.equal(a["audio_target"], b["audio_target"])
    assert [p["audio_class"] for p in ds.data] == [2, 2, 2, 2, 1]
    # pieces 2 and 3 are piece 1 again (item 0's remainder, then the short item 1): item 0's samples, so item 0's label
    assert all(torch.equal(ds.data[k]["audio_piece"], ds.data[1]["audio_piece"]) for k in (2, 3))
    assert torch.equal(ds.data[4]["audio_piece"], torch.from_numpy(items[2][:RF + WIN - 1]))
    assert all(type(p["audio_class"]) is int for p in ds.data)


def test_the_unset_path_is_the_parents(tmp_path):
    _, audio, _ = _files(tmp_path, LENGTHS, None)
    ds = _dataset(audio)
    assert all(sorted(p) == ["audio_piece", "audio_target"] for p in ds.data) and ds.labels_path is None
    from music_amd.faster_audio_data import audio_dataset
    positional = audio_dataset(audio, RF, WIN, False, 256)                       # the parent's signature still binds
    assert len(positional) == len(ds)


def test_bad_label_files_are_refused_at_load(tmp_path):
    _, audio, labels = _files(tmp_path, LENGTHS, LABELS[:-1])
    with pytest.raises(ValueError, match="3 labels for 4 items"):
        _dataset(audio, labels)
    for bad, n, what in ((LABELS[:-1] + [3], 3, "label 3"), ([2, -1, 0, 1], 3, "label -1"), ([2, -1, 0, 1], None, "label -1")):
        _, audio, labels = _files(tmp_path, LENGTHS, bad)
        with pytest.raises(ValueError, match=what):
            _dataset(audio, labels, n_classes=n)
    for bad in ({"0": 1}, [0, 1.0, 2, 0], [0, True, 2, 0], ["a", 0, 0, 0]):
        _, audio, labels = _files(tmp_path, LENGTHS, bad)
        with pytest.raises(ValueError, match="list of integers"):
            _dataset(audio, labels, n_classes=3)
    _, audio, labels = _files(tmp_path, LENGTHS, [2, 7, 1, 2])
    assert len(_dataset(audio, labels)) == 5                                      # without n_classes only the sign is checked


@pytest.mark.parametrize("shard", [None, (0, 2), (1, 2), (2, 3)])
def test_the_collate_hands_on_this_ranks_classes(tmp_path, shard, monkeypatch):
    from music_amd import faster_audio_data as fad
    monkeypatch.setattr(fad, "onehot_device", lambda codes, q, scrambled=True: codes)      # (the device's work)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _, audio, labels = _files(tmp_path, LENGTHS, LABELS)
    ds, plain = _dataset(audio, labels, n_classes=3), _dataset(audio)
    items = [ds[k] for k in (4, 0, 3, 1, 2)]
    want = [1, 2, 2, 2, 2]
    batch = fad._Collate(256, shard)(items)
    lo, hi = (0, len(items)) if shard is None else fad.shard_bounds(len(items), *shard)
    cls = batch["audio_class"]
    assert cls.dtype == torch.int64 and cls.device.type == "cpu" and cls.tolist() == want[lo:hi]
    assert batch["audio_piece"].shape[0] == hi - lo == cls.numel()
    # the parent's dicts without labels: the same keys as before, the same tensors
    ref = fad._Collate(256, shard)([plain[k] for k in (4, 0, 3, 1, 2)])
    assert sorted(ref) == sorted(k for k in batch if k != "audio_class")
    assert torch.equal(ref["audio_piece"], batch["audio_piece"]) and torch.equal(ref["audio_target"], batch["audio_target"])
    # a rank with no items: the parent's empty batch
    if shard is not None:
        empty = fad._Collate(256, (3, 4))(items[:1])
        assert empty == {"audio_piece": None, "audio_target": None, "dp_scale": 0.0}


def test_the_loader_takes_the_key_of_dataset_params(tmp_path, monkeypatch):
    from music_amd import faster_audio_data as fad
    monkeypatch.setattr(fad, "onehot_device", lambda codes, q, scrambled=True: codes)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _, audio, labels = _files(tmp_path, LENGTHS, LABELS)
    params = json.loads(json.dumps(dict(audio_path=audio, receptive_field=RF, window_length=WIN, batch_size=2, shuffle=False,
                                        num_workers=0, pin_memory=False, labels_path=labels)))
    seen = [b["audio_class"].tolist() for b in fad.audio_data_loader(**params)]
    assert seen == [[2, 2], [2, 2], [1]]
    del params["labels_path"]
    assert all("audio_class" not in b for b in fad.audio_data_loader(**params))
