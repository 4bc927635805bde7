"""music_amd/train.py with class dropout ("null_class" in the model's JSON, "class_dropout" / "class_dropout_seed" in train_params.json),
end to end on the device, on the smallest class-conditional configuration of tests/test_gpu_class_cond_train.py (four steps of four
clips):
  - class_dropout = 1 equals training with every label set to null_class, bit for bit;
  - class_dropout = 0 equals the run without the keys, bit for bit;
  - class_dropout = 0.5: two runs are bit-equal, a run resumed after its first epoch too (the draw is a function of the global step),
    the steps were handed the classes class_dropout.apply names, and the result is neither of the runs above;
  - a label equal to null_class, and the key without null_class, are refused before anything trains.
Run with -m gpu."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_class_cond_train import CFG, _ctor, _write_run

NULL = 1                                   # the labels of _write_run are [2, 0]: class 1 is nobody's
CFG_NULL = dict(CFG, null_class=NULL)


def _train(root, monkeypatch, extra, cfg=CFG_NULL, labels=None, epochs=2, resume_after_first=False):
    """one run of train() under `root`; returns the final .model state dict"""
    from music_amd import train as T
    monkeypatch.setattr(T, "wavenet", _ctor)
    os.makedirs(root)
    tp = _write_run(root, dict(extra, num_epochs=1 if resume_after_first else epochs), cfg=cfg)
    if labels is not None:
        json.dump(labels, open(root / "labels.json", "w"))
    monkeypatch.chdir(root)
    torch.manual_seed(0)
    T.train()
    if resume_after_first:
        json.dump(dict(tp, restore_model="wavenet1.model"), open(root / "params" / "train_params.json", "w"))
        T.train()
    return torch.load(root / "restore" / ("wavenet%d.model" % epochs))


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "autograd"])
def test_dropout_one_is_the_null_class_and_zero_is_the_parent_path(tmp_path, monkeypatch, fused):
    base = {"fused_step": fused, "objective": "nll" if not fused else "reference"}
    every = _train(tmp_path / "p1", monkeypatch, dict(base, class_dropout=1.0, class_dropout_seed=4))
    null = _train(tmp_path / "null", monkeypatch, base, cfg=CFG, labels=[NULL, NULL])
    assert _same(every, null)
    none = _train(tmp_path / "p0", monkeypatch, dict(base, class_dropout=0.0))
    parent = _train(tmp_path / "parent", monkeypatch, base, cfg=CFG)
    assert _same(none, parent)
    assert not _same(every, parent)
    # the null row of the embedding trains under p = 1 and never under p = 0; the labels' rows the other way round
    emb = "global_embedding.weight"
    assert not torch.equal(every[emb][NULL], parent[emb][NULL]) and not torch.equal(every[emb][[0, 2]], parent[emb][[0, 2]])


def test_half_dropout_is_deterministic_and_resumes_bit_for_bit(tmp_path, monkeypatch):
    from music_amd import class_dropout as cd
    from music_amd.engine_base import EngineBase
    seen = []
    real = EngineBase.stage_classes
    monkeypatch.setattr(EngineBase, "stage_classes", lambda self, classes, B: seen.append(torch.as_tensor(classes).tolist()) or real(self, classes, B))
    extra = {"fused_step": True, "save_optimizer_state": True, "class_dropout": 0.5, "class_dropout_seed": 11}
    a = _train(tmp_path / "a", monkeypatch, extra)
    first_run = list(seen)
    b = _train(tmp_path / "b", monkeypatch, extra)
    c = _train(tmp_path / "c", monkeypatch, extra, resume_after_first=True)
    assert _same(a, b) and _same(a, c)
    # the four steps' classes: the labels of the pieces (items of label 2, then 0: 4 pieces each) with the drawn clips set to NULL
    want = [cd.apply([lab] * 4, NULL, 11, step, 0, 0.5) for step, lab in enumerate([2, 0, 2, 0])]
    assert first_run == want and seen[len(first_run):2 * len(first_run)] == want and seen[2 * len(first_run):] == want
    flat = [v for row in want for v in row]
    assert NULL in flat and (2 in flat or 0 in flat), "p = 0.5 over 16 clips drew nothing or everything: pick another seed"
    other = _train(tmp_path / "d", monkeypatch, dict(extra, class_dropout_seed=12))
    assert not _same(a, other)


def test_refusals(tmp_path, monkeypatch):
    from music_amd import train as T
    monkeypatch.setattr(T, "wavenet", _ctor)
    for name, cfg, extra, labels, msg in (("a", dict(CFG, null_class=2), {"class_dropout": 0.5}, None, "null_class"),
                                          ("b", dict(CFG, null_class=2), {}, None, "null_class"),
                                          ("c", CFG, {"class_dropout": 0.5}, None, '"class_dropout" needs "null_class"'),
                                          ("d", CFG_NULL, {"class_dropout": 1.5}, None, "class_dropout"),
                                          ("e", CFG_NULL, {"class_dropout_seed": 3}, None, "class_dropout_seed")):
        root = tmp_path / name
        os.makedirs(root)
        _write_run(root, extra, cfg=cfg)
        monkeypatch.chdir(root)
        with pytest.raises(ValueError, match=msg):
            T.train()
        assert not os.path.exists(root / "restore")
