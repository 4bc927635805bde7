"""music_amd/ae_train.py with global class conditioning, end to end on the device: the two model keys, "labels_path", the classes on
the fused step and on the module path under both objectives, validation with "valid_labels_path", the checkpoint's keys.  The run is the one of tests/test_gpu_harness.py (the data, seed and parameters of
tests/golden/g9_ae_harness.json) with the keys added.  Run with -m gpu."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_ae_harness_cpu import g9, write_g9_run

E, NC = 6, 3


def _run(tmp_path, extra_train=None, labels=True, model=True):
    g = g9()
    if model:
        g = dict(g, model_params=dict(g["model_params"], conditioning="learned", global_classes=NC, global_channels=E))
    if labels:
        path = str(tmp_path / "labels.json")
        json.dump([k % NC for k in range(len(g["data_lens"]))], open(path, "w"))
        g = dict(g, dataset_params=dict(g["dataset_params"], labels_path=path))
    write_g9_run(tmp_path, g, extra_train)
    return g


@pytest.mark.parametrize("fused,objective", [(False, "reference"), (True, "reference"), (True, "nll"), (False, "nll")],
                         ids=["autograd", "fused_step", "fused_step_nll", "autograd_nll"])
def test_training_with_classes_writes_its_logs_and_checkpoints(tmp_path, monkeypatch, fused, objective):
    from music_amd import ae_train as A
    from music_amd.engine_base import EngineBase
    extra = {"fused_step": fused, "objective": objective, "ema_decay": 0.9}
    if objective == "nll":                       # validate on the training pickle itself: its labels are the held-out set's
        extra.update(valid_audio_path=str(tmp_path / "np_audio.pkl"), validate_every=1, valid_labels_path=str(tmp_path / "labels.json"))
    g = _run(tmp_path, extra)
    monkeypatch.chdir(tmp_path)
    seen = []
    real = EngineBase.stage_classes
    monkeypatch.setattr(EngineBase, "stage_classes", lambda self, classes, B: seen.append((classes, B)) or real(self, classes, B))
    torch.manual_seed(0)
    A.train()
    # every step handed the batch's classes on, from the host, one per clip
    assert seen and all(torch.is_tensor(c) and c.device.type == "cpu" and c.dtype == torch.int64 and c.numel() == B for c, B in seen)
    assert {int(v) for c, _ in seen for v in c} <= set(range(NC)) and len({int(v) for c, _ in seen for v in c}) > 1
    for line in open(tmp_path / "log" / "loss_log.log").read().strip().split("\n"):
        assert math.isfinite(float(line.split(" ")[-1]))
    if objective == "nll":
        assert all(math.isfinite(float(ln.split("nll is ")[1].split(",")[0])) for ln in open(tmp_path / "log" / "valid_log.log"))
    files = sorted(os.listdir(tmp_path / "restore"))
    assert any(f.endswith(".model") for f in files) and any(f.endswith(".ema") for f in files)
    N = len(g["model_params"]["dilations"])
    for f in files:
        ck = torch.load(tmp_path / "restore" / f)
        assert list(ck)[-(N + 2):] == ["de_gcond_layer_stack.%d.weight" % i for i in range(N)] + ["connection_gcond.weight", "global_embedding.weight"]
        assert tuple(ck["global_embedding.weight"].shape) == (NC, E) and all(bool(torch.isfinite(v).all()) for v in ck.values())
