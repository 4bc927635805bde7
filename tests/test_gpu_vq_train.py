"""music_amd/ae_train.py with a vq bottleneck, end to end on the device: the JSON keys, `"vq_init": "data"`, the loss with vq_loss in
it on both step forms, vq_log.log, the checkpoint.  The run is the one of tests/test_gpu_harness.py (the data, seed and parameters
of tests/golden/g9_ae_harness.json) with the three keys added.  Run with -m gpu."""
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_ae_harness_cpu import g9, write_g9_run

K = 16


@pytest.mark.parametrize("fused,objective,vq_init", [(False, "reference", "data"), (True, "reference", "data"), (True, "nll", "uniform"),
                                                     (False, "nll", "uniform")],
                         ids=["autograd", "fused_step", "fused_step_nll_uniform", "autograd_nll_uniform"])
def test_training_a_vq_autoencoder_writes_its_logs_and_checkpoints(tmp_path, monkeypatch, fused, objective, vq_init):
    from music_amd import ae_train as A
    g = g9()
    g = dict(g, model_params=dict(g["model_params"], conditioning="learned", bottleneck="vq", vq_codes=K, vq_beta=0.25))
    write_g9_run(tmp_path, g, {"fused_step": fused, "objective": objective, "vq_init": vq_init, "ema_decay": 0.9})
    monkeypatch.chdir(tmp_path)
    inits = []
    real = A.wavenet_autoencoder.init_codebook
    monkeypatch.setattr(A.wavenet_autoencoder, "init_codebook", lambda self, enc, seed=0: inits.append(tuple(enc.shape)) or real(self, enc, seed))
    torch.manual_seed(0)
    A.train()
    bw = g["model_params"]["en_bottleneck_width"]
    assert len(inits) == (1 if vq_init == "data" else 0) and all(s[1] == bw for s in inits)
    loss_lines = open(tmp_path / "log" / "loss_log.log").read().strip().split("\n")
    vq_lines = open(tmp_path / "log" / "vq_log.log").read().strip().split("\n")
    assert len(vq_lines) == len(loss_lines) >= 1
    for line in vq_lines:
        m = re.fullmatch(r"Trained over (\d+) pieces, vq mse (\S+), perplexity (\S+), codes used (\d+)", line)
        assert m, line
        mse, ppl, used = float(m.group(2)), float(m.group(3)), int(m.group(4))
        assert math.isfinite(mse) and mse > 0 and 1 <= used <= K and 1.0 - 1e-6 <= ppl <= used + 1e-4
    if vq_init == "data":
        assert int(vq_lines[0].split(" ")[-1]) >= 2                         # a codebook of frames: more than one code in use
    for line in loss_lines:
        assert math.isfinite(float(line.split(" ")[-1]))
    files = sorted(os.listdir(tmp_path / "restore"))
    assert any(f.endswith(".model") for f in files) and any(f.endswith(".ema") for f in files)
    for f in files:
        ck = torch.load(tmp_path / "restore" / f)
        assert list(ck)[-1] == "vq_codebook.weight" and tuple(ck["vq_codebook.weight"].shape) == (K, bw)
        assert bool(torch.isfinite(ck["vq_codebook.weight"]).all())
