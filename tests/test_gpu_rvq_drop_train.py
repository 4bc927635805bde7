"""music_amd/ae_train.py with quantiser dropout, end to end on the device: the JSON keys "vq_stage_dropout" / "vq_dropout_seed", the
stage counts ae_train passes from its global step on both step forms, and the `, active f0/f1/..` tail of vq_log.log.  The run is
the one of tests/test_gpu_vq_train.py (tests/golden/g9_ae_harness.json's data, seed and parameters) with the keys added.  -m gpu."""
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_ae_harness_cpu import g9, write_g9_run

K, S, SEED = 16, 3, 7


@pytest.mark.parametrize("fused,update", [(True, "ema"), (False, "gradient")], ids=["fused_step_ema", "autograd_gradient"])
def test_training_with_stage_dropout_logs_the_active_frames_of_the_steps_draw(tmp_path, monkeypatch, fused, update):
    from music_amd import ae_train as A
    from music_amd.vq_dropout import draw_stages
    g = g9()
    g = dict(g, model_params=dict(g["model_params"], conditioning="learned", bottleneck="vq", vq_codes=K, vq_beta=0.25, vq_stages=S,
                                  vq_update=update, vq_stage_dropout=0.5))
    write_g9_run(tmp_path, g, {"fused_step": fused, "vq_init": "data", "vq_dropout_seed": SEED})
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    A.train()
    loss_lines = open(tmp_path / "log" / "loss_log.log").read().strip().split("\n")
    vq_lines = open(tmp_path / "log" / "vq_log.log").read().strip().split("\n")
    assert len(vq_lines) == len(loss_lines) >= 3 and all(math.isfinite(float(line.split(" ")[-1])) for line in loss_lines)
    dropped = 0
    for line in vq_lines:
        m = re.fullmatch(r"Trained over (\d+) pieces, vq mse (\S+), perplexity (\S+), codes used (\d+).*, active (\d+)/(\d+)/(\d+)", line)
        assert m, line
        assert math.isfinite(float(m.group(2))) and float(m.group(2)) > 0
        active = [int(v) for v in m.groups()[4:]]
        # the line shows the step before it: global step N - 1, clips 0 .. B - 1 of the (one-rank) global batch; B is 2, or 1 on a ragged batch
        step = int(m.group(1)) - 1
        fits = []
        for B in (2, 1):
            n = draw_stages(SEED, step, 0, B, S, 0.5)
            if active[0] % B == 0:
                fits.append(active == [int((n > s).sum()) * (active[0] // B) for s in range(S)])
        assert any(fits), (line, step)
        dropped += active[-1] < active[0]
    assert dropped >= 1, "no logged step dropped a stage: the run decides nothing"
    ck = torch.load(tmp_path / "restore" / "wavenet_autoencoder2.model")
    assert "vq_dropout_calls" not in ck and tuple(ck["vq_codebook.weight"].shape) == (S * K, g["model_params"]["en_bottleneck_width"])
