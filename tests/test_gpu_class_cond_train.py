"""music_amd/train.py with a class-conditional WaveNet, end to end on the device: "labels_path" reaches the loader and the step, the
checkpoints (.model / .opt / .ema) carry the global block and a resumed run continues bit for bit, a checkpoint of the other mode is
refused by name, the guard skips a step whose class-embedding gradient is not finite and leaves the global block bit for bit, and two
ranks with two clips each equal one rank with the four (the rule and tolerances of tests/test_gpu_dist.py).  Run with -m gpu."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import ROOT

NC, E = 3, 6
CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=16, residual_channels=16, skip_channels=16,
           quantization_channels=256, use_bias=False, global_classes=NC, global_channels=E)
TAIL = ["gcond_layer_stack.%d.weight" % i for i in range(4)] + ["connection_gcond.weight", "global_embedding.weight"]


def _write_run(tmp, extra, cfg=CFG, labels=True):
    os.makedirs(tmp / "params")
    rng = np.random.default_rng(5)
    data = [rng.integers(0, 256, size=(l,)).astype(np.int32) for l in (417, 417)]                # 8 pieces: two batches of 4
    pickle.dump(data, open(tmp / "np_audio.pkl", "wb"))
    dp = dict(batch_size=4, shuffle=False, num_workers=0, pin_memory=False, audio_path=str(tmp / "np_audio.pkl"), receptive_field=17,
              window_length=100, cuda_available=False, quantization_channels=256)
    if labels:
        json.dump([2, 0], open(tmp / "labels.json", "w"))
        dp["labels_path"] = str(tmp / "labels.json")
    tp = dict(log_dir="./log/", restore_dir="./restore/", restore_model="", check_point_every=1, print_every=2, num_epochs=1,
              wavenet_params="", optimizer="adam", max_check_points=10, learning_rate=1e-3, momentum=0.9, device_ids=None, seed=3)
    tp.update(extra)
    for n, p in (("wavenet", cfg), ("dataset", dp), ("train", tp)):
        json.dump(p, open(tmp / "params" / (n + "_params.json"), "w"))
    return tp


def _ctor(**kw):
    from music_amd.model import wavenet
    net = wavenet(**kw)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    return net


@pytest.mark.parametrize("fused,objective", [(True, "reference"), (False, "nll")], ids=["fused_step", "autograd_nll"])
def test_train_with_labels_writes_its_checkpoints_and_resumes_bit_for_bit(tmp_path, monkeypatch, fused, objective):
    from music_amd import train as T
    from music_amd.engine_base import EngineBase
    extra = {"fused_step": fused, "objective": objective, "save_optimizer_state": True, "ema_decay": 0.9, "ema_warmup": True,
             "max_grad_norm": 0.05, "skip_nonfinite": True}
    if objective == "nll":
        extra.update(valid_audio_path=str(tmp_path / "straight" / "np_audio.pkl"), validate_every=2,
                     valid_labels_path=str(tmp_path / "straight" / "labels.json"))
    seen = []
    real = EngineBase.stage_classes
    monkeypatch.setattr(EngineBase, "stage_classes", lambda self, classes, B: seen.append((classes, B)) or real(self, classes, B))
    monkeypatch.setattr(T, "wavenet", _ctor)
    finals = {}
    for mode in ("straight", "resumed"):
        root = tmp_path / mode
        os.makedirs(root)
        tp = _write_run(root, dict(extra, num_epochs=2 if mode == "straight" else 1))
        monkeypatch.chdir(root)
        torch.manual_seed(0)
        T.train()
        if mode == "resumed":
            assert sorted(os.listdir(root / "restore")) == ["wavenet1.ema", "wavenet1.model", "wavenet1.opt"]
            json.dump(dict(tp, restore_model="wavenet1.model"), open(root / "params" / "train_params.json", "w"))
            T.train()
        finals[mode] = [torch.load(root / "restore" / ("wavenet2" + s)) for s in (".ema", ".model")]
    # every step handed the batch's classes on, from the host, one per clip, the labels of the items the pieces were cut from
    assert seen and all(torch.is_tensor(c) and c.device.type == "cpu" and c.dtype == torch.int64 and c.numel() == B for c, B in seen)
    assert {int(v) for c, _ in seen for v in c} == {0, 2}
    for a, b in zip(finals["straight"], finals["resumed"]):
        assert list(a) == list(b) and list(a)[-6:] == TAIL
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
    shadow, model = finals["straight"]
    assert tuple(model["global_embedding.weight"].shape) == (NC, E) and all(bool(torch.isfinite(v).all()) for v in model.values())
    assert any(not torch.equal(shadow[k], model[k]) for k in TAIL)
    first = torch.load(tmp_path / "straight" / "restore" / "wavenet1.model")
    assert all(not torch.equal(first[k], model[k]) for k in TAIL[:-1])             # the global block trains
    assert not torch.equal(first[TAIL[-1]][[0, 2]], model[TAIL[-1]][[0, 2]]) and torch.equal(first[TAIL[-1]][1], model[TAIL[-1]][1])
    opt = torch.load(tmp_path / "straight" / "restore" / "wavenet2.opt")
    assert opt["ema_updates"] == 4
    if objective == "nll":
        lines = open(tmp_path / "straight" / "log" / "valid_log.log").read().strip().split("\n")
        assert len(lines) == 2 and all(np.isfinite(float(ln.split("nll is ")[1].split(",")[0])) for ln in lines)


def test_labels_and_the_mode_go_together_and_a_checkpoint_of_the_other_mode_is_refused(tmp_path, monkeypatch):
    from music_amd import train as T
    plain = {k: v for k, v in CFG.items() if not k.startswith("global")}
    for name, cfg, labels, msg in (("a", CFG, False, '"labels_path"'), ("b", plain, True, '"global_classes" at 0')):
        root = tmp_path / name
        os.makedirs(root)
        _write_run(root, {}, cfg=cfg, labels=labels)
        monkeypatch.chdir(root)
        with pytest.raises(ValueError, match=msg):
            T.train()
    # a checkpoint of the plain model into the class-conditional one, and the other way round: refused whole, by name
    root = tmp_path / "c"
    os.makedirs(root)
    _write_run(root, {}, cfg=plain, labels=False)
    monkeypatch.chdir(root)
    T.train()
    assert os.path.exists(root / "restore" / "wavenet1.model")
    json.dump(CFG, open(root / "params" / "wavenet_params.json", "w"))
    tp = json.load(open(root / "params" / "train_params.json"))
    json.dump(dict(tp, restore_model="wavenet1.model"), open(root / "params" / "train_params.json", "w"))
    dp = json.load(open(root / "params" / "dataset_params.json"))
    json.dump([2, 0], open(root / "labels.json", "w"))
    json.dump(dict(dp, labels_path=str(root / "labels.json")), open(root / "params" / "dataset_params.json", "w"))
    with pytest.raises(RuntimeError, match="saved with global_classes=0, global_channels=0 but this model was built with global_classes=3"):
        T.train()


def test_the_guard_skips_a_non_finite_class_embedding_gradient():
    """a non-finite value planted in the class embedding's gradient: the guarded step is skipped and the global block (like every
    parameter, the moments and the shadow) stays bit for bit; the next clean step moves it"""
    net = _ctor(**CFG).cuda()
    eng = net._engine_for(next(net.parameters()).device)
    eng.adam_init(lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    rng = np.random.default_rng(3)
    T_ = net.receptive_field + 60
    codes = torch.from_numpy(rng.integers(0, 256, size=(2, T_ + 1)).astype(np.int32)).cuda()
    x = eng.onehot(codes[:, :T_].contiguous(), scrambled=False)
    target = codes[:, net.receptive_field:].to(torch.int64).contiguous().view(-1)
    classes = [1, 2]
    eng.loss_and_grad(x, target, classes=classes)
    eng.adam_step()
    before = eng.flat.clone()
    eng.loss_and_grad(x, target, classes=classes)
    emb = eng.spec.off["global_embedding.weight"]
    assert emb + NC * E == eng.spec.total
    eng.flat_grad[emb + 1 * E + 2] = float("inf")
    eng.adam_step()
    rep = eng.guard_report()
    assert torch.equal(before.view(torch.int32), eng.flat.view(torch.int32)), "a skipped step changed a parameter"
    assert int(rep["skipped"]) == 1 and int(rep["taken"]) == 1
    eng.loss_and_grad(x, target, classes=classes)
    eng.adam_step()
    assert not torch.equal(before[eng.n_gather:], eng.flat[eng.n_gather:]) and bool(torch.isfinite(eng.flat).all())


def test_two_ranks_with_two_clips_equal_one_rank_with_four(tmp_path):
    def run(nproc, shards, backend=None, launcher=True):
        env = dict(os.environ, PYTHONPATH=ROOT)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "WN_DIST_BACKEND"):
            env.pop(k, None)
        if backend:
            env["WN_DIST_BACKEND"] = backend
        worker = os.path.join(ROOT, "tests", "class_cond_dist_worker.py")
        cmd = ([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
                "--nproc-per-node", str(nproc), worker, str(tmp_path), str(shards)] if launcher else
               [sys.executable, worker, str(tmp_path), str(shards)])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return json.load(open(tmp_path / "dist_gpu.json"))
    whole = run(1, 2, launcher=False)
    many = run(2, 2, backend=None if torch.cuda.device_count() >= 2 else "gloo")
    assert whole["world"] == 1 and many["world"] == 2 and whole["gtail"] > 0
    for a, b in zip(many["losses"], whole["losses"]):
        assert abs(a - b) < 2e-5, (many["losses"], whole["losses"])
    assert abs(many["gsum"] - whole["gsum"]) < 1e-3 * whole["gsum"]
    assert abs(many["gtail"] - whole["gtail"]) < 1e-3 * whole["gtail"]
    assert abs(many["psum"] - whole["psum"]) < 1e-5 * whole["psum"]
    assert abs(many["ptail"] - whole["ptail"]) < 1e-5 * whole["ptail"]
