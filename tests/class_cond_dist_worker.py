"""Worker for tests/test_gpu_class_cond_train.py: the data-parallel step of a class-conditional WaveNet - every rank trains on its
contiguous chunk of ONE global batch of clips and classes, one flat all-reduce per step (the global block is part of the flat buffer),
1 / world inside Adam.  The protocol of tests/dist_worker_gpu.py."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = dict(filter_width=2, dilations=[1, 2, 4, 8], dilation_channels=64, residual_channels=64, skip_channels=256,
           quantization_channels=256, use_bias=False, global_classes=3, global_channels=12)
CLASSES = [2, 0, 2, 1]


def main():
    workdir = sys.argv[1]
    shards = int(sys.argv[2])                                       # logical shards of the global batch (2 clips each)
    from music_amd import dist as wdist
    from music_amd.model import wavenet
    rank, world, local = wdist.init_from_env()
    backend = torch.distributed.get_backend() if torch.distributed.is_initialized() else "none"
    torch.manual_seed(0)
    net = wavenet(**CFG)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    net = net.cuda()
    wdist.broadcast_parameters(net.parameters())
    eng = net._engine_for(torch.device("cuda", local))
    eng.adam_init(lr=1e-3)
    rng = np.random.default_rng(100)
    assert shards % world == 0 and 2 * shards == len(CLASSES)
    B, T = 2 * shards // world, net.receptive_field + 120
    codes = torch.from_numpy(rng.integers(0, 256, size=(2 * shards, T + 1)).astype(np.int32))[rank * B:(rank + 1) * B].cuda()
    classes = torch.tensor(CLASSES[rank * B:(rank + 1) * B])
    rf = net.receptive_field
    W = T - rf + 1
    losses, gsum, gtail = [], None, None
    for step in range(3):
        x = eng.onehot(codes[:, :T].contiguous(), scrambled=True)
        target = codes[:, rf:rf + W].to(torch.int64).contiguous().view(-1)
        loss = eng.loss_and_grad(x, target, classes=classes)
        if torch.distributed.is_initialized():
            torch.distributed.all_reduce(eng.flat_grad)
        eng.adam_step(gscale=1.0 / world)
        if torch.distributed.is_initialized():
            torch.distributed.all_reduce(loss)
            loss = loss / world
        losses.append(float(loss.item()))
        gsum = float(eng.flat_grad.abs().sum().item()) / world
        gtail = float(eng.flat_grad[eng.n_gather:].abs().sum().item()) / world
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
    torch.cuda.synchronize()
    if rank == 0:
        json.dump({"backend": backend, "world": world, "losses": losses, "gsum": gsum, "gtail": gtail,
                   "psum": float(eng.flat.double().abs().sum().item()),
                   "ptail": float(eng.flat[eng.n_gather:].double().abs().sum().item())}, open(os.path.join(workdir, "dist_gpu.json"), "w"))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
