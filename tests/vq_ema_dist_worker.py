"""Worker for tests/test_gpu_vq_ema_dist.py: one rank of a data-parallel run of an autoencoder whose vq codebook follows EMA
updates, stepping the way music_amd/ae_train.py does with "fused_step": loss_and_grad on this rank's shard, the sum all-reduce of
the flat gradient, the sum all-reduce of the per-code counts and sums (vq_stat), the Adam step with 1 / world - which ends with
wn_vq_ema_update.  argv: workdir.  In the second of the three steps rank 1's shard is EMPTY: it contributes zeros to both sums.
Every rank saves its codebook, its running state and the counts of the summed stat of every step."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, B_RANK, W = 32, 2, 320
CFG = dict(filter_width=2, quantization_channel=256, dilations=[1, 2, 4, 8], en_residual_channel=64, en_dilation_channel=64,
           en_bottleneck_width=16, en_pool_kernel_size=40, de_residual_channel=64, de_dilation_channel=64, de_skip_channel=256,
           use_bias=False, conditioning="learned", bottleneck="vq", vq_codes=K, vq_update="ema", vq_decay=0.9, vq_restart=0.95)


def main():
    workdir = sys.argv[1]
    from music_amd import dist as wdist
    from music_amd.model1 import wavenet_autoencoder
    rank, world, local = wdist.init_from_env()
    assert world == 2 and torch.distributed.is_initialized()
    torch.manual_seed(10 + rank)                             # the replicas start DIFFERENT: the broadcast makes them rank 0's
    net = wavenet_autoencoder(**CFG)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        net.reset_vq_ema_state()
    net = net.cuda()
    wdist.broadcast_parameters(list(net.parameters()) + list(net.buffers()))
    eng = net._engine_for(torch.device("cuda", local))
    eng.adam_init(lr=1e-3)
    rng = np.random.default_rng(7)
    T = net.receptive_field + W - 1
    counts = []
    for step in range(3):
        codes = torch.from_numpy(rng.integers(0, 256, size=(world * B_RANK, T)))          # the global batch; this rank's clips of it
        target = torch.from_numpy(rng.integers(0, 256, size=(world * B_RANK, W)).astype(np.int64))
        mine = slice(rank * B_RANK, (rank + 1) * B_RANK)
        if step == 1 and rank == 1:                          # an empty shard
            eng.flat_grad.zero_()
            eng.vq_stat.zero_()
        else:
            x = torch.nn.functional.one_hot(codes[mine], 256).permute(0, 2, 1).float().contiguous().cuda()
            eng.loss_and_grad(x, target[mine].reshape(-1).cuda(), net.engine_cond())
        wdist.allreduce_flat_(eng.flat_grad, average=False, scale=1.0)
        wdist.allreduce_flat_(eng.vq_stat, average=False, scale=1.0)
        counts.append(float(eng.vq_stat[:K].double().sum().item()))
        eng.adam_step(gscale=1.0 / world)
    torch.cuda.synchronize()
    torch.save({"codebook": net.vq_codebook.weight.detach().cpu().clone(), "state": net.vq_ema_state.cpu().clone(),
                "flat": eng.flat.cpu().clone(), "counts": counts, "restarted": eng.vq_restarted(),
                "frames_per_rank": B_RANK * (W // CFG["en_pool_kernel_size"])}, os.path.join(workdir, "vq_ema_rank%d.pt" % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
