"""Worker for tests/test_gpu_ema.py::test_two_ranks_keep_the_same_shadow: music_amd.train.train() on the device as one rank under
torch.distributed.run.  argv: workdir, poison_step (-1 = none): RANK 1 writes an inf into its local gradient of that global step
(counted from 0), before the all-reduce.  Every rank saves its engine's EMA shadow, the count of its updates and its parameters."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    workdir, poison_step = sys.argv[1], int(sys.argv[2])
    os.chdir(workdir)
    from music_amd import dist as wdist
    from music_amd import train as T
    from music_amd.model import wavenet
    st = {"step": -1, "nets": []}

    def ctor(**kw):
        net = wavenet(**kw)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)                                 # (default init: the double softmax makes every gradient tiny)
        st["nets"].append(net)
        return net
    T.wavenet = ctor
    real_flat = wdist.allreduce_flat_

    def flat_(flat_grad, *a, **kw):                         # the fused step's collective: once per global step
        st["step"] += 1
        if st["step"] == poison_step and wdist.rank() == 1:
            flat_grad[7] = float("inf")
        return real_flat(flat_grad, *a, **kw)
    wdist.allreduce_flat_ = flat_

    T.train()
    torch.cuda.synchronize()
    net = st["nets"][-1]
    eng = net._engine
    cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
    torch.save({"shadow": cpu(eng.ema.state_dict()), "updates": eng.ema.updates(eng.adam_state.get("guard")), "params": cpu(net.state_dict())},
               "shadow_rank%d.pt" % wdist.rank())
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
