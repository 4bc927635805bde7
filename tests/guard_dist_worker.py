"""Worker for tests/test_gpu_guard_surface.py::test_train_two_ranks_skip_the_same_step: music_amd.train.train() on the device, alone or as
one rank under torch.distributed.run.  argv: workdir, poison_step, omit_step (-1 = none).
  poison_step: RANK 1 writes an inf into its local gradient of that global step, before the all-reduce;
  omit_step:   the optimizer step of that global step is left out (how the reference run "skips" without any guard)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    workdir, poison_step, omit_step = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
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

    real_flat, real_grads = wdist.allreduce_flat_, wdist.allreduce_gradients

    def flat_(flat_grad, *a, **kw):                         # the fused step's collective: once per global step
        st["step"] += 1
        if st["step"] == poison_step and wdist.rank() == 1:
            flat_grad[7] = float("inf")
        return real_flat(flat_grad, *a, **kw)

    def grads_(params, *a, **kw):                           # the autograd path's
        params = list(params)
        st["step"] += 1
        if st["step"] == poison_step and wdist.rank() == 1:
            next(p for p in params if p.grad is not None).grad.view(-1)[7] = float("inf")
        return real_grads(params, *a, **kw)                 # (it calls the real allreduce_flat_ through the module: not counted twice)

    inner = {"busy": False}                                 # allreduce_gradients reaches allreduce_flat_ by its module name

    def flat_once(flat_grad, *a, **kw):
        if inner["busy"]:
            return real_flat(flat_grad, *a, **kw)
        return flat_(flat_grad, *a, **kw)

    def grads_once(params, *a, **kw):
        inner["busy"] = True
        try:
            return grads_(params, *a, **kw)
        finally:
            inner["busy"] = False
    wdist.allreduce_flat_, wdist.allreduce_gradients = flat_once, grads_once

    def omitting(real):
        def step(*a, **kw):
            if st["step"] == omit_step:
                return None
            return real(*a, **kw)
        return step
    real_engine_for, real_get_optimizer = wavenet._engine_for, T.get_optimizer

    def engine_for(self, device):
        eng = real_engine_for(self, device)
        if not getattr(eng, "_omit_wrapped", False):
            eng.adam_step, eng._omit_wrapped = omitting(eng.adam_step), True
        return eng

    def get_optimizer(*a, **kw):
        opt = real_get_optimizer(*a, **kw)
        opt.step = omitting(opt.step)
        return opt
    wavenet._engine_for, T.get_optimizer = engine_for, get_optimizer

    T.train()
    torch.cuda.synchronize()
    net = st["nets"][-1]
    torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "params_rank%d.pt" % wdist.rank())
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
