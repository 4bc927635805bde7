"""EMA shadow weights, kept on the device: the exponential moving average of the parameters that every WaveNet recipe samples from
instead of the last iterate (NSynth, arXiv 1704.01279: ``ExponentialMovingAverage(0.9999, num_updates=global_step)``).  The
reference keeps none.

``ShadowParams`` owns the shadow and is updated by ONE ``wn_ema_flat`` launch behind the optimizer's update (include/wavenet_hip.h)
- not by ``torch._foreach_lerp_`` over 123 tensors, and not on the host: under the guarded step (music_amd/guard.py) only the
device knows whether a step was taken and which step it was, so the launch reads the guard's ``wn_guard_state``: a skipped step
leaves the shadow bit for bit, and the warm-up counts the steps TAKEN.  ``guard.flat_step`` ends with that launch - the fused step
of the engines (``EngineBase.adam_init(ema_decay=...)``) and the flat optimizers of music_amd/train.py
(``get_optimizer(ema_decay=...)``) both go through it; a step on torch's own path ends with the same rule in plain torch
(``host_update``, from ``GuardedOptimizer._torch_step``).

Rule (float32; swa_utils.get_ema_avg_fn's lerp, TensorFlow's num_updates warm-up):
    d_eff = min(decay, (1 + T) / (10 + T)) with warm-up, else decay ;  w = 1 - d_eff ;  ema += w * (p - ema)
T = the number of this update: the host's ``n_updates`` unguarded, the device's count of taken steps + ``offset`` guarded.
"""
from collections import OrderedDict
from contextlib import contextmanager
import math

import numpy as np
import torch

from . import _lib
from .guard import _TAKEN


def ema_options(train_params):
    """(ema_decay or None, ema_warmup) from the optional JSON keys "ema_decay" (float) and "ema_warmup" (bool)."""
    d = train_params.get("ema_decay")
    return (None if d is None else float(d)), bool(train_params.get("ema_warmup"))


def weight(decay, warmup, T):
    """w of update number T as the kernel forms it: d_eff in double from the float32 decay, rounded once, then 1.0f - d_eff."""
    d = float(np.float32(decay))
    if warmup:
        T = max(1, int(T))
        d = min(d, (1.0 + T) / (10.0 + T))
    return float(np.float32(1.0) - np.float32(d))


def warmup_done(decay):
    """The first update number from which the warm-up no longer acts: (1 + T) / (10 + T) >= decay."""
    d = float(np.float32(decay))
    return max(1, int(math.ceil((10.0 * d - 1.0) / (1.0 - d))))


class ShadowParams:
    """The shadow of one module's parameters.  Storage: a clone of the engine's flat parameter buffer once the parameters live on
    one (`flat`; the per-name tensors are views of it), per-parameter clones before that.  Taken at bind() - construction of the
    optimizer / adam_init of the engine - hence from the initial or the restored weights."""

    def __init__(self, decay, warmup=False):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:                         # (NaN fails both comparisons)
            raise ValueError("ema_decay must lie in [0, 1), got %r" % decay)
        self.decay, self.warmup = decay, bool(warmup)
        self.n_updates = 0           # updates made so far, as far as the host knows (exact unguarded and on torch's path)
        self.offset = 0              # guarded: T = the device's count of taken steps + offset
        self.flat = None
        self.tensors = None          # OrderedDict name -> tensor, in the module's parameter order
        self._swapped = False

    # ---- storage
    def bind(self, named_params):
        """Take the shadow from (name, parameter) pairs unless there is one already."""
        if self.tensors is None:
            self.tensors = OrderedDict((n, p.detach().clone()) for n, p in named_params)
        return self

    def bind_engine(self, eng):
        """Move the shadow onto a clone of `eng`'s flat parameter buffer (what there is of it is kept; else eng.flat is cloned)."""
        if self.flat is not None and self.flat.device == eng.flat.device and self.flat.numel() == eng.flat.numel():
            return self
        flat = eng.flat.detach().clone()
        views = OrderedDict()
        for n in eng.param_names:
            o, shp = eng.spec.off[n], eng.spec.shape[n]
            views[n] = flat[o:o + int(np.prod(shp))].view(shp)
            if self.tensors is not None:
                views[n].copy_(self.tensors[n])
        self.flat, self.tensors = flat, views
        return self

    def state_dict(self):
        """The shadow under the module's keys (the tensors themselves, as nn.Module.state_dict gives them)."""
        if self.tensors is None:
            raise RuntimeError("music_amd.ema: the shadow has not been taken yet (no optimizer step, bind() or load_state_dict())")
        return OrderedDict((n, t.detach()) for n, t in self.tensors.items())

    def load_state_dict(self, sd, n_updates=None):
        """Restore a shadow saved by state_dict() (a "module." prefix is accepted, as train.load_model does)."""
        if list(sd.keys())[0][:7] == "module.":
            sd = OrderedDict((k[7:], v) for k, v in sd.items())
        if self.tensors is None:
            self.tensors = OrderedDict((n, v.detach().clone()) for n, v in sd.items())
        else:
            if list(sd.keys()) != list(self.tensors.keys()):
                raise KeyError("music_amd.ema: the keys of the shadow differ from the module's")
            with torch.no_grad():
                for n, t in self.tensors.items():
                    t.copy_(sd[n])
        if n_updates is not None:
            self.n_updates = int(n_updates)

    # ---- the count of updates
    def updates(self, guard=None):
        """Updates made so far; guarded, the device's count is read back (synchronises)."""
        if guard is not None:
            self.n_updates = int(guard.state[_TAKEN].item()) + self.offset
        return self.n_updates

    def continue_from(self, n_updates, taken_seed=None):
        """The next update is number n_updates + 1; `taken_seed`: what the guard's device counter starts from."""
        self.n_updates = int(n_updates)
        self.offset = 0 if taken_seed is None else self.n_updates - int(taken_seed)

    def check_step(self):
        if self._swapped:
            raise RuntimeError("music_amd.ema: an optimizer step while the parameters hold the shadow (inside swapped())")

    # ---- updates
    def update(self, eng, guard=None):
        """THE wn_ema_flat launch, behind the update of eng.flat on the current stream.  `guard`: the GradGuard whose wn_grad_guard
        decided this step."""
        self.check_step()
        self.bind_engine(eng)
        if guard is None:
            self.n_updates += 1
            t, state = self.n_updates, None
        else:
            t, state = self.offset, guard.state_ptr()
        _lib.call("wn_ema_flat", _lib.ptr(self.flat), _lib.ptr(eng.flat), eng.spec.total, self.decay, 1 if self.warmup else 0, t, state,
                  _lib.stream())

    def host_update(self, params, taken=True, guard=None):
        """The same rule with torch._foreach_lerp_, for a step on torch's own path; `params` in the order of bind().  Not run
        when the guard's host_rule skipped the step (`taken` False).  `guard`: T follows its count of taken steps."""
        self.check_step()
        if not taken:
            return
        params = list(params)
        if self.tensors is None:
            raise RuntimeError("music_amd.ema: host_update() before bind()")
        shadow = list(self.tensors.values())
        if len(shadow) != len(params):
            raise ValueError("music_amd.ema: %d parameters for a shadow of %d" % (len(params), len(shadow)))
        if shadow and shadow[0].device != params[0].device:                  # the module was moved after bind()
            for n, p in zip(list(self.tensors), params):
                self.tensors[n] = self.tensors[n].to(p.device)
            self.flat, shadow = None, list(self.tensors.values())
        self.n_updates = self.updates(guard) if guard is not None else self.n_updates + 1
        with torch.no_grad():
            torch._foreach_lerp_(shadow, [p.detach() for p in params], weight(self.decay, self.warmup, self.n_updates))

    # ---- swapping
    @contextmanager
    def swapped(self, model):
        """Inside, the module's parameters HOLD the shadow (their content, not their identity: the engine's flat buffer, and with
        it the weight packs and the decoder, see it).  On exit - also on an exception - parameters and shadow are back bit for
        bit.  An optimizer step inside raises RuntimeError."""
        self.check_step()
        named = list(model.named_parameters())
        self.bind(named)
        if [n for n, _ in named] != list(self.tensors):
            raise KeyError("music_amd.ema: the module's parameters are not the ones this shadow was taken from")
        saved = [p.detach().clone() for _, p in named]
        self._swapped = True
        try:
            with torch.no_grad():
                for n, p in named:
                    p.copy_(self.tensors[n])
            yield model
        finally:
            with torch.no_grad():
                for (_, p), s in zip(named, saved):
                    p.copy_(s)
            self._swapped = False


# ---------------------------------------------------------------- train() / ae_train: the .ema file beside every .model
BUFFER_KEYS = ("vq_ema_state",)     # a module's buffers that an .ema file carries beside the shadow (there is no average of them)


def save_shadow(shadow, path, model=None):
    """The shadow in the .model format (a bare state_dict pickle on the CPU): train.load_model(net, dir, "wavenet5.ema") reads it.
    `model`: its buffers named in BUFFER_KEYS (the running state of an EMA-updated vq codebook) are written behind the shadow as
    they are, so that the file loads into a model of the same mode."""
    sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in shadow.state_dict().items())
    if model is not None:
        for k, v in model.named_buffers():
            if k in BUFFER_KEYS:
                sd[k] = v.detach().cpu().clone()
    torch.save(sd, path)


def restore_shadow(shadow, path, n_updates, guard=None):
    """A resumed run: the shadow from `path` if it exists, else it stays what it was taken from, the restored weights (one
    printed line).  `n_updates`: the saved count ("ema_updates" of the .opt blob); None: the warm-up is treated as finished.
    `guard`: the (already seeded) GradGuard of the step, so that T continues from the count."""
    import os
    if os.path.exists(path):
        shadow.load_state_dict(OrderedDict((k, v) for k, v in torch.load(path, map_location="cpu").items() if k not in BUFFER_KEYS))
    else:
        print("No EMA shadow found at {}, it starts from the restored weights.".format(path))
    n = warmup_done(shadow.decay) if n_updates is None else int(n_updates)
    shadow.continue_from(n, None if guard is None else int(guard.state[_TAKEN].item()))


def make(decay, warmup=False):
    """ShadowParams(decay, warmup), or None when `decay` is unset."""
    return None if decay is None else ShadowParams(decay, warmup)
