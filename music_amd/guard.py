"""Guarded optimizer step: global-norm gradient clipping and the skipping of a non-finite step, decided on the device
(``wn_grad_guard`` + the ``*_guarded`` updates, include/wavenet_hip.h) - what ``torch.nn.utils.clip_grad_norm_`` plus a finiteness
check would do between ``backward()`` and ``step()``, without the 123 small launches and without the host reading the norm.

``GradGuard`` owns the device-resident ``wn_guard_state`` block and the scratch of one optimizer.  ``flat_step`` issues every update
of an engine's flat buffers, plain or guarded, and what follows it (the codebook's EMA update, the EMA shadow's): the fused step of
the engines (``engine_adam_step``) and the flat optimizers of music_amd/train.py end there.  ``GuardedOptimizer`` is what those
optimizers and the host-guarded ones of music_amd/ae_train.py share on torch's own path.  ``report()`` is the only synchronisation.
"""
import math
import sys

import torch

from . import _lib

_TAKEN, _CLIPPED, _SKIPPED = 2, 3, 4          # int64 words of wn_guard_state holding n_taken, n_clipped, n_skipped
BF16_HINT = 'net.precision = ("bf16x3", "bf16x3")'


def enabled(max_grad_norm, skip_nonfinite):
    return max_grad_norm is not None or bool(skip_nonfinite)


class GradGuard:
    def __init__(self, device, max_grad_norm=None, skip_nonfinite=False, betas=(0.0, 0.0)):
        self.max_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.betas = (float(betas[0]), float(betas[1]))
        self.state = torch.zeros(6, dtype=torch.int64, device=device)                  # wn_guard_state, zeroed
        self.partials = torch.zeros(_lib.GUARD_PARTIALS_BYTES // 8, dtype=torch.int64, device=device)
        self.base = 0                # taken steps the device counter was seeded with that are not steps of this optimizer

    # ---- device path
    def run(self, gptr, n, gscale=1.0):
        """The two launches of wn_grad_guard on the current stream; the guarded update follows with state_ptr()."""
        _lib.call("wn_grad_guard", gptr, n, gscale, self.max_norm, 1 if self.skip_nonfinite else 0, self.betas[0], self.betas[1],
                  self.partials.data_ptr(), self.state.data_ptr(), _lib.stream())

    def state_ptr(self):
        return self.state.data_ptr()

    def seed_taken(self, t, base=0):
        """Start the device's count of taken steps at `t` (a restored optimizer state)."""
        self.state[_TAKEN] = int(t)
        self.base = int(base)

    # ---- host path: the same rule with plain torch, for a step the one-launch path does not cover (a sync is fine there)
    def host_rule(self, params):
        """clip_grad_norm_ + finiteness check on the .grad of `params`.  False: the step is skipped (do not call torch's step)."""
        grads = [p.grad for p in params if p.grad is not None]
        if not grads:
            return True
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.detach().double()) for g in grads])).item()
        if self.skip_nonfinite and not math.isfinite(norm):
            self.state[_SKIPPED] += 1
            return False
        if self.max_norm > 0.0:
            applied = torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], self.max_norm)
            if self.max_norm / (float(applied) + 1e-6) < 1.0:            # the norm clip_grad_norm_ itself clipped by
                self.state[_CLIPPED] += 1
        self.state[_TAKEN] += 1
        return True

    # ---- read-back
    def report(self):
        """Reads the state block back (synchronises): norm / coef of the last device step, counters since the start."""
        raw = self.state.cpu().numpy().tobytes()
        s = _lib.GuardState.from_buffer_copy(raw)
        return dict(norm=float(s.norm), coef=float(s.coef), taken=int(s.n_taken) - self.base, clipped=int(s.n_clipped),
                    skipped=int(s.n_skipped), nonfinite=int(s.nonfinite))


# ---------------------------------------------------------------- the end of a step: every optimizer update on the flat buffers
def flat_step(eng, entry, gptr, state, plain, guarded, gd=None, shadow=None, gscale=1.0):
    """THE update of eng.flat and what follows it, on the current stream: `entry`(p, g, *state, n, *plain), or under the GradGuard
    `gd` its two launches and `entry`_guarded(p, g, *state, n, *guarded, the guard's state block); then the codebook's EMA update
    of an engine in that mode, then the `shadow`'s (music_amd/ema.py) - both reading the guard's decision.  The flat optimizers of
    music_amd/train.py and the fused step of the engines end here, so the order is written once.  `gptr`: the flat gradient,
    `state`: the optimizer's flat state buffers, `gscale`: what the guard measures the gradient with (the update's own is in the tails)."""
    n = eng.spec.total
    if gd is None:
        _lib.call(entry, _lib.ptr(eng.flat), gptr, *state, n, *plain, _lib.stream())
    else:
        gd.run(gptr, n, gscale)
        _lib.call(entry + "_guarded", _lib.ptr(eng.flat), gptr, *state, n, *guarded, gd.state_ptr(), _lib.stream())
    if getattr(eng, "vq_ema", False):
        eng.vq_ema_step(gd)
    if shadow is not None:
        shadow.update(eng, gd)


# ---------------------------------------------------------------- the fused step of an engine (EngineBase.adam_init / adam_step)
def adam_init_guard(state, device, max_grad_norm, skip_nonfinite):
    """adam_init of an engine: adds the guard to its adam_state when either option is set."""
    state["guard"] = (GradGuard(device, max_grad_norm, skip_nonfinite, (state["b1"], state["b2"]))
                      if enabled(max_grad_norm, skip_nonfinite) else None)
    return state


def engine_adam_step(eng, gscale=1.0):
    """torch.optim.Adam semantics on the engine's flat buffers: wn_adam_flat, or with adam_init's guard wn_grad_guard +
    wn_adam_flat_guarded, and the tail of flat_step.  adam_state["t"] counts the steps ISSUED; under the guard guard_report()
    replaces it by the device's count of steps taken."""
    s = eng.adam_state
    shadow = s.get("ema")
    if shadow is not None:
        shadow.check_step()
    s["t"] += 1
    hyper = (s["lr"], s["b1"], s["b2"], s["eps"])
    flat_step(eng, "wn_adam_flat", _lib.ptr(eng.flat_grad), (_lib.ptr(s["m"]), _lib.ptr(s["v"])),
              hyper + (1.0 - s["b1"] ** s["t"], 1.0 - s["b2"] ** s["t"], gscale), hyper + (gscale,), s.get("guard"), shadow, gscale)


def adam_step_guarded(eng, gscale):
    """The guarded form of engine_adam_step, for a caller that holds an engine whose adam_state has a guard."""
    assert eng.adam_state["guard"] is not None
    engine_adam_step(eng, gscale)


def engine_guard_report(eng):
    s = eng.adam_state
    if s is None or s.get("guard") is None:
        return None
    rep = s["guard"].report()
    s["t"] = rep["taken"]
    return rep


def engine_named_grads(eng):
    """(name, view of the engine's flat gradient) per parameter tensor."""
    out = []
    for n in eng.param_names:
        o, k = eng.spec.off[n], 1
        for d in eng.spec.shape[n]:
            k *= int(d)
        out.append((n, eng.flat_grad[o:o + k]))
    return out


class GuardedOptimizer:
    """Mixin in front of a torch optimizer class: the options, the lazily made GradGuard, torch's `step` counters kept equal to the
    device's count of steps TAKEN wherever torch reads them (state_dict(), a step on torch's own path), and the host form of the
    rule for such a step."""

    ema = None                   # the ShadowParams of music_amd/ema.py when ema_decay is set (_ema_setup), else None
    _model = None                # the module whose parameters these are, where the optimizer was given it

    def _guard_setup(self, max_grad_norm, skip_nonfinite):
        self._guard_opts = (max_grad_norm, bool(skip_nonfinite)) if enabled(max_grad_norm, skip_nonfinite) else None
        self._guard = None

    def _ema_setup(self, named_params, ema_decay, ema_warmup):
        """ema_decay set: `ema`, the shadow of the parameters, taken here; every step ends with its update."""
        from . import ema
        self.ema = ema.make(ema_decay, ema_warmup)
        if self.ema is not None:
            self.ema.bind(named_params)

    def _guard_seed_device(self, running):
        """Start the device's count from torch's step counters; the shadow's update number continues (its offset absorbs the
        difference; `running`: the count so far is read back from the device first)."""
        t, base = self._guard_seed()
        if self.ema is not None:
            self.ema.continue_from(self.ema.updates(self._guard if running else None), t)
        self._guard.seed_taken(t, base)

    def _guard_seed(self):
        """(count of taken steps to start the device from, how many of them are not this optimizer's): torch's step counters."""
        steps = [float(st["step"]) for st in self.state.values() if st.get("step") is not None]
        return (int(max(steps)) if steps else 0), 0

    def _guard_get(self, device):
        if self._guard is None:
            self._guard = GradGuard(device, self._guard_opts[0], self._guard_opts[1], self.param_groups[0].get("betas", (0.0, 0.0)))
            self._guard_seed_device(False)
        return self._guard

    def _guard_reseed(self):
        if self._guard is not None:
            self._guard_seed_device(True)

    def _guard_sync_steps(self):
        if self._guard is None:
            return
        t = self._guard.report()["taken"]
        for st in self.state.values():
            s = st.get("step")
            if torch.is_tensor(s):
                s.fill_(float(t))
            elif s is not None:
                st["step"] = t

    def state_dict(self):
        self._guard_sync_steps()
        return super().state_dict()

    def guard_report(self):
        """norm / coef / taken / clipped / skipped / nonfinite of the guard (synchronises); None before the first guarded step."""
        return None if self._guard is None else self._guard.report()

    def _torch_step(self, closure=None, checked=False):
        """torch's own step; guarded: the same rule on the host first (clip_grad_norm_, and a non-finite gradient is not applied).
        With `ema`, the shadow's update in plain torch follows a step that was taken (`checked`: the caller has made its
        check_step() already)."""
        params = [p for grp in self.param_groups for p in grp["params"]]
        if self.ema is not None and not checked:
            self.ema.check_step()
        taken, gd = True, None
        if self._guard_opts is None:
            loss = super().step(closure)
        else:
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
            gd = self._guard_get(params[0].device)
            self._guard_sync_steps()
            taken = gd.host_rule(params)
            if taken:
                super().step()
        # a model whose vq codebook follows EMA updates: its engine's update behind the parameters' and in front of the shadow's, as
        # in flat_step - but on the HOST's decision, which is why neither reads the guard's state block here
        eng = getattr(self._model, "_engine", None)
        if taken and eng is not None and getattr(eng, "vq_ema", False):
            eng.vq_ema_step()
        if self.ema is not None:
            self.ema.host_update(params, taken, gd)
        return loss


# ---------------------------------------------------------------- train() / ae_train: guard_log.log and the one warning
def guard_options(train_params):
    """(max_grad_norm or None, skip_nonfinite) from the optional JSON keys "max_grad_norm" (float) and "skip_nonfinite" (bool)."""
    m = train_params.get("max_grad_norm")
    return (None if m is None else float(m)), bool(train_params.get("skip_nonfinite"))


def guard_log_line(num_trained, rep, last):
    """One line of guard_log.log: pieces trained, the last norm, clipped / skipped steps since the line before (`last` = the
    report that line was made from, or None)."""
    dc = rep["clipped"] - (last["clipped"] if last else 0)
    ds = rep["skipped"] - (last["skipped"] if last else 0)
    return "Trained over %d pieces,Gradient norm is %s,clipped %d,skipped %d\n" % (num_trained, repr(float(rep["norm"])), dc, ds)


def nonfinite_tensors(named_grads):
    """Names of the tensors of (name, gradient) whose gradient holds a NaN or an inf (cold path: plain torch)."""
    return [n for n, g in named_grads if g is not None and not bool(torch.isfinite(g).all())]


def warn_skipped(names, file=None):
    print("music_amd: a training step was skipped: its gradient is not finite (%s).  A value beyond +-65504 overflows the default "
          "f16x3 forward; %s keeps the fp32 range." % (", ".join(names) if names else "no tensor of the CURRENT gradient", BF16_HINT),
          file=file or sys.stderr)


class GuardLog:
    """What train() does at each print_every on rank 0: append the guard_log.log line, and warn once when a step was skipped.  The
    tensors the warning names are BEST EFFORT: those non-finite in the gradient current at this print_every (nothing is read back
    per step), which is the skipped step's only when that step was the last one or the overflow persists."""

    def __init__(self, path, report, named_grads):
        self.path, self.report, self.named_grads = path, report, named_grads
        self.last, self.warned = None, False

    def tick(self, num_trained, write=True):
        rep = self.report()
        if rep is None:
            return None
        if write:
            with open(self.path, "a") as f:
                f.write(guard_log_line(num_trained, rep, self.last))
            if rep["skipped"] > 0 and not self.warned:
                self.warned = True
                warn_skipped(nonfinite_tensors(self.named_grads()))
        self.last = rep
        return rep
