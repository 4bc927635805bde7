"""Counterpart of the reference's ``wavenet/train.py`` for the MI355X path.

Same function names, JSON schema (./params/{train,wavenet,dataset}_params.json read relative to the
CWD), step order ``zero_grad -> forward -> CrossEntropyLoss(probs, target.view(-1)) -> backward ->
step`` (wavenet/train.py:171-182), batch counter and its recovery from the last log line
(:160-166,186), log-line formats (:189-191,217-218), checkpoint naming / rotation / ``module.``
stripping (:45-73,198-216).  The reference file itself cannot run on Python >= 3.7
(``.cuda(async=True)``), so this module is the drop-in.

Differences, all additive:
  * ``nn.DataParallel`` (one process, GPU-0 bottleneck) is replaced by one process per GPU
    (``torchrun --nproc-per-node N train.py``) with ONE flat RCCL all-reduce per step
    (music_amd/dist.py); each rank builds only its own shard of every global batch.
  * optional keys in train_params.json: ``"seed"`` (int), ``"fused_step"`` (bool: Adam only — the
    whole step runs as forward+CE+backward+flat-Adam kernels without autograd), ``"save_optimizer_state"``
    (bool, SURVEY 8f4: the reference drops the optimizer state at every checkpoint, so a resumed Adam /
    momentum run restarts cold; with this key ``wavenet{N}.opt`` is written next to ``wavenet{N}.model``
    and read back when that model is restored — the .model file itself stays the reference's format),
    ``"max_grad_norm"`` (float: the gradient is clipped to that global L2 norm, torch.nn.utils.clip_grad_norm_'s rule) and
    ``"skip_nonfinite"`` (bool: a step whose gradient holds a NaN or an inf is not applied) — both decided on the device
    (music_amd/guard.py), after the all-reduce under data parallelism so that every rank takes the same decision; rank 0 then
    appends a line per ``print_every`` to ``guard_log.log`` and warns once on stderr when a step was skipped (the tensors it
    names are those non-finite in the gradient current at that ``print_every``: best effort, nothing is read back per step).
    Scaling under data parallelism: a ragged shard's ``dp_scale`` differs per rank and has to multiply the local buffer before
    the sum; the 1 / world of the mean is folded into the guard's ``gscale`` on the fused step, while the autograd path keeps
    it in ``allreduce_gradients`` (the gradients are the optimizer's ``.grad`` tensors there, which torch's own step reads too).
    ``"ema_decay"`` (float) and ``"ema_warmup"`` (bool): an exponential moving average of the parameters is kept on the device
    (music_amd/ema.py: one launch behind every optimizer step; under the guard a skipped step leaves it alone and the warm-up
    counts the steps taken) and written as ``wavenet{N}.ema`` next to every ``wavenet{N}.model``, in the same format - so
    ``load_model(net, dir, "wavenet{N}.ema")`` and ``fast_generate.generate(dir, "wavenet{N}.ema", ...)`` sample from it.  A
    resumed run reads it back (with ``"save_optimizer_state"`` also the count of updates, ``"ema_updates"`` in the ``.opt`` blob).
"""
from collections import OrderedDict
from functools import cmp_to_key
import glob
import json
import os

import torch
import torch.nn as nn
import torch.optim as optim

try:
    from . import class_dropout
    from . import dist as wdist
    from . import ema
    from . import guard
    from . import objective as wobjective
    from .faster_audio_data import audio_data_loader
    from .model import wavenet
except ImportError:                                  # run as a script / bare modules from the CWD
    from music_amd import class_dropout
    from music_amd import dist as wdist
    from music_amd import ema
    from music_amd import guard
    from music_amd import objective as wobjective
    from music_amd.faster_audio_data import audio_data_loader
    from music_amd.model import wavenet


def get_params(json_dir):
    with open(json_dir, 'r') as f:
        return json.load(f)


def get_arguments():
    return (get_params('./params/train_params.json'),
            get_params('./params/wavenet_params.json'),
            get_params('./params/dataset_params.json'))


def _flat_layout(opt, model, plain_group):
    """(engine, params, flat gradient base pointer) when `opt` can take its step as ONE launch on the engine's flat buffers: one
    parameter group holding exactly the module's parameters in order, every parameter a view of the flat parameter buffer, every
    gradient a contiguous fp32 view of ONE flat gradient buffer at the same offsets (what the module's backward hands autograd),
    and `plain_group(group)` true (no option the kernel does not implement).  None otherwise: torch's own step runs."""
    eng = getattr(model, "_engine", None)
    if eng is None or getattr(eng, "flat", None) is None or len(opt.param_groups) != 1:
        return None
    grp = opt.param_groups[0]
    if not plain_group(grp):
        return None
    params = grp["params"]
    named = [p for _, p in model.named_parameters()]
    if len(params) != len(named) or any(a is not b for a, b in zip(params, named)):
        return None
    base = eng.flat.data_ptr()
    if any(p.data_ptr() != base + 4 * eng.spec.off[n] for n, p in zip(eng.param_names, params)):
        return None                                       # (the module was moved: its parameters left the flat buffer)
    g0 = params[0].grad
    if g0 is None or g0.dtype != torch.float32:
        return None
    gbase = g0.data_ptr() - 4 * eng.spec.off[eng.param_names[0]]
    if not all(p.grad is not None and p.grad.is_contiguous() and p.grad.data_ptr() == gbase + 4 * eng.spec.off[n]
               for n, p in zip(eng.param_names, params)):
        return None
    return eng, params, gbase


def _flat_views(opt, eng, params, key, cache, validate=True):
    """One flat buffer for the per-parameter state tensors `key`, the state entries being VIEWS of it (so `state_dict()` /
    `load_state_dict()` interchange with torch's optimizer).  Existing per-parameter tensors (a loaded state_dict, earlier torch
    steps) are adopted.  Returns (flat buffer, how many parameters had the entry before).  The cached buffer is for this engine and
    dropped by load_state_dict(); `validate`: it is also checked against the state entries, every step."""
    hit = cache.get(key)
    if hit is not None and hit[0] is eng and (not validate or all(opt.state[p].get(key) is v for p, v in zip(params, hit[2]))):
        return hit[1], len(params)
    flat = torch.zeros_like(eng.flat)
    had, views = 0, []
    for n, p in zip(eng.param_names, params):
        o, k = eng.spec.off[n], p.numel()
        st = opt.state[p]
        old = st.get(key)
        view = flat[o:o + k].view(p.shape)
        if old is not None:
            view.copy_(old)
            had += 1
        st[key] = view
        views.append(view)
    cache[key] = (eng, flat, views)
    return flat, had


def _step_counters(opt, params, cache, uniform=False, validate=True):
    """torch's `step` counters (a 0-d fp32 CPU tensor per parameter, made where there is none), bumped in one call on the plain
    path; under the guard they follow the device's count instead (GuardedOptimizer.state_dict()).  With `uniform`, counters that
    differ between the parameters give None: looked at where they are readied, and nothing is cached then, so the next step looks
    again (every change after that - a bump, torch's own step, the guard's count - is the same for all parameters)."""
    steps = cache.get("step")
    if steps is None or (validate and any(opt.state[p].get("step") is not t for p, t in zip(params, steps))):
        steps = []
        for p in params:
            st = opt.state[p]
            step = st.get("step")
            st["step"] = (torch.zeros((), dtype=torch.float32) if step is None else
                          torch.as_tensor(step, dtype=torch.float32).detach().cpu().reshape(()).clone())
            steps.append(st["step"])
        if uniform and any(float(t) != float(steps[0]) for t in steps):
            cache.pop("step", None)
            return None
        cache["step"] = steps
    return steps


class FlatOptimizer(guard.GuardedOptimizer):
    """Mixin in front of a torch optimizer class whose ``step()`` is ONE launch on the module's flat buffers when it can be.

    The module's parameters are views of one flat buffer (music_amd/engine.py) and the gradients autograd hands to them are views
    of one flat buffer too (``_WaveNetFunction.backward``), so the 123 per-tensor updates of the reference's optimizers
    (wavenet/train.py:28-42) are one elementwise pass.  The optimizer state is torch's own, its tensors being VIEWS of flat buffers:
    ``state_dict()`` / ``load_state_dict()`` interchange with torch's class, and any step the fast path does not cover (parameters
    not on the flat buffer yet, gradients that are not one flat tensor, an option the kernel does not implement, closures, several
    parameter groups) falls through to torch's own step on the same state.  A class gives `_covers(group)`, whether the kernel
    implements the group's options, and `_flat_args(eng, params, group)`, which readies the flat state and returns (entry point,
    state pointers, the plain and the guarded argument tail, the step counters the plain path bumps) or None for torch's path."""

    def __init__(self, model, *, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, **kw):
        super().__init__(model.parameters(), **kw)
        self._model, self._cache = model, {}     # _cache: the flat state buffers of _flat_views / _step_counters
        self._guard_setup(max_grad_norm, skip_nonfinite)
        self._ema_setup(model.named_parameters(), ema_decay, ema_warmup)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._cache = {}                                  # re-adopt the loaded tensors at the next step
        self._guard_reseed()

    @torch.no_grad()
    def step(self, closure=None):
        if self.ema is not None:
            self.ema.check_step()
        lay = _flat_layout(self, self._model, self._covers) if closure is None else None
        args = None if lay is None else self._flat_args(lay[0], lay[1], self.param_groups[0])
        if args is None:
            return self._torch_step(closure, checked=True)
        eng, _, gbase = lay
        entry, state, plain, guarded, steps = args
        gd = None if self._guard_opts is None else self._guard_get(eng.flat.device)
        if gd is None and steps:
            torch._foreach_add_(steps, 1.0)
        guard.flat_step(eng, entry, gbase, state, plain, guarded, gd, self.ema)
        return None


class FlatAdam(FlatOptimizer, optim.Adam):
    """``torch.optim.Adam(model.parameters(), lr)`` (wavenet/train.py:39-42) as ONE ``wn_adam_flat`` launch (see FlatOptimizer):
    torch's own state - per parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``; weight decay / amsgrad / maximize, and parameters at
    different step counts, fall through to torch."""

    @staticmethod
    def _covers(g):
        return not (g.get("weight_decay", 0) != 0 or g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"))

    def _flat_args(self, eng, params, grp):
        # the caches as they are until load_state_dict() or another engine, not checked against the state entries per step: on the
        # reference's own loop, where this optimizer sits, the three checks (0.04 ms of host time) showed
        m, _ = _flat_views(self, eng, params, "exp_avg", self._cache, validate=False)
        v, _ = _flat_views(self, eng, params, "exp_avg_sq", self._cache, validate=False)
        steps = _step_counters(self, params, self._cache, uniform=True, validate=False)
        if steps is None:
            return None                                   # parameters at different step counts: torch's per-tensor path
        t = float(steps[0])
        b1, b2 = grp["betas"]
        hyper = (float(grp["lr"]), b1, b2, grp["eps"])
        return ("wn_adam_flat", (m.data_ptr(), v.data_ptr()), hyper + (1.0 - b1 ** (t + 1.0), 1.0 - b2 ** (t + 1.0), 1.0), hyper + (1.0,), steps)


class FlatSGD(FlatOptimizer, optim.SGD):
    """``torch.optim.SGD(model.parameters(), lr, momentum)`` (wavenet/train.py:28-31) as ONE ``wn_sgd_flat`` launch (see
    FlatOptimizer): ``momentum_buffer`` per parameter; dampening, Nesterov, weight decay, maximize, and parameters with and without
    a momentum buffer mixed, fall through to torch."""

    @staticmethod
    def _covers(g):
        return (g.get("dampening", 0) == 0 and not g.get("nesterov") and g.get("weight_decay", 0) == 0 and not g.get("maximize")
                and not g.get("differentiable"))

    def _guard_seed(self):
        # torch's SGD keeps no step counter: existing momentum buffers mean "not the first step" (one step the guard did not see)
        have = any(st.get("momentum_buffer") is not None for st in self.state.values())
        return (1, 1) if have else (0, 0)

    def _flat_args(self, eng, params, grp):
        mom = float(grp["momentum"])
        buf, first = None, 0
        if mom != 0.0:
            have = sum(1 for p in params if self.state[p].get("momentum_buffer") is not None)
            if have not in (0, len(params)):
                return None
            buf = _flat_views(self, eng, params, "momentum_buffer", self._cache)[0].data_ptr()
            first = 1 if have == 0 else 0
        tail = (float(grp["lr"]), mom, 1.0)
        return "wn_sgd_flat", (buf,), tail + (first,), tail, None     # guarded, "first step" is the device's: the first step TAKEN


class FlatRMSprop(FlatOptimizer, optim.RMSprop):
    """``torch.optim.RMSprop(model.parameters(), lr, momentum=momentum)`` (wavenet/train.py:32-37) as ONE ``wn_rmsprop_flat`` launch
    (see FlatOptimizer): ``step``, ``square_avg``, ``momentum_buffer``; centered / weight decay / maximize fall through to torch."""

    @staticmethod
    def _covers(g):
        return (not g.get("centered") and g.get("weight_decay", 0) == 0 and not g.get("maximize") and not g.get("capturable")
                and not g.get("differentiable"))

    def _flat_args(self, eng, params, grp):
        mom = float(grp["momentum"])
        sq, _ = _flat_views(self, eng, params, "square_avg", self._cache)
        buf = _flat_views(self, eng, params, "momentum_buffer", self._cache)[0].data_ptr() if mom > 0.0 else None
        tail = (float(grp["lr"]), float(grp["alpha"]), float(grp["eps"]), mom, 1.0)
        return "wn_rmsprop_flat", (sq.data_ptr(), buf), tail, tail, _step_counters(self, params, self._cache)


def get_optimizer(model, optimizer_type, learning_rate, momentum, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                  ema_warmup=False):
    """wavenet/train.py:28-42 — 'sgd' / 'rmsprop' (with momentum) / 'adam'; anything else -> None.  Each is torch's own optimizer class
    (same hyper-parameters, same state_dict) whose step() is one launch on the module's flat buffers when it can be.  max_grad_norm / skip_nonfinite: the guarded
    step (music_amd/guard.py) - that launch becomes wn_grad_guard + the guarded update.  ema_decay / ema_warmup: `opt.ema`, the EMA
    shadow of the parameters (music_amd/ema.py; None when unset) - every step ends with its one wn_ema_flat launch; the shadow is
    not part of state_dict()."""
    kw = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup)
    if optimizer_type == 'sgd':
        return FlatSGD(model, lr=learning_rate, momentum=momentum, **kw)
    if optimizer_type == 'rmsprop':
        return FlatRMSprop(model, lr=learning_rate, momentum=momentum, **kw)
    if optimizer_type == 'adam':
        return FlatAdam(model, lr=learning_rate, **kw)          # an optim.Adam (same state_dict); one launch per step on the flat buffers


def save_model(model, num_iter, path):
    """``restore_dir + "wavenet{N}.model"`` = bare state_dict pickle (wavenet/train.py:45-50)."""
    checkpoint_path = path + "wavenet" + str(num_iter) + ".model"
    print("Storing checkpoint to {} ...".format(path))
    state = OrderedDict((k, v.detach().cpu().clone()) for k, v in model.state_dict().items())
    torch.save(state, checkpoint_path)
    print("Done!")


def load_model(model, path, model_name):
    """Returns the model, or None when the file does not exist (wavenet/train.py:53-73).  Keys
    saved from a DataParallel wrapper ("module." prefix) are accepted."""
    checkpoint_path = path + model_name
    print("Trying to restore saved checkpoint from ", "{}".format(checkpoint_path))
    if not os.path.exists(checkpoint_path):
        print("No checkpoint found!")
        return None
    print("Checkpoint found, restoring!")
    state_dict = torch.load(checkpoint_path, map_location="cpu")
    if list(state_dict.keys())[0][:6] == 'module':
        state_dict = OrderedDict((k[7:], v) for k, v in state_dict.items())
    model.load_state_dict(state_dict)
    return model


def _rotate_checkpoints(restore_dir, max_check_points):
    """Delete the numerically oldest wavenet{N}.model once max_check_points exist (:198-213)."""
    stored = glob.glob(restore_dir + "*.model")
    if len(stored) == max_check_points:
        def number(p):
            return int(p.split('/')[-1].split('.')[0][7:])
        stored = sorted(stored, key=cmp_to_key(lambda a, b: number(a) - number(b)))
        os.remove(stored[0])
        for suffix in (".opt", ".ema"):                               # its optimizer state and EMA shadow, if they were written
            if os.path.exists(stored[0][:-len(".model")] + suffix):
                os.remove(stored[0][:-len(".model")] + suffix)


def _optimizer_state(optimizer, engine):
    """What wavenet{N}.opt holds: the torch optimizer's state_dict, or the flat Adam buffers of the fused step."""
    if engine is not None and engine.adam_state is not None:
        engine.guard_report()                             # guarded: "t" = the steps the device took
        st = engine.adam_state
        return {"kind": "fused_adam", "m": st["m"].detach().cpu().clone(), "v": st["v"].detach().cpu().clone(), "t": int(st["t"])}
    return {"kind": "torch", "state": optimizer.state_dict()}


def _restore_optimizer_state(path, optimizer, engine_factory):
    """Load wavenet{N}.opt if it exists.  Returns the engine if the fused Adam state was restored."""
    if not os.path.exists(path):
        return None
    blob = torch.load(path, map_location="cpu")
    if blob.get("kind") == "fused_adam":
        engine = engine_factory()
        if engine is None:
            return None
        engine.adam_state["m"].copy_(blob["m"])
        engine.adam_state["v"].copy_(blob["v"])
        engine.adam_state["t"] = int(blob["t"])
        if engine.adam_state.get("guard") is not None:
            engine.adam_state["guard"].seed_taken(int(blob["t"]))
        return engine
    if blob.get("kind") == "torch" and optimizer is not None:
        optimizer.load_state_dict(blob["state"])
    return None


def _saved_ema_updates(path):
    """"ema_updates" of wavenet{N}.opt: the count of EMA updates at that checkpoint, or None (no file, or one without a shadow)."""
    if not os.path.exists(path):
        return None
    return torch.load(path, map_location="cpu").get("ema_updates")


def _resume_counter(log_dir):
    """Batches trained so far = third word of the last loss_log line (:160-166)."""
    with open(log_dir + 'loss_log.log', 'r') as f:
        lines = f.readlines()
    return int(lines[-1].split(' ')[2]) if lines else 0


def train():
    cuda_available = torch.cuda.is_available()
    train_params, wavenet_params, dataset_params = get_arguments()
    rank, world, local_rank = wdist.init_from_env()
    # every rank must draw the same shuffling permutation (each slices its chunk of the global batch): the JSON
    # "seed" if there is one, else one drawn on rank 0 and broadcast
    if world > 1:
        wdist.shared_seed(train_params.get("seed"))
    elif train_params.get("seed") is not None:
        torch.manual_seed(int(train_params["seed"]))

    net = wavenet(**wavenet_params)
    epoch_trained = 0
    restored_from = None
    if train_params["restore_model"]:
        net = load_model(net, train_params["restore_dir"], train_params["restore_model"])
        if net is None:
            print("Initialize network and train from scratch.")
            net = wavenet(**wavenet_params)
        else:
            epoch_trained = int(train_params["restore_model"].split('.')[0][7:])
            restored_from = train_params["restore_dir"] + train_params["restore_model"]

    if cuda_available is False and train_params["device_ids"] is not None:
        raise ValueError("Cuda is not avalable,", " can not train model using multi-gpu.")
    # optional keys: "objective": "nll" trains the negative log-likelihood under the per-timestep softmax instead of the reference's
    # loss; "valid_audio_path" + "validate_every" (steps) score held-out audio on rank 0 into valid_log.log (music_amd/objective.py)
    # "nll_windows" ({"stages": S, "codes": K} or [lo, hi] pairs; with "token_positions": true in dataset_params.json): the position
    # windows of the samplers applied to that objective - a prior over a residual quantiser's token stream trains on what it samples
    objective = wobjective.objective_option(train_params)
    nll_windows = wobjective.nll_windows_option(train_params, dataset_params, wavenet_params.get("quantization_channels"))
    # "ignore_token", "label_smoothing", "nll_stage_weights": the masked, weighted and smoothed "nll" (objective.wnll_option) - targets of
    # the ignored value (a dropped stage's -1, padding) are skipped, the loss is the weighted mean over the rest.  Under data
    # parallelism every rank normalises by its own sum of weights and the ranks are averaged as before: no collective is added
    wnll = wobjective.wnll_option(train_params, dataset_params)
    # "global_classes" / "global_channels" in the model's JSON: a class-conditional WaveNet.  The clips' classes come from
    # dataset_params.json's "labels_path" (a JSON list of integers, one per item of the audio pickle; "valid_labels_path" in
    # train_params.json for the held-out set) - as in music_amd/ae_train.py: the mode without labels is refused, labels without it too
    n_global = getattr(net, "global_classes", 0)
    if n_global and not dataset_params.get("labels_path"):
        raise ValueError('the model\'s parameters set "global_classes": %d, so dataset_params.json must name the clips\' classes with '
                         '"labels_path" (a JSON list of integers, one per item of the audio pickle)' % n_global)
    if dataset_params.get("labels_path"):
        if not n_global:
            raise ValueError('dataset_params.json has "labels_path" but the model\'s parameters leave "global_classes" at 0: nothing '
                             'would read the labels')
        dataset_params = dict(dataset_params, n_classes=n_global)         # a label outside [0, global_classes) raises at load
        if train_params.get("valid_audio_path") and int(train_params.get("validate_every") or 0) > 0 \
                and not train_params.get("valid_labels_path"):
            raise ValueError('train_params.json: validating a model with "global_classes" needs "valid_labels_path", the classes of the '
                             'items of "valid_audio_path"')
    # "phase_period": P in the model's JSON: a phase-conditioned WaveNet, a prior over a frame-major code stream of P stages.  Every
    # clip's stream position comes from the loader's "audio_pos", so the dataset must hand the positions out - refused here, at start,
    # the way "nll_windows" without them is
    phase_period = getattr(net, "phase_period", 0)
    if phase_period and not dataset_params.get("token_positions"):
        raise ValueError('the model\'s parameters set "phase_period": %d, which needs "token_positions": true in dataset_params.json (the '
                         'stream position of every clip)' % phase_period)
    # "null_class" in the model's JSON + "class_dropout": p (and "class_dropout_seed") here: classifier-free guidance training - each
    # step a clip's class becomes null_class with probability p (music_amd/class_dropout.py: a counter hash of the global step and the
    # clip's index in the global batch).  No clip may carry null_class as its label; validation scores the true labels.
    null_class = getattr(net, "null_class", None)
    class_drop = class_dropout.options(train_params, null_class)
    if null_class is not None:
        for key, path in (("labels_path", dataset_params.get("labels_path")), ("valid_labels_path", train_params.get("valid_labels_path"))):
            if path:
                with open(path) as f:
                    labels = json.load(f)
                if isinstance(labels, list) and null_class in labels:
                    raise ValueError('%s %s: item %d carries the label %d, the model\'s "null_class" (the class that stands for "no '
                                     'class" cannot be a clip\'s own)' % (key, path, labels.index(null_class), null_class))
    validation = wobjective.Validation.make(train_params, dataset_params) if rank == 0 else None
    if world > 1:
        # DataParallel semantics: the JSON batch_size is the GLOBAL batch, split evenly
        assert dataset_params["batch_size"] % world == 0
        dataset_params = dict(dataset_params, shard=(rank, world))
    dataloader = audio_data_loader(**dataset_params)
    if cuda_available:
        net = net.cuda()
    wdist.broadcast_parameters(list(net.parameters()))

    print("Start training.")
    print("Writing logging information to ", "{}".format(train_params["log_dir"]))
    print("Models are saved in {}".format(train_params["restore_dir"]))

    max_gn, skip_nf = guard.guard_options(train_params)
    guarded = guard.enabled(max_gn, skip_nf)
    ema_decay, ema_warmup = ema.ema_options(train_params)
    fused = bool(train_params.get("fused_step")) and train_params["optimizer"] == 'adam' and cuda_available
    optimizer = get_optimizer(net, train_params["optimizer"], train_params["learning_rate"],
                              train_params["momentum"], max_grad_norm=max_gn, skip_nonfinite=skip_nf,
                              ema_decay=None if fused else ema_decay, ema_warmup=ema_warmup)     # (fused: the engine keeps the shadow)
    loss_func = nn.CrossEntropyLoss()
    if cuda_available:
        loss_func = loss_func.cuda()
    is_writer = rank == 0
    loss_log_file = store_log_file = None
    if is_writer:
        os.makedirs(train_params["log_dir"], exist_ok=True)
        os.makedirs(train_params["restore_dir"], exist_ok=True)
        loss_log_file = open(train_params["log_dir"] + 'loss_log.log', 'a')
        store_log_file = open(train_params["log_dir"] + 'store_log.log', 'a')
    if world > 1:
        torch.distributed.barrier()
    num_trained = _resume_counter(train_params["log_dir"])

    device = next(net.parameters()).device
    total_loss = torch.zeros((), dtype=torch.float64, device=device)     # summed without host syncs
    engine = None
    keep_opt = bool(train_params.get("save_optimizer_state"))

    def _fused_engine():
        if not fused:
            return None
        e = net._engine_for(device)
        e.objective = objective
        e.adam_init(lr=train_params["learning_rate"], max_grad_norm=max_gn, skip_nonfinite=skip_nf, ema_decay=ema_decay,
                    ema_warmup=ema_warmup)
        return e

    def _shadow():
        """(the EMA shadow of this run or None, the GradGuard its updates follow or None)"""
        if fused:
            return (None, None) if engine is None else (engine.ema, engine.adam_state.get("guard"))
        return (None, None) if optimizer is None else (optimizer.ema, optimizer._guard)
    if keep_opt and restored_from is not None:
        engine = _restore_optimizer_state(restored_from[:-len(".model")] + ".opt", optimizer, _fused_engine)
    if ema_decay is not None and restored_from is not None:
        if fused and engine is None:
            engine = _fused_engine()
        ema.restore_shadow(_shadow()[0], restored_from[:-len(".model")] + ".ema",
                           _saved_ema_updates(restored_from[:-len(".model")] + ".opt") if keep_opt else None, _shadow()[1])
    guard_log = None
    if guarded and is_writer:
        guard_log = guard.GuardLog(
            train_params["log_dir"] + 'guard_log.log',
            lambda: (engine.guard_report() if engine is not None else None) if fused else optimizer.guard_report(),
            lambda: guard.engine_named_grads(engine) if fused else [(n, p.grad) for n, p in net.named_parameters()])
    for epoch in range(train_params["num_epochs"]):
        for i_batch, sampled_batch in enumerate(dataloader):
            piece = sampled_batch["audio_piece"]
            target = sampled_batch["audio_target"]
            # ragged last batch under data parallelism: weight of this rank's shard (0 and piece None = no items)
            dp_scale = float(sampled_batch.get("dp_scale", 1.0))
            if piece is not None:
                if cuda_available:
                    piece = piece.cuda(non_blocking=True)
                    target = target.cuda(non_blocking=True)
                target = target.view(-1)
            win_kw = {} if nll_windows is None else {"windows": nll_windows, "window_pos": sampled_batch.get("audio_pos")}     # (absent on an empty shard)
            cls_kw = {"classes": sampled_batch["audio_class"]} if n_global and "audio_class" in sampled_batch else {}
            if wnll is not None and piece is not None:
                cls_kw.update(wobjective.wnll_kwargs(wnll, sampled_batch, target.numel() // piece.shape[0], device))
            if phase_period and piece is not None:        # (a phase-conditioned prior: the clips' stream positions)
                cls_kw["phase_pos"] = sampled_batch["audio_pos"]
            if class_drop is not None and "classes" in cls_kw:
                cls_kw["classes"] = class_dropout.apply(cls_kw["classes"], null_class, class_drop[1], num_trained,
                                                        int(sampled_batch.get("first_clip", 0)), class_drop[0])
            loss = torch.zeros((), device=device)
            if fused:
                if engine is None:
                    engine = _fused_engine()
                if piece is not None:
                    loss = engine.loss_and_grad(piece.contiguous(), target, **win_kw, **cls_kw)
                else:
                    engine.flat_grad.zero_()
                if guarded:                               # the sum alone; 1 / world rides in the guard's and the update's gscale
                    wdist.allreduce_flat_(engine.flat_grad, average=False, scale=dp_scale)
                    engine.adam_step(gscale=1.0 / world)
                else:
                    wdist.allreduce_flat_(engine.flat_grad, average=True, scale=dp_scale)
                    engine.adam_step()
            else:
                optimizer.zero_grad()
                if piece is not None and objective == "nll":
                    loss = wobjective.nll_loss(net, piece, target, **win_kw, **cls_kw)
                    loss.backward()
                elif piece is not None:
                    logits = net(piece, **cls_kw)  # probabilities, named as in the reference (Q1)
                    loss = loss_func(logits, target)
                    loss.backward()
                wdist.allreduce_gradients(net.parameters(), average=True, scale=dp_scale)
                optimizer.step()
            loss = loss.detach() * dp_scale
            total_loss += loss.detach().double()
            num_trained += 1
            if num_trained % train_params["print_every"] == 0:
                if world > 1:
                    torch.distributed.all_reduce(total_loss)
                    total_loss /= world
                avg_loss = total_loss.item() / train_params["print_every"]
                if is_writer:
                    loss_log_file.writelines("Trained over " + str(num_trained) + " pieces," +
                                             "Average loss is " + str(avg_loss) + "\n")
                    loss_log_file.flush()
                if guard_log is not None:
                    guard_log.tick(num_trained)
                total_loss.zero_()
            if validation is not None:
                validation.tick(net, num_trained, _shadow()[0])

        if (epoch + 1) % train_params["check_point_every"] == 0 and is_writer:
            _rotate_checkpoints(train_params["restore_dir"], train_params["max_check_points"])
            save_model(net, epoch_trained + epoch + 1, train_params["restore_dir"])
            shadow, shadow_guard = _shadow()
            if shadow is not None:
                ema.save_shadow(shadow, train_params["restore_dir"] + "wavenet" + str(epoch_trained + epoch + 1) + ".ema")
            if keep_opt:
                blob = _optimizer_state(optimizer, engine)
                if shadow is not None:
                    blob["ema_updates"] = shadow.updates(shadow_guard)
                torch.save(blob, train_params["restore_dir"] + "wavenet" + str(epoch_trained + epoch + 1) + ".opt")
            store_log_file.writelines("Epoch " + str(epoch_trained + epoch + 1) + ", model saved!\n")
            store_log_file.flush()
    if is_writer:
        loss_log_file.close()
        store_log_file.close()


if __name__ == '__main__':
    train()
