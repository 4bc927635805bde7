"""Counterpart of the reference's ``wavenet_autoencoder/train.py`` (training harness of the
autoencoder) for the MI355X path.

The reference file is a tab-indented copy of ``wavenet/train.py`` that cannot run as shipped: it
imports ``faster_audio_data`` and reads ``./params/train_params.json`` / ``dataset_params.json`` that
only exist in ``wavenet/``, its ``model_params.json`` is invalid JSON, ``optim.sgd`` is a
typo (:28), ``sorted(keys=...)`` raises (:159) and ``int(name[7:])`` raises for its own checkpoint
names (:77-78).  This module keeps its surface and file formats - the reference's own line formats
``"Average loss is X\\n"`` (:144-146) and ``"Epoch{N}model saved!"`` (:164-166, no separators), checkpoints
``wavenet_autoencoder{N}.model`` - and fixes only what cannot work (the resume counter, which the reference parses out
of a loss line that does not contain it (:110-116: ``int("is")``), is the number of logged lines x print_every):

    get_optimizer(model, optimizer_type in {'sgd','RMSprop','Adam','lbfgs'}, learning_rate, momentum1)
    save_model(model, num_epoch, path)   -> path + "wavenet_autoencoder{N}.model"
    load_model(model, path, model_name)
    train()      reads ./params/train_params.json, ./params/model_params.json, ./params/dataset_params.json

Optional key in train_params.json (as in music_amd/train.py): ``"fused_step"`` (bool, Adam only) - the whole step runs
as forward + one softmax/CE/backward kernel + backward + flat Adam on the engine, without autograd.  ``"max_grad_norm"``
(float) and ``"skip_nonfinite"`` (bool): global-norm clipping of the gradient and the skipping of a non-finite step
(music_amd/guard.py; on the device for the fused step), with a line per ``print_every`` in ``guard_log.log``.  ``"ema_decay"``
(float) and ``"ema_warmup"`` (bool): the EMA shadow of the parameters (music_amd/ema.py; on the device for the fused step),
written as ``wavenet_autoencoder{N}.ema`` next to every checkpoint in the checkpoint's own format and read back when that
checkpoint is restored.

Optional key in model_params.json: ``"conditioning"`` (``"random"``, the default and the reference's behaviour: the decoder's N + 1
conditioning projections are drawn afresh in every forward; ``"learned"``: they are parameters of the model, trained, saved and
restored with it - music_amd/model1.py).  A checkpoint only loads into a model built with the mode it was saved with.
``"bottleneck"`` (``"continuous"``, the default; ``"vq"``: every pooled frame is replaced by its nearest row of a learned codebook,
VQ-VAE - needs ``"conditioning": "learned"``), ``"vq_codes"`` (codebook rows, 2 .. 1024, default 512) and ``"vq_beta"`` (weight of the
commitment term, default 0.25).  With it the loss of every step is the reconstruction loss plus ``vq_loss``, one line per
``print_every`` goes to ``vq_log.log`` (mse, perplexity of the code usage, codes used), and the optional train_params.json key
``"vq_init"`` (``"uniform"``, the default, or ``"data"``) initialises the codebook from the first batch's pre-quantisation
encoding (``net.init_codebook``) when training starts from scratch.
``"vq_update"`` (``"gradient"``, the default: the codebook is trained by its loss term; ``"ema"``: every row follows the
exponential moving average of the frames assigned to it, van den Oord et al. 2017 appendix A.1 - no learning rate, no optimizer
state, ``vq_loss`` is the commitment term alone), with ``"vq_decay"`` (in (0, 1), default 0.99), ``"vq_eps"`` (smoothing of the
usage, default 1e-5) and ``"vq_restart"`` (default 0 = off: a code whose running usage falls below it restarts from the batch mean
of one of the most used codes' frames).  The update runs on the device behind every optimizer step (a step the guard skips leaves it
alone); under data parallelism the per-code counts and sums are summed over the ranks first, so every replica makes the same update.
The ``vq_log.log`` line then ends with ``, restarted N``, the codes restarted since the line before.  A checkpoint carries the running
state (``vq_ema_state``) and only loads into a model built with the same ``"vq_update"``.
``"vq_stages"`` (1 .. 8, default 1; needs ``"bottleneck": "vq"``): residual vector quantisation - S codebooks of ``"vq_codes"`` rows,
stage s quantises what the stages before it left over and the decoder sees the sum of the S rows (S log2 K bits per frame; a prefix
of the stages is a coarser code).  ``vq_loss`` sums the stages' terms, every stage keeps its own EMA state and restarts, ``"vq_init":
"data"`` fills the stages in order from the residuals, the ``vq_log.log`` line reports the last stage's mse (q against e) and ends with
the per-stage figures, ``restarted`` sums the stages; a checkpoint only loads into a model of the same stage count.
``"vq_stage_dropout"`` (p in [0, 1], default 0 = off; needs ``"vq_stages"`` > 1): quantiser dropout (SoundStream, EnCodec, DAC) - in
every step a share p of the clips draws its own stage count n uniformly from 1 .. S and is quantised, scored and counted with its
first n stages only, the others use all S (p = 1 is SoundStream's rule, p = 0.5 DAC's): one model then serves every bitrate n log2 K,
and ``decode_codes`` of a prefix of the stages runs through tables that were trained on it.  The draw is a counter hash of the
optional train_params.json key ``"vq_dropout_seed"`` (default 0), the global step and the clip's index in the GLOBAL batch
(music_amd/vq_dropout.py): no RNG state, a resumed run and any data-parallel layout draw the same n for the same clip.  It adds no
parameter and no buffer, checkpoints load both ways.  ``"vq_init": "data"`` fills the stages from all-active residuals, as without it.
Only with p > 0 the ``vq_log.log`` line ends with ``, active f0/f1/..``, the frames that took part in each stage.  Later stages see
fewer frames (stage s a share 1 - p s / S), so with ``"vq_update": "ema"`` a ``"vq_restart"`` threshold bites them sooner.
``"global_classes"`` and ``"global_channels"`` (both 0, the default: off; both >= 1 together, ``"conditioning": "learned"`` required):
global class conditioning of the decoder - every clip has a class (speaker, instrument) whose learned embedding is projected into
every conditioning table (music_amd/model1.py).  The classes come from the optional dataset_params.json key ``"labels_path"``, a
JSON list of integers in [0, global_classes), one per item of the audio pickle (``"valid_labels_path"`` in train_params.json for the
held-out set); a model with the mode on and no ``"labels_path"`` is refused at start, as are labels without the mode.  A checkpoint
only loads into a model built with the same two values.
"""
import glob
import os

import torch
import torch.nn as nn
import torch.optim as optim

try:
    from . import dist as wdist
    from . import ema
    from . import guard
    from . import objective as wobjective
    from .faster_audio_data import audio_data_loader
    from .model1 import wavenet_autoencoder
    from .train import FlatOptimizer, get_params, load_model
except ImportError:
    from music_amd import dist as wdist
    from music_amd import ema
    from music_amd import guard
    from music_amd import objective as wobjective
    from music_amd.faster_audio_data import audio_data_loader
    from music_amd.model1 import wavenet_autoencoder
    from music_amd.train import FlatOptimizer, get_params, load_model

PREFIX = "wavenet_autoencoder"


def vq_stage_fields(stats):
    """The tail of a vq_log.log line with "vq_stages" > 1: every stage's mse, perplexity and codes used, behind the fields of stage 1."""
    fmt = lambda v: "[" + ", ".join("%.6g" % x for x in v.tolist()) + "]"
    return ", stage mse %s, stage perplexity %s, stage codes used %s" % (
        fmt(stats.stage_mse), fmt(stats.stage_perplexity), [int(v) for v in stats.stage_codes_used.tolist()])


def get_arguments():
    return (get_params('./params/train_params.json'), get_params('./params/model_params.json'),
            get_params('./params/dataset_params.json'))


def _host_guarded(cls):
    """`cls` (a torch optimizer class) with the guard's rule applied on the host before every step (music_amd/guard.py): the step of
    this harness is torch's own per-tensor path, where a read-back per step is already the rule.  With `ema` (ema_decay set) every
    step ends with the shadow's update (music_amd/ema.py), guarded or not."""
    class Guarded(FlatOptimizer, cls):                    # its constructor and load_state_dict; the step stays torch's
        def step(self, closure=None):
            return self._torch_step(closure)
    Guarded.__name__ = Guarded.__qualname__ = "Guarded" + cls.__name__
    return Guarded


def get_optimizer(model, optimizer_type, learning_rate, momentum1=False, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                  ema_warmup=False):
    """wavenet_autoencoder/train.py:26-34 (with ``optim.sgd`` spelled ``optim.SGD``).  max_grad_norm / skip_nonfinite: the same
    optimizer with its gradient clipped to that global norm / a non-finite step not applied; ema_decay / ema_warmup: with `ema`,
    the EMA shadow of the parameters, updated behind every step (neither for 'lbfgs', whose closure is evaluated many times per
    step).  All unset: torch's own class."""
    if guard.enabled(max_grad_norm, skip_nonfinite) or ema_decay is not None:
        kw = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup, lr=learning_rate)
        if optimizer_type == 'sgd':
            return _host_guarded(optim.SGD)(model, momentum=momentum1 or 0, **kw)
        if optimizer_type == 'RMSprop':
            return _host_guarded(optim.RMSprop)(model, momentum=momentum1 or 0, **kw)
        if optimizer_type == 'Adam':
            return _host_guarded(optim.Adam)(model, **kw)
        if optimizer_type == 'lbfgs':
            raise ValueError("max_grad_norm / skip_nonfinite / ema_decay do not apply to the 'lbfgs' optimizer")
        return None
    if optimizer_type == 'sgd':
        return optim.SGD(model.parameters(), lr=learning_rate, momentum=momentum1 or 0)
    if optimizer_type == 'RMSprop':
        return optim.RMSprop(model.parameters(), lr=learning_rate, momentum=momentum1 or 0)
    if optimizer_type == 'Adam':
        return optim.Adam(model.parameters(), lr=learning_rate)
    if optimizer_type == 'lbfgs':
        return optim.LBFGS(model.parameters(), lr=learning_rate)


def save_model(model, num_epoch, path):
    checkpoint_path = path + PREFIX + str(num_epoch) + '.model'
    print('Storing checkpoint to {}...'.format(path))
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, checkpoint_path)
    print('done')


def _resume_counter(log_dir, print_every):
    """Batches trained so far.  The reference reads word 2 of the last loss line (:110-116), but its own lines are
    "Average loss is X" (word 2 = "is"), so a second run on the same log directory dies there; one line is written
    every print_every batches, so the count is recovered from the number of lines (a line in the wavenet/train.py
    format "Trained over N pieces,..." - written by round-1 versions of this module - is honoured too)."""
    try:
        with open(log_dir + 'loss_log.log', 'r') as f:
            lines = [l for l in f.readlines() if l.strip()]
    except FileNotFoundError:
        return 0
    if not lines:
        return 0
    if lines[-1].startswith("Trained over "):
        return int(lines[-1].split(' ')[2])
    return len(lines) * print_every


def _epoch_of(name):
    return int(os.path.basename(name).split('.')[0][len(PREFIX):])


def _rotate_checkpoints(stored, max_check_points):
    """Delete the numerically oldest of the `stored` .model files once max_check_points exist, and its .ema with it."""
    if len(stored) == max_check_points:
        oldest = sorted(stored, key=_epoch_of)[0]
        os.remove(oldest)
        if os.path.exists(oldest[:-len(".model")] + ".ema"):
            os.remove(oldest[:-len(".model")] + ".ema")


def train():
    cuda_available = torch.cuda.is_available()
    train_params, model_params, dataset_params = get_arguments()
    rank, world, _ = wdist.init_from_env()
    if world > 1:
        train_params = dict(train_params, seed=wdist.shared_seed(train_params.get("seed")))
    elif train_params.get("seed") is not None:
        torch.manual_seed(int(train_params["seed"]))
    net = wavenet_autoencoder(**model_params)
    epoch_trained = 0
    restored_from = None
    if train_params["restore_model"]:
        restored = load_model(net, train_params["restore_dir"], train_params["restore_model"])
        if restored is None:
            print("Initialize network and train from scratch.")
        else:
            epoch_trained = _epoch_of(train_params["restore_model"])
            restored_from = train_params["restore_dir"] + train_params["restore_model"]
    if cuda_available is False and train_params["device_ids"] is not None:
        raise ValueError("Cuda is not avalable,", " can not train model using multi-gpu.")
    # optional keys "objective", "valid_audio_path", "validate_every": as in music_amd/train.py (music_amd/objective.py)
    objective = wobjective.objective_option(train_params)
    wnll = wobjective.wnll_option(train_params, dataset_params)       # "ignore_token", "label_smoothing", "nll_stage_weights": likewise
    n_global = getattr(net, "global_classes", 0)
    if n_global and not dataset_params.get("labels_path"):
        raise ValueError('model_params.json sets "global_classes": %d, so dataset_params.json must name the clips\' classes with '
                         '"labels_path" (a JSON list of integers, one per item of the audio pickle)' % n_global)
    if dataset_params.get("labels_path"):
        if not n_global:
            raise ValueError('dataset_params.json has "labels_path" but model_params.json leaves "global_classes" at 0: nothing would '
                             'read the labels')
        dataset_params = dict(dataset_params, n_classes=n_global)         # a label outside [0, global_classes) raises at load
        if train_params.get("valid_audio_path") and int(train_params.get("validate_every") or 0) > 0 \
                and not train_params.get("valid_labels_path"):
            raise ValueError('train_params.json: validating a model with "global_classes" needs "valid_labels_path", the classes of the '
                             'items of "valid_audio_path"')
    validation = wobjective.Validation.make(train_params, dataset_params) if rank == 0 else None
    if world > 1:
        assert dataset_params["batch_size"] % world == 0
        dataset_params = dict(dataset_params, shard=(rank, world))
    dataloader = audio_data_loader(**dataset_params)
    if cuda_available:
        net = net.cuda()
    wdist.broadcast_parameters(list(net.parameters()) + list(net.buffers()))      # (buffers: the running state of an EMA-updated codebook)
    max_gn, skip_nf = guard.guard_options(train_params)
    ema_decay, ema_warmup = ema.ema_options(train_params)
    fused = (bool(train_params.get("fused_step")) and cuda_available and
             str(train_params.get("optimizer_type", train_params.get("optimizer", "Adam"))).lower() == "adam")
    optimizer = get_optimizer(net, train_params.get("optimizer_type", train_params.get("optimizer", "Adam")),
                              train_params["learning_rate"], train_params.get("momentum", False), max_grad_norm=max_gn,
                              skip_nonfinite=skip_nf, ema_decay=None if fused else ema_decay, ema_warmup=ema_warmup)
    loss_func = nn.CrossEntropyLoss()
    is_writer = rank == 0
    loss_log_file = store_log_file = None
    if is_writer:
        os.makedirs(train_params["log_dir"], exist_ok=True)
        os.makedirs(train_params["restore_dir"], exist_ok=True)
        loss_log_file = open(train_params["log_dir"] + 'loss_log.log', 'a')
        store_log_file = open(train_params["log_dir"] + 'store_log.log', 'a')
    if world > 1:
        torch.distributed.barrier()
    num_trained = _resume_counter(train_params["log_dir"], train_params["print_every"])
    device = next(net.parameters()).device
    total_loss = torch.zeros((), dtype=torch.float64, device=device)
    step_seed = int(train_params.get("seed") or 0)
    engine = None
    if fused:
        engine = net._engine_for(device)
        engine.objective = objective
        engine.adam_init(lr=train_params["learning_rate"], max_grad_norm=max_gn, skip_nonfinite=skip_nf, ema_decay=ema_decay,
                         ema_warmup=ema_warmup)
    # the EMA shadow (music_amd/ema.py); no optimizer state is kept by this harness, so a resumed run's warm-up counts as finished
    shadow = engine.ema if fused else getattr(optimizer, "ema", None)
    if shadow is not None and restored_from is not None:
        ema.restore_shadow(shadow, restored_from[:-len(".model")] + ".ema", None,
                           engine.adam_state.get("guard") if fused else optimizer._guard)
    guard_log = None
    if guard.enabled(max_gn, skip_nf) and is_writer:
        guard_log = guard.GuardLog(
            train_params["log_dir"] + 'guard_log.log',
            lambda: engine.guard_report() if fused else optimizer.guard_report(),
            lambda: guard.engine_named_grads(engine) if fused else [(n, p.grad) for n, p in net.named_parameters()])
    is_vq = getattr(net, "bottleneck", "continuous") == "vq"
    is_vq_ema = is_vq and getattr(net, "vq_update", "gradient") == "ema"
    vq_drop = is_vq and getattr(net, "vq_stage_dropout", 0.0) > 0
    if vq_drop:
        net.vq_dropout_seed = int(train_params.get("vq_dropout_seed", 0))
    vq_init = train_params.get("vq_init", "uniform")
    if vq_init not in ("uniform", "data"):
        raise ValueError('train_params.json: "vq_init" must be "uniform" or "data", not %r' % (vq_init,))
    vq_init_pending = is_vq and vq_init == "data" and restored_from is None
    vq_log_file = open(train_params["log_dir"] + 'vq_log.log', 'a') if is_vq and is_writer else None
    for epoch in range(train_params["num_epochs"]):
        for i_batch, sampled_batch in enumerate(dataloader):
            piece, target = sampled_batch["audio_piece"], sampled_batch["audio_target"]
            # global class conditioning: the clips' classes, (B,) on the host, as ONE more keyword of the calls below - without it they
            # are made as they always were
            kw = {"classes": sampled_batch["audio_class"]} if "audio_class" in sampled_batch else {}
            if vq_drop and piece is not None:
                # quantiser dropout: the clips' stage counts from (seed, global step, global clip index), ONE more keyword as well
                kw["stages"] = net.draw_stages(piece.shape[0], step=num_trained, first_clip=int(sampled_batch.get("first_clip", 0)))
            dp_scale = float(sampled_batch.get("dp_scale", 1.0))      # ragged last batch, see faster_audio_data._Collate
            if piece is not None:
                target = target.view(-1)
                if wnll is not None:                          # (keys of objective "nll" alone: refused at start otherwise)
                    kw.update(wobjective.wnll_kwargs(wnll, sampled_batch, target.numel() // piece.shape[0], device))
            if vq_init_pending and piece is not None:
                # the codebook starts as K frames of the first batch's encoding in front of the quantiser (every replica from the
                # same frames: rank 0's, broadcast)
                vq_init_pending = False
                with torch.no_grad():
                    _, _, ws0 = net._engine_for(device).forward(piece.to(device).float().contiguous(), None, want_probs=False,
                                                                encode_only=True)
                net.init_codebook(ws0["enc_pre"], seed=step_seed)
                wdist.broadcast_parameters([net.vq_codebook.weight])
                net.reset_vq_ema_state()                      # (from the broadcast rows: the same running state on every replica)
                if shadow is not None and "vq_codebook.weight" in (getattr(shadow, "tensors", None) or {}):
                    shadow.tensors["vq_codebook.weight"].copy_(net.vq_codebook.weight.detach())      # the shadow was taken before
            if world > 1 and net.conditioning != "learned":
                # every replica must draw the SAME per-forward conditioning projections; learned ones are parameters
                torch.manual_seed(step_seed + num_trained)

            def closure():
                optimizer.zero_grad()
                loss = torch.zeros((), device=device)
                if piece is not None:
                    loss = wobjective.nll_loss(net, piece, target, **kw) if objective == "nll" else loss_func(net(piece, **kw), target)
                    if is_vq:
                        loss = loss + net.vq_loss
                    loss.backward()
                wdist.allreduce_gradients(net.parameters(), average=True, scale=dp_scale)
                return loss
            if fused:
                loss = torch.zeros((), device=device)
                if piece is not None:
                    loss = engine.loss_and_grad(piece.to(device).float().contiguous(), target.to(device), net.engine_cond(), **kw)
                else:
                    engine.flat_grad.zero_()
                    if is_vq_ema:
                        engine.vq_stat.zero_()                # an empty shard: no frames
                wdist.allreduce_flat_(engine.flat_grad, average=False, scale=dp_scale)
                if is_vq_ema:                                 # counts and sums of ALL ranks' frames: sums, so no dp_scale
                    wdist.allreduce_flat_(engine.vq_stat, average=False, scale=1.0)
                engine.adam_step(gscale=1.0 / wdist.world())
            else:
                loss = optimizer.step(closure) if isinstance(optimizer, optim.LBFGS) else closure()
                if is_vq_ema:
                    eng = net._engine_for(device)
                    if piece is None:
                        eng.vq_stat.zero_()
                    wdist.allreduce_flat_(eng.vq_stat, average=False, scale=1.0)
                if not isinstance(optimizer, optim.LBFGS):
                    optimizer.step()
                    if is_vq_ema and not isinstance(optimizer, guard.GuardedOptimizer):
                        eng.vq_ema_step()                     # (a GuardedOptimizer's step ends with it itself)
            loss = loss.detach() * dp_scale
            total_loss += loss.detach().double()
            num_trained += 1
            if num_trained % train_params["print_every"] == 0:
                if world > 1:
                    torch.distributed.all_reduce(total_loss)
                    total_loss /= world
                if is_writer:
                    loss_log_file.writelines('Average loss is ' + str(total_loss.item() / train_params["print_every"]) + '\n')
                    loss_log_file.flush()
                if guard_log is not None:
                    guard_log.tick(num_trained)
                stats = (engine.last_vq if fused else net.last_vq) if vq_log_file is not None else None
                if stats is not None:                         # (the last step's figures, read back where the loss is)
                    vq_log_file.writelines('Trained over %d pieces, vq mse %s, perplexity %s, codes used %d%s%s%s\n'
                                           % (num_trained, stats.mse.item(), stats.perplexity.item(), int(stats.codes_used.item()),
                                              ", restarted %d" % net._engine_for(device).vq_restarted() if is_vq_ema else "",
                                              vq_stage_fields(stats) if getattr(net, "vq_stages", 1) > 1 else "",
                                              ", active " + "/".join("%d" % v for v in stats.stage_frames.tolist()) if vq_drop else ""))
                    vq_log_file.flush()
                total_loss.zero_()
            if validation is not None:
                validation.tick(net, num_trained, shadow)
        if (epoch + 1) % train_params["check_point_every"] == 0 and is_writer:
            stored = glob.glob(train_params["restore_dir"] + "*.model")
            _rotate_checkpoints(stored, train_params["max_check_points"])
            save_model(net, epoch_trained + epoch + 1, train_params["restore_dir"])
            if shadow is not None:
                ema.save_shadow(shadow, train_params["restore_dir"] + PREFIX + str(epoch_trained + epoch + 1) + ".ema", net)
            store_log_file.writelines('Epoch' + str(epoch_trained + epoch + 1) + 'model saved!')
            store_log_file.flush()
    if is_writer:
        loss_log_file.close()
        store_log_file.close()
        if vq_log_file is not None:
            vq_log_file.close()


if __name__ == '__main__':
    train()
