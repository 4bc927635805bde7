"""The objective of the model the decoder samples from: the negative log-likelihood of every sample under the softmax over the Q
channels of ITS output column (``wn_step_nll`` / ``wn_step_softmax``, music_amd/csrc/wn_nll.hip).

The reference trains something else on purpose-reproduced quirks: cross entropy applied to probabilities of a softmax
that runs over time, on a scrambled one-hot.  Nothing of that changes here; this module is the opt-in
alternative, for ``wavenet`` and ``wavenet_autoencoder`` alike:

``nll_loss(net, x, target)``   mean nats per sample as a 0-d tensor attached to autograd (training)
``step_probs(net, x)``         (B W, Q) per-timestep probabilities, the distribution the decoder draws from
``score(net, x, target)``      per-clip nats, bits and accuracy of a checkpoint on held-out audio, no gradient

All three take ``windows=`` / ``window_pos=``: the samplers' position windows (``fast_generate.stage_windows``) applied to the
objective (``wn_win_step_nll`` / ``wn_win_step_softmax``), for a prior over a residual quantiser's interleaved token stream - the
softmax of a column is taken inside the pair of its stream position, which is what ``sample_code_stream`` draws from.

``nll_loss`` and ``score`` take ``weights=`` / ``ignore_index=`` / ``label_smoothing=`` (``wn_wstep_nll``): the weighted mean over the
columns that carry a target.  A column whose target is ``ignore_index`` (a dropped stage's -1, padding) or whose weight is 0 is
skipped - it adds nothing to the loss, to any gradient or to the count the mean is taken over.

There is no CPU path: the arithmetic runs through libwavenet_hip.so only.
"""
from contextlib import nullcontext
import math

import numpy as np
import torch

try:
    from . import faster_audio_data
    from .engine_base import OBJECTIVES, NllWindows, WorkspaceHold
except ImportError:                      # imported as a bare module
    from music_amd import faster_audio_data
    from music_amd.engine_base import OBJECTIVES, NllWindows, WorkspaceHold


def _dense_input(wave_sample):
    """float32 contiguous view of the input; a one-hot built from codes keeps its tag (music_amd/model.py)"""
    x = wave_sample.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        return x.float().contiguous()
    tag = getattr(wave_sample, "_wn_codes", None)
    if tag is not None and wave_sample._version == tag[2]:
        x._wn_codes = (tag[0], tag[1], x._version, tag[3])
    return x


def _forward_logits(net, wave_sample, classes=None, stages=None, phase_pos=None):
    """The module's forward up to the pre-softmax logits: (engine, workspace with the logits in ws["O"]).  The autoencoder draws its
    per-forward conditioning convs from the global RNG, as its own forward does (learned ones are parameters: nothing is drawn)."""
    if wave_sample.dim() != 3:
        raise ValueError("music_amd.objective: the input is a (B, Q, T) one-hot, got shape %s" % (tuple(wave_sample.shape),))
    if wave_sample.shape[2] - net.receptive_field + 1 <= 0:
        raise ValueError("wave sample not long enough")
    if hasattr(net, "check_classes"):
        net.check_classes(classes)                              # (a class-conditional WaveNet: required there, refused elsewhere)
    if hasattr(net, "check_phase"):
        net.check_phase(phase_pos)                              # (a phase-conditioned WaveNet: likewise)
    elif phase_pos is not None:
        raise ValueError("music_amd.objective: phase_pos is a phase-conditioned WaveNet's (phase_period)")
    eng = net._engine_for(wave_sample.device)
    x = _dense_input(wave_sample)
    if hasattr(net, "engine_cond"):
        kw = {} if stages is None else {"stages": stages}       # (quantiser dropout of a residual vq bottleneck: music_amd/vq_dropout.py)
        _, enc, ws = eng.forward(x, net.engine_cond(), want_probs=False, classes=classes, **kw)
        net.last_encoding = enc
    else:
        if stages is not None:
            raise ValueError("music_amd.objective: stages are the autoencoder's (quantiser dropout)")
        eng.pack_weights()
        kw = {} if classes is None else {"classes": classes}
        if phase_pos is not None:
            kw["phase_pos"] = phase_pos
        ws = eng.forward_logits(x, **kw)
    return eng, ws


def _flat_target(target, ws):
    target = target.reshape(-1)
    if target.numel() != ws["B"] * ws["W"]:
        raise ValueError("music_amd.objective: %d targets for %d clips of %d samples" % (target.numel(), ws["B"], ws["W"]))
    return target.to(device=ws["O"].device, dtype=torch.int64).contiguous()


class _NLLFunction(torch.autograd.Function):
    """forward_logits + wn_step_nll; the kernel leaves d loss / d logits in the backward workspace, so the backward is the engine's
    backward_from_dlogits scaled by the upstream scalar."""

    @staticmethod
    def forward(ctx, net, grad_on, wave_sample, target, classes, stages, windows, window_pos, phase_pos, wnll, *params):
        eng, ws = _forward_logits(net, wave_sample, classes, stages, phase_pos)
        need = grad_on and any(ctx.needs_input_grad)
        eng.step_nll(ws, _flat_target(target, ws), eng._bwd_workspace(ws)["dO"] if need else None, windows=windows,
                     window_pos=window_pos, **wnll)
        ctx.eng, ctx.ws, ctx.gen = eng, ws, ws["gen"]
        ctx.hold = WorkspaceHold(ws) if need else None          # see music_amd/model.py
        if getattr(eng, "vq", False):
            # a vq autoencoder: vq_loss is a second output of this node, which nll_loss leaves in net.vq_loss for the caller to add
            net.last_encoding_pre, net.vq_codes, net.last_vq = ws["enc_pre"], eng.vq_codes_of(ws), eng.last_vq
            ctx.set_materialize_grads(False)
            return ws["loss_part"].sum(), eng.last_vq.vq_loss
        return ws["loss_part"].sum()

    @staticmethod
    def backward(ctx, dloss, dvq=None):
        eng, ws = ctx.eng, ctx.ws
        if ws.get("gen") != ctx.gen:
            raise RuntimeError("music_amd.objective: the activations of this forward were overwritten by a later forward of the "
                               "same module before backward() ran")
        vq = getattr(eng, "vq", False)
        if vq:
            eng.vq_backward_scaled(ws, dloss, dvq)
            dloss = 1.0
        else:
            eng.backward_from_dlogits(ws)
        if ctx.hold is not None:
            ctx.hold.release()
        g = eng.flat_grad * dloss
        grads = []
        for name in eng.param_names:
            o, shp = eng.spec.off[name], eng.spec.shape[name]
            grads.append(g[o:o + int(np.prod(shp))].view(shp))
        din = eng.input_grad(ws) * dloss if ctx.needs_input_grad[2] else None
        return (None, None, din, None, None, None, None, None, None, None) + tuple(grads)


def _params(net):
    """the module's parameters in its engine's order (music_amd/model.py, music_amd/model1.py)"""
    return [p for _, p in net._named_ref_params()] if hasattr(net, "_named_ref_params") else list(net.parameters())


def _wnll(weights, ignore_index, label_smoothing):
    """the three keywords of the masked / weighted / smoothed objective as EngineBase.step_nll takes them"""
    return dict(weights=weights, ignore_index=ignore_index, label_smoothing=label_smoothing)


def nll_loss(net, x, target, classes=None, stages=None, windows=None, window_pos=None, phase_pos=None, weights=None, ignore_index=None,
             label_smoothing=0.0):
    """Mean negative log-likelihood (nats per sample) of `target` (B, W) or (B W,) int64 under the per-timestep softmax of
    net's logits for the one-hot x (B, Q, T): a 0-d tensor whose backward() gives the parameter gradients (and the input's, when it
    requires grad).  A target outside [0, Q) makes the loss NaN.  classes: one integer per clip for a model with global class
    conditioning - an autoencoder or a WaveNet (required there, refused elsewhere).  stages: the clips' stage counts under quantiser dropout, as the autoencoder's
    forward takes them (None: all stages - this function draws nothing).  windows: 1..16 (lo, hi) pairs (None: the engine's
    nll_windows) - the softmax of column c of clip b is taken inside the pair of stream position window_pos[b] + c; window_pos: None
    (0), an int, or one per clip (a sequence, or an int64 device tensor: no host synchronisation).  A target outside its window makes
    the loss NaN.  phase_pos: the stream position of every clip's first target for a phase-conditioned WaveNet (required there,
    refused elsewhere): one int, one per clip, or an int64 device tensor.
    weights ((B, W) or (B W,) floats >= 0, on the device or the host), ignore_index (an int) and label_smoothing (in [0, 1)), any of
    them set: the loss is sum(w l) / sum(w) over the columns that carry a target - one whose target is ignore_index or whose weight
    is 0 is skipped, whatever its target and logits hold - with l the smoothed cross entropy of
    torch.nn.functional.cross_entropy(label_smoothing=), taken inside the column's window.  A negative weight makes the loss NaN;
    with nothing counted the loss is 0."""
    out = _NLLFunction.apply(net, torch.is_grad_enabled(), x, target, classes, stages, windows, window_pos, phase_pos,
                             _wnll(weights, ignore_index, label_smoothing), *_params(net))
    if isinstance(out, tuple):                                  # a vq autoencoder: the caller adds net.vq_loss
        out, net.vq_loss = out
    return out


def step_probs(net, x, classes=None, windows=None, window_pos=None, phase_pos=None):
    """(B W, Q) probabilities: row b W + w is softmax over the Q logits of output column w of clip b - what the decoder samples
    from (the module's own forward returns the reference's chunk softmax instead).  windows / window_pos (nll_loss): the
    distribution a windowed decode draws from, an exact 0 outside the column's window.  phase_pos: nll_loss's."""
    with torch.no_grad():
        eng, ws = _forward_logits(net, x, classes, phase_pos=phase_pos)
        return eng.step_probs(ws, windows=windows, window_pos=window_pos)


def guided_probs(net, x, classes, guidance, windows=None, window_pos=None, phase_pos=None):
    """(B W, Q) float64: the teacher-forced distribution a classifier-free-guided decode draws sample w of clip b from
    (include/wavenet_hip.h, wn_cfg_decode_batch) - the forward the decoder is held to.  Two ``step_probs`` forwards, as `classes`
    (p_c) and with every clip as the model's ``null_class`` (p_u); the guided logits l_c + (s - 1)(l_c - l_u) differ from
    s log p_c - (s - 1) log p_u by a constant per row, so the result is p_c^s / p_u^(s-1) renormalised inside the column's window,
    computed in float64 logs.  guidance: a scale or one per clip.  An entry either forward gives an exact 0 (outside the window, or
    under float32's range) has probability 0."""
    null = getattr(net, "null_class", None)
    if null is None:
        raise ValueError('music_amd.objective.guided_probs: the model needs "null_class" (the class that stands for "no class")')
    B = x.size(0)
    pc = step_probs(net, x, classes=classes, windows=windows, window_pos=window_pos, phase_pos=phase_pos).double()
    pu = step_probs(net, x, classes=[int(null)] * B, windows=windows, window_pos=window_pos, phase_pos=phase_pos).double()
    s = torch.as_tensor(guidance, dtype=torch.float64).reshape(-1)
    if s.numel() not in (1, B) or not bool(torch.isfinite(s).all()):
        raise ValueError("music_amd.objective.guided_probs: guidance must be a finite number or one per clip (%d)" % B)
    s = s.expand(B).to(pc.device).repeat_interleave(pc.size(0) // B).view(-1, 1)
    inside = (pc > 0) & (pu > 0)
    one = torch.ones_like(pc)
    lg = s * torch.log(torch.where(inside, pc, one)) - (s - 1.0) * torch.log(torch.where(inside, pu, one))
    lg = torch.where(inside, lg, torch.full_like(lg, -float("inf")))
    e = torch.exp(lg - lg.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def score(net, x_or_codes, target, scrambled=False, classes=None, stages=None, windows=None, window_pos=None, phase_pos=None,
          weights=None, ignore_index=None, label_smoothing=0.0):
    """Held-out figures of net on one batch, forward only.  x_or_codes: the one-hot (B, Q, T) float, or the integer codes (B, T) -
    then the one-hot is laid out canonical, or as the loader scrambles it with `scrambled`.  Returns device tensors of
    shape (B,), float64: "nll" (mean nats per sample of each clip), "bits" (nll / ln 2) and "accuracy" (share of samples whose
    first-index argmax is the target); the per-clip means are taken on the device, nothing is read back.  stages: score a residual vq
    autoencoder with the first n stages (an int, or one per clip) - the coarser code's figures.  windows / window_pos (nll_loss): the
    figures of the windowed distribution, the honest bits per token of what sample_code_stream draws from.
    weights / ignore_index (nll_loss), either set: the three figures are the weighted means over the clip's counted columns, and
    "tokens" (B,) is the clip's sum of weights; a clip with none reports NaN for all three.  label_smoothing selects that launch
    too; the figures are unsmoothed."""
    with torch.no_grad():
        x = x_or_codes
        if x.dim() == 2:
            q = getattr(net, "quantization_channels", None) or net.quantization_channel
            x = faster_audio_data.onehot_device(x, q, scrambled)
        eng, ws = _forward_logits(net, x, classes, stages, phase_pos)
        # (the weights are checked and brought to the device ONCE, here: the launch and the means below take the same tensor)
        wt = eng._resolve_wnll(ws, weights, ignore_index, label_smoothing)
        wnll = {} if wt is None else _wnll(wt[0], ignore_index, label_smoothing)
        tgt = _flat_target(target, ws)
        row_nll, row_hit = eng.score_logits(ws, tgt, windows=windows, window_pos=window_pos, **wnll)
        B, W = ws["B"], ws["W"]
        if wt is None:
            nll = row_nll.view(B, W).double().mean(1)
            return {"nll": nll, "bits": nll / math.log(2.0), "accuracy": row_hit.view(B, W).double().mean(1)}
        # the kernel's rule for a column's weight, on the device; a skipped column's row_nll and row_hit are exact zeros
        wv = torch.ones(B * W, dtype=torch.float64, device=tgt.device) if wt[0] is None else wt[0].double()
        if ignore_index is not None:
            wv = torch.where(tgt == int(ignore_index), torch.zeros_like(wv), wv)
        wv = wv.view(B, W)
        tokens = wv.sum(1)
        nll = (wv * row_nll.view(B, W).double()).sum(1) / tokens             # (0 / 0: NaN for a clip with nothing counted)
        acc = (wv * row_hit.view(B, W).double()).sum(1) / tokens
        return {"nll": nll, "bits": nll / math.log(2.0), "accuracy": acc, "tokens": tokens}


# ---------------------------------------------------------------- train() / ae_train: the JSON keys
def objective_option(train_params):
    """The optional key "objective" of train_params.json: "reference" (default) or "nll"."""
    objective = train_params.get("objective", "reference")
    if objective not in OBJECTIVES:
        raise ValueError('train_params.json: "objective" must be one of %s, not %r' % (", ".join(OBJECTIVES), objective))
    return objective


def nll_windows_option(train_params, dataset_params, quantization_channels=None):
    """The optional key "nll_windows" of train_params.json: {"stages": S, "codes": K} - fast_generate.stage_windows(S, K), the table
    of a residual quantiser's token stream (tools/vq_codes_dataset.py) - or an explicit list of [lo, hi] pairs; None when unset.
    It needs "objective": "nll" (the reference's loss has no per-column softmax to window), "token_positions": true in
    dataset_params.json (every clip would otherwise be scored as if it started at stream position 0) and hi <= quantization_channels
    (default: dataset_params')."""
    spec = train_params.get("nll_windows")
    if spec is None:
        return None
    if objective_option(train_params) != "nll":
        raise ValueError('train_params.json: "nll_windows" needs "objective": "nll", not %r' % train_params.get("objective", "reference"))
    if not dataset_params.get("token_positions"):
        raise ValueError('train_params.json: "nll_windows" needs "token_positions": true in dataset_params.json (the stream position '
                         'of every clip)')
    if isinstance(spec, dict):
        if set(spec) != {"stages", "codes"}:
            raise ValueError('train_params.json: "nll_windows" as an object is {"stages": S, "codes": K}, got keys %s' % sorted(spec))
        try:                                 # (here, not at the top: fast_generate imports train, which imports this module)
            from .fast_generate import stage_windows
        except ImportError:
            from music_amd.fast_generate import stage_windows
        spec = stage_windows(spec["stages"], spec["codes"])
    q = dataset_params.get("quantization_channels", 256) if quantization_channels is None else quantization_channels
    try:
        return NllWindows(spec, int(q)).pairs
    except ValueError as e:
        raise ValueError('train_params.json: "nll_windows": %s' % e) from None


WNLL_KEYS = ("ignore_token", "label_smoothing", "nll_stage_weights")


def wnll_option(train_params, dataset_params):
    """The optional keys "ignore_token" (an int: targets of that value - a dropped stage's -1, padding - are skipped),
    "label_smoothing" (a float in [0, 1)) and "nll_stage_weights" (1..16 non-negative floats: the target at stream position p weighs
    list[p mod len]) of train_params.json: the masked, weighted and smoothed "nll" objective (wn_wstep_nll).  None when all are unset,
    else {"ignore_index", "label_smoothing", "stage_weights"}.  Each needs "objective": "nll" (the reference's loss has no per-column
    term to weight); "nll_stage_weights" needs "token_positions": true in dataset_params.json too, the stream position of every clip."""
    given = [k for k in WNLL_KEYS if train_params.get(k) is not None]
    if not given:
        return None
    if objective_option(train_params) != "nll":
        raise ValueError('train_params.json: "%s" needs "objective": "nll", not %r'
                         % (given[0], train_params.get("objective", "reference")))
    ignore, eps, sw = (train_params.get(k) for k in WNLL_KEYS)
    if ignore is not None and (isinstance(ignore, bool) or not isinstance(ignore, int)):
        raise ValueError('train_params.json: "ignore_token" must be an integer, not %r' % (ignore,))
    if eps is not None:
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= float(eps) < 1.0:
            raise ValueError('train_params.json: "label_smoothing" must be a number in [0, 1), not %r' % (eps,))
    if sw is not None:
        if not dataset_params.get("token_positions"):
            raise ValueError('train_params.json: "nll_stage_weights" needs "token_positions": true in dataset_params.json (the stream '
                             'position of every clip)')
        ok = isinstance(sw, list) and 1 <= len(sw) <= 16 and all(
            not isinstance(v, bool) and isinstance(v, (int, float)) and 0.0 <= float(v) < float("inf") for v in sw)
        if not ok:
            raise ValueError('train_params.json: "nll_stage_weights" must be a list of 1..16 non-negative numbers, not %r' % (sw,))
        sw = [float(v) for v in sw]
    return {"ignore_index": ignore, "label_smoothing": float(eps or 0.0), "stage_weights": sw}


def wnll_kwargs(option, batch, W, device):
    """nll_loss's / loss_and_grad's keywords for one batch under wnll_option's keys ({} when unset).  The stage weights become
    the (B, W) weights on the device, list[(audio_pos[b] + c) mod len] for target c of clip b, from the loader's "audio_pos" by
    index arithmetic there.  The table and the column offsets are uploaded ONCE per device and width and kept in `option`; with the
    loader's device positions a batch then issues device work only - no host-to-device copy, nothing read back, no synchronisation."""
    if option is None:
        return {}
    kw = {"ignore_index": option["ignore_index"], "label_smoothing": option["label_smoothing"]}
    if option["stage_weights"] is not None:
        device = torch.device(device)
        cache = option.setdefault("_device", {})
        if (device, W) not in cache:
            cache[device, W] = (torch.tensor(option["stage_weights"], dtype=torch.float32).to(device),
                                torch.arange(W, dtype=torch.int64).to(device))
        table, cols = cache[device, W]
        pos = torch.as_tensor(batch["audio_pos"]).to(device=device, dtype=torch.int64).reshape(-1, 1)
        kw["weights"] = table[(pos + cols) % table.numel()]
    return kw


class Validation:
    """Held-out scoring during training: every `validate_every` steps, `score` over the loader of "valid_audio_path" - under the
    EMA shadow's weights when there is one - and one line in valid_log.log.  make() returns None when the keys are unset: nothing
    is built and nothing is launched then."""

    @classmethod
    def make(cls, train_params, dataset_params):
        path, every = train_params.get("valid_audio_path"), int(train_params.get("validate_every") or 0)
        if not path or every <= 0:
            return None
        return cls(path, every, dataset_params, train_params["log_dir"], train_params.get("valid_labels_path"),
                   nll_windows_option(train_params, dataset_params), wnll_option(train_params, dataset_params))

    def __init__(self, audio_path, every, dataset_params, log_dir, labels_path=None, windows=None, wnll=None):
        # (the training set's labels name the training pickle's items: the held-out set's come from "valid_labels_path")
        params = {k: v for k, v in dataset_params.items() if k not in ("shard", "labels_path")}
        params.update(audio_path=audio_path, shuffle=False)
        if labels_path:
            params.update(labels_path=labels_path)
        self.every = every
        self.windows = windows               # ("nll_windows": the held-out figures are those of the windowed distribution)
        self.wnll = wnll                     # (wnll_option: the held-out means run over the counted targets, by their weights)
        self.loader = faster_audio_data.audio_data_loader(**params)
        self.log_path = log_dir + "valid_log.log"

    def run(self, net, shadow=None):
        """(nll, bits per sample, accuracy) over the held-out loader, as Python floats (the one read-back of a validation)"""
        total = None
        with (shadow.swapped(net) if shadow is not None else nullcontext()):
            for batch in self.loader:
                if batch["audio_piece"] is None:
                    continue
                kw = {"classes": batch["audio_class"]} if "audio_class" in batch else {}       # (global class conditioning)
                if self.windows is not None:
                    kw.update(windows=self.windows, window_pos=batch["audio_pos"])
                if getattr(net, "phase_period", 0):                                            # (a phase-conditioned prior)
                    kw.update(phase_pos=batch["audio_pos"])
                if self.wnll is not None:
                    target = batch["audio_target"]
                    kw.update(wnll_kwargs(self.wnll, batch, target.numel() // target.shape[0], next(net.parameters()).device))
                r = score(net, batch["audio_piece"], batch["audio_target"], **kw)
                if "tokens" in r:            # every counted target weighs its own weight: clips by their sums, an empty one not at all
                    tk = r["tokens"]
                    part = torch.stack([torch.where(tk > 0, r[k] * tk, torch.zeros_like(tk)).sum() for k in ("nll", "bits", "accuracy")]
                                       + [tk.sum()])
                else:
                    part = torch.stack([r["nll"].sum(), r["bits"].sum(), r["accuracy"].sum(), r["nll"].new_tensor(r["nll"].numel())])
                total = part if total is None else total + part
        if total is None:
            raise ValueError("music_amd.objective: the validation set holds no piece")
        return tuple((total[:3] / total[3]).tolist())

    def tick(self, net, num_trained, shadow=None):
        """after training step `num_trained`: validate and log when it is due"""
        if num_trained % self.every != 0:
            return None
        nll, bits, acc = self.run(net, shadow)
        with open(self.log_path, "a") as f:
            f.write("Trained over " + str(num_trained) + " pieces,Validation nll is " + str(nll) + ", bits per sample " + str(bits) +
                    ", accuracy " + str(acc) + "\n")
        return nll, bits, acc
