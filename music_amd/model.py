"""Drop-in counterpart of the reference's ``wavenet/model.py`` backed by the MI355X HIP kernels.

Same constructor kwargs, attributes, registered ``nn.Conv1d`` sub-modules (hence the same
``state_dict`` keys / shapes and the attribute access ``fast_generate.py`` relies on), same
``forward`` contract (wavenet/model.py:86-145): input ``(B, Q, T >= receptive_field)`` float ->
probabilities ``(B*(T-rf+1), Q)`` with the reference's CHUNK softmax semantics, and the same
``ValueError("wave sample not long enough")``.

The arithmetic runs only through libwavenet_hip.so (music_amd/engine.py).  There is no CPU
implementation: calling ``forward`` without a ROCm device raises.
"""
import math

import torch
import torch.nn as nn

try:
    from . import _lib, _losshook
    from .engine import WaveNetEngine, WorkspaceHold
    from .engine_generic import GenericWaveNetEngine
except ImportError:                      # imported as a bare module (`from model import wavenet`)
    from music_amd import _lib, _losshook
    from music_amd.engine import WaveNetEngine, WorkspaceHold
    from music_amd.engine_generic import GenericWaveNetEngine

_Probs = _losshook.Probs                 # the type of the module's output while a backward may follow


class _WaveNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, grad_on, wave_sample, classes, phase_pos, *params):
        eng = net._engine_for(wave_sample.device)
        x = wave_sample.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        else:
            tag = getattr(wave_sample, "_wn_codes", None)        # one-hot built from codes (engine.forward_logits)
            if tag is not None and wave_sample._version == tag[2]:
                x._wn_codes = (tag[0], tag[1], x._version, tag[3])
        kw = {} if classes is None else {"classes": classes}
        if phase_pos is not None:
            kw["phase_pos"] = phase_pos
        probs, ws = eng.forward(x, **kw)
        ctx.eng, ctx.ws, ctx.gen = eng, ws, ws["gen"]
        ctx.loss_hook = net._last_hook = _losshook.make(eng, ws, grad_on)
        # a forward that some backward may follow keeps its workspace: the next forward of this shape gets another one (several
        # micro-batches in flight, as the reference's autograd allows).  `grad_on` is torch.is_grad_enabled() as the caller saw
        # it (inside Function.forward it is always off, and needs_input_grad is True for parameters even under no_grad): an
        # inference forward holds nothing
        ctx.hold = WorkspaceHold(ws) if (grad_on and any(ctx.needs_input_grad)) else None
        # a fresh alias goes out: the workspace keeps `probs` for the backward, and the tensor autograd hangs this node on
        # must not be the one the workspace holds (workspace -> output -> node -> hold -> workspace would never die)
        return probs.detach()

    @staticmethod
    def backward(ctx, dprobs):
        eng, ws = ctx.eng, ctx.ws
        if ws.get("gen") != ctx.gen:
            raise RuntimeError("music_amd.wavenet: the activations of this forward were overwritten by a later "
                               "forward of the same module before backward() ran")
        if not _losshook.backward(ctx.loss_hook, eng, ws, dprobs):          # (the loss ran fused: see _losshook.py)
            eng.backward(ws, dprobs)
        if ctx.hold is not None:
            ctx.hold.release()           # (retain_graph + a second backward still works until the next forward reuses it)
        g = eng.flat_grad.clone()
        grads = []
        for name in eng.param_names:
            o, shp = eng.spec.off[name], eng.spec.shape[name]
            n = 1
            for s in shp:
                n *= s
            grads.append(g[o:o + n].view(shp))
        # the input's own gradient, when autograd asks for it (the reference's causal nn.Conv1d provides it, wavenet/model.py:104)
        din = eng.input_grad(ws) if ctx.needs_input_grad[2] else None
        return (None, None, din, None, None) + tuple(grads)


class wavenet(nn.Module):

    def __init__(self, filter_width, dilations, dilation_channels, residual_channels, skip_channels,
                 quantization_channels, use_bias, global_classes=0, global_channels=0, null_class=None, phase_period=0):
        super(wavenet, self).__init__()
        phase_period = 0 if phase_period is None else phase_period
        if isinstance(phase_period, bool) or not isinstance(phase_period, int) or not 0 <= phase_period <= _lib.PHASE_MAX_PERIOD:
            raise ValueError("music_amd.wavenet: phase_period must be an integer in [1, %d] (0 or absent: off), not %r"
                             % (_lib.PHASE_MAX_PERIOD, phase_period))
        self.phase_period = phase_period
        for key, val in (("global_classes", global_classes), ("global_channels", global_channels)):
            if isinstance(val, bool) or not isinstance(val, int) or val < 0:
                raise ValueError("music_amd.wavenet: %s must be an integer >= 0, not %r" % (key, val))
        if (global_classes > 0) != (global_channels > 0):
            raise ValueError("music_amd.wavenet: global_classes and global_channels must both be 0 (off) or both >= 1, not %r and %r"
                             % (global_classes, global_channels))
        if global_channels > _lib.GCOND_MAX_CHANNELS:
            raise ValueError("music_amd.wavenet: global_channels must lie in [1, %d], not %r" % (_lib.GCOND_MAX_CHANNELS, global_channels))
        self.global_classes, self.global_channels = global_classes, global_channels
        # classifier-free guidance: the row of the embedding that stands for "no class" (train.py's "class_dropout" trains it,
        # fast_generate's guidance= decodes against it).  It names an existing row: no parameter, no kernel, no state_dict key
        if null_class is not None:
            if isinstance(null_class, bool) or not isinstance(null_class, int) or not global_classes or not 0 <= null_class < global_classes:
                raise ValueError("music_amd.wavenet: null_class must be an integer in [0, global_classes) of a model with "
                                 "global_classes > 0, not %r (global_classes = %d)" % (null_class, global_classes))
        self.null_class = null_class
        self.filter_width = filter_width
        self.dilations = dilations
        self.dilation_channels = dilation_channels
        self.residual_channels = residual_channels
        self.skip_channels = skip_channels
        self.quantization_channels = quantization_channels
        self.use_bias = use_bias
        self.receptive_field = self.calc_receptive_field()
        # construction order (and therefore the default-init RNG stream) follows
        # wavenet/model.py:38-41: causal, then per dilation filter/gate/dense/skip, then post-process
        self.causal_layer = nn.Conv1d(quantization_channels, residual_channels, filter_width, bias=use_bias)
        self.dilation_layer_stack = nn.ModuleList()
        for d in dilations:
            self.dilation_layer_stack.extend([
                nn.Conv1d(residual_channels, dilation_channels, filter_width, dilation=d, bias=use_bias),
                nn.Conv1d(residual_channels, dilation_channels, filter_width, dilation=d, bias=use_bias),
                nn.Conv1d(dilation_channels, residual_channels, 1, bias=use_bias),
                nn.Conv1d(dilation_channels, skip_channels, 1, bias=use_bias)])
        self.post_process_1 = nn.Conv1d(skip_channels, skip_channels, 1, bias=use_bias)
        self.post_process_2 = nn.Conv1d(skip_channels, quantization_channels, 1, bias=use_bias)
        self.softmax = nn.Softmax(dim=1)     # the reference's nn.Softmax() resolves to dim 1 on 2-D input
        if global_classes > 0:
            # global conditioning on a class per clip (WaveNet paper section 2.5): [f; g]_i += G_i emb[c] in every block and
            # h += G_f emb[c] in front of post_process_1's ReLU, constant over time.  The G_i (2 D x E, gate rows first, like the
            # autoencoder's de_gcond_layer_stack), G_f and the embedding are registered - and drawn - BEHIND everything the model has
            # without them: a seed gives every earlier parameter the same value and flat offset.  No biases of their own.
            self.gcond_layer_stack = nn.ModuleList(nn.Conv1d(global_channels, 2 * dilation_channels, 1, bias=False) for _ in dilations)
            self.connection_gcond = nn.Conv1d(global_channels, skip_channels, 1, bias=False)
            self.global_embedding = nn.Embedding(global_classes, global_channels)
        if phase_period > 0:
            # phase conditioning (a prior over a residual quantiser's frame-major code stream: the stage is position mod P): a learned
            # column per phase, [f; g]_i(column) += phase_layer_stack.i[:, p mod P] in every block and h += connection_phase[:, p mod P]
            # in front of post_process_1's ReLU, p the stream position the column's output predicts.  Tables of shape (2 D, P), gate
            # rows first like gcond_layer_stack, and (S, P); registered - and drawn - BEHIND everything else, the global block
            # included.  Init: gcond_layer_stack's rule, nn.Conv1d's default (kaiming uniform with a = sqrt(5)) at fan-in P, which is
            # U(-1 / sqrt(P), 1 / sqrt(P)).  No biases.
            def table(rows):
                t = torch.empty(rows, phase_period)
                nn.init.kaiming_uniform_(t, a=math.sqrt(5))
                return nn.Parameter(t)
            self.phase_layer_stack = nn.ParameterList([table(2 * dilation_channels) for _ in dilations])
            self.connection_phase = table(skip_channels)
        self._engine = None
        self.precision = ("f16x3", "bf16x3")     # (forward, backward) arithmetic of the MFMA products
        # nn.CrossEntropyLoss()(net(x), target) with its default arguments runs as the engine's fused softmax + CE pass (the output
        # is a Tensor subclass that intercepts exactly that call; everything else sees an ordinary tensor).  False: torch's own
        self.fuse_loss = True
        self._last_hook = None

    def __getstate__(self):
        # copy.deepcopy / pickle / torch.save(module): the engine (HIP streams, workspaces, ctypes plans) stays behind and is rebuilt
        # on the copy's first forward; the parameters travel as tensors
        state = self.__dict__.copy()
        state["_engine"] = None
        state["_last_hook"] = None
        return state

    def __setstate__(self, state):
        super(wavenet, self).__setstate__(state)
        self.__dict__.setdefault("global_classes", 0)        # (a module pickled before the keys existed)
        self.__dict__.setdefault("global_channels", 0)
        self.__dict__.setdefault("null_class", None)
        self.__dict__.setdefault("phase_period", 0)

    def named_parameters(self, *args, **kwargs):
        """torch lists a module's own parameters in front of its children's; connection_phase, the one parameter this module owns
        directly, is the model's LAST (parameters(), the optimizers, the EMA shadow and the engine's flat buffer follow this order)"""
        last = self._parameters.get("connection_phase")
        tail = []
        for name, p in super(wavenet, self).named_parameters(*args, **kwargs):
            if last is not None and p is last:
                tail.append((name, p))
            else:
                yield name, p
        for item in tail:
            yield item

    def global_vectors(self, classes):
        """The (detached) embedding rows (B, E) of `classes`, B integers in [0, global_classes)."""
        if not self.global_classes:
            raise ValueError("music_amd.wavenet: global_vectors needs global_classes > 0")
        w = self.global_embedding.weight.detach()
        cls = torch.as_tensor(classes, dtype=torch.int64).reshape(-1)
        if cls.numel() and not (0 <= int(cls.min()) and int(cls.max()) < self.global_classes):
            raise ValueError("music_amd.wavenet: a class lies outside [0, %d) (global_classes)" % self.global_classes)
        return w[cls.to(w.device)]

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A checkpoint loads only into a model of the same mode, class count and embedding width: refused whole, by name."""
        emb = state_dict.get("global_embedding.weight", state_dict.get("module.global_embedding.weight"))
        saved = tuple(emb.shape) if emb is not None and emb.dim() == 2 else (0, 0)
        mine = (getattr(self, "global_classes", 0), getattr(self, "global_channels", 0))
        if saved != mine:
            raise RuntimeError("music_amd.wavenet: the checkpoint was saved with global_classes=%d, global_channels=%d but this model "
                               "was built with global_classes=%d, global_channels=%d (the keys of the model's parameters JSON); "
                               "nothing was loaded" % (saved + mine))
        ph = state_dict.get("connection_phase", state_dict.get("module.connection_phase"))
        saved_p, mine_p = int(ph.shape[1]) if ph is not None and ph.dim() == 2 else 0, getattr(self, "phase_period", 0)
        if saved_p != mine_p:
            raise RuntimeError("music_amd.wavenet: the checkpoint was saved with phase_period=%d (%s) but this model was built with "
                               "phase_period=%d (%s) (the key of the model's parameters JSON); nothing was loaded"
                               % (saved_p, "phase-conditioned" if saved_p else "off", mine_p, "phase-conditioned" if mine_p else "off"))
        return super(wavenet, self).load_state_dict(state_dict, *args, **kwargs)

    def check_phase(self, phase_pos):
        """phase_pos is refused with the mode off and required with it on - before an engine is built or anything is launched; a
        negative entry that is still on the host is refused here too"""
        P = getattr(self, "phase_period", 0)
        if (phase_pos is None) == bool(P):
            raise ValueError("music_amd.wavenet: phase_period = %d: phase_pos must be %s"
                             % (P, "None" if phase_pos is not None else "given, the stream position (>= 0) of every clip's first target"))
        if phase_pos is not None and not (torch.is_tensor(phase_pos) and phase_pos.device.type != "cpu"):
            vals = torch.as_tensor(phase_pos).reshape(-1)
            if vals.numel() and not vals.is_floating_point() and int(vals.min()) < 0:
                raise ValueError("music_amd.wavenet: a phase_pos is negative (%d): stream positions are >= 0" % int(vals.min()))

    def check_classes(self, classes):
        """classes are refused with the mode off and required with it on - before an engine is built or anything is launched"""
        n = getattr(self, "global_classes", 0)
        if (classes is None) == bool(n):
            raise ValueError("music_amd.wavenet: global_classes = %d: classes must be %s"
                             % (n, "None" if classes is not None else "given, one integer in [0, %d) per clip" % n))

    def calc_receptive_field(self):
        return (self.filter_width - 1) * (sum(self.dilations) + 1) + 1

    # ---- engine plumbing ------------------------------------------------------------------
    def _named_ref_params(self):
        """Parameters in the reference's state_dict order."""
        return list(self.named_parameters())

    def _engine_for(self, device):
        if device.type != "cuda":
            raise RuntimeError("music_amd.wavenet runs on an MI355X (ROCm) device only; there is no CPU path. "
                               "Move the module and its input to 'cuda'.")
        eng = self._engine
        named = self._named_ref_params()
        if eng is not None and eng.device == device and eng.mode_names == tuple(self.precision):
            # parameters must still alias the flat buffer (e.g. net.cpu().cuda() breaks that)
            p0 = named[0][1]
            if p0.data_ptr() == eng.flat.data_ptr() + 4 * eng.spec.off[named[0][0]]:
                return eng
        if any(p.device != device for _, p in named):
            raise RuntimeError("music_amd.wavenet: parameters and input are on different devices")
        if any(p.dtype != torch.float32 for _, p in named):
            # (.half() / .double() modules: the kernels keep float32 parameters and form fp32-grade products from 16-bit pieces,
            # DESIGN.md section 5; re-typing the module's parameters behind the caller's back would be worse than saying so)
            raise TypeError("music_amd.wavenet: parameters must be float32 (got %s)" % next(p.dtype for _, p in named if p.dtype != torch.float32))
        # the specialised kernels cover filter_width 2, 256 quantisation channels and up to 64 residual / dilation channels
        # (everything the reference ships and BASELINE.json names); any other constructor argument takes the general plan
        fast = (self.filter_width == 2 and self.quantization_channels == 256 and
                max(self.residual_channels, self.dilation_channels) <= 64)
        eng = (WaveNetEngine if fast else GenericWaveNetEngine)(
            self.dilations, self.residual_channels, self.dilation_channels, self.skip_channels,
            self.quantization_channels, self.filter_width, self.use_bias,
            mode_fwd=self.precision[0], mode_bwd=self.precision[1], device=device,
            **(dict(global_classes=self.global_classes, global_channels=self.global_channels) if self.global_classes else {}),
            **(dict(phase_period=self.phase_period) if getattr(self, "phase_period", 0) else {}))
        eng.mode_names = tuple(self.precision)
        assert [n for n, _ in named] == eng.param_names, "parameter order differs from the reference layout"
        with torch.no_grad():
            for name, p in named:
                view = eng.param_view(name)
                view.copy_(p.data)
                p.data = view                     # the module's parameters now ARE the flat buffer
        self._engine = eng
        return eng

    def forward(self, wave_sample, classes=None, phase_pos=None):
        """classes: one integer in [0, global_classes) per clip of a class-conditional model (required there), else None;
        phase_pos: the stream position of every clip's first target of a phase-conditioned model (one int for all clips, one per
        clip, or an int64 device tensor; required there), else None"""
        batch_size, original_channels, seq_len = wave_sample.size()
        output_width = seq_len - self.receptive_field + 1
        if output_width <= 0:
            raise ValueError("wave sample not long enough")
        self.check_classes(classes)
        self.check_phase(phase_pos)
        params = [p for _, p in self._named_ref_params()]
        self._last_hook = None
        out = _WaveNetFunction.apply(self, torch.is_grad_enabled(), wave_sample, classes, phase_pos, *params)
        hook, self._last_hook = self._last_hook, None
        return _losshook.wrap(out, hook) if self.fuse_loss else out


def predict_next(model, wave_var, quantization_channels=256):
    """wavenet/model.py:148-165 — argmax over the last chunk-row of the model output."""
    raw_out = model(wave_var)
    out = raw_out.view(-1, quantization_channels)
    last = out[-1, :].view(-1)
    _, predict = torch.topk(last, 1)
    return predict
