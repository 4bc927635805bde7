"""float64 torch restatement of the class-conditional WaveNet (music_amd/model.py with global_classes > 0; WaveNet paper section 2.5):
clip b of class c gets, constant over time,
    [f; g]_i[b][:, t] += G_i emb[c]     in every block   (rows of G_i: gate first, then filter)
    h[b][:, t]        += G_f emb[c]     on the output of post_process_1, in front of its ReLU
Forward to the logits, both objectives' losses, autograd gradients, the per-timestep probabilities (with position windows) and a
greedy roll-out.  tests/test_class_cond_cpu.py holds it to the oracle's WaveNet with the class terms folded into biases."""
from collections import OrderedDict

import torch
import torch.nn.functional as F


def receptive_field(filter_width, dilations):
    return (filter_width - 1) * (sum(dilations) + 1) + 1


def _b(params, name):
    return params.get(name + ".bias", None)


def global_block(params, n_blocks):
    """(G_0 .. G_N-1 as (2D, E), G_f (S, E), embedding (n, E))"""
    return ([params["gcond_layer_stack.%d.weight" % i][:, :, 0] for i in range(n_blocks)], params["connection_gcond.weight"][:, :, 0],
            params["global_embedding.weight"])


def logits(params, dilations, x, classes, filter_width=2):
    """x (B, Q, T), classes (B,) int64 -> pre-softmax (B, Q, W)"""
    out_w = x.size(2) - receptive_field(filter_width, dilations) + 1
    if out_w <= 0:
        raise ValueError("wave sample not long enough")
    G, Gf, emb = global_block(params, len(dilations))
    v = emb[classes]                                                   # (B, E)
    D = G[0].shape[0] // 2
    h = F.conv1d(x, params["causal_layer.weight"], _b(params, "causal_layer"))
    skip = None
    for i, d in enumerate(dilations):
        n = "dilation_layer_stack.%d"
        c = v @ G[i].t()                                               # (B, 2D): gate rows first
        f = F.conv1d(h, params[n % (4 * i) + ".weight"], _b(params, n % (4 * i)), dilation=d) + c[:, D:, None]
        g = F.conv1d(h, params[n % (4 * i + 1) + ".weight"], _b(params, n % (4 * i + 1)), dilation=d) + c[:, :D, None]
        z = torch.sigmoid(g) * torch.tanh(f)
        dense = F.conv1d(z, params[n % (4 * i + 2) + ".weight"], _b(params, n % (4 * i + 2)))
        h = dense + h[:, :, -dense.size(2):]
        s = F.conv1d(z[:, :, -out_w:], params[n % (4 * i + 3) + ".weight"], _b(params, n % (4 * i + 3)))
        skip = s if skip is None else skip + s
    h1 = F.conv1d(F.relu(skip), params["post_process_1.weight"], _b(params, "post_process_1")) + (v @ Gf.t())[:, :, None]
    return F.conv1d(F.relu(h1), params["post_process_2.weight"], _b(params, "post_process_2"))


def chunk_probs(lg):
    """the module's output: the reference's chunk softmax of the (B, Q, W) buffer viewed (-1, Q)"""
    return F.softmax(lg.contiguous().view(-1, lg.size(1)), dim=1)


def _window_mask(Q, W, B, windows, window_pos, like):
    """(B, W, Q) bool: inside the (lo, hi) pair of stream position window_pos[b] + w; all True without windows"""
    if windows is None:
        return torch.ones(B, W, Q, dtype=torch.bool)
    pos0 = [0] * B if window_pos is None else ([int(window_pos)] * B if isinstance(window_pos, int) else [int(p) for p in window_pos])
    q = torch.arange(Q)
    m = torch.zeros(B, W, Q, dtype=torch.bool)
    for b in range(B):
        for w in range(W):
            lo, hi = windows[(pos0[b] + w) % len(windows)]
            m[b, w] = (q >= lo) & (q < hi)
    return m


def step_probs(lg, windows=None, window_pos=None):
    """(B W, Q): softmax over the Q logits of every output column, inside the column's window (an exact 0 outside)"""
    B, Q, W = lg.shape
    m = _window_mask(Q, W, B, windows, window_pos, lg)
    x = lg.permute(0, 2, 1).masked_fill(~m, float("-inf"))
    return F.softmax(x, dim=2).reshape(B * W, Q)


def loss(params, dilations, x, target, classes, objective="reference", filter_width=2, windows=None, window_pos=None):
    lg = logits(params, dilations, x, classes, filter_width)
    if objective == "reference":                                       # CrossEntropyLoss on the chunk-softmax probabilities
        return F.cross_entropy(chunk_probs(lg), target.reshape(-1)), lg
    p = step_probs(lg, windows, window_pos)
    return -torch.log(p.gather(1, target.reshape(-1, 1))).mean(), lg


def loss_and_grads(params, dilations, x, target, classes, **kw):
    """(loss, logits, OrderedDict name -> gradient) on float64 copies of params"""
    leaf = OrderedDict((k, v.detach().double().clone().requires_grad_(True)) for k, v in params.items())
    val, lg = loss(leaf, dilations, x.double(), target, classes, **kw)
    grads = torch.autograd.grad(val, list(leaf.values()), allow_unused=True)
    return val.detach(), lg.detach(), OrderedDict((k, g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(leaf, grads))


def greedy_rollout(params, dilations, seed_codes, classes, n_steps, Q, filter_width=2, windows=None, pos0=0):
    """Free-running argmax decode in float64, one full forward per step: seed_codes (U, rf) int64 -> (codes (U, n_steps), the
    smallest top-2 logit margin met).  windows: the argmax of step n is taken inside the pair of position pos0 + n."""
    p64 = {k: v.detach().double() for k, v in params.items()}
    rf = receptive_field(filter_width, dilations)
    hist, out, margin = seed_codes.clone(), [], float("inf")
    for n in range(n_steps):
        x = F.one_hot(hist[:, -rf:], Q).permute(0, 2, 1).double()
        lg = logits(p64, dilations, x, classes, filter_width)[:, :, -1]                  # (U, Q)
        if windows is not None:
            lo, hi = windows[(pos0 + n) % len(windows)]
            mask = torch.full((Q,), float("-inf"), dtype=torch.float64)
            mask[lo:hi] = 0.0
            lg = lg + mask
        top = lg.topk(2, dim=1).values
        margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
        code = lg.argmax(1)
        out.append(code)
        hist = torch.cat([hist, code[:, None]], 1)
    return torch.stack(out, 1), margin


# ---------------------------------------------------------------------- the greedy roll-out cases of the decode tests
# Both decode kernel families: the matrix-core decoder (64 / 64 / 256 channels, Q = 256) and the fp32 kernel (Q = 100, the
# general plan).  tests/test_class_cond_cpu.py holds every step's float64 top-2 logit margin above 1e-4, so that a float32
# decoder within the project's bar picks the same code.
DECODE_CASES = {
    "mfma": dict(cfg=dict(filter_width=2, dilations=[1, 2, 4], dilation_channels=64, residual_channels=64, skip_channels=256,
                          quantization_channels=256, use_bias=False, global_classes=5, global_channels=7),
                 seed=11, classes=[3, 0, 3], steps=12),
    "fp32": dict(cfg=dict(filter_width=2, dilations=[1, 2, 4], dilation_channels=16, residual_channels=16, skip_channels=32,
                          quantization_channels=100, use_bias=True, global_classes=3, global_channels=64),
                 seed=12, classes=[2, 1, 2], steps=12),
}


def build(cfg, seed, scale=3.0):
    """music_amd.model.wavenet(**cfg) on the CPU under `seed`, every parameter scaled (default initialisation gives logits too flat
    for a margin)"""
    from music_amd.model import wavenet
    torch.manual_seed(seed)
    net = wavenet(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    return net


def seed_codes(U, n, Q, seed):
    return torch.randint(0, Q, (U, n), generator=torch.Generator().manual_seed(seed))
