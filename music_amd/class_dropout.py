"""Class dropout for a class-conditional WaveNet (classifier-free guidance, Ho & Salimans 2021): the host side of training.  Each step a
clip's class is replaced by the model's ``null_class`` - the row of the existing embedding that stands for "no class" - with
probability p, so ONE model learns the conditional and the unconditional distribution and the decoder can extrapolate from the
second towards the first (``guidance=`` of fast_generate, include/wavenet_hip.h: wn_cfg_decode_batch).

``draw_null``      the draw: the stateless splitmix64 counter hash of (seed, step, global clip index) that ``vq_dropout.draw_stages``
                   uses, under a domain constant of its own - no torch RNG, nothing to checkpoint; a resumed run and any data-parallel
                   layout drop the same clips
``apply``          a batch's classes with the drawn clips set to null_class
``options``        the keys "class_dropout" / "class_dropout_seed" of train_params.json
"""
import numpy as np

try:
    from .vq_dropout import _M64, _splitmix64, _splitmix64_int
except ImportError:
    from music_amd.vq_dropout import _M64, _splitmix64, _splitmix64_int

# the draw's domain: keeps it independent of draw_stages under the same (seed, step, clip) - a model may use both ("class dr", ASCII)
_DOMAIN = 0x636C617373206472


def draw_null(seed, step, first_clip, B, p):
    """Which of the clips first_clip .. first_clip + B - 1 of global step `step` lose their class: (B,) bool, True with probability
    p.  A pure function of its arguments: clip g of step t hashes (seed, t, g) once, the word's top 53 bits are a uniform of [0, 1)."""
    seed, step, first_clip, B = int(seed), int(step), int(first_clip), int(B)
    if B < 0 or step < 0 or first_clip < 0:
        raise ValueError("music_amd.class_dropout.draw_null: B >= 0, step >= 0 and first_clip >= 0 are required")
    if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("music_amd.class_dropout.draw_null: p must lie in [0, 1], not %r" % (p,))
    clip = np.arange(first_clip, first_clip + B, dtype=np.uint64)
    key = np.uint64(_splitmix64_int(((seed & _M64) ^ _DOMAIN) ^ _splitmix64_int(step & _M64)))
    a = _splitmix64(key ^ _splitmix64(clip))
    return (a >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < float(p)


def apply(classes, null_class, seed, step, first_clip, p):
    """`classes` (B integers: a sequence, an array or a tensor) with the clips ``draw_null`` names set to null_class - a tensor comes
    back as a tensor of its dtype and device, anything else as a list of Python ints; the input is left as it is."""
    import torch
    if isinstance(classes, torch.Tensor):
        drop = torch.from_numpy(draw_null(seed, step, first_clip, classes.numel(), p)).to(classes.device)
        return torch.where(drop.view(classes.shape), torch.full_like(classes, int(null_class)), classes)
    cls = [int(c) for c in classes]
    drop = draw_null(seed, step, first_clip, len(cls), p)
    return [int(null_class) if d else c for c, d in zip(cls, drop)]


def options(train_params, null_class):
    """("class_dropout" p, "class_dropout_seed") of train_params.json, or None when unset (nothing is drawn then: every launch and
    RNG draw is that of a run without the keys).  The keys need a model with "null_class" (`null_class`: the model's, or None)."""
    p = train_params.get("class_dropout")
    if p is None:
        if train_params.get("class_dropout_seed") is not None:
            raise ValueError('train_params.json: "class_dropout_seed" needs "class_dropout"')
        return None
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError('train_params.json: "class_dropout" must be a number in [0, 1], not %r' % (p,))
    if null_class is None:
        raise ValueError('train_params.json: "class_dropout" needs "null_class" in the model\'s parameters JSON (the class that stands '
                         'for "no class")')
    seed = train_params.get("class_dropout_seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError('train_params.json: "class_dropout_seed" must be an integer, not %r' % (seed,))
    return float(p), int(seed)
