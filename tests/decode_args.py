"""The argument list of the decode entry points (include/wavenet_hip.h), once, for the CPU checks of their refusals: every
entry takes a slice of it.  Pointers are never dereferenced by a refused call."""
import ctypes

P = 1 << 20            # "some non-NULL address"
_KEEP = []             # the host arrays of the last argument list stay alive
# (first, one past the last) argument of the full list each entry takes, before the stream
ARITY = {"wn_decode": (1, 29), "wn_decode_batch": (1, 33), "wn_decode_batch_pk": (1, 40), "wn_decode_batch_fw": (0, 40),
         "wn_decode_batch_cond": (0, 48), "wn_decode_batch_samp": (0, 51)}


def decode_args(entry, **over):
    """Arguments of a small valid conditioned call of `entry` (stream last), with `over` replacing single arguments by name."""
    dil = (ctypes.c_int32 * 2)(1, 2)
    qoff = (ctypes.c_int64 * 2)(0, 64)
    shift = (ctypes.c_int32 * 3)(2, 0, 0)
    cq = (ctypes.c_int32 * 3)(0, 5, 0)
    _KEEP[:] = [dil, qoff, shift, cq]
    a = dict(filter_width=2, n_layers=2, R=32, D=32, S=64, Q=256, dil=ctypes.cast(dil, ctypes.c_void_p),
             qoff=ctypes.cast(qoff, ctypes.c_void_p), queues=P, w_causal=P, b_causal=None, w_layers=P, layer_stride=4096,
             b_layers=None, w_p1=P, b_p1=None, w_p2=P, b_p2=None, note0=P, prev0=P, note_out=P, prev_out=P, forced=None,
             codes_out=P, probs_out=None, step0=0, n_steps=4, push_input=1, sync=P, n_utt=1, queues_ustride=0,
             temperature=0.0, seed=0, pk=None, pk_fg0=0, pk_d0=0, pk_lstride=0, pk_skip=-1, pk_p1=-1, pk_p2=-1,
             cond_fg=P, cond_fg_ustride=2 * 3 * 64, cond_p1=P, cond_p1_ustride=3 * 64,
             c_shift=ctypes.cast(shift, ctypes.c_void_p), c_q=ctypes.cast(cq, ctypes.c_void_p), le=3, pos0=-3,
             samp=None, top_k=0, top_p=1.0)
    unknown = set(over) - set(a) - {"stream"}
    assert not unknown, unknown
    a.update(over)
    lo, hi = ARITY[entry]
    return list(a.values())[lo:hi] + [over.get("stream")]
