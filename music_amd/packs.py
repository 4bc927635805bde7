"""The weight packs of every training engine: matrices of flat-parameter offsets (-1 = zero) in the layouts the kernels multiply,
and `PackSet`, the one registrar that turns them into packed-weight index maps, gradient matrices and the gather maps back to the
parameters.

A matrix is built ONCE, by placing a weight's offsets (`_Spec.conv`) into rows and columns; everything else is derived from it: the
fragment order of its pack (pack_index), and - for a matrix that wn_wgrad or a block kernel also writes a gradient in - where every
parameter's gradient sits (an entry p at (r, c) of the matrix at offset o of the gradient pack: o + r * cols + c).  No engine computes
such an offset by hand.

The three groups of matrices the two fast engines (engine.WaveNetEngine, model1._AutoencoderEngine) share are pure functions of offset
arrays: causal_mats, gated_mats (pair_mats: their block-diagonal forms), epilogue_mats.  The engines differ in where the filter and gate
rows come from, in their names, and in the ORDER they register in - which fixes every pack's and every gradient matrix's offset.

PyTorch is used for device memory only.  Nothing here imports oracle/.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .engine_base import _pad


def pack_positions(mt, ks, chained):
    """Logical A-fragment order -> (row, k) of the effective weight matrix.
    p = ((m*ks + s)*64 + lane)*8 + j ; row = 16m + (lane&15) ; k = kmap(s, lane>>4, j)."""
    m, s, lane, j = np.indices((mt, ks, 64, 8))
    row = 16 * m + (lane & 15)
    q = lane >> 4
    if chained:
        k = 32 * s + 16 * (j >> 2) + 4 * q + (j & 3)
    else:
        k = 32 * s + 8 * q + j
    return row.reshape(-1), k.reshape(-1)


def pack_index(weff, chained=False):
    """weff: int32 [Mp, Kp] of flat-parameter offsets (-1 = zero).  Returns idx[p] (int32)."""
    mp, kp = weff.shape
    assert mp % 16 == 0 and kp % 32 == 0
    row, k = pack_positions(mp // 16, kp // 32, chained)
    return weff[row, k].astype(np.int32)


def full(m, k):
    """An [m][k] map of flat-parameter offsets, all -1 (= zero)"""
    return np.full((m, k), -1, dtype=np.int64)


def diag(m32, rb, cb):
    """m32: [rb*32][cb*32] blocks of 32 x 32 -> [rb*64][cb*64] with every block doubled on the diagonal (clip A, clip B): what the
    64-channel block kernels multiply in pair mode"""
    out = full(rb * 64, cb * 64)
    for a_ in range(rb):
        for b_ in range(cb):
            blk = m32[a_ * 32:(a_ + 1) * 32, b_ * 32:(b_ + 1) * 32]
            for c_ in range(2):
                out[a_ * 64 + c_ * 32:a_ * 64 + (c_ + 1) * 32, b_ * 64 + c_ * 32:b_ * 64 + (c_ + 1) * 32] = blk
    return out


def transposed(w):
    return np.ascontiguousarray(w.T)


# ---------------------------------------------------------------------- the matrices of the fast engines
Causal = namedtuple("Causal", "w wT taps")
Gated = namedtuple("Gated", "fg d dT fgT pq")
Epilogue = namedtuple("Epilogue", "skip skipT p1 p1T p2 p2T")


def causal_mats(wc, CH):
    """wc: [R][Q][2] -> the forward matrix (rows R, K = [tap0 Q | tap1 Q]), its transpose for the gradient w.r.t. the INPUT (input_grad:
    rows Q, K = [tap1^T over dx0[t] | tap0^T over dx0[t+1]]), and the weight re-laid as [tap][q][ch] for the forward from codes
    (wn_causal_fwd_codes): a gather map over the flat parameter buffer (-1 = padded channel, reads as 0)"""
    R, Q, _ = wc.shape
    w, wT, taps = full(CH, 2 * Q), full(Q, 2 * CH), np.full((2, Q, CH), -1, dtype=np.int64)
    w[:R, :Q], w[:R, Q:] = wc[:, :, 0], wc[:, :, 1]
    wT[:, :R], wT[:, CH:CH + R] = wc[:, :, 1].T, wc[:, :, 0].T
    taps[:, :, :R] = wc.transpose(2, 1, 0)
    return Causal(w, wT, taps.reshape(-1).astype(np.int32))


def gated_mats(wf, wg, wd, CH):
    """wf, wg: the filter's and the gate's [D][R][2], wd: the dense [R][D], all padded to CH ->
      fg    rows [f(D) pad CH | g(D) pad CH], K = [tap0 CH | tap1 CH]
      d     rows R, K = D (packed in chained k order: its B fragments come from the z accumulators);  dT: Wd^T (rows D, K = R)
      fgT   the data gradient of fg: rows R, K = [W1^T over (df|dg) | W0^T over (df|dg)]
      pq    the same weights as two UNSHIFTED row blocks for the one-launch backward block (wn_resblock_bwd_pq):
            rows [0,CH) = W1^T (-> P), rows [CH,2CH) = W0^T (-> Q), K = (df | dg)"""
    D, R, _ = wf.shape
    fg, d, fgT = full(2 * CH, 2 * CH), full(CH, CH), full(CH, 4 * CH)
    for h, src in enumerate((wf, wg)):
        fg[h * CH:h * CH + D, :R], fg[h * CH:h * CH + D, CH:CH + R] = src[:, :, 0], src[:, :, 1]
        fgT[:R, h * CH:h * CH + D], fgT[:R, 2 * CH + h * CH:2 * CH + h * CH + D] = src[:, :, 1].T, src[:, :, 0].T
    d[:R, :D] = wd
    return Gated(fg, d, transposed(d), fgT, np.concatenate([fgT[:, :2 * CH], fgT[:, 2 * CH:]]))


def pair_mats(g):
    """The four matrices of a 32-channel block that the block kernels multiply, block-diagonal for two clips side by side (rows /
    columns of a 32-block: clip A then clip B) - what the 64-channel block kernels multiply in pair mode"""
    return Gated(diag(g.fg, 2, 2), diag(g.d, 1, 1), diag(g.dT, 1, 1), None, diag(g.pq, 2, 2))


def epilogue_mats(skips, p1, p2, CH, SP):
    """skips: per block the skip conv's [S][D], p1: [S][S], p2: [Q][S] -> the skip product over the concatenated z-crops (rows S,
    K = N * CH), the two post-processing products, and their transposes"""
    S, Q = p1.shape[0], p2.shape[0]
    skip, w1, w2 = full(SP, len(skips) * CH), full(SP, SP), full(Q, SP)
    for i, ws in enumerate(skips):
        skip[:S, i * CH:i * CH + ws.shape[1]] = ws
    w1[:S, :S], w2[:, :S] = p1, p2
    return Epilogue(skip, transposed(skip), w1, transposed(w1), w2, transposed(w2))


# ---------------------------------------------------------------------- the registrar
class PackSet:
    """Collects a plan's matrices in the order given: `fwd` / `bwd` packs (name -> matrix, in launch-pack order), the gradient matrices
    (`gp_off`: name -> (offset in the gradient pack, rows, cols), same layout as the forward pack of that name) and the bias rows behind
    them (`gp_bias_off`).  A matrix may still be filled after it was registered (several weights sharing one: `matrix`); the maps are
    derived when asked for."""

    def __init__(self, total):
        self.total = total                                   # elements of the flat parameter buffer
        self.f, self.b = {}, {}                              # name -> (matrix, chained k order)
        self.gp_off, self.gp_bias_off = {}, {}
        self.go = 0                                          # running offset into the gradient pack
        self._grads, self._bias = [], []

    def fwd(self, name, w, chained=False, grad=True, pair=False):
        """A forward pack and (grad) the gradient matrix of its layout; pair: a block-diagonal matrix, every parameter twice in it"""
        self.f[name] = (w, chained)
        if grad:
            self.gp_off[name] = (self.go, w.shape[0], w.shape[1])
            self._grads.append((self.go, w, pair))
            self.go += w.size
        return w

    def bwd(self, name, w, chained=False):
        self.b[name] = (w, chained)
        return w

    def matrix(self, packs, name, m, k):
        """The [m][k] matrix `name` of `packs` (self.f / self.b), registered empty at its first mention"""
        if name not in packs:
            (self.fwd if packs is self.f else self.bwd)(name, full(m, k))
        return packs[name][0]

    def epilogue(self, e, skip, p1, p2, chained_fwd):
        """The epilogue's three weights under the user's names: forward (+ "<name>c", chained k order: the fused forward epilogue
        takes relu(U) out of the accumulators), transposed, and "<name>Tc" for the fused backward epilogue"""
        self.fwd(skip, e.skip)
        self.bwd(skip + "T", e.skipT)
        self.bwd(skip + "Tc", e.skipT, chained=True)
        self.fwd(p1, e.p1)
        self.bwd(p1 + "T", e.p1T)
        self.bwd(p1 + "Tc", e.p1T, chained=True)
        if chained_fwd:
            self.fwd(p1 + "c", e.p1, chained=True, grad=False)
        self.fwd(p2, e.p2)
        if chained_fwd:
            self.fwd(p2 + "c", e.p2, chained=True, grad=False)
        self.bwd(p2 + "T", e.p2T)

    def bias(self, name, off, n, row_map=None, reserve=None):
        """Rows of the gradient pack for the bias `name` (n elements at `off` of the flat buffer; padded to 4).  row_map: gradient row
        of bias row r, with `reserve` rows - a bias whose gradient wn_bias_grad writes in another row order than the parameter's"""
        self.gp_bias_off[name] = self.go
        self._bias.append((off, self.go + (np.arange(n) if row_map is None else row_map)))
        self.go += _pad(n, 4) if reserve is None else reserve

    def gather_maps(self):
        """(gidx, gidx_pa, gidx_pb): flat parameter element -> offset in the gradient pack (-1: none); pair mode: a stack weight's
        gradient is the sum of its two copies in the block-diagonal matrix (wn_gather_grads2), A and B, everything else as in gidx"""
        gidx, ga, gb = (np.full(self.total, -1, dtype=np.int64) for _ in range(3))
        for o, w, pair in self._grads:
            r, c = np.nonzero(w >= 0)
            par, pos = w[r, c], o + r * w.shape[1] + c
            if pair:                                         # row-major: a parameter's copy of clip A comes first, clip B's last
                ga[par[::-1]], gb[par] = pos[::-1], pos
            else:
                gidx[par] = pos
        for off, rows in self._bias:
            gidx[off:off + len(rows)] = rows
        ga = np.where(ga >= 0, ga, gidx)
        return gidx, ga, gb

    def finish(self, packs, mode, device):
        """packs (self.f / self.b) -> (offset of every pack in halfs of the packed buffer, all index maps as one tensor, the packed buffer)"""
        halfs_per_frag = 1024 if mode in (_lib.F16X3, _lib.BF16X3) else 512
        offs, idx, o = {}, [], 0
        for name, (w, chained) in packs.items():
            offs[name] = o * halfs_per_frag // 512
            idx.append(pack_index(w, chained))
            o += len(idx[-1])
        idx_all = torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(device)
        return offs, idx_all, torch.zeros(o * halfs_per_frag // 512, dtype=torch.int16, device=device)
