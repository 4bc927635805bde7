"""float64 restatement of wn_gclass_fwd / wn_gclass_bwd (include/wavenet_hip.h): the tables of a class-conditional WaveNet - the
global class term of the conditioning projections alone, one column per clip - and their backward.  Rows of G_i come in the
reference's order (gate rows [0, Dd), filter rows [Dd, 2 Dd)); a class outside [0, n_cls) makes its clip NaN and is never an index.
Every function also returns the forward-error bound gamma(terms) * sum |a| |b| of its sums (valid for any summation order)."""
import numpy as np

U = 2.0 ** -24


def gamma(K):
    return (K + 2) * U / (1 - (K + 2) * U)


def class_vectors(emb, cls, n_cls):
    """(B, E) float64 embedding rows of the clips, NaN rows where the class lies outside [0, n_cls)"""
    emb, cls = np.asarray(emb, dtype=np.float64), np.asarray(cls)
    ok = (cls >= 0) & (cls < n_cls)
    return np.where(ok[:, None], emb[np.where(ok, cls, 0)], np.nan), ok


def gclass_fwd(G, Gf, emb, cls):
    """G (N, 2Dd, E), Gf (Sd, E), emb (n_cls, E), cls (B,) -> en (N, B, 2Dd), enf (B, Sd), and their bounds"""
    G, Gf = np.asarray(G, dtype=np.float64), np.asarray(Gf, dtype=np.float64)
    v, _ = class_vectors(emb, cls, len(emb))
    av, gm = np.abs(np.nan_to_num(v)), gamma(G.shape[2])
    en, enf = np.einsum("nce,be->nbc", G, v), np.einsum("ce,be->bc", Gf, v)
    return en, enf, gm * np.einsum("nce,be->nbc", np.abs(G), av), gm * np.einsum("ce,be->bc", np.abs(Gf), av)


def gclass_bwd(G, Gf, emb, cls, d_en, d_enf):
    """d_en (N, B, 2Dd), d_enf (B, Sd) -> (dG, dGf, d_emb), their bounds, and the number of clips of every class"""
    G, Gf, d_en, d_enf = (np.asarray(a, dtype=np.float64) for a in (G, Gf, d_en, d_enf))
    n_cls, B, R = len(emb), d_en.shape[1], G.shape[0] * G.shape[1] + Gf.shape[0]
    v, ok = class_vectors(emb, cls, n_cls)
    av, gk = np.abs(np.nan_to_num(v)), gamma(B)
    dG, dGf = np.einsum("nbc,be->nce", d_en, v), np.einsum("bc,be->ce", d_enf, v)
    dG_b, dGf_b = gk * np.einsum("nbc,be->nce", np.abs(d_en), av), gk * np.einsum("bc,be->ce", np.abs(d_enf), av)
    per_clip = np.einsum("nce,nbc->be", G, d_en) + np.einsum("ce,bc->be", Gf, d_enf)
    per_clip_abs = np.einsum("nce,nbc->be", np.abs(G), np.abs(d_en)) + np.einsum("ce,bc->be", np.abs(Gf), np.abs(d_enf))
    demb, demb_b = np.zeros((n_cls, G.shape[2])), np.zeros((n_cls, G.shape[2]))
    cls = np.asarray(cls)
    for b in range(B):
        if ok[b]:
            demb[cls[b]] += per_clip[b]
            demb_b[cls[b]] += per_clip_abs[b]
    count = np.bincount(cls[ok], minlength=n_cls)
    demb_b *= np.array([gamma(int(c) * R) for c in count])[:, None]
    return (dG, dGf, demb), (dG_b, dGf_b, demb_b), count


def table(en, CH, pair, fill):
    """en (N, B, 2Dd) in the reference's row order -> the block table [N][tensors][rows] (le = 1) of include/wavenet_hip.h: per clip
    (rows 2 CH: filter rows, then gate rows at CH) or as clip pairs (rows 4 CH); every other row = fill"""
    N, B, Dd = en.shape[0], en.shape[1], en.shape[2] // 2
    rows, nt = (4 * CH, B // 2) if pair else (2 * CH, B)
    tab = np.full((N, nt, rows), fill, dtype=en.dtype)
    for b in range(B):
        t, h = (b >> 1, b & 1) if pair else (b, 0)
        tab[:, t, h * CH:h * CH + Dd] = en[:, b, Dd:]
        g0 = (2 * CH if pair else CH) + h * CH
        tab[:, t, g0:g0 + Dd] = en[:, b, :Dd]
    return tab
