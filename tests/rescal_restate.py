"""RESCAL's canonical arithmetic restated in numpy. The exact float32 fma is
tests/transr_restate.py's (imported, not copied); the Test.h rank counts are tests/transh_restate.py's.

Every array is float32 and both chains are FUSED -- what the f32 MFMA returns bit for bit:

    M_r[i][j] = rel_matrices[r][i * d + j]                                       RESCAL.py:18-19
    tr(r,e)_i = fma(M_r[i][d-1], e_{d-1}, ... fma(M_r[i][0], e_0, +0.0f))        ascending j
    s(h,r,t)  = fma(h_{d-1}, tr(r,t)_{d-1}, ... fma(h_0, tr(r,t)_0, +0.0f))      ascending i
    forward = -s ; predict = s                                                   RESCAL.py:22, :44-46

fma(a, b, c) is symmetric in a and b, so a head-side candidate e scores sum_i e_i tr(r,t)_i and a
tail-side candidate sum_i h_i tr(r,e)_i by the same chain: one bit pattern per triple.
"""
import numpy as np

from transh_restate import F, rank_counts  # noqa: F401
from transr_restate import fma32

D = np.float64
U = 2.0 ** -24


def matrix(mats, r, d):
    return np.asarray(mats, F)[r].reshape(d, d)


def plane(ent, M):
    """tr(r, e) of entity rows e (..., d) under M (d, d): (..., d), the fused chain in ascending j."""
    e, M = np.asarray(ent, F), np.asarray(M, F)
    tr = np.zeros(e.shape[:-1] + (M.shape[0],), F)
    for j in range(M.shape[1]):
        tr = fma32(M[:, j], e[..., j, None], tr)
    return tr


def bilinear(h, tr):
    """s of rows h (..., d) against tr (..., d), broadcast: the fused chain in ascending i."""
    h, tr = np.broadcast_arrays(np.asarray(h, F), np.asarray(tr, F))
    s = np.zeros(h.shape[:-1], F)
    for i in range(h.shape[-1]):
        s = fma32(h[..., i], tr[..., i], s)
    return s


def row_scores(ent, mats, h, r, t):
    """predict (= +s) of the rows (h[i], r[i], t[i])."""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))
    ent = np.asarray(ent, F)
    out = np.zeros(len(h), F)
    for rr in np.unique(r):
        sel = np.nonzero(r == rr)[0]
        out[sel] = bilinear(ent[h[sel]], plane(ent[t[sel]], matrix(mats, rr, ent.shape[1])))
    return out


def sweep_scores(ent, mats, qh, qr, qt, mode):
    """(T, E) predictions of every query against every entity (mode 0 = head batch: the candidate
    replaces h; 1 = tail batch: it replaces t). mode: one value or one per query."""
    ent = np.asarray(ent, F)
    qh, qr, qt = (np.asarray(x, np.int64) for x in (qh, qr, qt))
    mode = np.broadcast_to(np.asarray(mode, np.int64), qh.shape)
    out = np.zeros((len(qh), ent.shape[0]), F)
    for r in np.unique(qr):
        pe = plane(ent, matrix(mats, r, ent.shape[1]))           # (E, d): this relation's plane
        for head in (True, False):
            sel = np.nonzero((qr == r) & ((mode == 0) == head))[0]
            if not len(sel):
                continue
            if head:
                out[sel] = bilinear(ent[None, :, :], pe[qt[sel]][:, None, :])
            else:
                out[sel] = bilinear(ent[qh[sel]][:, None, :], pe[None, :, :])
    return out


def gamma(n):
    return n * U / (1 - n * U)


def magnitude(ent, mats, h, r, t):
    """A = sum_i sum_j |h_i| |M_ij| |t_j| in float64, per row (h, r, t broadcast against each other;
    entity axes may be slices of the table)."""
    ent, mats = np.abs(np.asarray(ent, D)), np.abs(np.asarray(mats, D))
    d = ent.shape[1]
    h, r, t = np.broadcast_arrays(*(np.asarray(x, np.int64) for x in (h, r, t)))
    out = np.zeros(h.shape, D)
    for rr in np.unique(r):
        sel = r == rr
        out[sel] = np.einsum("ni,ij,nj->n", ent[h[sel]], mats[rr].reshape(d, d), ent[t[sel]])
    return out


def bound(d):
    """|a - b| <= bound(d) * A for two float32 evaluations a, b of the nested dot product in any
    order, fused or not: each is within gamma(2d + 1) A of the exact value (d products and d - 1
    additions per inner sum, d and d - 1 in the outer one, and the rounding of tr itself)."""
    return 2.0 * gamma(2 * d + 1)
