"""TransR's canonical arithmetic restated in numpy. The element-level helpers
(seq_dot, den, normalize, chain, query_vector, pred) and the Test.h rank counts are
tests/transh_restate.py's.

Every array is float32. The projection is the one FUSED chain of the project -- what the f32 MFMA
returns bit for bit -- so it needs an exact float32 fma, which numpy does not have: fma32 below.
Every other sum is a Python loop over k that starts from 0.0f with one rounding per operation.

    M_r[i][j] = transfer_matrix[r][i * dim_r + j]                               TransR.py:57
    m_j = fma(e_{dim_e-1}, M[dim_e-1][j], ... fma(e_0, M[0][j], +0.0f))        ascending i
    norm_flag: n = den(sum_j m_j m_j) (unfused), p_j = m_j / n ; r_hat = r / den(sum r_k r_k)
    else p = m, r_hat = r                                                       TransR.py:40-44
    tail batch q = p(h) + r_hat ; head batch q = -(r_hat - p(t))                TransR.py:46-49
    L1 s = s + |q_k - p(e)_k| ; L2 s = s + x x, then sqrt
    predict: s, or m - (m - s) for a model with a margin                        TransR.py:97-103
"""
import numpy as np

from transh_restate import F, chain, den, normalize, pred, query_vector, rank_counts, seq_dot  # noqa: F401

D = np.float64


def fma32(a, b, c):
    """The float32 nearest a * b + c (ties to even), one rounding, elementwise with broadcasting.
    The product of two float32 is exact in float64 (48 bits of 53). The float64 sum p + c is taken
    with a TwoSum; where it is inexact the sum is forced to ODD (the neighbour with the low
    mantissa bit set), so that the second rounding, float64 -> float32, sees on which side of a
    float32 midpoint the exact value lies: round-to-odd with 53 >= 24 + 2 bits makes the double
    rounding innocuous. (Finite values away from the float64 range limits.)"""
    a, b, c = (np.asarray(x, F).astype(D) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s, err = np.broadcast_arrays(s, err)
    s = np.array(s, D)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    if fix.any():
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s.astype(F)


def fma32_naive(a, b, c):
    """The double rounding fma32 avoids (for the test that shows the difference)."""
    a, b, c = (np.asarray(x, F).astype(D) for x in (a, b, c))
    return (a * b + c).astype(F)


def matrix(transfer_matrix, r, dim_e, dim_r):
    return np.asarray(transfer_matrix, F)[r].reshape(dim_e, dim_r)


def transfer(e, M):
    """m of entity rows e (..., dim_e) under M (dim_e, dim_r): the fused chain in ascending i."""
    e, M = np.asarray(e, F), np.asarray(M, F)
    m = np.zeros(e.shape[:-1] + (M.shape[1],), F)
    for i in range(M.shape[0]):
        m = fma32(e[..., i, None], M[i], m)
    return m


def project(e, M, norm_flag):
    """p of entity rows e under the relation whose matrix is M."""
    m = transfer(e, M)
    if not norm_flag:
        return m
    return (m / den(seq_dot(m, m))[..., None]).astype(F)


def relation_vectors(rel, norm_flag):
    return normalize(rel) if norm_flag else np.asarray(rel, F)


def score_rows(ent, rel, transfer_matrix, h, r, t, head, p_norm=1, norm_flag=True, margin=None):
    """predict of the rows (h[i], r[i], t[i]); head: the head_batch grouping h + (r - t)."""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))
    ent, rel = np.asarray(ent, F), np.asarray(rel, F)
    r_hat = relation_vectors(rel, norm_flag)
    anchor, cand = (t, h) if head else (h, t)
    out = np.zeros(len(h), F)
    for rr in np.unique(r):
        sel = np.nonzero(r == rr)[0]
        M = matrix(transfer_matrix, rr, ent.shape[1], rel.shape[1])
        pa, pc = project(ent[anchor[sel]], M, norm_flag), project(ent[cand[sel]], M, norm_flag)
        out[sel] = pred(chain(query_vector(pa, r_hat[rr], head), pc, p_norm), margin)
    return out


def sweep_scores(ent, rel, transfer_matrix, qh, qr, qt, qmode, p_norm=1, norm_flag=True, margin=None):
    """(Q, E) predictions of every query against every entity (qmode 0 = head batch)."""
    ent, rel = np.asarray(ent, F), np.asarray(rel, F)
    qh, qr, qt, qmode = (np.asarray(x, np.int64) for x in (qh, qr, qt, qmode))
    r_hat = relation_vectors(rel, norm_flag)
    out = np.zeros((len(qh), ent.shape[0]), F)
    for r in np.unique(qr):
        pe = project(ent, matrix(transfer_matrix, r, ent.shape[1], rel.shape[1]), norm_flag)   # (E, dim_r)
        for head in (True, False):
            sel = np.nonzero((qr == r) & ((qmode == 0) == head))[0]
            if not len(sel):
                continue
            anchor = qt[sel] if head else qh[sel]
            q = query_vector(pe[anchor], r_hat[r], head)  # (n, dim_r)
            out[sel] = pred(chain(q[:, None, :], pe[None, :, :], p_norm), margin)
    return out
