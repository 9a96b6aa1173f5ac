"""TransD's canonical arithmetic restated in numpy. The element-level helpers
(seq_dot, den, normalize, chain, query_vector, pred) and the Test.h rank counts are
tests/transh_restate.py's: the two models share them by construction.

Every array is float32 and every sum is a Python loop over k that starts from 0.0f, so each
chain is sequential in ascending k with one rounding per operation. Vectorised over rows only.

    s(e) = sum_{k < dim_e} e_k ep_k ; a = -s                          TransD.py:100
    u_k = e_k - a rp_k, k < dim_r (the first dim_r values of e)       TransD.py:62-68, :100
    n1 = den(sum u_k u_k)                                              TransD.py:99-103
    norm_flag: n2 = den(sum (u_k / n1)(u_k / n1)), N = n1 * n2 ; else N = n1     TransD.py:79-82
    p_k = u_k / N  (ONE division per element)
    r_hat = r / den(sum r_k r_k) with norm_flag, else r
    tail batch q = p(h) + r_hat ; head batch q = -(r_hat - p(t))      TransD.py:87-90
    L1 s = s + |q_k - p(e)_k| ; L2 s = s + x x, then sqrt
    predict: s, or m - (m - s) for a model with a margin              TransD.py:149-155
"""
import numpy as np

from transh_restate import F, chain, den, normalize, pred, query_vector, rank_counts, seq_dot  # noqa: F401


def transfer_s(ent, ent_transfer):
    """s(e) of every row, over the whole dim_e."""
    return seq_dot(np.asarray(ent, F), np.asarray(ent_transfer, F))


def a_and_n(e, s, rp, norm_flag):
    """(a, N) of entity rows e (..., dim_e) with their s (...) under the raw transfer row rp
    (dim_r,), and u (..., dim_r)."""
    rp = np.asarray(rp, F)
    a = (-np.asarray(s, F)).astype(F)
    u = (np.asarray(e, F)[..., :rp.shape[-1]] - a[..., None] * rp).astype(F)
    n1 = den(seq_dot(u, u))
    if not norm_flag:
        return a, n1, u
    v = (u / n1[..., None]).astype(F)
    return a, (n1 * den(seq_dot(v, v))).astype(F), u


def project(e, s, rp, norm_flag):
    """p of entity rows e under the relation whose raw transfer row is rp."""
    _, n, u = a_and_n(e, s, rp, norm_flag)
    return (u / n[..., None]).astype(F)


def relation_vectors(rel, norm_flag):
    return normalize(rel) if norm_flag else np.asarray(rel, F)


def score_rows(ent, ent_transfer, rel, rel_transfer, h, r, t, head, p_norm=1, norm_flag=True, margin=None):
    """predict of the rows (h[i], r[i], t[i]); head: the head_batch grouping h + (r - t)."""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))
    ent, ept, rpt = np.asarray(ent, F), np.asarray(ent_transfer, F), np.asarray(rel_transfer, F)
    r_hat = relation_vectors(rel, norm_flag)
    anchor, cand = (t, h) if head else (h, t)
    out = np.zeros(len(h), F)
    for rr in np.unique(r):
        sel = np.nonzero(r == rr)[0]
        pa = project(ent[anchor[sel]], transfer_s(ent[anchor[sel]], ept[anchor[sel]]), rpt[rr], norm_flag)
        pc = project(ent[cand[sel]], transfer_s(ent[cand[sel]], ept[cand[sel]]), rpt[rr], norm_flag)
        out[sel] = pred(chain(query_vector(pa, r_hat[rr], head), pc, p_norm), margin)
    return out


def sweep_scores(ent, ent_transfer, rel, rel_transfer, qh, qr, qt, qmode, p_norm=1, norm_flag=True, margin=None):
    """(Q, E) predictions of every query against every entity (qmode 0 = head batch)."""
    ent, rpt = np.asarray(ent, F), np.asarray(rel_transfer, F)
    qh, qr, qt, qmode = (np.asarray(x, np.int64) for x in (qh, qr, qt, qmode))
    r_hat = relation_vectors(rel, norm_flag)
    s = transfer_s(ent, ent_transfer)
    out = np.zeros((len(qh), ent.shape[0]), F)
    for r in np.unique(qr):
        pe = project(ent, s, rpt[r], norm_flag)          # (E, dim_r): this relation's projected table
        for head in (True, False):
            sel = np.nonzero((qr == r) & ((qmode == 0) == head))[0]
            if not len(sel):
                continue
            anchor = qt[sel] if head else qh[sel]
            q = query_vector(pe[anchor], r_hat[r], head)  # (n, dim_r)
            out[sel] = pred(chain(q[:, None, :], pe[None, :, :], p_norm), margin)
    return out
