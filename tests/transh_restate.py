"""TransH's canonical arithmetic restated in numpy, and the Test.h rank counts.

Every array is float32 and every sum is a Python loop over k that starts from 0.0f, so each
chain is sequential in ascending k with one rounding per operation (numpy's float32 multiply, add,
subtract, divide and sqrt are the IEEE ones; nothing is fused). Vectorised over rows only.

    w_hat = w / max(sqrt(sum w_k w_k), 1e-12)                       TransH.py:69
    a = sum e_k w_hat_k ; p_k = e_k - a w_hat_k                      TransH.py:73-76
    norm_flag: n = max(sqrt(sum p_k p_k), 1e-12), p_hat = p / n ; r_hat = r / max(|r|, 1e-12)
    tail batch q = p_hat(h) + r_hat ; head batch q = -(r_hat - p_hat(t))
    L1 s = s + |q_k - p_hat(e)_k| ; L2 s = s + x x, then sqrt
    predict: s, or m - (m - s) for a model with a margin            TransH.py:109-115
"""
import numpy as np

F = np.float32
EPS = F(1e-12)


def seq_dot(x, y):
    """sum_k x[..., k] * y[..., k], sequential in k from 0.0f (multiply, then add)."""
    x, y = np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F))
    s = np.zeros(x.shape[:-1], F)
    for k in range(x.shape[-1]):
        s = s + x[..., k] * y[..., k]
    return s


def den(ss):
    return np.maximum(np.sqrt(ss.astype(F)), EPS).astype(F)


def normalize(x):
    x = np.asarray(x, F)
    return (x / den(seq_dot(x, x))[..., None]).astype(F)


def project(e, w_hat, norm_flag):
    """p_hat of entity rows e (..., d) on the hyperplane of w_hat (broadcast against e)."""
    e = np.asarray(e, F)
    w_hat = np.asarray(w_hat, F)
    a = seq_dot(e, w_hat)
    p = (e - a[..., None] * w_hat).astype(F)
    if not norm_flag:
        return p
    return (p / den(seq_dot(p, p))[..., None]).astype(F)


def chain(q, p, p_norm):
    """The score chain over k of q (..., d) against p (..., d)."""
    q, p = np.broadcast_arrays(np.asarray(q, F), np.asarray(p, F))
    s = np.zeros(q.shape[:-1], F)
    for k in range(q.shape[-1]):
        x = q[..., k] - p[..., k]
        s = s + (np.abs(x) if p_norm == 1 else x * x)
    return np.sqrt(s).astype(F) if p_norm == 2 else s


def pred(s, margin):
    if margin is None:
        return s
    m = F(margin)
    return (m - (m - s)).astype(F)


def relation_vectors(rel, norm_vec, norm_flag):
    """(w_hat, r_hat) tables."""
    return normalize(norm_vec), (normalize(rel) if norm_flag else np.asarray(rel, F))


def query_vector(pa, rh, head):
    return (-(rh - pa)).astype(F) if head else (pa + rh).astype(F)


def score_rows(ent, rel, norm_vec, h, r, t, head, p_norm=1, norm_flag=True, margin=None):
    """predict of the rows (h[i], r[i], t[i]); head: the head_batch grouping h + (r - t)."""
    h, r, t = (np.asarray(x, np.int64) for x in (h, r, t))
    w_hat, r_hat = relation_vectors(rel, norm_vec, norm_flag)
    ent = np.asarray(ent, F)
    anchor, cand = (t, h) if head else (h, t)
    pa = project(ent[anchor], w_hat[r], norm_flag)
    pc = project(ent[cand], w_hat[r], norm_flag)
    return pred(chain(query_vector(pa, r_hat[r], head), pc, p_norm), margin)


def sweep_scores(ent, rel, norm_vec, qh, qr, qt, qmode, p_norm=1, norm_flag=True, margin=None):
    """(Q, E) predictions of every query against every entity (qmode 0 = head batch)."""
    ent = np.asarray(ent, F)
    qh, qr, qt, qmode = (np.asarray(x, np.int64) for x in (qh, qr, qt, qmode))
    w_hat, r_hat = relation_vectors(rel, norm_vec, norm_flag)
    out = np.zeros((len(qh), ent.shape[0]), F)
    for r in np.unique(qr):
        pe = project(ent, w_hat[r], norm_flag)          # (E, d): this relation's projected table
        for head in (True, False):
            sel = np.nonzero((qr == r) & ((qmode == 0) == head))[0]
            if not len(sel):
                continue
            anchor = qt[sel] if head else qh[sel]
            q = query_vector(pe[anchor], r_hat[r], head)  # (n, d)
            out[sel] = pred(chain(q[:, None, :], pe[None, :, :], p_norm), margin)
    return out


def rank_counts(scores, truth, known=None, allowed=None):
    """Test.h:65-192 for one batch of queries: (4, Q) int64 = raw, filt, raw_tc, filt_tc counts of
    entities j != truth with score[j] < score[truth] (strict: ties favour the truth, Test.h:83).
    known: per query, the entity ids the filter skips (_find, Test.h:85); allowed: (Q, E) bool,
    the type constraint of the query's relation and side (Test.h:88-98) or None."""
    scores = np.asarray(scores)
    Q, E = scores.shape
    out = np.zeros((4, Q), np.int64)
    for i in range(Q):
        tr = int(truth[i])
        beat = scores[i] < scores[i, tr]
        beat[tr] = False
        keep = np.ones(E, bool)
        if known is not None:
            k = np.asarray(known[i], np.int64)
            keep[k[(k >= 0) & (k < E)]] = False
        out[0, i] = beat.sum()
        out[1, i] = (beat & keep).sum()
        if allowed is not None:
            out[2, i] = (beat & allowed[i]).sum()
            out[3, i] = (beat & keep & allowed[i]).sum()
    return out
