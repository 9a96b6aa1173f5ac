"""Python restatements of triple classification, shared by test_tripleclass_cpu.py and
test_tripleclass_gpu.py (not a test module).

neg_test: getNegTest (Test.h:399-409) with Corrupt.h:7-83 and Random.h:18-29 in Python integers,
line for line, plus the one pinned rule: a kept entity that never occurs on that side of a train
triple draws rand_max(E - 2) and returns the draw unchanged (the reference reads row -1 there).
search / counts_at / accuracy: the threshold rule of include/mmre.h in numpy.
"""
import numpy as np

MASK64 = (1 << 64) - 1


def lcg_next(s):
    return (s * 25214903917 + 11) & MASK64


def _corrupt(T, val, lef, rig, n_ent, state, e, r):
    """corrupt_head (T = trainHead, val = column t) / corrupt_tail (T = trainTail, val = column h):
    returns (replacement, state). T rows are (h, r, t)."""
    state = lcg_next(state)
    if rig[e] < lef[e]:                       # absent: ll = -1, rr = 0 in the reference
        return state % (n_ent - 2), state
    lo, hi = lef[e] - 1, rig[e]
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if T[mid][1] >= r:
            hi = mid
        else:
            lo = mid
    ll = hi
    lo, hi = lef[e], rig[e] + 1
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if T[mid][1] <= r:
            lo = mid
        else:
            hi = mid
    rr = lo
    tmp = state % (n_ent - (rr - ll + 1))
    if tmp < T[ll][val]:
        return tmp, state
    if tmp > T[rr][val] - rr + ll - 1:
        return tmp + rr - ll + 1, state
    lo, hi = ll, rr + 1
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if T[mid][val] - mid + ll - 1 < tmp:
            lo = mid
        else:
            hi = mid
    return tmp + lo - ll + 1, state


def neg_test(index, test_h, test_r, test_t, state):
    """(neg_h, neg_t, coin, absent, state_after) for a mmre.data.TrainIndex and a test list."""
    head, tail = index.head_hrt.tolist(), index.tail_hrt.tolist()
    lh, rh, lt, rt = (x.tolist() for x in (index.lef_head, index.rig_head, index.lef_tail, index.rig_tail))
    n = len(test_h)
    nh, nt = np.array(test_h, np.int64), np.array(test_t, np.int64)
    coin, absent = np.zeros(n, bool), np.zeros(n, bool)
    state = int(state)
    for i in range(n):
        h, r, t = int(test_h[i]), int(test_r[i]), int(test_t[i])
        state = lcg_next(state)
        coin[i] = state % 1000 < 500
        if coin[i]:
            absent[i] = rh[h] < lh[h]
            nt[i], state = _corrupt(head, 2, lh, rh, index.n_ent, state, h, r)
        else:
            absent[i] = rt[t] < lt[t]
            nh[i], state = _corrupt(tail, 0, lt, rt, index.n_ent, state, t, r)
    return nh, nt, coin, absent, state


def counts_at(pos, neg, thr):
    """(P, A, n_nan) at a threshold: NaN scores are never <= it."""
    pos, neg = np.asarray(pos, np.float32), np.asarray(neg, np.float32)
    with np.errstate(invalid="ignore"):
        P = int((pos <= np.float32(thr)).sum())
        A = P + int((neg <= np.float32(thr)).sum())
    return P, A, int(np.isnan(pos).sum() + np.isnan(neg).sum())


def search(pos, neg):
    """(threshold, P, A, n_nan): the smallest candidate among those maximising 2 P - A, candidates
    being the non-NaN scores; (nan, 0, 0, n_nan) without one."""
    pos, neg = np.asarray(pos, np.float32).reshape(-1), np.asarray(neg, np.float32).reshape(-1)
    n_nan = int(np.isnan(pos).sum() + np.isnan(neg).sum())
    ps, ns = np.sort(pos[~np.isnan(pos)]), np.sort(neg[~np.isnan(neg)])
    cands = np.unique(np.concatenate([ps, ns]) + np.float32(0.0))      # ascending; -0 is +0
    if len(cands) == 0:
        return float("nan"), 0, 0, n_nan
    P = np.searchsorted(ps, cands, side="right")
    N = np.searchsorted(ns, cands, side="right")
    best = int(np.argmax(2 * P - (P + N)))                               # the first maximum
    return float(cands[best]), int(P[best]), int(P[best] + N[best]), n_nan


def accuracy(P, A, n_pos, n_neg):
    """(2 P + F - A) / T in Python floats, as Tester.py:108 / :146 evaluate it."""
    return (2 * float(P) + float(n_neg) - A) / float(n_pos + n_neg)
