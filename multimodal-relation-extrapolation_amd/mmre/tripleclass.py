"""Triple classification engine (csrc/tripleclass.hip).

Replaces the reference's path (OpenKE/openke/config/Tester.py:93-151 over Base.so's getTestBatch,
Test.h:393-422): one corrupted copy of every test triple from thread 0's LCG, bit-exact with
Base.so; model.predict on the positive and the negative rows; the threshold that separates the
two score sets best, found without a sort. `evaluate_triple_classification` enqueues all three
stages in one call (mmre_tc_evaluate); the accuracy is formed on the host in double, which is the
reference's Python float. The pinned semantics (ties, NaN, no score above the threshold, a kept
entity absent from train) are stated at the entry points in include/mmre.h.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .data import TrainIndex
from .link import MODEL_IDS, ScoreSpec

INDEX_KEYS = ("head_hrt", "tail_hrt", "lef_head", "rig_head", "lef_tail", "rig_tail")


def device_index(index: TrainIndex, device):
    """The six train-index arrays the corruption reads, on `device`, with the two sizes."""
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(index, k))).to(device) for k in INDEX_KEYS}
    d["n_ent"], d["train_total"] = index.n_ent, index.train_total
    return d


def advance_state(seed_state: int, n_test: int) -> int:
    """Thread 0's state after one getNegTest over n_test triples (two draws each)."""
    return int(_lib.lib().mmre_tc_advance(int(seed_state) & (2 ** 64 - 1), int(n_test)))


def _i64(x, dev):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int64)))
    return t.to(dev).to(torch.int64).contiguous()


def _f32(x, dev):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    return t.detach().to(dev).float().contiguous().reshape(-1)


def classification_negatives(index, test_h, test_r, test_t, seed_state: int, device=None):
    """getNegTest (Test.h:399-409) on the GPU: (neg_h, neg_t) int64 device tensors for the test
    triples in the order given (testList order for Base.so's list); the negative's relation is the
    positive's. seed_state: thread 0's state before the call; the state after it is
    advance_state(seed_state, n). Enqueues only."""
    dev = torch.device(device) if device is not None else (
        test_h.device if isinstance(test_h, torch.Tensor) and test_h.is_cuda else torch.device("cuda:0"))
    d = device_index(index, dev)
    h, r, t = (_i64(x, dev) for x in (test_h, test_r, test_t))
    n = int(h.shape[0])
    neg_h = torch.empty(n, dtype=torch.int64, device=dev)
    neg_t = torch.empty(n, dtype=torch.int64, device=dev)
    call("mmre_tc_negatives", *(ptr(d[k]) for k in INDEX_KEYS), int(d["train_total"]), int(d["n_ent"]), ptr(h),
         ptr(r), ptr(t), n, int(seed_state) & (2 ** 64 - 1), ptr(neg_h), ptr(neg_t), stream_ptr(dev))
    return neg_h, neg_t


def _tables(spec: ScoreSpec):
    _lib.require_cuda(spec.ent, spec.rel, spec.ent_im, spec.rel_im)
    c = lambda x: None if x is None else x.detach().contiguous().float()
    return c(spec.ent), c(spec.rel), c(spec.ent_im), c(spec.rel_im)


def _model_args(spec, ent, rel, ent_im, rel_im):
    return (MODEL_IDS[spec.model], int(bool(spec.norm_flag)), int(spec.pred_kind), float(spec.margin), ptr(ent),
            ptr(ent_im), ptr(rel), ptr(rel_im), int(ent.shape[0]), int(rel.shape[0]), int(spec.dim),
            float(spec.phase_denom))


def classification_scores(spec: ScoreSpec, pos_h, pos_r, pos_t, neg_h, neg_t, neg_r=None):
    """model.predict ('normal' mode) of the positive rows and of the negative rows, bit for bit
    (mmre_tc_scores): two float32 device tensors. neg_r None: the positives' relations."""
    ent, rel, ent_im, rel_im = _tables(spec)
    dev = ent.device
    ph, pr, pt, nh, nt = (_i64(x, dev) for x in (pos_h, pos_r, pos_t, neg_h, neg_t))
    nr = None if neg_r is None else _i64(neg_r, dev)
    n = int(ph.shape[0])
    pos = torch.empty(n, dtype=torch.float32, device=dev)
    neg = torch.empty(n, dtype=torch.float32, device=dev)
    call("mmre_tc_scores", *_model_args(spec, ent, rel, ent_im, rel_im), ptr(ph), ptr(pr), ptr(pt), ptr(nh), ptr(nr),
         ptr(nt), n, ptr(pos), ptr(neg), stream_ptr(dev))
    return pos, neg


def _decode(out, n_pos, n_neg):
    o = out.cpu().numpy()
    thr = float(np.array([int(o[0])], np.uint32).view(np.float32)[0])
    P, A, n_nan = int(o[1]), int(o[2]), int(o[3])
    acc = float(_lib.lib().mmre_tc_accuracy(P, A, int(n_pos), int(n_neg)))
    return dict(threshold=thr, accuracy=acc, P=P, A=A, n_nan=n_nan, n_pos=int(n_pos), n_neg=int(n_neg))


def _threshold(pos_scores, neg_scores, thr):
    dev = next((x.device for x in (pos_scores, neg_scores) if isinstance(x, torch.Tensor) and x.is_cuda),
               torch.device("cuda:0"))
    pos, neg = _f32(pos_scores, dev), _f32(neg_scores, dev)
    n_pos, n_neg = int(pos.shape[0]), int(neg.shape[0])
    if n_pos + n_neg == 0:
        return dict(threshold=float("nan") if thr is None else float(thr), accuracy=float("nan"), P=0, A=0, n_nan=0,
                    n_pos=0, n_neg=0)
    out = torch.empty(4, dtype=torch.int64, device=dev)
    work, nbytes = None, 0
    if thr is None:
        nbytes = int(_lib.lib().mmre_tc_threshold_workspace(n_pos, n_neg))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("mmre_tc_threshold", ptr(pos) if n_pos else None, n_pos, ptr(neg) if n_neg else None, n_neg,
         0 if thr is None else 1, 0.0 if thr is None else float(thr), ptr(out), ptr(work), nbytes, stream_ptr(dev))
    return _decode(out, n_pos, n_neg)


def best_threshold(pos_scores, neg_scores):
    """get_best_threshlod's search (mmre_tc_threshold) over any positive and negative score arrays
    (numpy or torch; the lengths may differ). Returns dict(threshold, accuracy, P, A, n_nan, n_pos,
    n_neg): the smallest threshold among those of the highest accuracy of the rule `score <= thr`."""
    return _threshold(pos_scores, neg_scores, None)


def accuracy_at(pos_scores, neg_scores, thr):
    """The same dict at a given threshold: one counting pass, no search."""
    return _threshold(pos_scores, neg_scores, float(thr))


def evaluate_triple_classification(spec: ScoreSpec, test_h, test_r, test_t, train_index, seed_state: int,
                                   threshold=None):
    """The whole task in one enqueued call (mmre_tc_evaluate): negatives of the test triples from
    thread 0's `seed_state`, both prediction arrays, and the best threshold (or the counts at a given
    one). Returns dict(accuracy, threshold, P, A, n_nan, n_pos, n_neg, neg_h, neg_t, pos_scores,
    neg_scores (numpy), seed_state_after). A TransH, TransD or TransR spec composes the same result from
    classification_negatives, its engine's score_rows (mmre.transh / mmre.transd / mmre.transr) and
    best_threshold / accuracy_at."""
    if spec.model in ("transh", "transh_l2"):
        from .transh import score_rows
        return _evaluate_rows(score_rows, spec, test_h, test_r, test_t, train_index, seed_state, threshold)
    if spec.model in ("transd", "transd_l2"):
        from .transd import score_rows
        return _evaluate_rows(score_rows, spec, test_h, test_r, test_t, train_index, seed_state, threshold)
    if spec.model in ("transr", "transr_l2"):
        from .transr import score_rows
        return _evaluate_rows(score_rows, spec, test_h, test_r, test_t, train_index, seed_state, threshold)
    if spec.model == "rescal":
        from .rescal import score_rows
        return _evaluate_rows(score_rows, spec, test_h, test_r, test_t, train_index, seed_state, threshold)
    ent, rel, ent_im, rel_im = _tables(spec)
    dev = ent.device
    d = device_index(train_index, dev)
    h, r, t = (_i64(x, dev) for x in (test_h, test_r, test_t))
    n = int(h.shape[0])
    neg_h = torch.empty(n, dtype=torch.int64, device=dev)
    neg_t = torch.empty(n, dtype=torch.int64, device=dev)
    pos = torch.empty(n, dtype=torch.float32, device=dev)
    neg = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    work, nbytes = None, 0
    if threshold is None:
        nbytes = int(_lib.lib().mmre_tc_threshold_workspace(n, n))
        work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call("mmre_tc_evaluate", *_model_args(spec, ent, rel, ent_im, rel_im), *(ptr(d[k]) for k in INDEX_KEYS),
         int(d["train_total"]), ptr(h), ptr(r), ptr(t), n, int(seed_state) & (2 ** 64 - 1),
         0 if threshold is None else 1, 0.0 if threshold is None else float(threshold), ptr(neg_h), ptr(neg_t),
         ptr(pos), ptr(neg), ptr(out), ptr(work), nbytes, stream_ptr(dev))
    if n == 0:
        res = dict(threshold=float("nan") if threshold is None else float(threshold), accuracy=float("nan"), P=0,
                   A=0, n_nan=0, n_pos=0, n_neg=0)
    else:
        res = _decode(out, n, n)
    res.update(neg_h=neg_h.cpu().numpy(), neg_t=neg_t.cpu().numpy(), pos_scores=pos.cpu().numpy(),
               neg_scores=neg.cpu().numpy(), seed_state_after=advance_state(seed_state, n))
    return res


def _evaluate_rows(score_rows, spec, test_h, test_r, test_t, train_index, seed_state, threshold):
    """The task composed around a model's row kernel: score_rows(spec, h, r, t) -> predict values."""
    _lib.require_cuda(spec.ent)
    dev = spec.ent.device
    h, r, t = (_i64(x, dev) for x in (test_h, test_r, test_t))
    n = int(h.shape[0])
    neg_h, neg_t = classification_negatives(train_index, h, r, t, seed_state, device=dev)
    pos = score_rows(spec, h, r, t)
    neg = score_rows(spec, neg_h, r, neg_t)
    res = best_threshold(pos, neg) if threshold is None else accuracy_at(pos, neg, threshold)
    res.update(neg_h=neg_h.cpu().numpy(), neg_t=neg_t.cpu().numpy(), pos_scores=pos.cpu().numpy(),
               neg_scores=neg.cpu().numpy(), seed_state_after=advance_state(seed_state, n))
    return res
