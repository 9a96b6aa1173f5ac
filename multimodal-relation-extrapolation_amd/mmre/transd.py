"""TransD engine (csrc/transh.hip, the TransD part): link prediction with entities moved by the
transfer vectors of the entity and of the query's relation, and predict for arbitrary rows.

For OpenKE/openke/module/model/TransD.py the Tester loop (Tester.py:70-91) of getHeadBatch /
getTailBatch -> TransD.predict -> testHead / testTail (Test.h:65-192) becomes ONE enqueued
evaluation (mmre_transd_evaluate). An entity's operand is (e[:dim_r] + s(e) r_p) / N(r, e) with
s(e) = e . e_p: TransH's staged element with the table (-s, N) in place of (a, n) and the raw
rel_transfer rows in place of the unit normals, so the host plan (`mmre.transh.plan_tiles`: one
relation per 128-row query tile) and the sweep are TransH's; only the prologue is TransD's.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .transh import TILE, TransHSweep, plan_tiles  # noqa: F401  (the plan and the run are TransH's)

MODEL_IDS = {"transd": 7, "transd_l2": 8}


def is_transd(spec) -> bool:
    return spec is not None and spec.model in MODEL_IDS


def _tables(spec):
    """(ent, ent_transfer, rel, rel_transfer) as contiguous float32, and (dim_e, dim_r)."""
    if spec.ent_transfer is None or spec.rel_transfer is None:
        raise ValueError("a TransD ScoreSpec needs ent_transfer and rel_transfer (TransD.py:20-21)")
    _lib.require_cuda(spec.ent, spec.rel, spec.ent_transfer, spec.rel_transfer)
    c = lambda x: x.detach().contiguous().float()
    ent, ept, rel, rpt = c(spec.ent), c(spec.ent_transfer), c(spec.rel), c(spec.rel_transfer)
    dim_e, dim_r = int(ent.shape[1]), int(rel.shape[1])
    if tuple(ept.shape) != tuple(ent.shape) or tuple(rpt.shape) != tuple(rel.shape):
        raise ValueError("TransD: ent_transfer as ent (E, dim_e), rel_transfer as rel (R, dim_r)")
    if int(spec.dim) != dim_r or (spec.dim_e and int(spec.dim_e) != dim_e):
        raise ValueError("TransD: ScoreSpec.dim is dim_r (rel's width) and dim_e ent's width")
    if dim_e < dim_r:
        raise ValueError("TransD: dim_e >= dim_r (an entity row is cut to dim_r values, never padded)")
    return (ent, ept, rel, rpt), (dim_e, dim_r)


def score_rows(spec, h, r, t, mode: str = "normal", pred_kind: int | None = None):
    """TransD.predict of the rows (h[i], r[i], t[i]) -- or, with pred_kind=4 on a model with a
    margin, TransD.forward -- on the device (mmre_transd_score_rows), bit for bit what the sweep
    scores for the same triple and mode. mode "head_batch" takes the grouping h + (r - t), every
    other mode (h + r) - t (TransD.py:87-90). h / r / t: int64 device tensors of one length.
    Returns a float32 device tensor. Enqueues only."""
    (ent, ept, rel, rpt), (dim_e, dim_r) = _tables(spec)
    dev = ent.device
    h, r, t = (x.to(dev).to(torch.int64).contiguous().reshape(-1) for x in (h, r, t))
    n = int(h.shape[0])
    if int(r.shape[0]) != n or int(t.shape[0]) != n:
        raise ValueError("score_rows: h, r and t must have one length")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    call("mmre_transd_score_rows", MODEL_IDS[spec.model], int(bool(spec.norm_flag)),
         int(spec.pred_kind if pred_kind is None else pred_kind), float(spec.margin), ptr(ent), ptr(ept), ptr(rel),
         ptr(rpt), int(ent.shape[0]), int(rel.shape[0]), dim_e, dim_r, ptr(h), ptr(r), ptr(t), n,
         1 if mode == "head_batch" else 0, ptr(out), stream_ptr(dev))
    return out


class TransDSweep(TransHSweep):
    """Device-resident TransD link-prediction evaluator for one model snapshot: TransHSweep's
    run(...) -- the same contract and result dict -- over TransD's tables and entry points."""

    def __init__(self, spec):
        if not is_transd(spec):
            raise ValueError(f"TransDSweep: not a TransD spec ({spec.model!r})")
        self.spec = spec
        self.model_id = MODEL_IDS[spec.model]
        (self._ent, self._ept, self._rel, self._rpt), (self.dim_e, self.dim_r) = _tables(spec)
        # the sweep's planes are made on the first dim_r columns (TransD.py:62-68)
        self._narrow = self._ent if self.dim_e == self.dim_r else self._ent[:, :self.dim_r].contiguous()
        self.device = self._ent.device
        self.n_ent, self.n_rel = int(self._ent.shape[0]), int(self._rel.shape[0])

    def _workspace(self, n_tiles, n_used, n_entries):
        return _lib.lib().mmre_transd_workspace(self.n_ent, self.n_rel, self.dim_e, self.dim_r, n_tiles, n_used,
                                                n_entries)

    def _evaluate(self, *rest):
        s = self.spec
        call("mmre_transd_evaluate", self.model_id, int(bool(s.norm_flag)), int(s.pred_kind), float(s.margin),
             ptr(self._ent), ptr(self._ept), ptr(self._rel), ptr(self._rpt), ptr(self._narrow), self.n_ent, self.n_rel,
             self.dim_e, self.dim_r, *rest)
