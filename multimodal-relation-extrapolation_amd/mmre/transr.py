"""TransR engine (csrc/transr.hip): link prediction with entities projected by the matrix of the
query's relation, and predict for arbitrary rows.

For OpenKE/openke/module/model/TransR.py the Tester loop (Tester.py:70-91) of getHeadBatch /
getTailBatch -> TransR.predict -> testHead / testTail (Test.h:65-192) becomes ONE enqueued
evaluation (mmre_transr_evaluate). An entity's operand is normalize(e . M_r): a GEMM per relation
that occurs in the queries, made on the matrix cores into one k-major plane per relation, which
the sweep stages as it is. The host plan (`mmre.transh.plan_tiles`: one relation per 128-row
query tile) and run() are TransH's. The workspace holds every used relation's plane at once
(round_up(dim_r, 8) x round_up(E, 128) floats each).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .transh import TILE, TransHSweep, plan_tiles  # noqa: F401  (the plan and the run are TransH's)

MODEL_IDS = {"transr": 9, "transr_l2": 10}
MAX_DIM = 512


def is_transr(spec) -> bool:
    return spec is not None and spec.model in MODEL_IDS


def _tables(spec):
    """(ent, rel, transfer_matrix) as contiguous float32, and (dim_e, dim_r)."""
    if spec.transfer_matrix is None:
        raise ValueError("a TransR ScoreSpec needs transfer_matrix (TransR.py:22)")
    _lib.require_cuda(spec.ent, spec.rel, spec.transfer_matrix)
    c = lambda x: x.detach().contiguous().float()
    ent, rel, tm = c(spec.ent), c(spec.rel), c(spec.transfer_matrix)
    dim_e, dim_r = int(ent.shape[1]), int(rel.shape[1])
    if tuple(tm.shape) != (int(rel.shape[0]), dim_e * dim_r):
        raise ValueError("TransR: transfer_matrix is (R, dim_e * dim_r)")
    if int(spec.dim) != dim_r or (spec.dim_e and int(spec.dim_e) != dim_e):
        raise ValueError("TransR: ScoreSpec.dim is dim_r (rel's width) and dim_e ent's width")
    return (ent, rel, tm), (dim_e, dim_r)


def score_rows(spec, h, r, t, mode: str = "normal", pred_kind: int | None = None):
    """TransR.predict of the rows (h[i], r[i], t[i]) -- or, with pred_kind=4 on a model with a
    margin, TransR.forward -- on the device (mmre_transr_score_rows), bit for bit what the sweep
    scores for the same triple and mode. mode "head_batch" takes the grouping h + (r - t), every
    other mode (h + r) - t (TransR.py:46-49). h / r / t: int64 device tensors of one length.
    Returns a float32 device tensor. Enqueues only."""
    (ent, rel, tm), (dim_e, dim_r) = _tables(spec)
    dev = ent.device
    h, r, t = (x.to(dev).to(torch.int64).contiguous().reshape(-1) for x in (h, r, t))
    n = int(h.shape[0])
    if int(r.shape[0]) != n or int(t.shape[0]) != n:
        raise ValueError("score_rows: h, r and t must have one length")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    call("mmre_transr_score_rows", MODEL_IDS[spec.model], int(bool(spec.norm_flag)),
         int(spec.pred_kind if pred_kind is None else pred_kind), float(spec.margin), ptr(ent), ptr(rel), ptr(tm),
         int(ent.shape[0]), int(rel.shape[0]), dim_e, dim_r, ptr(h), ptr(r), ptr(t), n,
         1 if mode == "head_batch" else 0, ptr(out), stream_ptr(dev))
    return out


class TransRSweep(TransHSweep):
    """Device-resident TransR link-prediction evaluator for one model snapshot: TransHSweep's
    run(...) -- the same contract and result dict -- over TransR's tables and entry points."""

    def __init__(self, spec):
        if not is_transr(spec):
            raise ValueError(f"TransRSweep: not a TransR spec ({spec.model!r})")
        self.spec = spec
        self.model_id = MODEL_IDS[spec.model]
        (self._ent, self._rel, self._tm), (self.dim_e, self.dim_r) = _tables(spec)
        self.device = self._ent.device
        self.n_ent, self.n_rel = int(self._ent.shape[0]), int(self._rel.shape[0])

    def _workspace(self, n_tiles, n_used, n_entries):
        return _lib.lib().mmre_transr_workspace(self.n_ent, self.n_rel, self.dim_e, self.dim_r, n_tiles, n_used,
                                                n_entries)

    def _evaluate(self, *rest):
        s = self.spec
        call("mmre_transr_evaluate", self.model_id, int(bool(s.norm_flag)), int(s.pred_kind), float(s.margin),
             ptr(self._ent), ptr(self._rel), ptr(self._tm), self.n_ent, self.n_rel, self.dim_e, self.dim_r, *rest)
