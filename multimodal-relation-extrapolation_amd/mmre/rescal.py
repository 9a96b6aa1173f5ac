"""RESCAL engine (csrc/rescal.hip): link prediction with the bilinear score of the query's relation
matrix, and predict for arbitrary rows.

For OpenKE/openke/module/model/RESCAL.py the Tester loop (Tester.py:70-91) of getHeadBatch /
getTailBatch -> RESCAL.predict -> testHead / testTail (Test.h:65-192) becomes ONE enqueued
evaluation (mmre_rescal_evaluate). s(h, r, t) = sum_i h_i (M_r t)_i: for every relation that occurs
in the queries the plane P_r = E . M_r^T is made on the matrix cores, a tail-side query multiplies
the raw row h with P_r and a head-side query column t of P_r with the raw entity table, so a query
tile holds the queries of one (relation, side). The host plan is `mmre.transh.plan_tiles` over the
key 2 * relation + side (`plan_keys`), run() is TransH's. The workspace holds every used relation's
plane at once plus the k-major copy of the entity table (round_up(dim, 16) x round_up(E, 128)
floats each).

predict is +s (RESCAL.py:44-46 returns -forward and forward is -s): the Tester ranks ascending on
+s, as the reference does, and pred_kind 0 serves it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .transh import TILE, TransHSweep, plan_tiles  # noqa: F401  (the plan and the run are TransH's)

MODEL_IDS = {"rescal": 11}
MAX_DIM = 512


def is_rescal(spec) -> bool:
    return spec is not None and spec.model in MODEL_IDS


def plan_keys(qr, qmode, tile: int = TILE):
    """`plan_tiles` with the key 2 * relation + side (side = qmode: 0 head batch, 1 tail batch) in
    the relation's place: every tile holds queries of one relation AND one side, a key's tiles are
    consecutive, a side without queries has no tile. tiles[:, 0] is the key; `used` the relations
    that occur (either side), ascending -- what the planes are made for."""
    qr = np.asarray(qr, np.int64).reshape(-1)
    qmode = np.asarray(qmode, np.int64).reshape(-1)
    if len(qr) != len(qmode) or (len(qmode) and (qmode.min() < 0 or qmode.max() > 1)):
        raise ValueError("plan_keys: one mode (0 head batch, 1 tail batch) per query")
    plan = plan_tiles(2 * qr + qmode, tile)
    plan["used"] = np.unique(plan["used"] >> 1).astype(np.int32)
    return plan


def _tables(spec):
    """(ent, rel_matrices) as contiguous float32, and dim."""
    if spec.rel_matrices is None:
        raise ValueError("a RESCAL ScoreSpec needs rel_matrices (RESCAL.py:12)")
    _lib.require_cuda(spec.ent, spec.rel_matrices)
    c = lambda x: x.detach().contiguous().float()
    ent, mats = c(spec.ent), c(spec.rel_matrices)
    dim = int(ent.shape[1])
    if mats.dim() != 2 or int(mats.shape[1]) != dim * dim:
        raise ValueError("RESCAL: rel_matrices is (R, dim * dim)")
    if int(spec.dim) != dim:
        raise ValueError("RESCAL: ScoreSpec.dim is ent's width")
    return (ent, mats), dim


def score_rows(spec, h, r, t, mode: str = "normal", pred_kind: int | None = None):
    """RESCAL.predict of the rows (h[i], r[i], t[i]) -- or, with pred_kind=2, RESCAL.forward -- on
    the device (mmre_rescal_score_rows), bit for bit what the sweep scores for the same triple on
    either side (the score does not depend on `mode`, which is accepted for the other engines'
    signature). h / r / t: int64 device tensors of one length. Returns a float32 device tensor.
    Enqueues only."""
    (ent, mats), dim = _tables(spec)
    dev = ent.device
    h, r, t = (x.to(dev).to(torch.int64).contiguous().reshape(-1) for x in (h, r, t))
    n = int(h.shape[0])
    if int(r.shape[0]) != n or int(t.shape[0]) != n:
        raise ValueError("score_rows: h, r and t must have one length")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    call("mmre_rescal_score_rows", MODEL_IDS[spec.model], int(spec.pred_kind if pred_kind is None else pred_kind),
         ptr(ent), ptr(mats), int(ent.shape[0]), int(mats.shape[0]), dim, ptr(h), ptr(r), ptr(t), n, ptr(out),
         stream_ptr(dev))
    return out


class RescalSweep(TransHSweep):
    """Device-resident RESCAL link-prediction evaluator for one model snapshot: TransHSweep's
    run(...) -- the same contract and result dict -- over RESCAL's tables and entry points, with
    the plan of `plan_keys` (made here from qr and qmode when the caller passes none)."""

    def __init__(self, spec):
        if not is_rescal(spec):
            raise ValueError(f"RescalSweep: not a RESCAL spec ({spec.model!r})")
        self.spec = spec
        self.model_id = MODEL_IDS[spec.model]
        (self._ent, self._mats), self.dim = _tables(spec)
        self.device = self._ent.device
        self.n_ent, self.n_rel = int(self._ent.shape[0]), int(self._mats.shape[0])

    def run(self, qh, qr, qt, qmode, filt=None, type_masks=None, buffers=None, plan=None, events=None):
        if plan is None and int(qh.shape[0]):
            plan = plan_keys(qr.cpu().numpy(), qmode.cpu().numpy())
        return super().run(qh, qr, qt, qmode, filt=filt, type_masks=type_masks, buffers=buffers, plan=plan,
                           events=events)

    def _workspace(self, n_tiles, n_used, n_entries):
        return _lib.lib().mmre_rescal_workspace(self.n_ent, self.n_rel, self.dim, n_tiles, n_used, n_entries)

    def _evaluate(self, *rest):
        call("mmre_rescal_evaluate", self.model_id, int(self.spec.pred_kind), ptr(self._ent), ptr(self._mats),
             self.n_ent, self.n_rel, self.dim, *rest)
