"""TransH engine (csrc/transh.hip): link prediction with entities projected on the hyperplane of
the query's relation, and predict for arbitrary rows.

Replaces, for OpenKE/openke/module/model/TransH.py, what mmre.link replaces for TransE: the Tester
loop (Tester.py:70-91) of getHeadBatch / getTailBatch -> TransH.predict -> testHead / testTail
(Test.h:65-192) becomes ONE enqueued evaluation (mmre_transh_evaluate). An entity's operand
depends on the query's relation, so the host plans the sweep's 128-row query tiles by relation
(`plan_tiles`): every tile holds queries of one relation, and the device projects the entity
values with that relation's normal as it stages them.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

MODEL_IDS = {"transh": 5, "transh_l2": 6}
TILE = 128


def is_transh(spec) -> bool:
    return spec is not None and spec.model in MODEL_IDS


def plan_tiles(qr, tile: int = TILE):
    """Query tiles of one relation each, in pure numpy. qr: the queries' relations, in the
    caller's order. Returns dict(perm int32 [Q]: the stable order by relation; tiles int32 [T, 3]:
    (relation, first row of perm, rows <= tile), a relation's tiles consecutive, an absent relation
    none; used int32: the relations that occur, ascending; padding: T * tile / Q, the sweep's cost
    over an unplanned one (1.0 for no query))."""
    qr = np.asarray(qr, np.int64).reshape(-1)
    perm = np.argsort(qr, kind="stable").astype(np.int32)
    used, cnt = np.unique(qr, return_counts=True)
    starts = np.zeros(len(cnt), np.int64)
    np.cumsum(cnt[:-1], out=starts[1:])
    per = (cnt + tile - 1) // tile
    t_rel = np.repeat(np.arange(len(cnt)), per)
    t_idx = np.arange(len(t_rel)) - np.repeat(np.cumsum(per) - per, per)
    t_first = starts[t_rel] + t_idx * tile
    t_rows = np.minimum(cnt[t_rel] - t_idx * tile, tile)
    tiles = np.stack([used[t_rel], t_first, t_rows], 1).astype(np.int32).reshape(-1, 3)
    return dict(perm=perm, tiles=np.ascontiguousarray(tiles), used=used.astype(np.int32),
                padding=float(len(tiles) * tile / len(qr)) if len(qr) else 1.0)


def _tables(spec):
    if spec.norm_vec is None:
        raise ValueError("a TransH ScoreSpec needs norm_vec (the hyperplane normals, TransH.py:19)")
    _lib.require_cuda(spec.ent, spec.rel, spec.norm_vec)
    c = lambda x: x.detach().contiguous().float()
    return c(spec.ent), c(spec.rel), c(spec.norm_vec)


def score_rows(spec, h, r, t, mode: str = "normal", pred_kind: int | None = None):
    """TransH.predict of the rows (h[i], r[i], t[i]) -- or, with pred_kind=4 on a model with a
    margin, TransH.forward -- on the device (mmre_transh_score_rows), bit for bit what the sweep
    scores for the same triple and mode. mode "head_batch" takes the grouping h + (r - t), every
    other mode (h + r) - t (TransH.py:61-64). h / r / t: int64 device tensors of one length.
    Returns a float32 device tensor. Enqueues only."""
    ent, rel, nv = _tables(spec)
    dev = ent.device
    h, r, t = (x.to(dev).to(torch.int64).contiguous().reshape(-1) for x in (h, r, t))
    n = int(h.shape[0])
    if int(r.shape[0]) != n or int(t.shape[0]) != n:
        raise ValueError("score_rows: h, r and t must have one length")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    call("mmre_transh_score_rows", MODEL_IDS[spec.model], int(bool(spec.norm_flag)),
         int(spec.pred_kind if pred_kind is None else pred_kind), float(spec.margin), ptr(ent), ptr(rel), ptr(nv),
         int(ent.shape[0]), int(rel.shape[0]), int(spec.dim), ptr(h), ptr(r), ptr(t), n,
         1 if mode == "head_batch" else 0, ptr(out), stream_ptr(dev))
    return out


class TransHSweep:
    """Device-resident TransH link-prediction evaluator for one model snapshot."""

    def __init__(self, spec):
        if not is_transh(spec):
            raise ValueError(f"TransHSweep: not a TransH spec ({spec.model!r})")
        self.spec = spec
        self.model_id = MODEL_IDS[spec.model]
        self._ent, self._rel, self._nv = _tables(spec)
        self.device = self._ent.device
        self.n_ent, self.n_rel = int(self._ent.shape[0]), int(self._rel.shape[0])
        if tuple(self._nv.shape) != tuple(self._rel.shape):
            raise ValueError("TransH: norm_vec and rel must have one shape")

    # the two calls a model of this sweep family makes with its own tables (mmre.transd overrides them)
    def _workspace(self, n_tiles, n_used, n_entries):
        return _lib.lib().mmre_transh_workspace(self.n_ent, self.n_rel, int(self.spec.dim), n_tiles, n_used, n_entries)

    def _evaluate(self, *rest):
        s = self.spec
        call("mmre_transh_evaluate", self.model_id, int(bool(s.norm_flag)), int(s.pred_kind), float(s.margin),
             ptr(self._ent), ptr(self._rel), ptr(self._nv), self.n_ent, self.n_rel, int(s.dim), *rest)

    def run(self, qh, qr, qt, qmode, filt=None, type_masks=None, buffers=None, plan=None, events=None):
        """qh/qr/qt int64 and qmode int8 device tensors; filt: filter groups (FilterIndex.groups)
        or None; type_masks: (head, tail) uint32 device bitsets or None; plan: plan_tiles(qr) when
        the caller has it (else qr is read back once). events: optional (start, end)
        torch.cuda.Event pair recorded around the whole enqueued evaluation.
        Returns dict(counts=(4, Q) int32 [raw, filt, raw_tc, filt_tc], truth=(Q,), padding)."""
        dev, who = self.device, type(self).__name__
        n = int(qh.shape[0])
        b = buffers if buffers is not None else {}
        if b.get("th_n") != n:
            b["counts"] = torch.empty((4, n), dtype=torch.int32, device=dev)
            b["truth"] = torch.empty(n, dtype=torch.float32, device=dev)
            b["th_n"] = n
        if n == 0:
            return dict(counts=b["counts"], truth=b["truth"], padding=1.0)
        if filt is not None and len(filt) != 5:
            raise ValueError(f"{who} takes filter groups (FilterIndex.groups)")
        if plan is None:
            plan = plan_tiles(qr.cpu().numpy())
        if b.get("th_plan") is not plan:
            slot = np.full(self.n_rel, -1, np.int32)
            used = plan["used"]
            if len(used) and (used.min() < 0 or used.max() >= self.n_rel):
                raise ValueError(f"{who}: a query's relation is outside the relation table")
            slot[used] = np.arange(len(used), dtype=np.int32)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            b["th_dev"] = tuple(to(a) for a in (plan["perm"], plan["tiles"], used, slot))
            b["th_plan"] = plan
        perm, tiles, used, slot = b["th_dev"]
        n_tiles, n_used = int(tiles.shape[0]), int(used.shape[0])
        gqo = gq = off = ids = entry_q = None
        n_groups = n_entries = 0
        if filt is not None:
            gqo, gq, off, ids, entry_q = filt
            n_groups, n_entries = int(gqo.shape[0]) - 1, int(ids.shape[0])
        need = int(self._workspace(n_tiles, n_used, n_entries))
        wk = b.get("th_work")
        if wk is None or wk.numel() < need:
            wk = b["th_work"] = torch.empty(need, dtype=torch.uint8, device=dev)
        th, tt = (None, None) if type_masks is None else type_masks
        if events is not None:
            events[0].record()
        self._evaluate(ptr(qh), ptr(qr), ptr(qt), ptr(qmode), n, ptr(perm), ptr(tiles), n_tiles, ptr(used), n_used,
                       ptr(slot), ptr(gqo), ptr(gq), n_groups, ptr(off), ptr(ids) if n_entries else None,
                       ptr(entry_q) if n_entries else None, n_entries, ptr(th), ptr(tt), ptr(b["counts"]),
                       ptr(b["truth"]), ptr(wk), int(wk.numel()), stream_ptr(dev))
        if events is not None:
            events[1].record()
        return dict(counts=b["counts"], truth=b["truth"], padding=plan["padding"])
