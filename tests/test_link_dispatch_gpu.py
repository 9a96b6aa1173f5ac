"""One case per branch of the link sweeps' host dispatch (csrc/link.hip, link_valu.hip), at the smallest shape
that still has two tiles on each axis and a ragged tail: E = 300 (three 128-entity tiles, the
last one ragged), Q = 130 (two query tiles), R = 5; d = 20 for TransE L1 / L2 and RotatE, 16 and
24 for DistMult and ComplEx. Inputs as test_link_gpu._random_case(with_ties=True) builds them (a
third of the queries then share their neighbour's (mode, r, anchor), so filter groups have members).

Bar, as test_link_gpu.test_random_bit_exact: score rows bit-equal to oracle.link_predict, raw and
filtered counts equal to oracle.test_rank, and with type lists the two type-constrained columns.

The oracle derives the prediction kind from (model, margin): it expresses kinds 0 and 1 for
TransE L1 / L2, 2 for DistMult / ComplEx and 3 for RotatE. Every other (model, pred_kind) takes the
second route: the count-only result is compared with counts computed in torch from the score rows
and truth scores a score-storing run of the same (model, pred_kind) left, with the same strict <
on float32 (`_counts`; on the oracle's kinds it is held equal to oracle.test_rank as well). Entity
slices are checked through `_counts` restricted to the slice's columns, on either route."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from test_link_gpu import _random_case

pytestmark = pytest.mark.gpu
E, Q, R = 300, 130, 5
MARGIN = 4.0
SHAPES = [("transe", 20), ("transe_l2", 20), ("rotate", 20), ("distmult", 16), ("distmult", 24), ("complex", 16),
          ("complex", 24)]
ORACLE_KINDS = {"transe": (0, 1), "transe_l2": (0, 1), "distmult": (2,), "complex": (2,), "rotate": (3,)}
FILTER_ENVS = ("MMRE_L1_FILTER", "MMRE_MFMA_FILTER", "MMRE_FUSED_EVAL", "MMRE_BF3_RAW", "MMRE_L1_BITS",
               "MMRE_BF3_WIDE", "MMRE_BF3_QT", "MMRE_GROUP_CAP")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in FILTER_ENVS:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, **env):
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


class Case:
    """Tables, queries, filter index and type lists of one (model, d); the references, computed once."""

    def __init__(self, model, d):
        from mmre.link import FilterIndex
        self.model, self.d = model, d
        seed = 100 * d + len(model)
        self.ent, self.rel, self.ent_im, self.rel_im, qh, qr, qt, qm = _random_case(model, E, R, d, Q, seed,
                                                                                     with_ties=True)
        for i in range(1, Q, 3):  # share the neighbour's key: groups of two and three members
            qm[i], qr[i] = qm[i - 1], qr[i - 1]
            if qm[i] == 0:
                qt[i] = qt[i - 1]
            else:
                qh[i] = qh[i - 1]
        self.qh, self.qr, self.qt, self.qm = qh, qr, qt, qm
        rng = np.random.default_rng(seed + 1)
        th, tr, tt = rng.integers(0, E, 4 * E), rng.integers(0, R, 4 * E), rng.integers(0, E, 4 * E)
        self.th, self.tr, self.tt = np.r_[th, qh], np.r_[tr, qr], np.r_[tt, qt]
        self.heads = [np.unique(np.r_[rng.choice(E, E // 3, replace=False), qh[qr == r]]) for r in range(R)]
        self.tails = [np.unique(np.r_[rng.choice(E, E // 3, replace=False), qt[qr == r]]) for r in range(R)]
        self.index = FilterIndex(self.th, self.tr, self.tt, E, R, self.heads, self.tails)
        self.truth_id = np.where(qm == 0, qh, qt)
        # what orc_test_rank looks up, as (Q, E) masks
        self.known = np.zeros((Q, E), bool)
        self.typed = np.zeros((Q, E), bool)
        for q in range(Q):
            if qm[q] == 0:
                self.known[q, self.th[(self.tr == qr[q]) & (self.tt == qt[q])]] = True
            else:
                self.known[q, self.tt[(self.tr == qr[q]) & (self.th == qh[q])]] = True
            self.typed[q, (self.heads if qm[q] == 0 else self.tails)[qr[q]]] = True
        self._stored = {}

    def spec(self, pk):
        from mmre.link import ScoreSpec, rotate_phase_denom
        dev = torch.device("cuda:0")
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        pd = rotate_phase_denom(MARGIN, 2.0, self.d) if self.model == "rotate" else 0.0
        return ScoreSpec(model=self.model, ent=t(self.ent), rel=t(self.rel), dim=self.d, ent_im=t(self.ent_im),
                         rel_im=t(self.rel_im), norm_flag=self.model.startswith("transe"), pred_kind=pk,
                         margin=MARGIN, phase_denom=pd)

    def run(self, pk, tc=False, scores=False, entity_range=None):
        """LinkSweep.run with filter groups (restricted to the slice); the buffers' path flags."""
        from mmre.link import LinkSweep, group_args
        dev = torch.device("cuda:0")
        spec = self.spec(pk)
        lists = self.index.groups(self.qh, self.qr, self.qt, self.qm, entity_range=entity_range,
                                  **group_args(spec, tc))
        filt = tuple(torch.from_numpy(a).to(dev) for a in lists)
        masks = tuple(torch.from_numpy(m).to(dev) for m in self.index.type_masks()) if tc else None
        sw = LinkSweep(spec)
        b = sw.alloc_queries(Q)
        to = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)
        fused = sw._fusable(filt, masks, scores, True, None, True)
        res = sw.run(to(self.qh, np.int64), to(self.qr, np.int64), to(self.qt, np.int64), to(self.qm, np.int8),
                     filt=filt, type_masks=masks, return_scores=scores, buffers=b, entity_range=entity_range)
        torch.cuda.synchronize()
        out = {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}
        out["path"] = ("fused" if fused else "l1q" if b["l1q_used"] else "bf3_rows" if b["bf3_raw"] else
                       "bf3" if b["bf3_used"] else "plain")
        out["stats"] = sw.filter_stats(b)
        return out

    def oracle_pred(self, oracle_mod, pk):
        """(Q, E) oracle predictions in query order, or None where the oracle has no such kind."""
        if pk not in ORACLE_KINDS[self.model]:
            return None
        key = ("oracle", pk)
        if key not in self._stored:
            okw = dict(ent_im=self.ent_im, rel_im=self.rel_im, norm_flag=self.model.startswith("transe"),
                       margin=None if (self.model.startswith("transe") and pk == 0) else MARGIN,
                       phase_denom=self.spec(pk).phase_denom)
            pred = np.empty((Q, E), np.float32)
            ranks = np.empty((Q, 4), np.int64)
            hrt = oracle_mod.sorted_hrt(self.th, self.tr, self.tt)
            for mode_id, mode, lists in ((0, "head_batch", self.heads), (1, "tail_batch", self.tails)):
                sel = self.qm == mode_id
                pred[sel] = oracle_mod.link_predict(self.model, mode, self.ent, self.rel, self.qh[sel], self.qr[sel],
                                                    self.qt[sel], **okw)
                toff = np.cumsum([0] + [len(x) for x in lists])
                tids = np.concatenate([np.asarray(x, np.int64) for x in lists])
                ranks[sel] = oracle_mod.test_rank(mode, pred[sel], self.qh[sel], self.qr[sel], self.qt[sel], hrt,
                                                  toff, tids)
            self._stored[key] = (pred, ranks)
        return self._stored[key]

    def expected(self, oracle_mod, pk, lo=0, hi=E):
        """(Q, 4) counts over the entities [lo, hi): oracle.test_rank where the oracle has the kind
        (whole table), else `_counts` of a score-storing run's rows and truths."""
        o = self.oracle_pred(oracle_mod, pk)
        if o is not None:
            pred, ranks = o
            truth = pred[np.arange(Q), self.truth_id]
            c = _counts(self, pred, truth, 0, E)
            assert np.array_equal(c, ranks)  # the torch count is orc_test_rank's
            return ranks if (lo, hi) == (0, E) else _counts(self, pred, truth, lo, hi)
        key = ("stored", pk)
        if key not in self._stored:
            r = self.run(pk, tc=False, scores=True)
            assert r["path"] == "plain"
            self._stored[key] = (r["scores"], r["truth"])
        return _counts(self, *self._stored[key], lo, hi)


def _counts(c, scores, truth, lo, hi):
    """Test.h's four counts from score rows: strict < on float32, the truth's own column excluded."""
    s = torch.from_numpy(np.ascontiguousarray(scores, np.float32))
    better = s < torch.from_numpy(np.ascontiguousarray(truth, np.float32))[:, None]
    better[torch.arange(Q), torch.from_numpy(c.truth_id)] = False
    better[:, :lo] = False
    better[:, hi:] = False
    known, typed = torch.from_numpy(c.known), torch.from_numpy(c.typed)
    cols = (better, better & ~known, better & typed, better & typed & ~known)
    return torch.stack([x.sum(1) for x in cols], 1).numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(model, d):
    return Case(model, d)


def _check(c, oracle_mod, out, pk, tc, lo=0, hi=E):
    want = c.expected(oracle_mod, pk, lo, hi)
    cols = [0, 1, 2, 3] if tc else [0, 1]
    assert np.array_equal(out["counts"].T[:, cols], want[:, cols])
    o = c.oracle_pred(oracle_mod, pk)
    if o is not None:
        assert np.array_equal(out["truth"], o[0][np.arange(Q), c.truth_id])
        if out["scores"] is not None:
            assert np.array_equal(out["scores"], o[0])
    else:  # the stored rows carry their own truths
        rows, truth = c._stored[("stored", pk)] if out["scores"] is None else (out["scores"], out["truth"])
        assert np.array_equal(out["truth"], truth)
        assert np.array_equal(truth, rows[np.arange(Q), c.truth_id])


@pytest.mark.parametrize("scores", [0, 1])
@pytest.mark.parametrize("tc", [0, 1])
@pytest.mark.parametrize("pk", [0, 1, 2, 3])
@pytest.mark.parametrize("model,d", SHAPES)
def test_separate_path_filters_off(oracle_mod, monkeypatch, model, d, pk, tc, scores):
    """mmre_link_sweep: k_sweep_valu / k_sweep_mfma at every (TC, STORE) and both epilogues."""
    _setenv(monkeypatch, MMRE_L1_FILTER=0, MMRE_MFMA_FILTER=0, MMRE_FUSED_EVAL=0)
    c = _case(model, d)
    out = c.run(pk, tc=bool(tc), scores=bool(scores))
    assert out["path"] == "plain" and out["stats"] is None
    _check(c, oracle_mod, out, pk, tc)


@pytest.mark.parametrize("pk", [0, 1])
@pytest.mark.parametrize("tc", [0, 1])
@pytest.mark.parametrize("bits", [None, 8, 16])
def test_l1_filter(oracle_mod, monkeypatch, bits, tc, pk):
    """mmre_link_sweep_l1q: the 8-bit, 16-bit and gated f32 sweeps, tight and uniform bound."""
    _setenv(monkeypatch, MMRE_FUSED_EVAL=0, MMRE_L1_BITS=bits)
    c = _case("transe", 20)
    out = c.run(pk, tc=bool(tc))
    assert out["path"] == "l1q"
    if bits is not None and not out["stats"]["fallback"]:
        assert out["stats"]["bits"] == bits
    _check(c, oracle_mod, out, pk, tc)


@pytest.mark.parametrize("pk,wide,qt", [(2, 0, None), (2, 1, None), (2, 1, 128), (0, 0, None), (0, 1, None)])
@pytest.mark.parametrize("model,d", [s for s in SHAPES if s[0] in ("distmult", "complex")])
def test_split_bf16_filter(oracle_mod, monkeypatch, model, d, pk, wide, qt):
    """mmre_link_sweep_bf3: the 128 x 128 sweep at both epilogues, the wide one at both query tiles."""
    _setenv(monkeypatch, MMRE_BF3_RAW=0, MMRE_BF3_WIDE=wide, MMRE_BF3_QT=qt)
    c = _case(model, d)
    out = c.run(pk)
    assert out["path"] == "bf3"
    _check(c, oracle_mod, out, pk, False)


@pytest.mark.parametrize("pk,wide", [(2, 0), (2, 1), (0, 0)])
def test_split_bf16_raw_rows(oracle_mod, monkeypatch, pk, wide):
    """mmre_link_sweep_bf3_rows: DistMult with K = d sweeps the raw table."""
    _setenv(monkeypatch, MMRE_BF3_WIDE=wide)
    c = _case("distmult", 16)
    out = c.run(pk)
    assert out["path"] == "bf3_rows"
    _check(c, oracle_mod, out, pk, False)


@pytest.mark.parametrize("bits", [None, 8, 16])
@pytest.mark.parametrize("cap", [None, 1, 8])
def test_fused_evaluation(oracle_mod, monkeypatch, cap, bits):
    """mmre_link_evaluate_l1q: ungrouped (its own choice at this size) and the grouped sweeps."""
    _setenv(monkeypatch, MMRE_GROUP_CAP=cap, MMRE_L1_BITS=bits)
    c = _case("transe", 20)
    out = c.run(0)
    assert out["path"] == "fused"
    if bits is not None and not out["stats"]["fallback"]:
        assert out["stats"]["bits"] == bits
    _check(c, oracle_mod, out, 0, False)


SLICES = {
    "sweep_range_valu": ("transe_l2", 20, 1, "plain", dict(MMRE_L1_FILTER=0, MMRE_MFMA_FILTER=0, MMRE_FUSED_EVAL=0)),
    "sweep_range_mfma": ("complex", 24, 2, "plain", dict(MMRE_L1_FILTER=0, MMRE_MFMA_FILTER=0, MMRE_FUSED_EVAL=0)),
    "sweep_l1q": ("transe", 20, 0, "l1q", dict(MMRE_FUSED_EVAL=0)),
    "sweep_bf3": ("complex", 24, 2, "bf3", {}),
    "sweep_bf3_rows": ("distmult", 16, 2, "bf3_rows", {}),
    "fused": ("transe", 20, 0, "fused", {}),
    "fused_grouped": ("transe", 20, 0, "fused", dict(MMRE_GROUP_CAP=8)),
}


@pytest.mark.parametrize("name", list(SLICES))
def test_entity_slice(oracle_mod, monkeypatch, name):
    """The entities [128, 300) alone: the slice's pointer offsets, e_base and tile counts."""
    model, d, pk, path, env = SLICES[name]
    _setenv(monkeypatch, **env)
    c = _case(model, d)
    out = c.run(pk, entity_range=(128, E))
    assert out["path"] == path
    _check(c, oracle_mod, out, pk, False, 128, E)
