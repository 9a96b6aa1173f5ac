"""TransH without a GPU: the restatement of DESIGN.md §3 (tests/transh_restate.py) against the
reference's fixture, the host plan of one-relation query tiles, and the error codes of the TransH
entry points for arguments they refuse before anything is launched (addresses never dereferenced)."""
import itertools
import os

import numpy as np
import pytest
import torch  # noqa: F401  (the library binds to torch's HIP runtime)

import transh_restate as R
from conftest import GOLDEN

SMALL = os.path.join(GOLDEN, "data", "small")
CONFIGS = [("l1_norm", dict(p_norm=1, norm_flag=True, margin=None)),
           ("l2_norm", dict(p_norm=2, norm_flag=True, margin=None)),
           ("l1_nonorm_margin", dict(p_norm=1, norm_flag=False, margin=5.0))]
TRANSH_L1, TRANSH_L2 = 5, 6


# ------------------------------------------------------------------ restatement vs golden ---
@pytest.fixture(scope="module")
def small():
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    ds = OpenKEDataset(SMALL)
    return ds, FilterIndex(*ds.all_triples(), ds.n_ent, ds.n_rel)


def dataset_counts(scores, qh, qr, qt, head, ds, index):
    n = len(qh)
    off, ids = index.filters(qh, qr, qt, np.zeros(n, np.int8) if head else np.ones(n, np.int8))
    known = [ids[off[i]:off[i + 1]] for i in range(n)]
    allowed = np.zeros((n, ds.n_ent), bool)
    for i in range(n):
        allowed[i, np.asarray((ds.type_heads if head else ds.type_tails)[qr[i]], np.int64)] = True
    return R.rank_counts(scores, qh if head else qt, known, allowed)


@pytest.mark.parametrize("name,kw", CONFIGS)
def test_restatement_matches_the_reference(golden, small, name, kw):
    g = golden("transh_small")
    ds, index = small
    ent, rel, nv = (g[f"{name}.{k}.weight"] for k in ("ent_embeddings", "rel_embeddings", "norm_vector"))
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    T = len(qh)
    for side, head in (("head", True), ("tail", False)):
        s = R.sweep_scores(ent, rel, nv, qh, qr, qt, np.full(T, 0 if head else 1), **kw)
        ref = g[f"{name}.pred_{side}"]
        assert np.all(np.abs(s[:len(ref)] - ref) <= 1e-4 * np.maximum(1, np.abs(ref))), side
        c = dataset_counts(s, qh, qr, qt, head, ds, index)
        assert np.array_equal(c[:2].T, g[f"{name}.tc0_{side}_counts"][:, :2]), side
        assert np.array_equal(c.T, g[f"{name}.tc1_{side}_counts"]), side
        # the row restatement is the sweep restatement's diagonal, bit for bit
        rows = R.score_rows(ent, rel, nv, qh, qr, qt, head, **kw)
        assert np.array_equal(rows, s[np.arange(T), qh if head else qt])


# ------------------------------------------------------------------------------ the plan ---
def check_plan(qr, plan, tile=128):
    perm, tiles = plan["perm"], plan["tiles"]
    assert perm.dtype == np.int32 and tiles.dtype == np.int32 and tiles.shape[1:] == (3,)
    assert np.array_equal(np.sort(perm), np.arange(len(qr)))                # every query once
    inv = np.empty(len(qr), np.int64)
    inv[perm] = np.arange(len(qr))
    assert np.array_equal(perm[inv], np.arange(len(qr)))                    # the permutation round-trips
    covered = np.zeros(len(qr), int)
    for rel, first, rows in tiles:
        assert 1 <= rows <= tile
        assert np.all(qr[perm[first:first + rows]] == rel)                  # one relation per tile
        covered[first:first + rows] += 1
    assert np.all(covered == 1)
    # stable: a relation's queries keep the caller's order
    for rel in np.unique(qr):
        mine = perm[qr[perm] == rel]
        assert np.all(np.diff(mine) > 0)
    want = sum(-(-int(c) // tile) for c in np.bincount(qr) if c)
    assert len(tiles) == want
    assert set(tiles[:, 0].tolist()) == set(np.unique(qr).tolist()) == set(plan["used"].tolist())
    if len(qr):
        assert plan["padding"] == len(tiles) * tile / len(qr)


def test_plan_tiles():
    from mmre.transh import plan_tiles
    counts = [0, 1, 127, 128, 129, 300]
    rng = np.random.default_rng(3)
    qr = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    plan = plan_tiles(qr)
    check_plan(qr, plan)
    assert 0 not in plan["used"]                                            # an absent relation: no tile
    assert sorted(np.bincount(plan["tiles"][:, 0], minlength=6).tolist()) == [0, 1, 1, 1, 2, 3]
    check_plan(np.zeros(0, np.int64), plan_tiles(np.zeros(0, np.int64)))
    one = np.full(300, 4)
    check_plan(one, plan_tiles(one))
    assert plan_tiles(one)["tiles"].tolist() == [[4, 0, 128], [4, 128, 128], [4, 256, 44]]
    each = np.arange(50)[::-1].copy()
    check_plan(each, plan_tiles(each))
    assert plan_tiles(each)["padding"] == 128.0
    check_plan(qr, plan_tiles(qr, tile=64), tile=64)


# ------------------------------------------------------------------------------- the ABI ---
ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, aligned, never dereferenced

EVAL = ("model", "norm_flag", "pred_kind", "margin", "ent", "rel", "norm", "n_ent", "n_rel", "dim", "qh", "qr", "qt",
        "qmode", "n_query", "perm", "tiles", "n_tiles", "used", "n_used", "rel_slot", "grp_qoff", "grp_q", "n_groups",
        "filt_off", "filt_ids", "entry_q", "n_entries", "type_head", "type_tail", "counts", "truth", "work",
        "work_bytes", "stream")
ROWS = ("model", "norm_flag", "pred_kind", "margin", "ent", "rel", "norm", "n_ent", "n_rel", "dim", "h", "r", "t",
        "n_rows", "head_batch", "out", "stream")
SIZES = dict(model=TRANSH_L1, norm_flag=1, pred_kind=0, margin=0.0, n_ent=300, n_rel=5, dim=16, n_query=130, n_tiles=6,
             n_used=5, n_groups=40, n_entries=7, work_bytes=1 << 62, stream=None, n_rows=9, head_batch=0,
             type_head=None, type_tail=None)


def run(params, name, **over):
    from mmre import _lib
    a = {p: SIZES[p] if p in SIZES else fake() for p in params}
    assert set(over) <= set(a)
    a.update(over)
    return getattr(_lib.lib(), name)(*[a[p] for p in params])


def test_entry_points_exist_with_signatures():
    from mmre import _lib
    L = _lib.lib()
    for name, n in (("mmre_transh_workspace", 6), ("mmre_transh_evaluate", len(EVAL)),
                    ("mmre_transh_score_rows", len(ROWS))):
        assert getattr(L, name, None) is not None, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    from mmre.link import MODEL_IDS
    assert MODEL_IDS["transh"] == TRANSH_L1 and MODEL_IDS["transh_l2"] == TRANSH_L2


def test_evaluate_error_codes():
    from mmre import _lib
    ev = lambda **o: run(EVAL, "mmre_transh_evaluate", **o)
    for p in ("ent", "rel", "norm", "qh", "qr", "qt", "qmode", "perm", "tiles", "used", "rel_slot", "counts", "truth",
              "work"):
        assert ev(**{p: None}) == ARG, p                    # a null table or array
    for m in (-1, 0, 1, 4, 7):
        assert ev(model=m) == MODEL, m                      # TransE .. RotatE have their own entry points
    assert ev(model=TRANSH_L2, dim=0) == SHAPE
    assert ev(dim=0) == SHAPE and ev(dim=-3) == SHAPE
    need = _lib.lib().mmre_transh_workspace(300, 5, 16, 6, 5, 7)
    assert need > 0
    assert ev(work_bytes=need - 1) == WORKSPACE and ev(work_bytes=0) == WORKSPACE
    # the exact size passes the workspace check: only with a fault that is answered earlier can
    # the call be made without a device, so pair it with one
    assert ev(work_bytes=need, n_query=0) == ARG
    for f in (dict(n_query=0), dict(n_ent=0), dict(n_rel=0), dict(n_tiles=0), dict(n_used=0), dict(n_used=6),
              dict(pred_kind=2), dict(pred_kind=-1), dict(type_head=fake()), dict(type_tail=fake()),
              dict(grp_q=None), dict(filt_off=None), dict(filt_ids=None), dict(entry_q=None), dict(n_groups=0)):
        assert ev(**f) == ARG, f
    assert ev(model=9, ent=None, dim=0, work_bytes=0) == MODEL   # the model answers first
    assert ev(ent=None, dim=0, work_bytes=0) == ARG
    assert ev(dim=0, work_bytes=0) == SHAPE
    assert ev(n_ent=(1 << 31) - 200) == SHAPE                    # entity ids stay int32


def test_score_rows_error_codes():
    rows = lambda **o: run(ROWS, "mmre_transh_score_rows", **o)
    for p in ("ent", "rel", "norm", "h", "r", "t", "out"):
        assert rows(**{p: None}) == ARG, p
    for m in (-1, 0, 4, 7):
        assert rows(model=m) == MODEL, m
    assert rows(dim=0) == SHAPE
    assert rows(pred_kind=5) == ARG and rows(n_rows=-1) == ARG and rows(n_ent=0) == ARG
    assert rows(n_rows=0, h=None, r=None, t=None, out=None) == 0  # nothing to score, nothing launched


def test_workspace_sizes():
    from mmre import _lib
    ws = _lib.lib().mmre_transh_workspace
    for bad in ((0, 5, 16, 6, 5, 7), (300, 0, 16, 6, 5, 7), (300, 5, 0, 6, 5, 7), (300, 5, 16, -1, 5, 7)):
        assert ws(*bad) == 0, bad
    # O(n_used * E + E * d): linear in the used relations with slope 2 * e_pad floats, no
    # n_used * E * d term
    a, b = ws(14541, 237, 200, 300, 10, 0), ws(14541, 237, 200, 300, 110, 0)
    assert b - a == 100 * 2 * 14592 * 4
    assert ws(14541, 237, 200, 300, 237, 0) < 237 * 14541 * 200 * 4 // 20   # projected tables: 2.76 GB


def test_old_entry_points_refuse_the_new_ids():
    import test_link_abi_cpu as old
    for m in (TRANSH_L1, TRANSH_L2):
        assert old.run("sweep", model=m) == MODEL
        assert old.run("prepare_entities", model=m) == MODEL
        assert old.run("truth_grouped", model=m) == MODEL


def test_score_spec_and_routing():
    from mmre.link import MODEL_IDS, ScoreSpec, evaluate_relation_prediction
    spec = ScoreSpec(model="transh", ent=torch.zeros(4, 8), rel=torch.zeros(2, 8), dim=8, norm_vec=torch.zeros(2, 8))
    assert spec.norm_vec is not None and MODEL_IDS[spec.model] == TRANSH_L1
    assert ScoreSpec(model="transe", ent=spec.ent, rel=spec.rel, dim=8).norm_vec is None
    with pytest.raises(NotImplementedError, match="TransH"):
        evaluate_relation_prediction(spec, [0], [0], [1])


def test_model_class_mirrors_the_reference():
    from openke.module.model import TransH
    m = TransH(ent_tot=7, rel_tot=3, dim=8, p_norm=2, norm_flag=False, margin=4.0, epsilon=2.0)
    base = {"zero_const", "pi_const"}  # BaseModule's, as in the reference
    tables = {"ent_embeddings.weight", "rel_embeddings.weight", "norm_vector.weight"}
    assert set(m.state_dict()) == base | tables | {"margin", "embedding_range"}
    assert not m.margin.requires_grad and m.margin_flag and float(m.embedding_range) == 0.75
    for emb in (m.ent_embeddings, m.rel_embeddings, m.norm_vector):
        assert float(emb.weight.abs().max()) <= 0.75
    assert m.ns_spec() is None
    s = m.score_spec()
    assert (s.model, s.pred_kind, s.margin, s.norm_flag) == ("transh_l2", 1, 4.0, False) and s.norm_vec is m.norm_vector.weight
    m2 = TransH(ent_tot=7, rel_tot=3, dim=8)
    assert set(m2.state_dict()) == base | tables
    assert m2.score_spec().pred_kind == 0 and m2.score_spec().model == "transh"
    # forward on the CPU is the reference's torch ops: differentiable, all three modes
    data = {"batch_h": torch.arange(7), "batch_t": torch.tensor([2]), "batch_r": torch.tensor([1]), "mode": "head_batch"}
    out = m2(data)
    assert out.shape == (7,)
    out.sum().backward()
    assert all(e.weight.grad is not None for e in (m2.ent_embeddings, m2.rel_embeddings, m2.norm_vector))
    want = R.score_rows(*(p.detach().numpy() for p in (m2.ent_embeddings.weight, m2.rel_embeddings.weight,
                                                        m2.norm_vector.weight)),
                        np.arange(7), np.full(7, 1), np.full(7, 2), True)
    assert np.allclose(out.detach().numpy(), want, rtol=1e-5, atol=1e-6)
