"""RESCAL without a GPU: the restatement of DESIGN.md §3 (tests/rescal_restate.py) against rational
arithmetic and against the reference's fixture, the plan over (relation, side) keys, the model
class, the routing, and the error codes of the RESCAL entry points for arguments they refuse before
anything is launched (addresses never dereferenced)."""
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import rescal_restate as R
from conftest import GOLDEN
from test_transr_cpu import dataset_counts, nearest_f32

SMALL = os.path.join(GOLDEN, "data", "small")
CONFIGS = [("d32", 32), ("d40", 40)]
TABLES = ("ent_embeddings", "rel_matrices")
RESCAL = 11


# ----------------------------------------------------------------- restatement vs rationals ---
def test_restatement_is_the_two_fused_chains():
    """A few rows in rational arithmetic: one rounding per fma, ascending j inside, ascending i
    outside, both from +0."""
    rng = np.random.default_rng(3)
    d, E, NR = 5, 6, 2
    ent = rng.standard_normal((E, d)).astype(np.float32)
    mats = rng.standard_normal((NR, d * d)).astype(np.float32)
    ent[4] = -ent[1]                                         # cancelling sums
    h, r, t = np.array([0, 1, 4, 5, 3]), np.array([0, 1, 1, 0, 1]), np.array([2, 4, 1, 5, 0])
    fr = lambda x: Fraction(float(x))
    want = []
    for hh, rr, tt in zip(h, r, t):
        M = mats[rr].reshape(d, d)
        s = np.float32(0.0)
        for i in range(d):
            tr = np.float32(0.0)
            for j in range(d):
                tr = nearest_f32(fr(M[i, j]) * fr(ent[tt, j]) + fr(tr))
            s = nearest_f32(fr(ent[hh, i]) * fr(tr) + fr(s))
        want.append(s)
    got = R.row_scores(ent, mats, h, r, t)
    assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float32))
    # the sweep restatement holds the same bits on either side
    for mode in (0, 1):
        s = R.sweep_scores(ent, mats, h, r, t, mode)
        assert s.shape == (len(h), E)
        assert np.array_equal(s[np.arange(len(h)), h if mode == 0 else t], got)
    mixed = R.sweep_scores(ent, mats, h, r, t, np.array([0, 1, 0, 1, 1]))
    assert np.array_equal(mixed[0], R.sweep_scores(ent, mats, h, r, t, 0)[0])
    assert np.array_equal(mixed[1], R.sweep_scores(ent, mats, h, r, t, 1)[1])
    # the bound's figure at d = 32, and the magnitude
    assert abs(R.bound(32) - 7.7e-6) < 1e-7
    A = R.magnitude(ent, mats, h, r, t)
    ref = [float(np.abs(ent[a].astype(np.float64)) @ np.abs(mats[b].astype(np.float64)).reshape(d, d)
                 @ np.abs(ent[c].astype(np.float64))) for a, b, c in zip(h, r, t)]
    assert np.allclose(A, ref, rtol=1e-12)
    exact = [float(sum(fr(ent[a, i]) * fr(mats[b].reshape(d, d)[i, j]) * fr(ent[c, j]) for i in range(d)
                       for j in range(d))) for a, b, c in zip(h, r, t)]
    assert np.all(np.abs(got.astype(np.float64) - exact) <= 0.5 * R.bound(d) * A)


# ------------------------------------------------------------------ restatement vs golden ---
@pytest.fixture(scope="module")
def small():
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    ds = OpenKEDataset(SMALL)
    return ds, FilterIndex(*ds.all_triples(), ds.n_ent, ds.n_rel)


@pytest.mark.parametrize("name,d", CONFIGS)
def test_restatement_matches_the_reference(golden, small, name, d):
    g = golden("rescal_small")
    ds, index = small
    ent, mats = (g[f"{name}.{k}.weight"] for k in TABLES)
    assert ent.shape == (257, d) and mats.shape == (13, d * d)
    assert float(g[f"{name}.scale"]) == 8.0                  # make_rescal.py: both tables stored times 8
    assert float(g[f"{name}.restate_dev"]) <= R.bound(d)
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    T, ids = len(qh), np.arange(257)
    for side, head in (("head", True), ("tail", False)):
        s = R.sweep_scores(ent, mats, qh, qr, qt, 0 if head else 1)
        ref = g[f"{name}.pred_{side}"]
        n = len(ref)
        A = R.magnitude(ent, mats, ids[None, :] if head else qh[:n, None], qr[:n, None],
                        qt[:n, None] if head else ids[None, :])
        diff = np.abs(s[:n].astype(np.float64) - ref)
        print(f"{name} {side}: restatement within {float((diff / A).max()):.3g} A of the reference "
              f"(bound {R.bound(d):.3g} A), largest deviation {diff.max():.3g}")
        assert np.all(diff <= R.bound(d) * A), side                                  # condition 2
        assert float(g[f"{name}.max_abs_dev_{side}"]) < 0.5 * float(g[f"{name}.gap_{side}"])
        c = dataset_counts(s, qh, qr, qt, head, ds, index)
        assert np.array_equal(c[:2].T, g[f"{name}.tc0_{side}_counts"][:, :2]), side  # condition 3
        assert np.array_equal(c.T, g[f"{name}.tc1_{side}_counts"]), side
        # the row restatement is the sweep restatement's diagonal, bit for bit
        assert np.array_equal(R.row_scores(ent, mats, qh, qr, qt), s[np.arange(T), qh if head else qt])


# --------------------------------------------------------------------------------- the plan ---
def test_plan_over_relation_side_keys():
    from mmre.rescal import plan_keys
    from mmre.transh import plan_tiles
    from test_transh_cpu import check_plan
    rng = np.random.default_rng(9)
    # relation 0: 129 tail-side queries and no head-side one; 1: both sides; 2: none; 3: head side only
    qr = np.concatenate([np.zeros(129), np.ones(40), np.full(3, 3)]).astype(np.int64)
    qm = np.concatenate([np.ones(129), rng.integers(0, 2, 40), np.zeros(3)]).astype(np.int8)
    qm[129], qm[130] = 0, 1
    order = rng.permutation(len(qr))
    qr, qm = qr[order], qm[order]
    plan = plan_keys(qr, qm)
    key = 2 * qr + qm
    ref = plan_tiles(key)
    check_plan(key, dict(plan, used=ref["used"]))            # plan_tiles' contract, over keys
    assert np.array_equal(plan["perm"], ref["perm"]) and np.array_equal(plan["tiles"], ref["tiles"])
    tiles = plan["tiles"]
    assert tiles[:, 0].tolist() == [1, 1, 2, 3, 6]           # a key's tiles consecutive, absent sides none
    assert tiles[:, 2].tolist()[:2] == [128, 1]              # 129 queries of one key: 128 + 1
    assert plan["used"].dtype == np.int32 and plan["used"].tolist() == [0, 1, 3]
    assert plan["padding"] == 5 * 128 / len(qr)
    small = plan_keys(qr, qm, tile=3)
    assert small["tiles"][:, 2].max() == 3 and len(small["tiles"]) == 43 + sum(-(-int(c) // 3) for c in
                                                                                 np.bincount(key[qr == 1])) + 1
    with pytest.raises(ValueError, match="mode"):
        plan_keys([0, 1], [0, 2])
    empty = plan_keys([], [])
    assert len(empty["tiles"]) == 0 and len(empty["used"]) == 0 and empty["padding"] == 1.0


# ------------------------------------------------------------------------------- the ABI ---
ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
_addr = itertools.count(1 << 21, 4096)
fake = lambda: next(_addr)  # distinct, aligned, never dereferenced

EVAL = ("model", "pred_kind", "ent", "rel_matrices", "n_ent", "n_rel", "dim", "qh", "qr", "qt", "qmode", "n_query",
        "perm", "tiles", "n_tiles", "used", "n_used", "rel_slot", "grp_qoff", "grp_q", "n_groups", "filt_off",
        "filt_ids", "entry_q", "n_entries", "type_head", "type_tail", "counts", "truth", "work", "work_bytes", "stream")
ROWS = ("model", "pred_kind", "ent", "rel_matrices", "n_ent", "n_rel", "dim", "h", "r", "t", "n_rows", "out", "stream")
SIZES = dict(model=RESCAL, pred_kind=0, n_ent=300, n_rel=5, dim=24, n_query=130, n_tiles=6, n_used=5, n_groups=40,
             n_entries=7, work_bytes=1 << 62, stream=None, n_rows=9, type_head=None, type_tail=None)


def run(params, name, **over):
    from mmre import _lib
    a = {p: SIZES[p] if p in SIZES else fake() for p in params}
    assert set(over) <= set(a)
    a.update(over)
    return getattr(_lib.lib(), name)(*[a[p] for p in params])


def test_entry_points_exist_with_signatures():
    from mmre import _lib
    L = _lib.lib()
    for name, n in (("mmre_rescal_workspace", 6), ("mmre_rescal_evaluate", len(EVAL)),
                    ("mmre_rescal_score_rows", len(ROWS))):
        assert getattr(L, name, None) is not None, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    from mmre import rescal, transh
    from mmre.link import MODEL_IDS
    assert MODEL_IDS["rescal"] == RESCAL and rescal.MODEL_IDS == {"rescal": 11}
    assert rescal.plan_tiles is transh.plan_tiles and rescal.TILE == transh.TILE   # imported, not copied
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mmre.h")).read()
    for word in ("MMRE_RESCAL = 11", "mmre_rescal_workspace(", "mmre_rescal_evaluate(", "mmre_rescal_score_rows(",
                 "d_rel_matrices"):
        assert word in header, word


def test_evaluate_error_codes():
    from mmre import _lib
    ev = lambda **o: run(EVAL, "mmre_rescal_evaluate", **o)
    for p in ("ent", "rel_matrices", "qh", "qr", "qt", "qmode", "perm", "tiles", "used", "rel_slot", "counts", "truth",
              "work"):
        assert ev(**{p: None}) == ARG, p                    # a null table or array
    for m in list(range(-1, 11)) + [12]:
        assert ev(model=m) == MODEL, m                      # models 0 .. 10 have their own entry points
    assert ev(dim=0) == SHAPE and ev(dim=-3) == SHAPE and ev(dim=513) == SHAPE
    need = _lib.lib().mmre_rescal_workspace(300, 5, 24, 6, 5, 7)
    assert need > 0
    assert ev(work_bytes=need - 1) == WORKSPACE and ev(work_bytes=0) == WORKSPACE
    assert ev(dim=1, work_bytes=0) == WORKSPACE and ev(dim=512, work_bytes=0) == WORKSPACE
    assert ev(work_bytes=need, n_query=0) == ARG
    for f in (dict(n_query=0), dict(n_ent=0), dict(n_rel=0), dict(n_tiles=0), dict(n_used=0), dict(n_used=6),
              dict(pred_kind=1), dict(pred_kind=3), dict(pred_kind=-1), dict(type_head=fake()), dict(type_tail=fake()),
              dict(grp_q=None), dict(filt_off=None), dict(filt_ids=None), dict(entry_q=None), dict(n_groups=0)):
        assert ev(**f) == ARG, f
    assert ev(pred_kind=2, work_bytes=0) == WORKSPACE       # -s: forward's order
    assert ev(model=5, ent=None, dim=0, work_bytes=0) == MODEL     # the model answers first
    assert ev(ent=None, dim=0, work_bytes=0) == ARG                # then null pointers
    assert ev(dim=0, work_bytes=0) == SHAPE                        # then the shape, then the workspace
    assert ev(n_ent=(1 << 31) - 200) == SHAPE                      # entity ids stay int32


def test_score_rows_error_codes():
    rows = lambda **o: run(ROWS, "mmre_rescal_score_rows", **o)
    for p in ("ent", "rel_matrices", "h", "r", "t", "out"):
        assert rows(**{p: None}) == ARG, p
    for m in list(range(-1, 11)) + [12]:
        assert rows(model=m) == MODEL, m
    assert rows(dim=0) == SHAPE and rows(dim=513) == SHAPE
    assert rows(model=6, ent=None, dim=0) == MODEL and rows(ent=None, dim=0) == ARG
    assert rows(pred_kind=5) == ARG and rows(pred_kind=-1) == ARG and rows(n_rows=-1) == ARG and rows(n_ent=0) == ARG
    assert rows(n_rows=0, h=None, r=None, t=None, out=None) == 0  # nothing to score, nothing launched


def test_workspace_sizes():
    from mmre import _lib
    ws = _lib.lib().mmre_rescal_workspace
    for bad in ((0, 5, 24, 6, 5, 7), (300, 0, 24, 6, 5, 7), (300, 5, 0, 6, 5, 7), (300, 5, 513, 6, 5, 7),
                (300, 5, 24, -1, 5, 7), (300, 5, 24, 6, -1, 7), (300, 5, 24, 6, 5, -1)):
        assert ws(*bad) == 0, bad
    assert ws(300, 5, 1, 6, 5, 7) > 0 and ws(300, 5, 512, 6, 5, 7) > 0
    # every used relation's plane is held at once: linear in n_used, one round_up(d, 16) x e_pad plane each
    e_pad = 14592                                            # FB15K237: 14,541 entities in 114 tiles
    a, b = ws(14541, 237, 50, 320, 10, 0), ws(14541, 237, 50, 320, 110, 0)
    assert b - a == 100 * 64 * e_pad * 4
    assert ws(14541, 237, 50, 320, 0, 0) > 64 * e_pad * 4    # the k-major copy of the entity table is there too
    full = ws(14541, 237, 50, 320, 237, 0)
    assert 238 * 64 * e_pad * 4 <= full < 238 * 64 * e_pad * 4 + (16 << 20)   # 889 MB of planes (mmre.h)
    c2 = ws(14541, 237, 50, 320, 29, 0)
    assert 30 * 64 * e_pad * 4 <= c2 < 30 * 64 * e_pad * 4 + (16 << 20)       # 29 used relations: 112 MB
    prev = 0
    for n_used in range(0, 12):
        cur = ws(300, 5, 24, 6, n_used, 7)
        assert cur > prev
        prev = cur
    base = (300, 5, 24, 6, 5, 7)
    for i in (0, 2, 3, 4, 5):
        more = list(base)
        more[i] = base[i] * 3 + 200 if i != 2 else 500
        assert ws(*more) >= ws(*base), i


def test_other_entry_points_refuse_rescal():
    import test_link_abi_cpu as link
    import test_transd_cpu as td
    import test_transh_cpu as th
    import test_transr_cpu as tr
    import test_tripleclass_cpu as tc
    from mmre import _lib
    L = _lib.lib()
    for name in link.PARAMS:
        if "model" in link.PARAMS[name]:
            # (the raw-row split-bf16 sweep names anything but DistMult a SHAPE fault, as for every other id)
            assert link.run(name, model=RESCAL) == (SHAPE if name == "sweep_bf3_rows" else MODEL), name
    for name in ("scores", "evaluate"):
        assert tc.run(name, model=RESCAL) == MODEL, name
    assert th.run(th.EVAL, "mmre_transh_evaluate", model=RESCAL) == MODEL
    assert th.run(th.ROWS, "mmre_transh_score_rows", model=RESCAL) == MODEL
    assert td.run(td.EVAL, "mmre_transd_evaluate", model=RESCAL) == MODEL
    assert td.run(td.ROWS, "mmre_transd_score_rows", model=RESCAL) == MODEL
    assert tr.run(tr.EVAL, "mmre_transr_evaluate", model=RESCAL) == MODEL
    assert tr.run(tr.ROWS, "mmre_transr_score_rows", model=RESCAL) == MODEL
    assert not L.mmre_ns_fused_supported(RESCAL, 64, 4, 0)
    assert L.mmre_rel_workspace(RESCAL, 5, 8) < 0


# --------------------------------------------------------------------- spec, routing, model ---
def test_score_spec_and_routing():
    from mmre.link import LinkSweep, MODEL_IDS, ScoreSpec, evaluate_relation_prediction
    from mmre.rescal import RescalSweep, is_rescal, score_rows
    z = torch.zeros
    spec = ScoreSpec(model="rescal", ent=z(4, 6), rel=None, dim=6, rel_matrices=z(2, 36))
    assert is_rescal(spec) and MODEL_IDS[spec.model] == RESCAL
    plain = ScoreSpec(model="transe", ent=spec.ent, rel=z(2, 6), dim=6)
    assert plain.rel_matrices is None and not is_rescal(plain)
    with pytest.raises(ValueError, match="RescalSweep"):
        LinkSweep(spec)
    with pytest.raises(NotImplementedError, match="RESCAL"):
        evaluate_relation_prediction(spec, [0], [0], [1])
    with pytest.raises(ValueError, match="not a RESCAL spec"):
        RescalSweep(plain)
    # the tables are checked before anything touches the device
    with pytest.raises(ValueError, match="rel_matrices"):
        score_rows(ScoreSpec(model="rescal", ent=z(4, 6), rel=None, dim=6), [0], [0], [1])


def test_model_class_mirrors_the_reference():
    from openke.module.model import RESCAL as Model
    torch.manual_seed(7)
    m = Model(ent_tot=7, rel_tot=3, dim=6)
    base = {"zero_const", "pi_const"}  # BaseModule's, as in the reference
    assert set(m.state_dict()) == base | {"ent_embeddings.weight", "rel_matrices.weight"}
    assert list(m.state_dict())[-2:] == ["ent_embeddings.weight", "rel_matrices.weight"]   # the reference's order
    assert tuple(m.ent_embeddings.weight.shape) == (7, 6) and tuple(m.rel_matrices.weight.shape) == (3, 36)
    assert Model(ent_tot=7, rel_tot=3).dim == 100
    # the initialisation order: entities first, then the matrices, both xavier_uniform
    # (nn.Embedding draws its own normal weights first: two draws precede the xavier ones)
    torch.manual_seed(7)
    torch.nn.Embedding(7, 6), torch.nn.Embedding(3, 36)
    e2 = torch.nn.init.xavier_uniform_(torch.empty(7, 6))
    r2 = torch.nn.init.xavier_uniform_(torch.empty(3, 36))
    assert torch.equal(m.ent_embeddings.weight.detach(), e2) and torch.equal(m.rel_matrices.weight.detach(), r2)
    assert m.ns_spec() is None and not any(hasattr(m, k) for k in ("fused_ns", "fused_ns_transd", "fused_ns_transr"))
    s = m.score_spec()
    assert (s.model, s.pred_kind, s.margin, s.dim, s.rel) == ("rescal", 0, 0.0, 6, None)
    assert s.rel_matrices is m.rel_matrices.weight and s.ent is m.ent_embeddings.weight
    # forward on the CPU is the reference's torch ops, in every mode, differentiable into both tables
    ent, mats = m.ent_embeddings.weight.detach().numpy(), m.rel_matrices.weight.detach().numpy()
    for data, (h, r, t) in (
            ({"batch_h": torch.arange(7), "batch_t": torch.tensor([2]), "batch_r": torch.tensor([1]),
              "mode": "head_batch"}, (np.arange(7), np.full(7, 1), np.full(7, 2))),
            ({"batch_h": torch.tensor([3]), "batch_t": torch.arange(7), "batch_r": torch.tensor([0]),
              "mode": "tail_batch"}, (np.full(7, 3), np.full(7, 0), np.arange(7))),
            ({"batch_h": torch.tensor([0, 5, 6]), "batch_t": torch.tensor([1, 5, 2]), "batch_r": torch.tensor([2, 0, 1]),
              "mode": "normal"}, (np.array([0, 5, 6]), np.array([2, 0, 1]), np.array([1, 5, 2])))):
        m.zero_grad()
        out = m(data)
        assert out.shape == (len(h),)
        want = -R.row_scores(ent, mats, h, r, t)
        assert np.all(np.abs(out.detach().numpy() - want) <= R.bound(6) * R.magnitude(ent, mats, h, r, t))
        out.sum().backward()
        for emb in (m.ent_embeddings, m.rel_matrices):
            assert emb.weight.grad is not None and float(emb.weight.grad.abs().sum()) > 0
        reg = m.regularization(data)
        want_reg = ((ent[h] ** 2).mean() + (ent[t] ** 2).mean() + (mats[r] ** 2).mean()) / 3
        assert abs(float(reg.detach()) - want_reg) < 1e-6
