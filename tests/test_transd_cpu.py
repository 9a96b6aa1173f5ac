"""TransD without a GPU: the restatement of DESIGN.md §3 (tests/transd_restate.py) against the
reference's fixture, the identity that lets TransH's kernels serve TransD, the model class, the
routing, and the error codes of the TransD entry points for arguments they refuse before anything
is launched (addresses never dereferenced)."""
import itertools
import os

import numpy as np
import pytest
import torch

import transd_restate as D
import transh_restate as H
from conftest import GOLDEN

SMALL = os.path.join(GOLDEN, "data", "small")
CONFIGS = [("l1_norm", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, margin=None)),
           ("l2_norm_narrow", dict(dim_e=40, dim_r=32, p_norm=2, norm_flag=True, margin=None)),
           ("l1_nonorm_margin", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=False, margin=5.0))]
TABLES = ("ent_embeddings", "ent_transfer", "rel_embeddings", "rel_transfer")
TRANSD_L1, TRANSD_L2 = 7, 8
REL = 1e-6  # tests/golden/make_transh.py's bound on the restatement, carried over


def calc(kw):
    return {k: kw[k] for k in ("p_norm", "norm_flag", "margin")}


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
    return D.rank_counts(scores, qh if head else qt, known, allowed)


@pytest.mark.parametrize("name,kw", CONFIGS)
def test_restatement_matches_the_reference(golden, small, name, kw):
    g = golden("transd_small")
    ds, index = small
    tabs = [g[f"{name}.{k}.weight"] for k in TABLES]
    assert tabs[0].shape == (257, kw["dim_e"]) and tabs[3].shape == (13, kw["dim_r"])
    assert float(g[f"{name}.restate_rel_dev"]) <= REL
    m = float(g[f"{name}.margin"][0])                        # NaN: a model without a margin
    assert (kw["margin"] is None and np.isnan(m)) or m == kw["margin"]
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    T = len(qh)
    for side, head in (("head", True), ("tail", False)):
        s = D.sweep_scores(*tabs, qh, qr, qt, np.full(T, 0 if head else 1), **calc(kw))
        ref = g[f"{name}.pred_{side}"]
        dev = np.abs(s[:len(ref)].astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)
        assert dev.max() <= REL, (side, dev.max())
        c = dataset_counts(s, qh, qr, qt, head, ds, index)
        assert np.array_equal(c[:2].T, g[f"{name}.tc0_{side}_counts"][:, :2]), side
        assert np.array_equal(c.T, g[f"{name}.tc1_{side}_counts"]), side
        # the row restatement is the sweep restatement's diagonal, bit for bit
        rows = D.score_rows(*tabs, qh, qr, qt, head, **calc(kw))
        assert np.array_equal(rows, s[np.arange(T), qh if head else qt])


# --------------------------------------------------------------- the kernel-reuse identity ---
def hand_placed(rng, E, R, dim_e, dim_r):
    """Random tables with the rows of the GPU test placed by hand (tests/test_transd_gpu.py)."""
    f = np.float32
    ent = rng.uniform(-0.5, 0.5, (E, dim_e)).astype(f)
    ept = rng.uniform(-0.5, 0.5, (E, dim_e)).astype(f)
    rel = rng.uniform(-0.5, 0.5, (R, dim_r)).astype(f)
    rpt = rng.uniform(-0.5, 0.5, (R, dim_r)).astype(f)
    ent[1] = 0.0                                            # a zero entity row
    ept[2] = 0.0                                            # s = 0
    rpt[1] = 0.0                                            # u = e
    rel[2] = 0.0                                            # a zero relation row
    c = f(0.75)                                             # u cancels under relation 3: e[:dim_r] = c rp, s = -c
    ent[3, :dim_r], ent[3, dim_r:] = c * rpt[3], 0.0
    ept[3] = -c * ent[3] / f((ent[3].astype(np.float64) ** 2).sum())
    rpt[4] *= f(7.0) / f(np.sqrt((rpt[4].astype(np.float64) ** 2).sum()))   # a transfer row of length 7
    ent[5], ept[5] = ent[6], ept[6]                         # an exact copy, both rows
    return ent, ept, rel, rpt


@pytest.mark.parametrize("norm_flag", [True, False])
@pytest.mark.parametrize("p_norm", [1, 2])
@pytest.mark.parametrize("dim_e,dim_r", [(20, 20), (28, 20)])
def test_transh_element_on_the_transd_table_is_transd(dim_e, dim_r, p_norm, norm_flag):
    """k_sweep_transh stages p = (e - a w) / n. With a = -s, w = the raw rel_transfer row and n = N
    that is TransD's operand, so TransH's chain over it is TransD's score, bit for bit."""
    rng = np.random.default_rng(7 + dim_e)
    E, R = 40, 6
    ent, ept, rel, rpt = hand_placed(rng, E, R, dim_e, dim_r)
    Q = 60
    qh, qt, qr = rng.integers(0, E, Q), rng.integers(0, E, Q), rng.integers(0, R, Q)
    qm = rng.integers(0, 2, Q)
    qr[:6] = np.arange(6)
    qh[:6], qt[:6] = [1, 2, 3, 3, 5, 6], [3, 1, 6, 2, 6, 5]
    want = D.sweep_scores(ent, ept, rel, rpt, qh, qr, qt, qm, p_norm, norm_flag, 5.0)
    s = D.transfer_s(ent, ept)
    r_hat = D.relation_vectors(rel, norm_flag)
    got = np.zeros_like(want)
    for r in range(R):
        a, n, _ = D.a_and_n(ent, s, rpt[r], norm_flag)
        assert np.all(np.isfinite(n)) and np.all(n > 0)
        p = ((ent[:, :dim_r] - a[:, None] * rpt[r]) / n[:, None]).astype(np.float32)   # th_p<true>
        for i in np.nonzero(qr == r)[0]:
            head = qm[i] == 0
            q = H.query_vector(p[qt[i] if head else qh[i]], r_hat[r], head)
            got[i] = H.pred(H.chain(q[None, :], p, p_norm), 5.0)
    assert np.array_equal(got, want)
    # the sign identities behind a = -s: (-s) x == -(s x), y - (-z) == y + z
    x = rpt[qr][:, 0]
    assert np.array_equal((-s[qh]) * x, -(s[qh] * x))
    assert np.array_equal(ent[qh, 0] - (-s[qh]) * x, ent[qh, 0] + s[qh] * x)
    # hand-placed rows: the cancelling entity has s = -c and u ~ 0 under relation 3 only; the zero
    # rows project to 0; the copy scores as its source
    a3, n3, u3 = D.a_and_n(ent[3], s[3], rpt[3], norm_flag)
    assert abs(float(a3) - 0.75) < 1e-6 and float(np.abs(u3).max()) < 1e-6
    assert not D.project(ent[1], s[1], rpt[0], norm_flag).any() and s[1] == 0 and s[2] == 0
    assert np.array_equal(want[:, 5], want[:, 6])


# ------------------------------------------------------------------------------- the ABI ---
ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, aligned, never dereferenced

EVAL = ("model", "norm_flag", "pred_kind", "margin", "ent", "ent_transfer", "rel", "rel_transfer", "ent_narrow",
        "n_ent", "n_rel", "dim_e", "dim_r", "qh", "qr", "qt", "qmode", "n_query", "perm", "tiles", "n_tiles", "used",
        "n_used", "rel_slot", "grp_qoff", "grp_q", "n_groups", "filt_off", "filt_ids", "entry_q", "n_entries",
        "type_head", "type_tail", "counts", "truth", "work", "work_bytes", "stream")
ROWS = ("model", "norm_flag", "pred_kind", "margin", "ent", "ent_transfer", "rel", "rel_transfer", "n_ent", "n_rel",
        "dim_e", "dim_r", "h", "r", "t", "n_rows", "head_batch", "out", "stream")
SIZES = dict(model=TRANSD_L1, norm_flag=1, pred_kind=0, margin=0.0, n_ent=300, n_rel=5, dim_e=24, dim_r=16, n_query=130,
             n_tiles=6, n_used=5, n_groups=40, n_entries=7, work_bytes=1 << 62, stream=None, n_rows=9, head_batch=0,
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
    for name, n in (("mmre_transd_workspace", 7), ("mmre_transd_evaluate", len(EVAL)),
                    ("mmre_transd_score_rows", len(ROWS))):
        assert getattr(L, name, None) is not None, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    from mmre import transd
    from mmre.link import MODEL_IDS
    assert MODEL_IDS["transd"] == TRANSD_L1 and MODEL_IDS["transd_l2"] == TRANSD_L2
    assert transd.MODEL_IDS == {"transd": 7, "transd_l2": 8}
    from mmre import transh
    assert transd.plan_tiles is transh.plan_tiles and transd.TILE == transh.TILE   # imported, not copied
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mmre.h")).read()
    for word in ("MMRE_TRANSD_L1 = 7", "MMRE_TRANSD_L2 = 8", "mmre_transd_workspace(", "mmre_transd_evaluate(",
                 "mmre_transd_score_rows("):
        assert word in header, word


def test_evaluate_error_codes():
    from mmre import _lib
    ev = lambda **o: run(EVAL, "mmre_transd_evaluate", **o)
    for p in ("ent", "ent_transfer", "rel", "rel_transfer", "ent_narrow", "qh", "qr", "qt", "qmode", "perm", "tiles",
              "used", "rel_slot", "counts", "truth", "work"):
        assert ev(**{p: None}) == ARG, p                    # a null table or array
    for m in (-1, 0, 1, 4, 5, 6, 9):
        assert ev(model=m) == MODEL, m                      # TransE .. TransH have their own entry points
    assert ev(model=TRANSD_L2, dim_r=0) == SHAPE and ev(dim_r=-3) == SHAPE
    assert ev(dim_e=15) == SHAPE and ev(dim_e=0) == SHAPE   # dim_e < dim_r
    need = _lib.lib().mmre_transd_workspace(300, 5, 24, 16, 6, 5, 7)
    assert need > 0
    assert ev(work_bytes=need - 1) == WORKSPACE and ev(work_bytes=0) == WORKSPACE
    # the exact size passes the workspace check: only with a fault that is answered earlier can
    # the call be made without a device, so pair it with one
    assert ev(work_bytes=need, n_query=0) == ARG
    for f in (dict(n_query=0), dict(n_ent=0), dict(n_rel=0), dict(n_tiles=0), dict(n_used=0), dict(n_used=6),
              dict(pred_kind=2), dict(pred_kind=-1), dict(type_head=fake()), dict(type_tail=fake()),
              dict(grp_q=None), dict(filt_off=None), dict(filt_ids=None), dict(entry_q=None), dict(n_groups=0)):
        assert ev(**f) == ARG, f
    assert ev(model=5, ent=None, dim_e=3, work_bytes=0) == MODEL   # the model answers first
    assert ev(ent=None, dim_e=3, work_bytes=0) == ARG              # then null pointers
    assert ev(dim_e=3, work_bytes=0) == SHAPE                      # then the shape, then the workspace
    assert ev(n_ent=(1 << 31) - 200) == SHAPE                      # entity ids stay int32


def test_score_rows_error_codes():
    rows = lambda **o: run(ROWS, "mmre_transd_score_rows", **o)
    for p in ("ent", "ent_transfer", "rel", "rel_transfer", "h", "r", "t", "out"):
        assert rows(**{p: None}) == ARG, p
    for m in (-1, 0, 4, 5, 6, 9):
        assert rows(model=m) == MODEL, m
    assert rows(dim_r=0) == SHAPE and rows(dim_e=15) == SHAPE
    assert rows(model=6, ent=None, dim_e=3) == MODEL and rows(ent=None, dim_e=3) == ARG
    assert rows(pred_kind=5) == ARG and rows(n_rows=-1) == ARG and rows(n_ent=0) == ARG
    assert rows(n_rows=0, h=None, r=None, t=None, out=None) == 0  # nothing to score, nothing launched


def test_workspace_sizes():
    from mmre import _lib
    ws, th = _lib.lib().mmre_transd_workspace, _lib.lib().mmre_transh_workspace
    for bad in ((0, 5, 24, 16, 6, 5, 7), (300, 0, 24, 16, 6, 5, 7), (300, 5, 24, 0, 6, 5, 7), (300, 5, 15, 16, 6, 5, 7),
                (300, 5, 24, 16, -1, 5, 7), (300, 5, 24, 16, 6, -1, 7), (300, 5, 24, 16, 6, 5, -1)):
        assert ws(*bad) == 0, bad
    # the layout: TransH's workspace at dim_r, then s -- e_pad floats -- whatever dim_e is
    for shape in ((300, 5, 16, 6, 5, 7), (14541, 237, 200, 300, 29, 0), (1, 1, 1, 0, 0, 0)):
        n_ent, n_rel, dim_r = shape[:3]
        e_pad = -(-n_ent // 128) * 128
        want = th(*shape) + -(-e_pad * 4 // 256) * 256
        assert ws(n_ent, n_rel, dim_r, dim_r, *shape[3:]) == want, shape
        assert ws(n_ent, n_rel, dim_r + 40, dim_r, *shape[3:]) == want, shape
    # monotone in every size it depends on
    base = (300, 5, 24, 16, 6, 5, 7)
    for i in (0, 1, 3, 4, 5, 6):
        more = list(base)
        more[i] = base[i] * 3 + 200
        if i == 3:
            more[2] = more[3]
        assert ws(*more) >= ws(*base), i
    a, b = ws(14541, 237, 200, 200, 300, 10, 0), ws(14541, 237, 200, 200, 300, 110, 0)
    assert b - a == 100 * 2 * 14592 * 4                     # linear in the used relations, no E * d term


def test_older_entry_points_refuse_the_new_ids():
    import test_link_abi_cpu as link
    import test_ns_abi_cpu as ns
    import test_transh_cpu as th
    import test_transh_train_cpu as tht
    import test_tripleclass_cpu as tc
    from mmre import _lib
    L = _lib.lib()
    for m in (TRANSD_L1, TRANSD_L2):
        for name in link.PARAMS:
            if "model" in link.PARAMS[name]:
                # (the raw-row split-bf16 sweep names anything but DistMult a SHAPE fault, as for every other id)
                assert link.run(name, model=m) == (SHAPE if name == "sweep_bf3_rows" else MODEL), (name, m)
        for name in ns.PARAMS:
            if "model" in ns.PARAMS[name]:
                for n, ex in ns.both(name):
                    assert ns.run(n, ex, model=m) == MODEL, (n, ex, m)
        assert not L.mmre_ns_fused_supported(m, 64, 4, 0)
        for name in ("scores", "evaluate"):
            assert tc.run(name, model=m) == MODEL, (name, m)
        assert th.run(th.EVAL, "mmre_transh_evaluate", model=m) == MODEL
        assert th.run(th.ROWS, "mmre_transh_score_rows", model=m) == MODEL
        for name in tht.PARAMS:
            assert tht.run(name, model=m) == MODEL, (name, m)
        assert not L.mmre_transh_ns_supported(m, 64, 4)
        assert L.mmre_rel_workspace(m, 5, 8) < 0
        assert L.mmre_rel_evaluate(m, 1, 0, 0.0, fake(), None, fake(), None, 40, 5, 16, 0.0, fake(), fake(), fake(), 9,
                                   None, None, fake(), fake(), None, fake(), 1 << 40, None) == MODEL


# --------------------------------------------------------------------- spec, routing, model ---
def test_score_spec_and_routing():
    from mmre.link import LinkSweep, MODEL_IDS, ScoreSpec, evaluate_relation_prediction
    from mmre.transd import is_transd
    z = torch.zeros
    spec = ScoreSpec(model="transd", ent=z(4, 10), rel=z(2, 8), dim=8, ent_transfer=z(4, 10), rel_transfer=z(2, 8),
                     dim_e=10)
    assert is_transd(spec) and MODEL_IDS[spec.model] == TRANSD_L1
    plain = ScoreSpec(model="transe", ent=spec.ent, rel=spec.rel, dim=8)
    assert plain.ent_transfer is None and plain.rel_transfer is None and plain.dim_e == 0 and not is_transd(plain)
    with pytest.raises(ValueError, match="TransDSweep"):
        LinkSweep(spec)
    with pytest.raises(NotImplementedError, match="TransD"):
        evaluate_relation_prediction(spec, [0], [0], [1])


def test_model_class_mirrors_the_reference():
    from openke.module.model import TransD
    m = TransD(ent_tot=7, rel_tot=3, dim_e=10, dim_r=8, p_norm=2, norm_flag=False, margin=4.0, epsilon=2.0)
    base = {"zero_const", "pi_const"}  # BaseModule's, as in the reference
    tables = {f"{k}.weight" for k in TABLES}
    assert set(m.state_dict()) == base | tables | {"margin", "ent_embedding_range", "rel_embedding_range"}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items() if k in tables} == {
        "ent_embeddings.weight": (7, 10), "ent_transfer.weight": (7, 10), "rel_embeddings.weight": (3, 8),
        "rel_transfer.weight": (3, 8)}
    assert not m.margin.requires_grad and m.margin_flag
    assert float(m.ent_embedding_range) == np.float32(0.6) and float(m.rel_embedding_range) == 0.75
    for emb, bound in ((m.ent_embeddings, 0.6), (m.ent_transfer, 0.6), (m.rel_embeddings, 0.75), (m.rel_transfer, 0.75)):
        assert float(emb.weight.detach().abs().max()) <= np.float32(bound)
    assert m.ns_spec() is None and not hasattr(m, "fused_ns")
    s = m.score_spec()
    assert (s.model, s.pred_kind, s.margin, s.norm_flag, s.dim, s.dim_e) == ("transd_l2", 1, 4.0, False, 8, 10)
    assert s.ent_transfer is m.ent_transfer.weight and s.rel_transfer is m.rel_transfer.weight
    m2 = TransD(ent_tot=7, rel_tot=3, dim_e=8, dim_r=8)
    assert set(m2.state_dict()) == base | tables and not m2.margin_flag
    assert m2.score_spec().pred_kind == 0 and m2.score_spec().model == "transd"
    # xavier_uniform: bound sqrt(6 / (rows + cols))
    assert float(m2.ent_embeddings.weight.detach().abs().max()) <= np.sqrt(6.0 / 15) + 1e-6
    m3 = TransD(ent_tot=7, rel_tot=3, dim_e=8, dim_r=8, margin=3.0)     # a margin without epsilon: xavier, margin kept
    assert m3.margin_flag and set(m3.state_dict()) == base | tables | {"margin"}
    # forward on the CPU is the reference's torch ops: differentiable into all four tables
    data = {"batch_h": torch.arange(7), "batch_t": torch.tensor([2]), "batch_r": torch.tensor([1]), "mode": "head_batch"}
    out = m2(data)
    assert out.shape == (7,)
    out.sum().backward()
    for emb in (m2.ent_embeddings, m2.ent_transfer, m2.rel_embeddings, m2.rel_transfer):
        assert emb.weight.grad is not None and float(emb.weight.grad.abs().sum()) > 0
    want = D.score_rows(*(getattr(m2, k).weight.detach().numpy() for k in TABLES), np.arange(7), np.full(7, 1),
                        np.full(7, 2), True)
    assert np.allclose(out.detach().numpy(), want, rtol=1e-5, atol=1e-6)
    assert float(m2.regularization(data)) > 0


@pytest.mark.parametrize("name,kw", CONFIGS)
def test_forward_equals_the_reference_rows(golden, name, kw):
    from openke.module.model import TransD
    g = golden("transd_small")
    model = TransD(ent_tot=257, rel_tot=13, dim_e=kw["dim_e"], dim_r=kw["dim_r"], p_norm=kw["p_norm"],
                   norm_flag=kw["norm_flag"], margin=kw["margin"])
    sd = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in g.items()
          if k.startswith(name + ".") and k.endswith((".weight", ".margin", "_const")) and not np.isnan(v).any()}
    model.load_state_dict(sd, strict=True)
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    ids = torch.arange(257)
    for side in ("head", "tail"):
        ref = g[f"{name}.pred_{side}"]
        for i in range(len(ref)):
            one = lambda x: torch.tensor([int(x[i])])
            data = {"batch_h": ids if side == "head" else one(qh), "batch_t": one(qt) if side == "head" else ids,
                    "batch_r": one(qr), "mode": side + "_batch"}
            fwd = model(data)
            got = (model.margin - fwd if model.margin_flag else fwd).detach().numpy()   # predict's transform
            assert np.all(np.abs(got - ref[i]) <= 1e-4 * np.maximum(1, np.abs(ref[i]))), (side, i)


def test_constructor_errors():
    from openke.module.model import TransD
    with pytest.raises(ValueError, match="paddings"):
        TransD(ent_tot=7, rel_tot=3, dim_e=8, dim_r=10)
    with pytest.raises(ValueError, match="p_norm"):
        TransD(ent_tot=7, rel_tot=3, dim_e=8, dim_r=8, p_norm=3)
