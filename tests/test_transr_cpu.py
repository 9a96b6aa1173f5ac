"""TransR without a GPU: the exact float32 fma of the restatement (tests/transr_restate.py) against
rational arithmetic, the restatement of DESIGN.md §3 against the reference's fixture and against
the model's own torch ops, the model class, the routing, and the error codes of the TransR entry
points for arguments they refuse before anything is launched (addresses never dereferenced)."""
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import transr_restate as R
from conftest import GOLDEN

SMALL = os.path.join(GOLDEN, "data", "small")
CONFIGS = [("l1_norm", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=True, margin=None)),
           ("l2_norm_wide", dict(dim_e=40, dim_r=24, p_norm=2, norm_flag=True, rand_init=True, margin=None)),
           ("l1_nonorm_margin_tall", dict(dim_e=24, dim_r=40, p_norm=1, norm_flag=False, rand_init=True, margin=5.0)),
           ("l1_identity", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=False, margin=None))]
TABLES = ("ent_embeddings", "rel_embeddings", "transfer_matrix")
TRANSR_L1, TRANSR_L2 = 9, 10
REL = 1e-6  # tests/golden/make_transh.py's bound on the restatement, carried over


def calc(kw):
    return {k: kw[k] for k in ("p_norm", "norm_flag", "margin")}


# ------------------------------------------------------------------------------- fma32 ---
def nearest_f32(x: Fraction) -> np.float32:
    """The float32 nearest the rational x, ties to even (normal range; 0 for x == 0)."""
    if x == 0:
        return np.float32(0.0)
    sign, ax = (-1 if x < 0 else 1), abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()
    if Fraction(2) ** e > ax:
        e -= 1                                              # 2^e <= ax < 2^(e + 1)
    assert Fraction(2) ** e <= ax < Fraction(2) ** (e + 1) and -126 <= e <= 126
    q = ax / Fraction(2) ** (e - 23)                        # the significand in units of one ulp
    n, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and n % 2 == 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))   # exact: n has <= 25 bits


def midpoint_triples():
    """(a, b, c) whose exact a * b + c lies 2^-70 beside a float32 MIDPOINT. With a = 2^-12 (1 + 2^-23)
    and b = 2^-12 (1 - 2^-23) the product is 2^-24 (1 - 2^-46); for c = 1 + j 2^-23 the midpoint
    above c is c + 2^-24, so a b + c is that midpoint - 2^-70 (rounds DOWN to c) and -a b + (c + ulp)
    the same midpoint + 2^-70 (rounds UP to c + ulp). The float64 sum lands ON the midpoint and its
    cast ties to even: wrong for odd j in the first family and for even j in the second."""
    f = np.float32
    a, b, ulp = f(2.0 ** -12 * (1 + 2.0 ** -23)), f(2.0 ** -12 * (1 - 2.0 ** -23)), 2.0 ** -23
    out = []
    for j in range(1, 40):
        c = f(1.0 + j * ulp)
        out += [(a, b, c), (f(-a), b, f(c + ulp)), (f(-a), b, f(-c)), (a, b, f(-(c + ulp)))]
    return out


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(5)
    n = 4000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    # cancelling triples: c close to -a * b, where the sum keeps few of the product's bits
    c[:1000] = -(a[:1000].astype(np.float64) * b[:1000]).astype(np.float32)
    mids = midpoint_triples()
    a = np.concatenate([a, np.array([t[0] for t in mids], np.float32)])
    b = np.concatenate([b, np.array([t[1] for t in mids], np.float32)])
    c = np.concatenate([c, np.array([t[2] for t in mids], np.float32)])
    got, naive = R.fma32(a, b, c), R.fma32_naive(a, b, c)
    fr = lambda x: Fraction(float(x))
    wrong_naive = 0
    for i in range(len(a)):
        want = nearest_f32(fr(a[i]) * fr(b[i]) + fr(c[i]))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)
        wrong_naive += int(i >= n and naive[i] != want)
    print(f"double rounding differs from the exact fma on {wrong_naive} of the {len(mids)} midpoint triples")
    assert wrong_naive == len(mids) // 2                    # the midpoint triples are where it fails: every other one
    # broadcasting, as transfer() uses it
    m = R.fma32(a[:6, None], b[None, :5], np.zeros((6, 5), np.float32))
    assert m.shape == (6, 5) and m.dtype == np.float32
    assert np.array_equal(m, (a[:6, None].astype(np.float64) * b[None, :5]).astype(np.float32))


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
    g = golden("transr_small")
    ds, index = small
    tabs = [g[f"{name}.{k}.weight"] for k in TABLES]
    assert tabs[0].shape == (257, kw["dim_e"]) and tabs[2].shape == (13, kw["dim_e"] * kw["dim_r"])
    assert float(g[f"{name}.restate_rel_dev"]) <= REL
    # (make_transr.py: one configuration's xavier matrices are stored times 8, the others as drawn)
    assert float(g[f"{name}.matrix_scale"]) == (8.0 if name == "l1_nonorm_margin_tall" else 1.0)
    m = float(g[f"{name}.margin"][0])                        # NaN: a model without a margin
    assert (kw["margin"] is None and np.isnan(m)) or m == kw["margin"]
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    T = len(qh)
    for side, head in (("head", True), ("tail", False)):
        s = R.sweep_scores(*tabs, qh, qr, qt, np.full(T, 0 if head else 1), **calc(kw))
        ref = g[f"{name}.pred_{side}"]
        dev = np.abs(s[:len(ref)].astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)
        assert dev.max() <= REL, (side, dev.max())
        c = dataset_counts(s, qh, qr, qt, head, ds, index)
        assert np.array_equal(c[:2].T, g[f"{name}.tc0_{side}_counts"][:, :2]), side
        assert np.array_equal(c.T, g[f"{name}.tc1_{side}_counts"]), side
        # the row restatement is the sweep restatement's diagonal, bit for bit
        rows = R.score_rows(*tabs, qh, qr, qt, head, **calc(kw))
        assert np.array_equal(rows, s[np.arange(T), qh if head else qt])


# -------------------------------------------------------- restatement vs the model's torch ops ---
@pytest.mark.parametrize("dim_e,dim_r,p_norm,norm_flag,margin,rand_init",
                         [(32, 32, 1, True, None, True), (40, 24, 2, True, None, True), (24, 40, 1, False, 5.0, True),
                          (32, 32, 1, True, None, False), (200, 200, 1, True, None, True)])
def test_restatement_matches_forward_on_the_cpu(dim_e, dim_r, p_norm, norm_flag, margin, rand_init):
    from openke.module.model import TransR
    torch.manual_seed(11)
    E, NR = 40, 3
    model = TransR(ent_tot=E, rel_tot=NR, dim_e=dim_e, dim_r=dim_r, p_norm=p_norm, norm_flag=norm_flag,
                   rand_init=rand_init, margin=margin)
    tabs = [getattr(model, k).weight.detach().numpy() for k in TABLES]
    ids = torch.arange(E)
    worst = 0.0
    for mode, head in (("head_batch", True), ("tail_batch", False)):
        for r, anchor in ((0, 3), (2, 17)):
            one = lambda x: torch.tensor([x])
            data = {"batch_h": ids if head else one(anchor), "batch_t": one(anchor) if head else ids,
                    "batch_r": one(r), "mode": mode}
            with torch.no_grad():
                fwd = model(data)
            ref = (model.margin - fwd if model.margin_flag else fwd).numpy().astype(np.float64)   # predict's transform
            h = np.arange(E) if head else np.full(E, anchor)
            t = np.full(E, anchor) if head else np.arange(E)
            got = R.score_rows(*tabs, h, np.full(E, r), t, head, p_norm, norm_flag, margin)
            worst = max(worst, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)).max()))
    print(f"({dim_e}, {dim_r}) p{p_norm} norm {norm_flag}: restatement within {worst:.3g} relative of forward")
    assert worst <= REL


# ------------------------------------------------------------------------------- the ABI ---
ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, aligned, never dereferenced

EVAL = ("model", "norm_flag", "pred_kind", "margin", "ent", "rel", "transfer_matrix", "n_ent", "n_rel", "dim_e", "dim_r",
        "qh", "qr", "qt", "qmode", "n_query", "perm", "tiles", "n_tiles", "used", "n_used", "rel_slot", "grp_qoff",
        "grp_q", "n_groups", "filt_off", "filt_ids", "entry_q", "n_entries", "type_head", "type_tail", "counts", "truth",
        "work", "work_bytes", "stream")
ROWS = ("model", "norm_flag", "pred_kind", "margin", "ent", "rel", "transfer_matrix", "n_ent", "n_rel", "dim_e", "dim_r",
        "h", "r", "t", "n_rows", "head_batch", "out", "stream")
SIZES = dict(model=TRANSR_L1, norm_flag=1, pred_kind=0, margin=0.0, n_ent=300, n_rel=5, dim_e=24, dim_r=16, n_query=130,
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
    for name, n in (("mmre_transr_workspace", 7), ("mmre_transr_evaluate", len(EVAL)),
                    ("mmre_transr_score_rows", len(ROWS))):
        assert getattr(L, name, None) is not None, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    from mmre import transh, transr
    from mmre.link import MODEL_IDS
    assert MODEL_IDS["transr"] == TRANSR_L1 and MODEL_IDS["transr_l2"] == TRANSR_L2
    assert transr.MODEL_IDS == {"transr": 9, "transr_l2": 10}
    assert transr.plan_tiles is transh.plan_tiles and transr.TILE == transh.TILE   # imported, not copied
    assert transr.TransRSweep.run is transh.TransHSweep.run
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mmre.h")).read()
    for word in ("MMRE_TRANSR_L1 = 9", "MMRE_TRANSR_L2 = 10", "mmre_transr_workspace(", "mmre_transr_evaluate(",
                 "mmre_transr_score_rows(", "d_transfer_matrix"):
        assert word in header, word


def test_evaluate_error_codes():
    from mmre import _lib
    ev = lambda **o: run(EVAL, "mmre_transr_evaluate", **o)
    for p in ("ent", "rel", "transfer_matrix", "qh", "qr", "qt", "qmode", "perm", "tiles", "used", "rel_slot", "counts",
              "truth", "work"):
        assert ev(**{p: None}) == ARG, p                    # a null table or array
    for m in (-1, 0, 1, 4, 5, 6, 7, 8, 11):
        assert ev(model=m) == MODEL, m                      # TransE .. TransD have their own entry points
    assert ev(model=TRANSR_L2, dim_r=0) == SHAPE and ev(dim_r=-3) == SHAPE and ev(dim_r=513) == SHAPE
    assert ev(dim_e=0) == SHAPE and ev(dim_e=513) == SHAPE
    need = _lib.lib().mmre_transr_workspace(300, 5, 24, 16, 6, 5, 7)
    assert need > 0
    assert ev(work_bytes=need - 1) == WORKSPACE and ev(work_bytes=0) == WORKSPACE
    # both orders and the largest dims pass the shape check (the workspace answers next)
    assert ev(dim_e=15, work_bytes=0) == WORKSPACE and ev(dim_e=512, dim_r=512, work_bytes=0) == WORKSPACE
    # the exact size passes the workspace check: only with a fault that is answered earlier can
    # the call be made without a device, so pair it with one
    assert ev(work_bytes=need, n_query=0) == ARG
    for f in (dict(n_query=0), dict(n_ent=0), dict(n_rel=0), dict(n_tiles=0), dict(n_used=0), dict(n_used=6),
              dict(pred_kind=2), dict(pred_kind=-1), dict(type_head=fake()), dict(type_tail=fake()),
              dict(grp_q=None), dict(filt_off=None), dict(filt_ids=None), dict(entry_q=None), dict(n_groups=0)):
        assert ev(**f) == ARG, f
    assert ev(model=5, ent=None, dim_e=0, work_bytes=0) == MODEL   # the model answers first
    assert ev(ent=None, dim_e=0, work_bytes=0) == ARG              # then null pointers
    assert ev(dim_e=0, work_bytes=0) == SHAPE                      # then the shape, then the workspace
    assert ev(n_ent=(1 << 31) - 200) == SHAPE                      # entity ids stay int32


def test_score_rows_error_codes():
    rows = lambda **o: run(ROWS, "mmre_transr_score_rows", **o)
    for p in ("ent", "rel", "transfer_matrix", "h", "r", "t", "out"):
        assert rows(**{p: None}) == ARG, p
    for m in (-1, 0, 4, 5, 6, 7, 8, 11):
        assert rows(model=m) == MODEL, m
    assert rows(dim_r=0) == SHAPE and rows(dim_e=0) == SHAPE and rows(dim_r=513) == SHAPE and rows(dim_e=513) == SHAPE
    assert rows(model=6, ent=None, dim_e=0) == MODEL and rows(ent=None, dim_e=0) == ARG
    assert rows(pred_kind=5) == ARG and rows(n_rows=-1) == ARG and rows(n_ent=0) == ARG
    assert rows(n_rows=0, h=None, r=None, t=None, out=None) == 0  # nothing to score, nothing launched


def test_workspace_sizes():
    from mmre import _lib
    ws = _lib.lib().mmre_transr_workspace
    for bad in ((0, 5, 24, 16, 6, 5, 7), (300, 0, 24, 16, 6, 5, 7), (300, 5, 24, 0, 6, 5, 7), (300, 5, 0, 16, 6, 5, 7),
                (300, 5, 513, 16, 6, 5, 7), (300, 5, 24, 513, 6, 5, 7), (300, 5, 24, 16, -1, 5, 7),
                (300, 5, 24, 16, 6, -1, 7), (300, 5, 24, 16, 6, 5, -1)):
        assert ws(*bad) == 0, bad
    assert ws(300, 5, 16, 24, 6, 5, 7) > 0                  # dim_e < dim_r is served
    # every used relation's plane is held at once: linear in n_used, one kp x e_pad plane each,
    # whatever dim_e is
    a, b = ws(14208, 237, 200, 200, 300, 10, 0), ws(14208, 237, 200, 200, 300, 110, 0)
    assert b - a == 100 * 200 * 14208 * 4
    assert ws(14208, 237, 40, 200, 300, 10, 0) == a
    c2 = ws(14208, 237, 200, 200, 300, 29, 0)
    assert 29 * 200 * 14208 * 4 <= c2 < 29 * 200 * 14208 * 4 + (40 << 20)     # the C2 shape: 330 MB of planes
    base = (300, 5, 24, 16, 6, 5, 7)
    for i in (0, 1, 3, 4, 5, 6):
        more = list(base)
        more[i] = base[i] * 3 + 200
        assert ws(*more) >= ws(*base), i


def test_older_entry_points_refuse_the_new_ids():
    import test_transd_cpu as td
    import test_transh_cpu as th
    import test_tripleclass_cpu as tc
    import test_link_abi_cpu as link
    from mmre import _lib
    L = _lib.lib()
    for m in (TRANSR_L1, TRANSR_L2):
        for name in link.PARAMS:
            if "model" in link.PARAMS[name]:
                # (the raw-row split-bf16 sweep names anything but DistMult a SHAPE fault, as for every other id)
                assert link.run(name, model=m) == (SHAPE if name == "sweep_bf3_rows" else MODEL), (name, m)
        for name in ("scores", "evaluate"):
            assert tc.run(name, model=m) == MODEL, (name, m)
        assert th.run(th.EVAL, "mmre_transh_evaluate", model=m) == MODEL
        assert th.run(th.ROWS, "mmre_transh_score_rows", model=m) == MODEL
        assert td.run(td.EVAL, "mmre_transd_evaluate", model=m) == MODEL
        assert td.run(td.ROWS, "mmre_transd_score_rows", model=m) == MODEL
        assert not L.mmre_ns_fused_supported(m, 64, 4, 0)
        assert L.mmre_rel_workspace(m, 5, 8) < 0


# --------------------------------------------------------------------- spec, routing, model ---
def test_score_spec_and_routing():
    from mmre.link import LinkSweep, MODEL_IDS, ScoreSpec, evaluate_relation_prediction
    from mmre.transr import is_transr
    z = torch.zeros
    spec = ScoreSpec(model="transr", ent=z(4, 10), rel=z(2, 8), dim=8, dim_e=10, transfer_matrix=z(2, 80))
    assert is_transr(spec) and MODEL_IDS[spec.model] == TRANSR_L1 and MODEL_IDS["transr_l2"] == TRANSR_L2
    plain = ScoreSpec(model="transe", ent=spec.ent, rel=spec.rel, dim=8)
    assert plain.transfer_matrix is None and not is_transr(plain)
    import dataclasses
    assert [f.name for f in dataclasses.fields(ScoreSpec)][-1] == "transfer_matrix"
    with pytest.raises(ValueError, match="TransRSweep"):
        LinkSweep(spec)
    with pytest.raises(NotImplementedError, match="TransR"):
        evaluate_relation_prediction(spec, [0], [0], [1])


@pytest.mark.parametrize("dim_e,dim_r", [(10, 8), (8, 8), (6, 9)])
def test_model_class_mirrors_the_reference(dim_e, dim_r):
    from openke.module.model import TransE, TransR
    m = TransR(ent_tot=7, rel_tot=3, dim_e=dim_e, dim_r=dim_r, p_norm=2, norm_flag=False, margin=4.0)
    base = {"zero_const", "pi_const"}  # BaseModule's, as in the reference
    tables = {f"{k}.weight" for k in TABLES}
    assert set(m.state_dict()) == base | tables | {"margin"}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items() if k in tables} == {
        "ent_embeddings.weight": (7, dim_e), "rel_embeddings.weight": (3, dim_r),
        "transfer_matrix.weight": (3, dim_e * dim_r)}
    assert not m.margin.requires_grad and m.margin_flag and m.rand_init is False
    # the identity initialisation (TransR.py:23-29): ones on the diagonal of the dim_e x dim_r view
    eye = np.zeros((dim_e, dim_r), np.float32)
    eye[np.arange(min(dim_e, dim_r)), np.arange(min(dim_e, dim_r))] = 1.0
    for r in range(3):
        assert np.array_equal(m.transfer_matrix.weight.detach().numpy()[r].reshape(dim_e, dim_r), eye)
    assert m.ns_spec() is None and not hasattr(m, "fused_ns") and not hasattr(m, "fused_ns_transd")
    s = m.score_spec()
    assert (s.model, s.pred_kind, s.margin, s.norm_flag, s.dim, s.dim_e) == ("transr_l2", 1, 4.0, False, dim_r, dim_e)
    assert s.transfer_matrix is m.transfer_matrix.weight
    m2 = TransR(ent_tot=7, rel_tot=3, dim_e=dim_e, dim_r=dim_r, rand_init=True)
    assert set(m2.state_dict()) == base | tables and not m2.margin_flag
    assert m2.score_spec().pred_kind == 0 and m2.score_spec().model == "transr"
    # xavier_uniform: bound sqrt(6 / (rows + cols))
    assert float(m2.transfer_matrix.weight.detach().abs().max()) <= np.sqrt(6.0 / (3 + dim_e * dim_r)) + 1e-6
    assert float(m2.transfer_matrix.weight.detach().abs().max()) > 0
    # forward on the CPU is the reference's torch ops: differentiable into all three tables
    data = {"batch_h": torch.arange(7), "batch_t": torch.tensor([2]), "batch_r": torch.tensor([1]), "mode": "head_batch"}
    out = m2(data)
    assert out.shape == (7,)
    out.sum().backward()
    for emb in (m2.ent_embeddings, m2.rel_embeddings, m2.transfer_matrix):
        assert emb.weight.grad is not None and float(emb.weight.grad.abs().sum()) > 0
    assert float(m2.regularization(data)) > 0
    # TransE's parameters load (BaseModule.set_parameters, strict=False): the example's pretraining
    if dim_e == dim_r:
        e = TransE(ent_tot=7, rel_tot=3, dim=dim_e)
        before = m.transfer_matrix.weight.detach().clone()
        m.set_parameters(e.get_parameters())
        assert torch.equal(m.ent_embeddings.weight, e.ent_embeddings.weight)
        assert torch.equal(m.rel_embeddings.weight, e.rel_embeddings.weight)
        assert torch.equal(m.transfer_matrix.weight, before)


def test_constructor_errors():
    from openke.module.model import TransR
    with pytest.raises(ValueError, match="p_norm"):
        TransR(ent_tot=7, rel_tot=3, dim_e=8, dim_r=8, p_norm=3)
