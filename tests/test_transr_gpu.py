"""TransR on the GPU: the MFMA projection, the sweep over its planes and the row kernel
(csrc/transr.hip) against the numpy restatement of DESIGN.md §3 (tests/transr_restate.py) at the
shapes where the kernels change path, against the reference's fixture
(tests/golden/transr_small.npz), and through the OpenKE surfaces."""
import os

import numpy as np
import pytest
import torch

import transr_restate as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SMALL = os.path.join(GOLDEN, "data", "small")
DEV = "cuda:0"
TABLES = ("ent_embeddings", "rel_embeddings", "transfer_matrix")

# ------------------------------------------------------------------------ synthetic edges ---
E, N_REL = 300, 8                                   # entity tiles 128 / 128 / 44
PER_REL = [0, 1, 127, 128, 129, 300, 2, 64]         # queries per relation, both modes mixed
COPY, ZERO_E, SRC, LAST = 5, 7, 11, E - 1           # hand-placed entity rows (SRC: the row COPY copies)
R_ZERO_M, R_ZERO_REL, R_IDENT, R_ZCOL = 2, 3, 4, 5  # hand-placed relations
ZCOL = 3                                            # the zero column of relation 5's matrix


def make_case(dim_e, dim_r):
    """Tables, queries, known triples and type lists of the synthetic case at one (dim_e, dim_r)
    (host arrays), after tests/test_transd_gpu.py's make_case."""
    f = np.float32
    rng = np.random.default_rng(300 + 7 * dim_e + dim_r)
    ent = rng.uniform(-0.5, 0.5, (E, dim_e)).astype(f)
    rel = rng.uniform(-0.5, 0.5, (N_REL, dim_r)).astype(f)
    tm = rng.uniform(-0.5, 0.5, (N_REL, dim_e, dim_r)).astype(f)
    tm[R_ZERO_M] = 0.0                                               # every entity projects to 0: all tie
    tm[R_IDENT] = 0.0
    tm[R_IDENT][np.arange(min(dim_e, dim_r)), np.arange(min(dim_e, dim_r))] = 1.0   # TransR.py:24-27
    tm[R_ZCOL][:, min(ZCOL, dim_r - 1)] = 0.0                        # m_3 = 0 for every entity (the last column below dim_r 4)
    rel[R_ZERO_REL] = 0.0
    ent[ZERO_E] = 0.0                                                # m = 0: the 1e-12 clamp
    tm = tm.reshape(N_REL, dim_e * dim_r)
    qr = np.repeat(np.arange(N_REL), PER_REL)
    n = len(qr)
    qh, qt = rng.integers(0, E, n), rng.integers(0, E, n)
    qm = rng.integers(0, 2, n).astype(np.int8)
    # the special rows as truths and anchors, under the relation they are special for and others
    first = {r: int(np.nonzero(qr == r)[0][0]) for r in range(N_REL) if PER_REL[r]}
    i5, i2, i3, i4 = first[R_ZCOL], first[R_ZERO_M], first[R_ZERO_REL], first[R_IDENT]
    qt[i5 + 2], qm[i5 + 2] = LAST, 1                                 # truth 299 (tail side)
    qh[i5 + 3], qm[i5 + 3] = LAST, 0                                 # truth 299 (head side)
    qh[i5 + 4], qm[i5 + 4] = ZERO_E, 0                               # the zero entity as truth
    qt[i5 + 5], qm[i5 + 5] = ZERO_E, 0                               # ... and as the anchor
    qt[i5 + 7], qm[i5 + 7] = LAST, 0                                 # 299 as the anchor (head batch)
    qh[i5 + 8], qm[i5 + 8] = LAST, 1                                 # 299 as the anchor (tail batch)
    qh[i2], qm[i2] = ZERO_E, 0
    qt[i2 + 1], qm[i2 + 1] = LAST, 1
    qh[i3], qm[i3] = ZERO_E, 0
    qt[i3 + 1], qm[i3 + 1] = LAST, 1
    qt[i4], qm[i4] = COPY, 1
    qh[i4 + 1], qm[i4 + 1] = ZERO_E, 1
    # an exact copy of a truth entity: it ties with that truth everywhere and must not be counted
    src = SRC
    qt[i5 + 6], qm[i5 + 6] = SRC, 1
    ent[COPY] = ent[src]
    qr = qr.astype(np.int64)
    order = rng.permutation(n)                                       # the caller's order is not by relation
    qh, qr, qt, qm = qh[order], qr[order], qt[order], qm[order]
    kn = 4000
    kh, kr, kt = rng.integers(0, E, kn), rng.integers(0, N_REL, kn), rng.integers(0, E, kn)
    # every fourth known triple shares a query's (h, r) or (r, t), so the filter lists are not empty
    pick = rng.integers(0, n, kn // 4)
    kh[:kn // 8], kr[:kn // 8] = qh[pick[:kn // 8]], qr[pick[:kn // 8]]
    kr[kn // 8:kn // 4], kt[kn // 8:kn // 4] = qr[pick[kn // 8:]], qt[pick[kn // 8:]]
    kh, kr, kt = (np.concatenate([a, b]) for a, b in ((kh, qh), (kr, qr), (kt, qt)))
    th = [np.sort(rng.choice(E, int(rng.integers(20, E)), replace=False)) for _ in range(N_REL)]
    tt = [np.sort(rng.choice(E, int(rng.integers(20, E)), replace=False)) for _ in range(N_REL)]
    return dict(ent=ent, rel=rel, tm=tm, qh=qh, qr=qr, qt=qt, qm=qm, known=(kh, kr, kt), types=(th, tt), src=src,
                E=E, n_rel=N_REL, per_rel=PER_REL, r_zero_m=R_ZERO_M, tiles_per_rel=[0, 1, 1, 1, 1, 1, 2, 3])


# The reduced case of the widths whose float32-fma restatement of the full case takes ten seconds and
# more (dim_e * dim_r > 40,000): three relations -- the zero matrix, the identity, a random one --
# over two entity tiles, the second one partial, with the zero entity, the copied entity and the
# last entity as truth and as anchor.
E_RED, PER_REL_RED = 200, [20, 60, 120]
REDUCED_ABOVE = 40_000


def make_reduced_case(dim_e, dim_r):
    f = np.float32
    n_rel, last = len(PER_REL_RED), E_RED - 1
    rng = np.random.default_rng(900 + 7 * dim_e + dim_r)
    ent = rng.uniform(-0.5, 0.5, (E_RED, dim_e)).astype(f)
    rel = rng.uniform(-0.5, 0.5, (n_rel, dim_r)).astype(f)
    tm = rng.uniform(-0.5, 0.5, (n_rel, dim_e, dim_r)).astype(f)
    tm[0] = 0.0                                                      # every entity projects to 0: all tie
    tm[1] = 0.0
    tm[1][np.arange(min(dim_e, dim_r)), np.arange(min(dim_e, dim_r))] = 1.0   # TransR.py:24-27
    ent[ZERO_E] = 0.0                                                # m = 0: the 1e-12 clamp
    ent[COPY] = ent[SRC]
    tm = tm.reshape(n_rel, dim_e * dim_r)
    qr = np.repeat(np.arange(n_rel), PER_REL_RED)
    n = len(qr)
    qh, qt = rng.integers(0, E_RED, n), rng.integers(0, E_RED, n)
    qm = rng.integers(0, 2, n).astype(np.int8)
    for r in range(n_rel):                                           # the special rows under every relation
        i = int(np.nonzero(qr == r)[0][0])
        qh[i], qm[i] = ZERO_E, 0                                     # the zero entity as truth
        qt[i + 1], qm[i + 1] = ZERO_E, 0                             # ... and as the anchor
        qt[i + 2], qm[i + 2] = last, 1                               # truth 199 (tail side)
        qh[i + 3], qm[i + 3] = last, 0                               # truth 199 (head side)
        qt[i + 4], qm[i + 4] = last, 0                               # 199 as the anchor (head batch)
        qh[i + 5], qm[i + 5] = last, 1                               # 199 as the anchor (tail batch)
        qt[i + 6], qm[i + 6] = SRC, 1                                # COPY ties with this truth
        qt[i + 7], qm[i + 7] = COPY, 1
    qr = qr.astype(np.int64)
    order = rng.permutation(n)
    qh, qr, qt, qm = qh[order], qr[order], qt[order], qm[order]
    kn = 800
    kh, kr, kt = rng.integers(0, E_RED, kn), rng.integers(0, n_rel, kn), rng.integers(0, E_RED, kn)
    pick = rng.integers(0, n, kn // 4)
    kh[:kn // 8], kr[:kn // 8] = qh[pick[:kn // 8]], qr[pick[:kn // 8]]
    kr[kn // 8:kn // 4], kt[kn // 8:kn // 4] = qr[pick[kn // 8:]], qt[pick[kn // 8:]]
    kh, kr, kt = (np.concatenate([a, b]) for a, b in ((kh, qh), (kr, qr), (kt, qt)))
    th = [np.sort(rng.choice(E_RED, int(rng.integers(20, E_RED)), replace=False)) for _ in range(n_rel)]
    tt = [np.sort(rng.choice(E_RED, int(rng.integers(20, E_RED)), replace=False)) for _ in range(n_rel)]
    return dict(ent=ent, rel=rel, tm=tm, qh=qh, qr=qr, qt=qt, qm=qm, known=(kh, kr, kt), types=(th, tt), src=SRC,
                E=E_RED, n_rel=n_rel, per_rel=PER_REL_RED, r_zero_m=0, tiles_per_rel=[1, 1, 1])


_cases = {}


def case(dims):
    """The synthetic case at `dims` with its filter index and device copies, built once."""
    if dims not in _cases:
        from mmre.link import FilterIndex
        c = (make_reduced_case if dims[0] * dims[1] > REDUCED_ABOVE else make_case)(*dims)
        idx = FilterIndex(*c["known"], c["E"], c["n_rel"], *c["types"])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        c["index"] = idx
        c["groups"] = tuple(to(a) for a in idx.groups(c["qh"], c["qr"], c["qt"], c["qm"]))
        c["masks"] = tuple(to(m) for m in idx.type_masks())
        c["dev"] = {k: to(c[k]) for k in ("ent", "rel", "tm", "qh", "qr", "qt", "qm")}
        off, ids = idx.filters(c["qh"], c["qr"], c["qt"], c["qm"])
        c["lists"] = [ids[off[i]:off[i + 1]] for i in range(len(c["qh"]))]
        allowed = np.zeros((len(c["qh"]), c["E"]), bool)
        for i, (r, m) in enumerate(zip(c["qr"], c["qm"])):
            allowed[i, c["types"][0 if m == 0 else 1][r]] = True
        c["allowed"] = allowed
        c["truth_id"] = np.where(c["qm"] == 0, c["qh"], c["qt"])
        c["want"] = {}
        _cases[dims] = c
    return _cases[dims]


def restated(c, p_norm, norm_flag, margin):
    """The restatement's (Q, E) scores and (4, Q) counts of one configuration, computed once."""
    key = (p_norm, norm_flag, margin)
    if key not in c["want"]:
        s = R.sweep_scores(c["ent"], c["rel"], c["tm"], c["qh"], c["qr"], c["qt"], c["qm"], p_norm, norm_flag, margin)
        c["want"][key] = s, R.rank_counts(s, c["truth_id"], c["lists"], c["allowed"])
    return c["want"][key]


def spec_of(c, p_norm, norm_flag, margin):
    from mmre.link import ScoreSpec
    d = c["dev"]
    return ScoreSpec(model="transr" if p_norm == 1 else "transr_l2", ent=d["ent"], rel=d["rel"],
                     dim=d["rel"].shape[1], norm_flag=norm_flag, pred_kind=0 if margin is None else 1,
                     margin=margin or 0.0, dim_e=d["ent"].shape[1], transfer_matrix=d["tm"])


# (20, 20): kp padded to 24 rows; (72, 72): nine stages; (28, 20) and (20, 28): both orders;
# (33, 31): off every MFMA multiple in K and N; (200, 200): the example's width, two column chunks
SMALL_DIMS = [(20, 20), (72, 72), (28, 20), (20, 28), (33, 31)]
PARAMS = [(d, p, nf, m) for d in SMALL_DIMS for p in (1, 2) for nf in (True, False) for m in (None, 5.0)]
PARAMS += [((200, 200), 1, True, m) for m in (None, 5.0)]


@pytest.mark.parametrize("dims,p_norm,norm_flag,margin", PARAMS)
def test_sweep_equals_the_restatement(dims, p_norm, norm_flag, margin):
    check_sweep(dims, p_norm, norm_flag, margin)


# k_tr_project off the widths above. (1, 1): one value; (16, 7) / (17, 7): one K block and one row
# into the second; (7, 1): a single column; (40, 128) / (40, 129): a full column chunk and one column
# into the next; (256, 256): the last full second chunk; (512, 7) and (7, 512): 32 K blocks under
# one partly filled tile, and four chunks over half a K block; (512, 512): the widest the shape
# check accepts, and the largest dynamic LDS request of the library. Above REDUCED_ABOVE the reduced case.
OTHER_DIMS = [(1, 1), (16, 7), (17, 7), (7, 1), (40, 128), (40, 129), (256, 256), (512, 7), (7, 512), (512, 512)]


@pytest.mark.parametrize("p_norm,norm_flag", [(1, True), (2, False)])
@pytest.mark.parametrize("dims", OTHER_DIMS)
def test_sweep_equals_the_restatement_at_other_widths(dims, p_norm, norm_flag):
    check_sweep(dims, p_norm, norm_flag, None)


def check_sweep(dims, p_norm, norm_flag, margin):
    from mmre.transr import TransRSweep, plan_tiles, score_rows
    c = case(dims)
    d = c["dev"]
    Q = len(c["qh"])
    E, N_REL = c["E"], c["n_rel"]
    want_s, want = restated(c, p_norm, norm_flag, margin)
    spec = spec_of(c, p_norm, norm_flag, margin)
    sw = TransRSweep(spec)
    assert (sw.dim_e, sw.dim_r) == dims
    plan = plan_tiles(c["qr"])
    assert sorted(np.bincount(plan["tiles"][:, 0], minlength=N_REL).tolist()) == c["tiles_per_rel"]
    res = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], filt=c["groups"], type_masks=c["masks"], plan=plan)
    got = res["counts"].cpu().numpy()
    truth = res["truth"].cpu().numpy()
    print(f"dims {dims} p{p_norm} norm {norm_flag} margin {margin}: counts differing "
          f"{int((got != want).any(0).sum())} of {Q} queries, truth differing "
          f"{int((truth != want_s[np.arange(Q), c['truth_id']]).sum())}, padding {res['padding']:.2f}")
    assert np.array_equal(got, want)
    # the sweep's threshold is the restatement's score of the truth, bit for bit
    assert np.array_equal(truth, want_s[np.arange(Q), c["truth_id"]])
    # two runs give the same bits
    again = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], filt=c["groups"], type_masks=c["masks"], plan=plan)
    assert np.array_equal(again["counts"].cpu().numpy(), got) and np.array_equal(again["truth"].cpu().numpy(), truth)
    # without type masks (and without a filter): the raw and filtered columns alone
    plain = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], filt=c["groups"], plan=plan)["counts"].cpu().numpy()
    assert np.array_equal(plain[:2], want[:2]) and not plain[2:].any()
    raw = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], plan=plan)["counts"].cpu().numpy()
    assert np.array_equal(raw[0], want[0]) and np.array_equal(raw[1], want[0])
    # predict in head_batch / tail_batch mode: every query's whole row, bit-equal to the restatement
    ids = torch.arange(E, device=DEV)
    got_s = np.empty((Q, E), np.float32)
    for head in (True, False):
        sel = np.nonzero((c["qm"] == 0) == head)[0]
        n = len(sel)
        anchor = (d["qt"] if head else d["qh"])[torch.from_numpy(sel).to(DEV)]
        cand = ids.repeat_interleave(n)                              # candidate i of query j at [i * n + j]
        rows = score_rows(spec, cand if head else anchor.repeat(E), d["qr"][torch.from_numpy(sel).to(DEV)].repeat(E),
                          anchor.repeat(E) if head else cand, mode="head_batch" if head else "tail_batch")
        got_s[sel] = rows.cpu().numpy().reshape(E, n).T
    print(f"  rows differing from the restatement: {int((got_s != want_s).sum())} of {got_s.size}")
    assert np.array_equal(got_s, want_s)
    # ... and the counts recomputed on the host from predict's scores are the sweep's
    assert np.array_equal(R.rank_counts(got_s, c["truth_id"], c["lists"], c["allowed"]), got)
    # the copied entity ties with its truth and is not counted: it never beats it
    qi = int(np.nonzero((c["qt"] == c["src"]) & (c["qm"] == 1))[0][0])
    assert got_s[qi, COPY] == got_s[qi, c["src"]]
    assert np.array_equal(got_s[:, COPY], got_s[:, c["src"]])
    # under the all-zero matrix every candidate ties with the truth: every count is 0
    zm = c["qr"] == c["r_zero_m"]
    assert zm.sum() == c["per_rel"][c["r_zero_m"]] and not got[:, zm].any()
    assert np.all(got_s[zm] == got_s[zm][:, :1])


def test_rows_outside_the_tables_get_nan_and_empty_rows():
    from mmre.transr import score_rows
    c = case((28, 20))
    spec = spec_of(c, 1, True, None)
    t = lambda *x: torch.tensor(x, device=DEV)
    out = score_rows(spec, t(0, E, 1, -1, 2), t(1, 1, N_REL, 1, 2), t(3, 3, 3, 3, E + 5)).cpu().numpy()
    assert np.isfinite(out[0]) and np.isnan(out[1:]).all()
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    empty = score_rows(spec, none, none, none)
    assert empty.shape == (0,) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------- golden ---
CONFIGS = [("l1_norm", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=True)),
           ("l2_norm_wide", dict(dim_e=40, dim_r=24, p_norm=2, norm_flag=True, rand_init=True)),
           ("l1_nonorm_margin_tall", dict(dim_e=24, dim_r=40, p_norm=1, norm_flag=False, rand_init=True, margin=5.0)),
           ("l1_identity", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=False))]


def golden_model(g, name, kw, dl):
    from openke.module.model import TransR
    model = TransR(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), **kw)
    sd = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in g.items()
          if k.startswith(name + ".") and k.endswith((".weight", ".margin", "_const")) and not np.isnan(v).any()}
    model.load_state_dict(sd, strict=True)
    return model


@pytest.mark.parametrize("tc", [False, True])
@pytest.mark.parametrize("name,kw", CONFIGS)
def test_tester_matches_the_reference(golden, name, kw, tc):
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("transr_small")
    dl = TestDataLoader(SMALL, "link")
    tester = Tester(model=golden_model(g, name, kw, dl), data_loader=dl, use_gpu=True)
    mrr, mr, hit10, hit3, hit1 = tester.run_link_prediction(type_constrain=tc)
    ref = g[f"{name}.tc{int(tc)}_metrics"]
    print(name, tc, "got", (mrr, mr, hit10, hit3, hit1), "ref", ref.tolist())
    assert np.array_equal(np.array([hit10, hit3, hit1], np.float32), ref[2:])
    assert abs(mrr - ref[0]) < 1e-6 and abs(mr - ref[1]) < 1e-3
    head, tail = tester.last["counts"]
    cols = 4 if tc else 2
    assert np.array_equal(head[:cols].T, g[f"{name}.tc{int(tc)}_head_counts"][:, :cols])
    assert np.array_equal(tail[:cols].T, g[f"{name}.tc{int(tc)}_tail_counts"][:, :cols])


@pytest.mark.parametrize("name,kw", CONFIGS)
def test_predict_and_forward_match_the_reference(golden, name, kw):
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("transr_small")
    dl = TestDataLoader(SMALL, "link")
    model = golden_model(g, name, kw, dl)
    tester = Tester(model=model, data_loader=dl, use_gpu=True)
    for i, (dh, dt) in enumerate(dl):
        if i >= len(g[f"{name}.pred_head"]):
            break
        for data, side in ((dh, "head"), (dt, "tail")):
            ref = g[f"{name}.pred_{side}"][i]
            got = tester.test_one_step(data)
            assert got.shape == ref.shape
            assert np.all(np.abs(got - ref) <= 1e-4 * np.maximum(1, np.abs(ref))), (name, side, i)
            model.zero_grad()
            fwd = model({k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in data.items()})
            assert fwd.requires_grad
            asp = (model.margin - fwd if model.margin_flag else fwd).detach().cpu().numpy()   # predict's transform
            assert np.all(np.abs(asp - ref) <= 1e-4 * np.maximum(1, np.abs(ref))), (name, side, i)
            fwd.sum().backward()
            for emb in (model.ent_embeddings, model.rel_embeddings, model.transfer_matrix):
                gr = emb.weight.grad
                assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0.0


# ----------------------------------------------------------------------------- surfaces ---
def test_the_example_flow_on_the_small_dataset(tmp_path):
    """The reference's examples/train_transr_FB15K237.py flow on the small dataset: one epoch of
    TransE on the fused path, its parameters loaded into TransR, two epochs of
    NegativeSampling(TransR, MarginLoss(4.0)) on autograd, a checkpoint round trip into a fresh
    model and run_link_prediction."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransE, TransR
    from openke.module.strategy import NegativeSampling
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    torch.manual_seed(0)
    n_ent, n_rel = tdl.get_ent_tot(), tdl.get_rel_tot()
    transe = TransE(ent_tot=n_ent, rel_tot=n_rel, dim=32, p_norm=1, norm_flag=True)
    model_e = NegativeSampling(model=transe, loss=MarginLoss(margin=5.0), batch_size=tdl.get_batch_size())
    transr = TransR(ent_tot=n_ent, rel_tot=n_rel, dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=False)
    model_r = NegativeSampling(model=transr, loss=MarginLoss(margin=4.0), batch_size=tdl.get_batch_size())
    Trainer(model=model_e, data_loader=tdl, train_times=1, alpha=0.5, use_gpu=True).run()
    transr.set_parameters(transe.get_parameters())
    for k in ("ent_embeddings", "rel_embeddings"):
        assert torch.equal(getattr(transr, k).weight.detach().cpu(), getattr(transe, k).weight.detach().cpu())
    tables = [getattr(transr, k).weight for k in TABLES]
    before = [p.detach().clone() for p in tables]
    trainer = Trainer(model=model_r, data_loader=tdl, train_times=2, alpha=1.0, use_gpu=True)
    trainer.run()
    assert trainer.used_one_call_step is False
    print("epoch losses", trainer.log)
    assert len(trainer.log) == 2 and trainer.log[1] < trainer.log[0]
    for b, p in zip(before, tables):
        assert not torch.equal(b.to(p.device), p.detach())
    path = str(tmp_path / "transr.ckpt")
    transr.save_checkpoint(path)
    fresh = TransR(ent_tot=n_ent, rel_tot=n_rel, dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=False)
    fresh.load_checkpoint(path)
    for k in TABLES:
        assert torch.equal(getattr(transr, k).weight.detach().cpu(), getattr(fresh, k).weight.detach().cpu())
    dl = TestDataLoader(SMALL, "link")
    ra = Tester(model=transr, data_loader=dl, use_gpu=True).run_link_prediction(type_constrain=False)
    rb = Tester(model=fresh, data_loader=dl, use_gpu=True).run_link_prediction(type_constrain=False)
    assert ra == rb and 0.0 < ra[0] <= 1.0


def test_tester_surfaces(golden):
    from mmre import transr
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("transr_small")
    name, kw = CONFIGS[1]                                            # dim_e 40 > dim_r 24
    dl = TestDataLoader(SMALL, "link")
    tester = Tester(model=golden_model(g, name, kw, dl), data_loader=dl, use_gpu=True)
    acc, thr = tester.run_triple_classification()
    pos, neg = tester.last["pos_scores"], tester.last["neg_scores"]
    n = len(dl.test_h)
    assert pos.shape == neg.shape == (n,)
    assert abs(acc - ((pos <= thr).sum() + (neg > thr).sum()) / (2 * n)) < 1e-12
    assert set(tester.last) >= {"accuracy", "threshold", "P", "A", "n_nan", "n_pos", "n_neg", "neg_h", "neg_t",
                                "pos_scores", "neg_scores", "seed_state_after"}
    # the positives' scores are predict's, and both arrays transr.score_rows', bit for bit
    rows = tester.model.predict({"batch_h": dl.test_h, "batch_t": dl.test_t, "batch_r": dl.test_r, "mode": "normal"})
    assert np.array_equal(rows, pos)
    spec = tester.model.score_spec()
    to = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(DEV)
    assert np.array_equal(transr.score_rows(spec, to(dl.test_h), to(dl.test_r), to(dl.test_t)).cpu().numpy(), pos)
    assert np.array_equal(transr.score_rows(spec, to(tester.last["neg_h"]), to(dl.test_r),
                                            to(tester.last["neg_t"])).cpu().numpy(), neg)
    acc2, thr2 = tester.run_triple_classification(threshlod=thr)
    assert thr2 == thr
    with pytest.raises(NotImplementedError, match="TransR"):
        tester.run_relation_prediction()
