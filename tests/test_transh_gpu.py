"""TransH on the GPU: the fused hyperplane-projected sweep (csrc/transh.hip) against the numpy
restatement of DESIGN.md §3 (tests/transh_restate.py) at the shapes where the kernels change path,
against the reference's fixture (tests/golden/transh_small.npz), and through the OpenKE surfaces."""
import os

import numpy as np
import pytest
import torch

import transh_restate as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SMALL = os.path.join(GOLDEN, "data", "small")
DEV = "cuda:0"

# ------------------------------------------------------------------------ synthetic edges ---
E, N_REL = 300, 8                                   # entity tiles 128 / 128 / 44
PER_REL = [0, 1, 127, 128, 129, 300, 2, 64]         # queries per relation, both modes mixed
COPY, ZERO_E, ON_NORMAL, LAST = 5, 7, 9, E - 1      # hand-placed entity rows
R_ZERO_REL, R_LONG_NORMAL, R_NORMAL_OF_9, R_ZERO_NORMAL = 3, 4, 5, 6


def make_case(dim):
    """Tables, queries, known triples and type lists of the synthetic case at one dim (host arrays)."""
    rng = np.random.default_rng(100 + dim)
    ent = rng.uniform(-0.5, 0.5, (E, dim)).astype(np.float32)
    rel = rng.uniform(-0.5, 0.5, (N_REL, dim)).astype(np.float32)
    nv = rng.uniform(-0.5, 0.5, (N_REL, dim)).astype(np.float32)
    nv[R_ZERO_NORMAL] = 0.0                                          # w_hat = 0: no projection
    nv[R_LONG_NORMAL] *= np.float32(7.0) / np.sqrt((nv[R_LONG_NORMAL].astype(np.float64) ** 2).sum())  # length 7
    rel[R_ZERO_REL] = 0.0
    ent[ZERO_E] = 0.0
    ent[ON_NORMAL] = np.float32(3.0) * R.normalize(nv[R_NORMAL_OF_9])  # projects to ~0 under relation 5
    qr = np.repeat(np.arange(N_REL), PER_REL)
    n = len(qr)
    qh, qt = rng.integers(0, E, n), rng.integers(0, E, n)
    qm = rng.integers(0, 2, n).astype(np.int8)
    # the special rows as truths and anchors, under the relation they are special for and others
    first = {r: int(np.nonzero(qr == r)[0][0]) for r in range(N_REL) if PER_REL[r]}
    i5, i6, i3, i4 = first[R_NORMAL_OF_9], first[R_ZERO_NORMAL], first[R_ZERO_REL], first[R_LONG_NORMAL]
    qh[i5], qm[i5] = ON_NORMAL, 0                                    # truth = the entity on the normal
    qt[i5 + 1], qm[i5 + 1] = ON_NORMAL, 0                            # ... and as the anchor
    qt[i5 + 2], qm[i5 + 2] = LAST, 1                                 # truth 299 (tail side)
    qh[i5 + 3], qm[i5 + 3] = LAST, 0                                 # truth 299 (head side)
    qh[i5 + 4], qm[i5 + 4] = ZERO_E, 0
    qt[i5 + 5], qm[i5 + 5] = ZERO_E, 0
    qt[i6], qm[i6] = LAST, 1
    qh[i3], qm[i3] = ZERO_E, 0
    qt[i4], qm[i4] = COPY, 1
    # an exact copy of a truth entity: it ties with that truth everywhere and must not be counted
    src = int(qt[i5 + 6])
    qm[i5 + 6] = 1
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
    return dict(ent=ent, rel=rel, nv=nv, qh=qh, qr=qr, qt=qt, qm=qm, known=(kh, kr, kt), types=(th, tt), src=src)


_cases = {}


def case(dim):
    """The synthetic case at `dim` with its filter index and device copies, built once."""
    if dim not in _cases:
        from mmre.link import FilterIndex
        c = make_case(dim)
        idx = FilterIndex(*c["known"], E, N_REL, *c["types"])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        c["index"] = idx
        c["groups"] = tuple(to(a) for a in idx.groups(c["qh"], c["qr"], c["qt"], c["qm"]))
        c["masks"] = tuple(to(m) for m in idx.type_masks())
        c["dev"] = {k: to(c[k]) for k in ("ent", "rel", "nv", "qh", "qr", "qt", "qm")}
        off, ids = idx.filters(c["qh"], c["qr"], c["qt"], c["qm"])
        c["lists"] = [ids[off[i]:off[i + 1]] for i in range(len(c["qh"]))]
        allowed = np.zeros((len(c["qh"]), E), bool)
        for i, (r, m) in enumerate(zip(c["qr"], c["qm"])):
            allowed[i, c["types"][0 if m == 0 else 1][r]] = True
        c["allowed"] = allowed
        c["truth_id"] = np.where(c["qm"] == 0, c["qh"], c["qt"])
        _cases[dim] = c
    return _cases[dim]


def spec_of(c, p_norm, norm_flag, margin):
    from mmre.link import ScoreSpec
    d = c["dev"]
    return ScoreSpec(model="transh" if p_norm == 1 else "transh_l2", ent=d["ent"], rel=d["rel"], dim=d["ent"].shape[1],
                     norm_flag=norm_flag, pred_kind=0 if margin is None else 1, margin=margin or 0.0, norm_vec=d["nv"])


@pytest.mark.parametrize("margin", [None, 5.0])
@pytest.mark.parametrize("norm_flag", [True, False])
@pytest.mark.parametrize("p_norm", [1, 2])
@pytest.mark.parametrize("dim", [20, 72])   # kp padded at 20 (24 rows); 72: nine stages
def test_sweep_equals_the_restatement(dim, p_norm, norm_flag, margin):
    check_sweep(dim, p_norm, norm_flag, margin)


# 1: one value per row; 8: one K stage, kp = dim; 9: the second stage holds one row and seven of
# padding; 512: mmre_transh_evaluate's shape check has no upper bound -- 64 stages
@pytest.mark.parametrize("p_norm,norm_flag", [(1, True), (2, False)])
@pytest.mark.parametrize("dim", [1, 8, 9, 512])
def test_sweep_equals_the_restatement_at_other_widths(dim, p_norm, norm_flag):
    check_sweep(dim, p_norm, norm_flag, None)


def check_sweep(dim, p_norm, norm_flag, margin):
    from mmre.transh import TransHSweep, plan_tiles, score_rows
    c = case(dim)
    d = c["dev"]
    Q = len(c["qh"])
    want_s = R.sweep_scores(c["ent"], c["rel"], c["nv"], c["qh"], c["qr"], c["qt"], c["qm"], p_norm, norm_flag, margin)
    want = R.rank_counts(want_s, c["truth_id"], c["lists"], c["allowed"])
    spec = spec_of(c, p_norm, norm_flag, margin)
    sw = TransHSweep(spec)
    plan = plan_tiles(c["qr"])
    assert sorted(np.bincount(plan["tiles"][:, 0], minlength=N_REL).tolist()) == [0, 1, 1, 1, 1, 1, 2, 3]
    res = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], filt=c["groups"], type_masks=c["masks"], plan=plan)
    got = res["counts"].cpu().numpy()
    print(f"dim {dim} p{p_norm} norm {norm_flag} margin {margin}: counts differing "
          f"{int((got != want).any(0).sum())} of {Q} queries, padding {res['padding']:.2f}")
    assert np.array_equal(got, want)
    # the sweep's threshold is the restatement's score of the truth, bit for bit
    assert np.array_equal(res["truth"].cpu().numpy(), want_s[np.arange(Q), c["truth_id"]])
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
    assert np.array_equal(got_s, want_s)
    # ... and the counts recomputed on the host from predict's scores are the sweep's
    assert np.array_equal(R.rank_counts(got_s, c["truth_id"], c["lists"], c["allowed"]), got)
    # the copied entity ties with its truth and is not counted: it never beats it
    qi = int(np.nonzero((c["qt"] == c["src"]) & (c["qm"] == 1))[0][0])
    assert got_s[qi, COPY] == got_s[qi, c["src"]]


# ------------------------------------------------------------------------------- golden ---
CONFIGS = [("l1_norm", dict(dim=32, p_norm=1, norm_flag=True)),
           ("l2_norm", dict(dim=32, p_norm=2, norm_flag=True)),
           ("l1_nonorm_margin", dict(dim=32, p_norm=1, norm_flag=False, margin=5.0))]


def golden_model(g, name, kw, dl):
    from openke.module.model import TransH
    model = TransH(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), **kw)
    sd = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in g.items()
          if k.startswith(name + ".") and k.endswith((".weight", "margin", "_const"))}
    model.load_state_dict(sd, strict=True)
    return model


@pytest.mark.parametrize("tc", [False, True])
@pytest.mark.parametrize("name,kw", CONFIGS)
def test_tester_matches_the_reference(golden, name, kw, tc):
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("transh_small")
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
    g = golden("transh_small")
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
            for emb in (model.ent_embeddings, model.rel_embeddings, model.norm_vector):
                gr = emb.weight.grad
                assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0.0


# ----------------------------------------------------------------------------- surfaces ---
def test_trainer_runs_transh_on_autograd():
    """The reference's examples/train_transh_FB15K237.py flow on the small dataset: two epochs of
    NegativeSampling(TransH, MarginLoss(4.0)) with SGD move all three tables and lower the loss."""
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransH
    from openke.module.strategy import NegativeSampling
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    torch.manual_seed(0)
    transh = TransH(ent_tot=tdl.get_ent_tot(), rel_tot=tdl.get_rel_tot(), dim=32, p_norm=1, norm_flag=True)
    before = [p.detach().clone() for p in (transh.ent_embeddings.weight, transh.rel_embeddings.weight,
                                           transh.norm_vector.weight)]
    model = NegativeSampling(model=transh, loss=MarginLoss(margin=4.0), batch_size=tdl.get_batch_size())
    trainer = Trainer(model=model, data_loader=tdl, train_times=2, alpha=1.0, use_gpu=True)
    trainer.run()
    assert trainer.used_one_call_step is False
    print("epoch losses", trainer.log)
    assert len(trainer.log) == 2 and trainer.log[1] < trainer.log[0]
    for b, p in zip(before, (transh.ent_embeddings.weight, transh.rel_embeddings.weight, transh.norm_vector.weight)):
        assert not torch.equal(b.to(p.device), p.detach())


def test_tester_surfaces(golden):
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("transh_small")
    name, kw = CONFIGS[2]
    dl = TestDataLoader(SMALL, "link")
    tester = Tester(model=golden_model(g, name, kw, dl), data_loader=dl, use_gpu=True)
    acc, thr = tester.run_triple_classification()
    pos, neg = tester.last["pos_scores"], tester.last["neg_scores"]
    n = len(dl.test_h)
    assert pos.shape == neg.shape == (n,)
    assert abs(acc - ((pos <= thr).sum() + (neg > thr).sum()) / (2 * n)) < 1e-12
    assert set(tester.last) >= {"accuracy", "threshold", "P", "A", "n_nan", "n_pos", "n_neg", "neg_h", "neg_t",
                                "pos_scores", "neg_scores", "seed_state_after"}
    # the positives' scores are predict's, bit for bit
    rows = tester.model.predict({"batch_h": dl.test_h, "batch_t": dl.test_t, "batch_r": dl.test_r, "mode": "normal"})
    assert np.array_equal(rows, pos)
    acc2, thr2 = tester.run_triple_classification(threshlod=thr)
    assert thr2 == thr
    with pytest.raises(NotImplementedError, match="TransH"):
        tester.run_relation_prediction()


def test_transe_counts_unchanged(golden):
    """An existing model's evaluation beside the new path: TransE on the small set, the reference's counts."""
    from openke.config import Tester
    from openke.data import TestDataLoader
    from openke.module.model import TransE
    g = golden("link_small")
    dl = TestDataLoader(SMALL, "link")
    model = TransE(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=32, p_norm=1, norm_flag=True)
    model.load_state_dict({k[len("transe."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("transe.")},
                          strict=False)
    tester = Tester(model=model, data_loader=dl, use_gpu=True)
    tester.run_link_prediction(type_constrain=True)
    head, tail = tester.last["counts"]
    assert np.array_equal(head.T, g["transe_tc1_head_counts"]) and np.array_equal(tail.T, g["transe_tc1_tail_counts"])
