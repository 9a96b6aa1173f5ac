"""RESCAL on the GPU: the MFMA planes, the sweep with a per-tile entity operand and the row kernel
(csrc/rescal.hip) against the numpy restatement of DESIGN.md §3 (tests/rescal_restate.py) at the
shapes where the kernels change path, against the reference's fixture
(tests/golden/rescal_small.npz), through the OpenKE surfaces, and where a workgroup sweeps several
units (after tests/test_sweep_units_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import rescal_restate as R
import tc_restate as TC
import test_sweep_units_cpu as U
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SMALL = os.path.join(GOLDEN, "data", "small")
DEV = "cuda:0"
TABLES = ("ent_embeddings", "rel_matrices")


def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def spec_of(ent, mats, pred_kind=0):
    from mmre.link import ScoreSpec
    return ScoreSpec(model="rescal", ent=ent, rel=None, dim=int(ent.shape[1]), pred_kind=pred_kind, rel_matrices=mats)


# ------------------------------------------------------------------------ synthetic edges ---
E, N_REL = 130, 5                                   # two entity tiles, the second with two live columns
PER_REL = [129, 40, 0, 12, 12]                      # queries per relation (relation 2: none)
PER_REL_FEW = [4, 10, 0, 6, 8]                      # dim 512: a handful
R_TAIL_ONLY, R_BOTH, R_NONE, R_ZERO_M, R_EDGE = range(5)
COPY, ZERO_E, SRC, LAST = 5, 7, 11, E - 1           # hand-placed entity rows (COPY copies SRC)
OUTSIDE = E + 3                                     # a listed id outside the table


def make_case(d):
    f = np.float32
    rng = np.random.default_rng(500 + d)
    ent = rng.uniform(-0.5, 0.5, (E, d)).astype(f)
    mats = rng.uniform(-0.5, 0.5, (N_REL, d * d)).astype(f)
    mats[R_ZERO_M] = 0.0                            # every score is 0: all tie
    ent[ZERO_E] = 0.0
    ent[COPY] = ent[SRC]
    per_rel = PER_REL_FEW if d == 512 else PER_REL
    qr = np.repeat(np.arange(N_REL), per_rel)
    n = len(qr)
    qh, qt = rng.integers(0, E, n), rng.integers(0, E, n)
    qm = rng.integers(0, 2, n).astype(np.int8)
    qm[qr == R_TAIL_ONLY] = 1                       # tiles of 128 + 1 on the tail side, no head-side tile
    i = int(np.nonzero(qr == R_EDGE)[0][0])
    qt[i], qm[i] = LAST, 1                          # truth E - 1 (tail side)
    qh[i + 1], qm[i + 1] = LAST, 0                  # truth E - 1 (head side)
    qt[i + 2], qm[i + 2] = LAST, 0                  # E - 1 as the anchor (head side)
    qh[i + 3], qm[i + 3] = LAST, 1                  # ... and on the tail side
    qh[i + 4], qm[i + 4] = ZERO_E, 0                # the zero row as truth
    qt[i + 5], qm[i + 5] = ZERO_E, 0                # ... and as the anchor: every score 0
    qt[i + 6], qm[i + 6] = SRC, 1                   # COPY ties with this truth and is not counted
    qh[i + 7], qm[i + 7] = COPY, 0                  # the copy as truth: SRC ties with it
    order = rng.permutation(n)                      # the caller's order is not by relation
    qh, qr, qt, qm = qh[order], qr[order].astype(np.int64), qt[order], qm[order]
    kn = 600                                        # known triples: half of them share a query's (h, r) or (r, t)
    kh, kr, kt = rng.integers(0, E, kn), rng.integers(0, N_REL, kn), rng.integers(0, E, kn)
    keep = qr != R_ZERO_M                           # relation 3's queries share nothing on purpose, and their own
    pick = rng.choice(np.nonzero(keep)[0], kn // 2)  # triples are not known: some lists stay empty
    kh[:kn // 4], kr[:kn // 4] = qh[pick[:kn // 4]], qr[pick[:kn // 4]]
    kr[kn // 4:kn // 2], kt[kn // 4:kn // 2] = qr[pick[kn // 4:]], qt[pick[kn // 4:]]
    kh, kr, kt = (np.concatenate([a, b[keep]]) for a, b in ((kh, qh), (kr, qr), (kt, qt)))
    th = [np.sort(rng.choice(E, int(rng.integers(20, E)), replace=False)) for _ in range(N_REL)]
    tt = [np.sort(rng.choice(E, int(rng.integers(20, E)), replace=False)) for _ in range(N_REL)]
    return dict(ent=ent, mats=mats, qh=qh, qr=qr, qt=qt, qm=qm, known=(kh, kr, kt), types=(th, tt), per_rel=per_rel)


_cases = {}


def case(d):
    """The synthetic case at dim d with its filter index, device copies and restated scores, built once."""
    if d not in _cases:
        from mmre.link import FilterIndex
        c = make_case(d)
        idx = FilterIndex(*c["known"], E, N_REL, *c["types"])
        q = (c["qh"], c["qr"], c["qt"], c["qm"])
        gqo, gq, off, ids, entry_q = idx.groups(*q)
        foff, fids = idx.filters(*q)
        lists = [fids[foff[i]:foff[i + 1]] for i in range(len(c["qh"]))]
        c["truth_id"] = np.where(c["qm"] == 0, c["qh"], c["qt"])
        # the filter CSR: an empty group, a group that lists the truth, and -- placed by hand -- an id
        # outside the table in a group of three or more, which the host lists of its members drop
        sizes = np.diff(off)
        assert sizes.min() == 0 and sizes.max() >= 3
        assert any(c["truth_id"][i] in lists[i] for i in range(len(lists)))
        g = int(np.nonzero(sizes >= 3)[0][0])
        old = int(ids[off[g] + 1])
        ids = ids.copy()
        ids[off[g] + 1] = OUTSIDE
        for qi in gq[gqo[g]:gqo[g + 1]]:
            lists[qi] = lists[qi][lists[qi] != old]
        c["groups"] = tuple(to(a) for a in (gqo, gq, off, ids, entry_q))
        c["lists"] = lists
        c["masks"] = tuple(to(m) for m in idx.type_masks())
        allowed = np.zeros((len(c["qh"]), E), bool)
        for i, (r, m) in enumerate(zip(c["qr"], c["qm"])):
            allowed[i, c["types"][0 if m == 0 else 1][r]] = True
        c["allowed"] = allowed
        c["dev"] = {k: to(c[k]) for k in ("ent", "mats", "qh", "qr", "qt", "qm")}
        c["want_s"] = R.sweep_scores(c["ent"], c["mats"], c["qh"], c["qr"], c["qt"], c["qm"])
        c["want"] = R.rank_counts(c["want_s"], c["truth_id"], lists, allowed)
        _cases[d] = c
    return _cases[d]


# 1: one value; 15 / 16 / 17: around one 16-row stage; 50: the example's width (four stages, the
# last with two live rows); 200: 13 stages, four row chunks of the plane kernel; 512: the widest
DIMS = [1, 15, 16, 17, 50, 200, 512]


@pytest.mark.parametrize("d", DIMS)
def test_sweep_equals_the_restatement(d):
    from mmre.rescal import RescalSweep, plan_keys, score_rows
    c = case(d)
    dv = c["dev"]
    Q = len(c["qh"])
    want_s, want = c["want_s"], c["want"]
    spec = spec_of(dv["ent"], dv["mats"])
    sw = RescalSweep(spec)
    assert sw.dim == d and (sw.n_ent, sw.n_rel) == (E, N_REL)
    plan = plan_keys(c["qr"], c["qm"])
    keys = plan["tiles"][:, 0].tolist()
    if d != 512:
        assert keys[:2] == [1, 1] and plan["tiles"][:2, 2].tolist() == [128, 1]      # 129 tail-side queries
        assert 0 not in keys and set(keys) == {1, 2, 3, 6, 7, 8, 9}                  # both sides elsewhere
    assert plan["used"].tolist() == [0, 1, 3, 4]                                     # relation 2: no plane
    q = (dv["qh"], dv["qr"], dv["qt"], dv["qm"])
    res = sw.run(*q, filt=c["groups"], type_masks=c["masks"], plan=plan)
    got, truth = res["counts"].cpu().numpy(), res["truth"].cpu().numpy()
    print(f"d {d}: counts differing {int((got != want).any(0).sum())} of {Q} queries, truth differing "
          f"{int((truth != want_s[np.arange(Q), c['truth_id']]).sum())}, padding {res['padding']:.2f}")
    assert np.array_equal(got, want)
    # the sweep's threshold is the restatement's score of the truth, bit for bit
    assert np.array_equal(truth, want_s[np.arange(Q), c["truth_id"]])
    assert (want[1] < want[0]).any() and (want[3] < want[2]).any() and want[0].max() > 64
    # two runs give the same bits; the plan made inside run() is the same plan
    again = sw.run(*q, filt=c["groups"], type_masks=c["masks"])
    assert np.array_equal(again["counts"].cpu().numpy(), got) and np.array_equal(again["truth"].cpu().numpy(), truth)
    # type masks off (the filter alone), then no filter either
    plain = sw.run(*q, filt=c["groups"], plan=plan)["counts"].cpu().numpy()
    assert np.array_equal(plain[:2], want[:2]) and not plain[2:].any()
    raw = sw.run(*q, plan=plan)["counts"].cpu().numpy()
    assert np.array_equal(raw[0], want[0]) and np.array_equal(raw[1], want[0])
    # score_rows: every query's whole row on its side, bit-equal to the restatement
    ids = torch.arange(E, device=DEV)
    got_s = np.empty((Q, E), np.float32)
    for head in (True, False):
        sel = np.nonzero((c["qm"] == 0) == head)[0]
        n = len(sel)
        st = torch.from_numpy(sel).to(DEV)
        anchor = (dv["qt"] if head else dv["qh"])[st]
        cand = ids.repeat_interleave(n)                              # candidate i of query j at [i * n + j]
        rows = score_rows(spec, cand if head else anchor.repeat(E), dv["qr"][st].repeat(E),
                          anchor.repeat(E) if head else cand)
        got_s[sel] = rows.cpu().numpy().reshape(E, n).T
    print(f"  rows differing from the restatement: {int((got_s != want_s).sum())} of {got_s.size}")
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(R.rank_counts(got_s, c["truth_id"], c["lists"], c["allowed"]), got)
    # pred_kind 2 is forward's -s: the same bits with the sign flipped, ranked the other way round
    fwd = score_rows(spec, dv["qh"], dv["qr"], dv["qt"], pred_kind=2).cpu().numpy()
    assert np.array_equal(fwd, -truth)
    neg = RescalSweep(spec_of(dv["ent"], dv["mats"], pred_kind=2)).run(*q, plan=plan)
    assert np.array_equal(neg["truth"].cpu().numpy(), -truth)
    assert np.array_equal(neg["counts"].cpu().numpy()[0], R.rank_counts(-want_s, c["truth_id"])[0])
    # the copied row ties with its source everywhere: as candidate it never beats the truth SRC
    assert np.array_equal(got_s[:, COPY], got_s[:, SRC])
    qi = int(np.nonzero((c["qt"] == SRC) & (c["qm"] == 1) & (c["qr"] == R_EDGE))[0][0])
    assert got_s[qi, COPY] == truth[qi]
    # the zero row scores 0 against everything; as the anchor it makes every candidate tie
    assert not got_s[:, ZERO_E][c["qm"] == 0].any()
    qz = int(np.nonzero((c["qt"] == ZERO_E) & (c["qm"] == 0) & (c["qr"] == R_EDGE))[0][0])
    assert not got_s[qz].any() and not got[:, qz].any()
    # the last entity as truth, on both sides
    assert ((c["truth_id"] == LAST) & (c["qm"] == 0)).any() and ((c["truth_id"] == LAST) & (c["qm"] == 1)).any()
    # under the all-zero matrix every score is 0 and every count 0
    zm = c["qr"] == R_ZERO_M
    assert zm.sum() == c["per_rel"][R_ZERO_M] and not got[:, zm].any() and not got_s[zm].any()


def test_ids_outside_the_tables():
    from mmre.rescal import RescalSweep, plan_keys, score_rows
    c = case(17)
    dv = c["dev"]
    spec = spec_of(dv["ent"], dv["mats"])
    t = lambda *x: torch.tensor(x, device=DEV)
    out = score_rows(spec, t(0, E, 1, -1, 2), t(1, 1, N_REL, 1, 2), t(3, 3, 3, 3, E + 5)).cpu().numpy()
    assert np.isfinite(out[0]) and np.isnan(out[1:]).all()
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    empty = score_rows(spec, none, none, none)
    assert empty.shape == (0,) and empty.dtype == torch.float32
    # queries with a head or a tail outside the table, on both sides, among good ones: NaN
    # threshold, never counted, and the others' counts as they were
    n = 40
    qh, qr, qt, qm = (c[k][:n].copy() for k in ("qh", "qr", "qt", "qm"))
    bad = [3, 8, 21, 30]
    qh[3], qm[3] = E, 0
    qt[8], qm[8] = -1, 0
    qh[21], qm[21] = -2, 1
    qt[30], qm[30] = E + 70, 1
    sw = RescalSweep(spec)
    res = sw.run(to(qh), to(qr), to(qt), to(qm), plan=plan_keys(qr, qm))
    got, truth = res["counts"].cpu().numpy(), res["truth"].cpu().numpy()
    good = np.setdiff1d(np.arange(n), bad)
    assert np.isnan(truth[bad]).all() and not got[:, bad].any()
    assert np.array_equal(got[0][good], c["want"][0][good])
    assert np.array_equal(truth[good], c["want_s"][good, c["truth_id"][good]])
    # a relation outside the table is refused on the host before anything is launched ...
    qr2 = qr.copy()
    qr2[5] = N_REL
    with pytest.raises(ValueError, match="outside the relation table"):
        sw.run(to(qh), to(qr2), to(qt), to(qm), plan=plan_keys(qr2, qm))
    # ... and a query whose relation is not its tile's key, or is outside the table under a plan
    # that does not know it, is emptied by the device: NaN threshold, counts 0
    res = sw.run(to(qh), to(qr2), to(qt), to(qm), plan=plan_keys(qr, qm))
    got2, truth2 = res["counts"].cpu().numpy(), res["truth"].cpu().numpy()
    assert np.isnan(truth2[bad + [5]]).all() and not got2[:, bad + [5]].any()
    keep = np.setdiff1d(good, [5])
    assert np.array_equal(got2[0][keep], c["want"][0][keep])


# ------------------------------------------------------------------------------- golden ---
CONFIGS = [("d32", 32), ("d40", 40)]


def golden_model(g, name, d, dl):
    from openke.module.model import RESCAL
    model = RESCAL(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), dim=d)
    sd = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in g.items()
          if k.startswith(name + ".") and k.endswith((".weight", "_const"))}
    model.load_state_dict(sd, strict=True)
    return model


@pytest.mark.parametrize("tc", [False, True])
@pytest.mark.parametrize("name,d", CONFIGS)
def test_tester_matches_the_reference(golden, name, d, tc):
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("rescal_small")
    dl = TestDataLoader(SMALL, "link")
    tester = Tester(model=golden_model(g, name, d, dl), data_loader=dl, use_gpu=True)
    metrics = tester.run_link_prediction(type_constrain=tc)
    ref = g[f"{name}.tc{int(tc)}_metrics"]
    print(name, tc, "got", metrics, "ref", ref.tolist())
    head, tail = tester.last["counts"]
    cols = 4 if tc else 2
    assert np.array_equal(head[:cols].T, g[f"{name}.tc{int(tc)}_head_counts"][:, :cols])
    assert np.array_equal(tail[:cols].T, g[f"{name}.tc{int(tc)}_tail_counts"][:, :cols])
    assert np.array_equal(np.array(metrics, np.float32), ref)       # (mrr, mr, hit10, hit3, hit1)


@pytest.mark.parametrize("name,d", CONFIGS)
def test_predict_and_rows_match_the_reference(golden, name, d):
    from mmre.rescal import RescalSweep, plan_keys, score_rows
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("rescal_small")
    dl = TestDataLoader(SMALL, "link")
    model = golden_model(g, name, d, dl)
    tester = Tester(model=model, data_loader=dl, use_gpu=True)
    ent, mats = (g[f"{name}.{k}.weight"] for k in TABLES)
    qh, qr, qt = (g[f"{name}.{k}"] for k in ("qh", "qr", "qt"))
    ids = np.arange(dl.get_ent_tot())
    for i, (dh, dt) in enumerate(dl):
        if i >= len(g[f"{name}.pred_head"]):
            break
        for data, side in ((dh, "head"), (dt, "tail")):
            ref = g[f"{name}.pred_{side}"][i]
            got = tester.test_one_step(data)
            head = side == "head"
            A = R.magnitude(ent, mats, ids if head else qh[i], qr[i], qt[i] if head else ids)
            dev = np.abs(got.astype(np.float64) - ref)
            print(f"{name} {side} {i}: predict within {float((dev / A).max()):.3g} A (bound {R.bound(d):.3g} A)")
            assert got.shape == ref.shape and np.all(dev <= R.bound(d) * A), (name, side, i)
    # score_rows and the sweep's truth are the restatement's bits
    T = len(qh)
    spec = model.score_spec()
    want = R.row_scores(ent, mats, qh, qr, qt)
    assert np.array_equal(score_rows(spec, to(qh), to(qr), to(qt)).cpu().numpy(), want)
    q4 = [np.concatenate([x, x]) for x in (qh, qr, qt)] + [np.repeat([0, 1], T).astype(np.int8)]
    res = RescalSweep(spec).run(*(to(x) for x in q4), plan=plan_keys(q4[1], q4[3]))
    assert np.array_equal(res["truth"].cpu().numpy(), np.concatenate([want, want]))
    for mode in (0, 1):
        s = R.sweep_scores(ent, mats, qh, qr, qt, mode)
        raw = R.rank_counts(s, qh if mode == 0 else qt)[0]
        assert np.array_equal(res["counts"].cpu().numpy()[0][mode * T:(mode + 1) * T], raw)


# ----------------------------------------------------------------------------- surfaces ---
def test_predict_modes_and_forward():
    """predict in the three modes through the model class is score_rows' bits; forward() -- torch
    ops -- is within the derived bound of -score_rows."""
    from mmre.rescal import score_rows
    from openke.module.model import RESCAL
    d = 50
    torch.manual_seed(3)
    model = RESCAL(ent_tot=E, rel_tot=N_REL, dim=d).to(DEV)
    model.ent_embeddings.weight.data *= 8.0
    model.rel_matrices.weight.data *= 8.0
    spec = model.score_spec()
    ent, mats = (getattr(model, k).weight.detach().cpu().numpy() for k in TABLES)
    ids = np.arange(E)
    one = lambda x: np.full(E, x)
    rng = np.random.default_rng(1)
    nh, nr, nt = rng.integers(0, E, 24), rng.integers(0, N_REL, 24), rng.integers(0, E, 24)
    for mode, data, (h, r, t) in (
            ("head_batch", dict(batch_h=ids, batch_t=np.array([LAST]), batch_r=np.array([1])), (ids, one(1), one(LAST))),
            ("tail_batch", dict(batch_h=np.array([4]), batch_t=ids, batch_r=np.array([3])), (one(4), one(3), ids)),
            ("normal", dict(batch_h=nh, batch_t=nt, batch_r=nr), (nh, nr, nt))):
        data = dict(data, mode=mode)
        rows = score_rows(spec, to(h), to(r), to(t)).cpu().numpy()
        assert np.array_equal(rows, R.row_scores(ent, mats, h, r, t))
        got = model.predict(data)
        assert got.dtype == np.float32 and np.array_equal(got, rows), mode
        with torch.no_grad():
            fwd = model({k: (to(v) if isinstance(v, np.ndarray) else v) for k, v in data.items()}).cpu().numpy()
        A = R.magnitude(ent, mats, h, r, t)
        dev = np.abs(fwd.astype(np.float64) + rows)
        print(f"{mode}: forward within {float((dev / A).max()):.3g} A of -score_rows (bound {R.bound(d):.3g} A)")
        assert np.all(dev <= R.bound(d) * A), mode


def test_triple_classification(golden):
    from mmre import rescal
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("rescal_small")
    dl = TestDataLoader(SMALL, "link")
    tester = Tester(model=golden_model(g, "d40", 40, dl), data_loader=dl, use_gpu=True)
    acc, thr = tester.run_triple_classification()
    pos, neg = tester.last["pos_scores"], tester.last["neg_scores"]
    n = len(dl.test_h)
    assert pos.shape == neg.shape == (n,)
    # both arrays are score_rows' bits on the same negatives, the positives' predict's
    spec = tester.model.score_spec()
    i64 = lambda a: to(np.asarray(a, np.int64))
    assert np.array_equal(rescal.score_rows(spec, i64(dl.test_h), i64(dl.test_r), i64(dl.test_t)).cpu().numpy(), pos)
    assert np.array_equal(rescal.score_rows(spec, i64(tester.last["neg_h"]), i64(dl.test_r),
                                            i64(tester.last["neg_t"])).cpu().numpy(), neg)
    rows = tester.model.predict({"batch_h": dl.test_h, "batch_t": dl.test_t, "batch_r": dl.test_r, "mode": "normal"})
    assert np.array_equal(rows, pos)
    ent, mats = (g[f"d40.{k}.weight"] for k in TABLES)
    assert np.array_equal(pos, R.row_scores(ent, mats, dl.test_h, dl.test_r, dl.test_t))
    # the threshold and the accuracy are the restatement's on those arrays
    want_thr, P, A, n_nan = TC.search(pos, neg)
    assert n_nan == 0 and thr == want_thr and acc == TC.accuracy(P, A, n, n)
    assert (tester.last["P"], tester.last["A"]) == (P, A)
    acc2, thr2 = tester.run_triple_classification(threshlod=thr)
    assert thr2 == thr
    with pytest.raises(NotImplementedError, match="RESCAL"):
        tester.run_relation_prediction()


def test_training_step_on_autograd():
    """One NegativeSampling(RESCAL, MarginLoss(1.0)) step on the autograd path: the gradients of
    both tables equal a float64 copy's (torch against torch, at float32 rounding)."""
    from openke.module.loss import MarginLoss
    from openke.module.model import RESCAL
    from openke.module.strategy import NegativeSampling
    B, NEG, d = 8, 3, 20
    torch.manual_seed(5)
    model = RESCAL(ent_tot=40, rel_tot=4, dim=d).to(DEV)
    model.ent_embeddings.weight.data *= 8.0
    model.rel_matrices.weight.data *= 8.0
    ns = NegativeSampling(model=model, loss=MarginLoss(margin=1.0), batch_size=B)
    assert model.ns_spec() is None and ns._transh_fused({}, "normal") is None
    rng = np.random.default_rng(2)
    n = B * (1 + NEG)
    data = {"batch_h": to(rng.integers(0, 40, n)), "batch_t": to(rng.integers(0, 40, n)),
            "batch_r": to(rng.integers(0, 4, n)), "mode": "normal"}
    loss = ns(data)
    assert loss.requires_grad and float(loss.detach()) > 0.0
    loss.backward()
    ref = RESCAL(ent_tot=40, rel_tot=4, dim=d).to(DEV).double()
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    ns64 = NegativeSampling(model=ref, loss=MarginLoss(margin=1.0).double(), batch_size=B)
    loss64 = ns64(data)
    assert loss64.dtype == torch.float64
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-5 * abs(float(loss64.detach()))
    for k in TABLES:
        got, want = getattr(model, k).weight.grad.double(), getattr(ref, k).weight.grad
        assert float(want.abs().max()) > 0.0
        worst = float((got - want).abs().max() / want.abs().max())
        print(f"{k}: gradient within {worst:.3g} of the largest element")
        assert worst <= 1e-5, k


def test_the_example_flow_on_the_small_dataset(tmp_path):
    """The reference's examples/train_rescal_FB15K237.py flow on the small dataset: two epochs of
    NegativeSampling(RESCAL, MarginLoss(1.0)) with Adagrad on autograd, a checkpoint round trip into
    a fresh model and run_link_prediction."""
    from openke.config import Tester, Trainer
    from openke.data import TestDataLoader, TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import RESCAL
    from openke.module.strategy import NegativeSampling
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    torch.manual_seed(0)
    n_ent, n_rel = tdl.get_ent_tot(), tdl.get_rel_tot()
    rescal = RESCAL(ent_tot=n_ent, rel_tot=n_rel, dim=50)
    model = NegativeSampling(model=rescal, loss=MarginLoss(margin=1.0), batch_size=tdl.get_batch_size())
    tables = [getattr(rescal, k).weight for k in TABLES]
    before = [p.detach().clone() for p in tables]
    trainer = Trainer(model=model, data_loader=tdl, train_times=2, alpha=0.1, use_gpu=True, opt_method="adagrad")
    trainer.run()
    assert trainer.used_one_call_step is False
    print("epoch losses", trainer.log)
    assert len(trainer.log) == 2 and trainer.log[1] < trainer.log[0]
    for b, p in zip(before, tables):
        assert not torch.equal(b.to(p.device), p.detach())
    path = str(tmp_path / "rescal.ckpt")
    rescal.save_checkpoint(path)
    fresh = RESCAL(ent_tot=n_ent, rel_tot=n_rel, dim=50)
    fresh.load_checkpoint(path)
    for k in TABLES:
        assert torch.equal(getattr(rescal, k).weight.detach().cpu(), getattr(fresh, k).weight.detach().cpu())
    dl = TestDataLoader(SMALL, "link")
    ra = Tester(model=rescal, data_loader=dl, use_gpu=True).run_link_prediction(type_constrain=False)
    rb = Tester(model=fresh, data_loader=dl, use_gpu=True).run_link_prediction(type_constrain=False)
    assert ra == rb and 0.0 < ra[0] <= 1.0


# ------------------------------------------------------------- several units per workgroup ---
NARROW, WIDE = 6, 40                                # kp 16: one K stage per unit; kp 48: three


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def unit_queries(n_ent, n_rel, per_key, seed, absent=()):
    """`per_key` queries per (relation, side), both sides of every relation but the absent ones, in
    an order that is not by key; the zero row, the copied row and the last row stand as truth and
    as anchor under the first relation with queries."""
    rng = np.random.default_rng(seed)
    rels = np.array([r for r in range(n_rel) if r not in absent])
    qr = np.repeat(rels, 2 * per_key)
    qm = np.tile(np.repeat([0, 1], per_key), len(rels)).astype(np.int8)
    n = len(qr)
    qh, qt = rng.integers(0, n_ent, n), rng.integers(0, n_ent, n)
    if per_key >= 3:
        qh[0], qt[1], qh[2] = ZERO_E, ZERO_E, n_ent - 1                 # head side: truth 0-row, anchor 0-row, last
        qt[per_key], qt[per_key + 1], qh[per_key + 2] = SRC, n_ent - 1, n_ent - 1   # tail side
    order = rng.permutation(n)
    return qh[order], qr[order].astype(np.int64), qt[order], qm[order]


def unit_tables(n_ent, n_rel, d, seed):
    rng = np.random.default_rng(seed)
    ent = rng.uniform(-0.5, 0.5, (n_ent, d)).astype(np.float32)
    mats = rng.uniform(-0.5, 0.5, (n_rel, d * d)).astype(np.float32)
    ent[ZERO_E] = 0.0
    ent[COPY] = ent[SRC]
    return ent, mats


def keyed_mixed_plan(qr, qm, tile_of_key, default=1):
    """tests/test_sweep_units_cpu.py's mixed_plan over the (relation, side) keys, `used` per relation."""
    from mmre.rescal import plan_keys
    plan = U.mixed_plan(2 * np.asarray(qr, np.int64) + qm, tile_of_key, default)
    plan["used"] = plan_keys(qr, qm)["used"]
    return plan


A_E, A_REL, A_ABSENT = 2200, 131, (0, 77, 130)
_shape_a = {}


def shape_a():
    """128 relations with queries on both sides, `per` per (relation, side) in tiles of one row --
    every eighth key in tiles of three: the smallest `per` at which every XCD group has four units
    for each of its workgroups of the production grid (16 x 4 x CUs at the most)."""
    if not _shape_a:
        n_et = -(-A_E // U.TE)
        tile_of = lambda key: 3 if key % 8 == 3 else 1
        per = 12
        while True:
            n_qt = sum(-(-per // tile_of(2 * r + s)) for r in range(A_REL) if r not in A_ABSENT for s in (0, 1))
            if min(U.UnitMap(g, 8, n_qt, n_et).count for g in range(8)) >= 4 * 8 * cus():
                break
            per += 1
        qh, qr, qt, qm = unit_queries(A_E, A_REL, per, seed=61, absent=A_ABSENT)
        plan = keyed_mixed_plan(qr, qm, {k: 3 for k in range(2 * A_REL) if tile_of(k) == 3})
        assert len(plan["tiles"]) == n_qt
        _shape_a.update(q=(qh, qr, qt, qm), plan=plan, per=per, truth_id=np.where(qm == 0, qh, qt))
    return _shape_a


def check_grid_a(s):
    """The arithmetic that makes shape A mean something, from the device's CU count, before any launch."""
    n_cu = cus()
    tiles = s["plan"]["tiles"]
    n_qt, n_et = len(tiles), -(-A_E // U.TE)
    assert n_et == 18 and set(tiles[:, 2].tolist()) <= {1, 2, 3} and 3 in tiles[:, 2]
    assert sorted(set(range(A_REL)) - set(s["plan"]["used"].tolist())) == list(A_ABSENT)
    # both sides are mixed: the key -- entity operand and side -- changes every `per` tiles at the most
    assert set((tiles[:, 0] & 1).tolist()) == {0, 1}
    assert np.diff(np.nonzero(np.diff(tiles[:, 0]))[0]).max() <= s["per"]
    assert U.sweep_units(n_qt, n_et) >= 64 * n_cu                     # the grid is 16 x resident, not the unit count
    for per in (1, 2, 3, 4):                                          # whatever the occupancy: at most 4 per CU
        g, n_groups = U.launch_grid(n_qt, n_et, per * n_cu)
        assert g == 16 * per * n_cu and n_groups == 8
        assert min(U.UnitMap(grp, 8, n_qt, n_et).count for grp in range(8)) // (g // 8) >= 4
    visits, per_wg, crossing, leftover = U.walk(n_qt, n_et, 64 * n_cu, 8)
    assert np.all(visits == 1) and per_wg.min() >= 4 and crossing > 32 * n_cu and leftover == 2 * n_qt
    return per_wg


@pytest.mark.parametrize("d", [NARROW, WIDE])
def test_several_units_per_workgroup(d):
    from mmre.rescal import RescalSweep, plan_keys
    s = shape_a()
    per_wg = check_grid_a(s)
    qh, qr, qt, qm = s["q"]
    Q = len(qh)
    ent, mats = unit_tables(A_E, A_REL, d, seed=70 + d)
    from mmre.link import FilterIndex
    types = np.random.default_rng(8).random((2, A_REL, A_E)) < 0.5    # [head side / tail side][relation][entity]
    idx = FilterIndex(qh, qr, qt, A_E, A_REL, [np.nonzero(x)[0] for x in types[0]], [np.nonzero(x)[0] for x in types[1]])
    masks = tuple(to(m) for m in idx.type_masks())
    # the restatement: every query at one stage; at three stages the queries of every twelfth tile
    # (with the hand-placed ones), the others' counts held to the full-tile run below
    if d == NARROW:
        sel = np.arange(Q)
    else:
        perm, tiles = s["plan"]["perm"], s["plan"]["tiles"]
        sel = np.unique(np.concatenate([perm[f:f + n] for k, f, n in tiles[::12]] +
                                       [np.nonzero((qr == qr[perm[0]]))[0]]))
    want_s = R.sweep_scores(ent, mats, qh[sel], qr[sel], qt[sel], qm[sel])
    allowed = types[np.where(qm[sel] == 0, 0, 1), qr[sel]]
    want = R.rank_counts(want_s, s["truth_id"][sel], None, allowed)
    sw = RescalSweep(spec_of(to(ent), to(mats)))
    dq = tuple(to(x) for x in (qh, qr, qt, qm))
    res = sw.run(*dq, type_masks=masks, plan=s["plan"])
    got, truth = res["counts"].cpu().numpy(), res["truth"].cpu().numpy()
    print(f"d {d}: {len(s['plan']['tiles'])} query tiles, {per_wg.min()}..{per_wg.max()} units per workgroup, "
          f"counts differing {int((got[:, sel] != want).any(0).sum())} of {len(sel)} restated queries, truth "
          f"differing {int((truth != R.row_scores(ent, mats, qh, qr, qt)).sum())} of {Q}")
    assert np.array_equal(got[0, sel], want[0]) and np.array_equal(got[2, sel], want[2])
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[3], got[2])          # no filter
    assert np.array_equal(truth, R.row_scores(ent, mats, qh, qr, qt))
    assert want[0].max() > 1000 and (want[2] < want[0]).any()
    again = sw.run(*dq, type_masks=masks, plan=s["plan"])
    assert np.array_equal(again["counts"].cpu().numpy(), got) and np.array_equal(again["truth"].cpu().numpy(), truth)
    # the padded rows count nothing: full 128-row tiles give every query the same counts
    full = sw.run(*dq, type_masks=masks, plan=plan_keys(qr, qm))["counts"].cpu().numpy()
    assert np.array_equal(full, got)
    # a relation without a query leaves the others' counts as they were
    keep = np.nonzero(qr % 16 != 7)[0]
    sub = sw.run(*(to(x[keep]) for x in (qh, qr, qt, qm)), plan=plan_keys(qr[keep], qm[keep], tile=2))
    assert np.array_equal(sub["counts"].cpu().numpy()[0], got[0][keep])
    assert np.array_equal(sub["truth"].cpu().numpy(), truth[keep])


C_E, C_REL = 1100, 6


def test_fewer_units_than_workgroups():
    from mmre.link import FilterIndex
    from mmre.rescal import RescalSweep, plan_keys
    qh, qr, qt, qm = unit_queries(C_E, C_REL, 70, seed=67, absent=(2,))
    plan = plan_keys(qr, qm)
    n_qt, n_et = len(plan["tiles"]), -(-C_E // U.TE)
    assert (n_qt, n_et) == (10, 9)
    n_cu = cus()
    g, n_groups = U.launch_grid(n_qt, n_et, n_cu)                     # the unit count, whatever the occupancy
    assert (g, n_groups) == (160, 8) == U.launch_grid(n_qt, n_et, 4 * n_cu)
    visits, per_wg, crossing, leftover = U.walk(n_qt, n_et, g, n_groups)
    assert np.all(visits == 1) and (per_wg == 0).sum() == 70 and per_wg.max() == 1 and leftover == 10
    ent, mats = unit_tables(C_E, C_REL, WIDE, seed=71)
    rng = np.random.default_rng(9)
    types = rng.random((2, C_REL, C_E)) < 0.5
    idx = FilterIndex(qh, qr, qt, C_E, C_REL, [np.nonzero(x)[0] for x in types[0]], [np.nonzero(x)[0] for x in types[1]])
    want_s = R.sweep_scores(ent, mats, qh, qr, qt, qm)
    truth_id = np.where(qm == 0, qh, qt)
    foff, fids = idx.filters(qh, qr, qt, qm)
    lists = [fids[foff[i]:foff[i + 1]] for i in range(len(qh))]
    want = R.rank_counts(want_s, truth_id, lists, types[np.where(qm == 0, 0, 1), qr])
    sw = RescalSweep(spec_of(to(ent), to(mats)))
    res = sw.run(*(to(x) for x in (qh, qr, qt, qm)), filt=tuple(to(a) for a in idx.groups(qh, qr, qt, qm)),
                 type_masks=tuple(to(m) for m in idx.type_masks()), plan=plan)
    got, truth = res["counts"].cpu().numpy(), res["truth"].cpu().numpy()
    print(f"idle workgroups: counts differing {int((got != want).any(0).sum())} of {len(qh)} queries")
    assert np.array_equal(got, want) and np.array_equal(truth, want_s[np.arange(len(qh)), truth_id])
