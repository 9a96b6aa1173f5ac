"""TransR training on the HIP path (csrc/transh_train.hip's TransR part, mmre.transr_ns): the fused
loss, the grouped f32-MFMA GEMMs (projection, entity gradient, matrix gradient) and the row-owner
sums against float64, at every width class, batch class, hub size and option, the in-pass SGD
step, and the surfaces (NegativeSampling, Trainer).

Yardstick, tolerances and seeds: tests/transr_train_cases.py. Scores within 1e-4 max(1, |s|), loss
within 1e-5 relative, each gradient table within 1e-4 of that table's largest reference entry (per
row for the clamp cases); two runs bit-equal (loss and gradients); rows the batch does not touch
exactly zero; no NaN.

Boundaries of the kernels, and where they are tested:
  - width: the MFMA's K step (2) and N step (32), the GEMMs' K block (32) and column chunk (128),
    the dmat tile (64 x 128), 16-byte loads (dims that are / are not multiples of 4), and the row
    kernels' NC = 1 / 2 / 4 / 8 from dim_r <= 64 / 128 / 256 / 512, with dim_e above and below
    dim_r (test_widths);
  - a positive's K + 1 rows over its four waves, the hinge's 64-lane stride, K = 512
    (test_batch_classes);
  - the MFMA row tile TR_TM = 32 slots, the rank segment TR_ISEG = 1,024 slots and the dmat
    segment TR_DSEG = 1,024 slots of one relation, and the relation owner's TH_SEG = 1,024 batch
    rows (test_hub_relation, test_hub_edges, test_several_row_tiles);
  - the entity owner's list classes: up to 64 slots, up to TH_REGL_LIST = 1,024, longer
    (test_hub_entity).
"""
import os

import numpy as np
import pytest
import torch

import transr_train_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "small") + "/"
KEYS = C.KEYS


def _spec(c):
    from mmre.transr_ns import TRSpec
    return TRSpec(c["p_norm"], c["de"], c["dr"], c["nf"], c["model_margin"])


def _run(c, opt_factory=None, pass_optimizer=False, pre_grad=False):
    """Forward + backward on fresh device copies of the case's tables; with opt_factory, that
    optimizer over them steps afterwards (pass_optimizer: it is also handed to fused_ns_loss)."""
    from mmre.transr_ns import fused_ns_loss
    T = {k: c["tabs"][k].to(DEV).clone().requires_grad_(True) for k in KEYS}
    opt = opt_factory([T[k] for k in KEYS]) if opt_factory is not None else None
    if pre_grad:
        T["rel"].grad = torch.zeros_like(T["rel"])
    loss, score = fused_ns_loss(_spec(c), *(T[k] for k in KEYS), c["h"].to(DEV), c["t"].to(DEV), c["r"].to(DEV),
                                c["B"], c["K"], c["margin"], c["adv"], c["regul"],
                                optimizer=opt if pass_optimizer else None)
    out = dict(loss=loss.detach().cpu(), score=score.detach().cpu())
    loss.backward()
    out["grads"] = {k: T[k].grad.clone() for k in KEYS}
    if opt is not None:
        out["claimed"] = len(getattr(opt, "_fused_done", {}))
        opt.step()
        out["params"] = {k: T[k].detach().clone() for k in KEYS}
    torch.cuda.synchronize()
    return out


def _touched(c):
    ent, rel = np.zeros(c["n_ent"], bool), np.zeros(c["n_rel"], bool)
    ent[c["h"].numpy()] = True
    ent[c["t"].numpy()] = True
    rel[c["r"].numpy()] = True
    return {"ent": ent, "rel": rel, "transfer_matrix": rel}


def _check(c, label="", both_sides=True, per_row=False):
    """What every case asserts; returns the first run."""
    ref_loss, rs, rg, (x_min, hinge_min, active) = c["ref"]
    assert C.clear(c["ref"], c["B"], c["K"], both_sides)  # on the CPU, before any GPU call
    a, b = _run(c), _run(c)
    serr = np.abs(a["score"].numpy() - rs).max()
    print(f"{label} seed {c['seed']} slots {c['slots']}: loss {float(a['loss']):.9g} ref {ref_loss:.9g} "
          f"(relative {abs(float(a['loss']) - ref_loss) / abs(ref_loss):.3g}); score err {serr:.3g} of "
          f"{np.abs(rs).max():.3g}; L1 clearance {x_min:.3g}, min hinge gap {hinge_min:.3g}, active {active:.2f}")
    G = {k: a["grads"][k].cpu().double().numpy() for k in KEYS}
    for k in KEYS:
        scale = np.abs(rg[k]).max(axis=1, keepdims=True) if per_row else np.abs(rg[k]).max()
        with np.errstate(invalid="ignore", divide="ignore"):
            relerr = np.nanmax(np.where(scale > 0, np.abs(G[k] - rg[k]) / scale, 0.0))
        print(f"  grad {k}: err {np.abs(G[k] - rg[k]).max():.3g} of {np.abs(rg[k]).max():.3g} (relative {relerr:.3g})")
    assert np.isfinite(float(a["loss"])) and np.isfinite(a["score"].numpy()).all()
    assert np.all(np.abs(a["score"].numpy() - rs) <= 1e-4 * np.maximum(1.0, np.abs(rs)))
    assert abs(float(a["loss"]) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert torch.equal(a["loss"], b["loss"])
    touched = _touched(c)
    for k in KEYS:
        assert np.isfinite(G[k]).all(), k
        if per_row:  # each row against its own largest reference entry (clamped rows carry 1e12 coefficients)
            bound = 1e-4 * np.abs(rg[k]).max(axis=1, keepdims=True)
            assert np.all(np.abs(G[k] - rg[k]) <= bound), (k, np.abs(G[k] - rg[k]).max())
        else:
            assert np.abs(G[k] - rg[k]).max() <= 1e-4 * np.abs(rg[k]).max(), (k, np.abs(G[k] - rg[k]).max())
        assert torch.equal(a["grads"][k], b["grads"][k]), k   # bit-reproducible
        assert not G[k][~touched[k]].any(), k                 # rows outside the batch: exactly zero
    return a


# ---- 1. widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("de,dr", C.WIDTHS)
@pytest.mark.parametrize("p_norm,nf", C.COMBOS)
def test_widths(p_norm, nf, de, dr):
    _check(C.case(p_norm, nf, de, dr, 4, 3), f"p{p_norm} norm {nf} d ({de}, {dr})")


def test_identity_matrices():
    """The model's own initialisation (no rand_init): M_r the dim_e x dim_r identity."""
    c = C.case(*C.IDENTITY, identity=True)
    M = c["tabs"]["transfer_matrix"].view(c["n_rel"], c["de"], c["dr"])
    assert torch.equal(M[1], torch.eye(c["de"], c["dr"]))
    _check(c, "identity matrices")


# ---- 2. batch classes ------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", C.BATCH_CLASSES)
@pytest.mark.parametrize("de,dr", C.CLASS_DIMS)
@pytest.mark.parametrize("p_norm,nf", C.COMBOS)
def test_batch_classes(p_norm, nf, de, dr, B, K):
    c = C.case(p_norm, nf, de, dr, B, K)
    if K > 1 and C.R > 1 and B * K > 40:  # the layout's random rows: some relation differs from its positive's
        assert bool((c["r"][c["B"]:] != c["r"][:c["B"]].repeat(c["K"])).any())
    _check(c, f"p{p_norm} norm {nf} d ({de}, {dr}) B {B} K {K}")


@pytest.mark.parametrize("B,K", C.L1_WIDE)
def test_l1_wide(B, K):
    _check(C.case(1, True, 200, 200, B, K), f"L1 d 200 B {B} K {K}")


@pytest.mark.parametrize("p_norm,de,dr", ((2, 200, 200), (1, 9, 7)))
def test_several_row_tiles(p_norm, de, dr):
    """Six relations with more than TR_TM slots each."""
    c = C.case(p_norm, True, de, dr, *C.MULTI_TILE)
    assert c["slots"] > 6 * 4 * C.TR_TM
    _check(c, f"p{p_norm} d ({de}, {dr}) B {c['B']} K {c['K']}")


# ---- 3. hubs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", C.HUB_SEG)
def test_hub_relation(B, K):
    """One relation owns every slot: past TR_ISEG = TR_DSEG slots and TH_SEG rows, and a few row tiles."""
    c = C.case(1, True, 9, 7, B, K, n_rel=1)
    if B >= 205:
        assert c["slots"] > C.TR_DSEG and c["slots"] > C.TR_ISEG and B * (1 + K) >= C.TH_SEG
    else:
        assert C.TR_TM < c["slots"] < 4 * C.TR_TM
    _check(c, f"R 1 B {B} K {K}")


def test_hub_edges():
    """One-relation batches whose slot counts lie on either side of TR_TM and of TR_DSEG = TR_ISEG."""
    cs = [C.case(1, True, 9, 7, B, K, n_rel=1) for B, K in C.HUB_EDGE]
    assert cs[0]["slots"] <= C.TR_TM < cs[1]["slots"] < 2 * C.TR_TM
    assert C.TR_DSEG - 8 <= cs[2]["slots"] <= C.TR_DSEG == C.TR_ISEG < cs[3]["slots"] <= C.TR_DSEG + 8
    for c in cs:
        _check(c, f"R 1 B {c['B']} K {c['K']}")


@pytest.mark.parametrize("B,K", C.HUB_SEG_WIDE)
def test_hub_relation_wide(B, K):
    c = C.case(2, False, 200, 200, B, K, n_rel=1)
    assert c["slots"] > C.TR_DSEG
    _check(c, f"R 1 d 200 B {B} K {K}")


@pytest.mark.parametrize("B,K", C.HUB_HEAD)
def test_hub_entity(B, K):
    c = C.case(1, True, 9, 7, B, K, one_head=True)
    assert int((c["h"][:B] == 3).sum()) == B > 64 and (B > C.TH_REGL_LIST) == (B == 1100)
    _check(c, f"one head B {B} K {K}")


def test_hub_entity_wide():
    _check(C.case(2, True, 200, 200, 70, 3, one_head=True), "one head d 200")


# ---- 4. options ------------------------------------------------------------------------------
@pytest.mark.parametrize("p_norm,nf", C.OPTION_COMBOS)
@pytest.mark.parametrize("opt", ("model_margin", "adv", "regul0"))
def test_options(p_norm, nf, opt):
    kw = {"model_margin": dict(model_margin=6.0), "adv": dict(adv=1.0), "regul0": dict(regul=0.0)}[opt]
    _check(C.case(p_norm, nf, 200, 200, 5, 25, **kw), f"p{p_norm} norm {nf} {opt}")


@pytest.mark.parametrize("p_norm,nf", C.OPTION_COMBOS)
def test_regulariser_alone(p_norm, nf):
    """A loss margin so negative that no hinge term is active: the gradient is the regulariser's,
    in all three tables, with the factor 2 S of its square (TransR.regularization)."""
    c = C.case(p_norm, nf, 200, 200, 5, 25, loss_margin=-1000.0, both_sides=False)
    assert c["ref"][3][2] == 0.0 and all(np.abs(c["ref"][2][k]).max() > 0 for k in KEYS)
    a = _check(c, f"p{p_norm} norm {nf} regulariser alone", both_sides=False)
    N = len(c["r"])
    tabs = {k: c["tabs"][k].double().numpy() for k in KEYS}
    h, t, r = (c[k].numpy() for k in ("h", "t", "r"))
    S = ((tabs["ent"][h] ** 2).mean() + (tabs["ent"][t] ** 2).mean() + (tabs["rel"][r] ** 2).mean()
         + (tabs["transfer_matrix"][r] ** 2).mean()) / 4.0
    occ_r = np.bincount(r, minlength=c["n_rel"])[:, None]
    occ_e = (np.bincount(h, minlength=c["n_ent"]) + np.bincount(t, minlength=c["n_ent"]))[:, None]
    for k, occ, n in (("ent", occ_e, c["de"]), ("rel", occ_r, c["dr"]), ("transfer_matrix", occ_r, c["de"] * c["dr"])):
        want = 0.5 * 2.0 * S * 2.0 * occ * tabs[k] / (4.0 * N * n)   # regul 2 S (2 w / (N n)) / 4 per gathered row
        got = a["grads"][k].cpu().double().numpy()
        assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), k


# ---- 5. clamps -------------------------------------------------------------------------------
@pytest.mark.parametrize("p_norm,nf", C.COMBOS)
def test_clamps(p_norm, nf):
    c = C.case(p_norm, nf, *C.CLAMP_DIMS, 4, 3, zero_rows=True)
    tabs = c["tabs"]
    assert not tabs["ent"][int(c["h"][0])].any() and not tabs["transfer_matrix"][int(c["r"][0])].any()
    assert (not tabs["rel"][int(c["r"][-1])].any()) == nf
    if nf:  # m = 0 under the clamp: the reference's gradient into the zero matrix carries the 1e12
        assert np.abs(c["ref"][2]["transfer_matrix"][int(c["r"][0])]).max() > 1e9
    _check(c, f"p{p_norm} norm {nf} clamps", per_row=True)


# ---- 6. in-pass SGD --------------------------------------------------------------------------
@pytest.mark.parametrize("p_norm,nf,de,dr", ((1, True, 200, 200), (2, False, 65, 64)))
def test_in_pass_sgd(p_norm, nf, de, dr):
    from mmre.optim import SGD, Adagrad
    c = C.case(p_norm, nf, de, dr, 4, 3) if de == 65 else C.case(p_norm, nf, de, dr, 5, 25)
    sgd = lambda ps: SGD(ps, lr=0.5)
    plain, fused = _run(c, sgd), _run(c, sgd, pass_optimizer=True)
    assert plain["claimed"] == 0 and fused["claimed"] == 3      # step() skips the three tables
    for k in KEYS:
        assert torch.equal(plain["params"][k], fused["params"][k]), k          # bit-equal parameters
        assert torch.equal(plain["grads"][k], fused["grads"][k]), k            # gradients still written
        assert not torch.equal(fused["params"][k], c["tabs"][k].to(DEV)), k
    # nothing claimed, and step() gives the same parameters: a table already has a gradient; momentum (its first
    # step is the plain one); torch's SGD (p - lr g: the fma's rounding apart)
    pre = _run(c, sgd, pass_optimizer=True, pre_grad=True)
    mom = _run(c, lambda ps: SGD(ps, lr=0.5, momentum=0.9), pass_optimizer=True)
    tor = _run(c, lambda ps: torch.optim.SGD(ps, lr=0.5), pass_optimizer=True)
    assert pre["claimed"] == 0 and mom["claimed"] == 0 and tor["claimed"] == 0
    for k in KEYS:
        tol = 1e-6 * float(plain["params"][k].abs().max())
        assert torch.equal(pre["params"][k], plain["params"][k]), k
        assert torch.allclose(mom["params"][k], plain["params"][k], rtol=0, atol=tol), k
        assert torch.allclose(tor["params"][k], plain["params"][k], rtol=0, atol=tol), k
    # Adagrad is ignored by the path: its own step() updates
    ada = _run(c, lambda ps: Adagrad(ps, lr=0.5), pass_optimizer=True)
    assert ada["claimed"] == 0
    T = {k: c["tabs"][k].to(DEV).clone().requires_grad_(True) for k in KEYS}
    ref = torch.optim.Adagrad([T[k] for k in KEYS], lr=0.5)
    for k in KEYS:
        T[k].grad = plain["grads"][k].clone()
    ref.step()
    for k in KEYS:
        assert torch.allclose(ada["params"][k], T[k].detach(), rtol=0, atol=1e-6 * float(T[k].detach().abs().max())), k


# ---- 7. training score against predict -------------------------------------------------------
@pytest.mark.parametrize("p_norm,nf", C.COMBOS)
def test_score_against_predict(p_norm, nf):
    from mmre.link import ScoreSpec
    from mmre.transr import score_rows
    c = C.case(p_norm, nf, 256, 200, 4, 3)
    a = _run(c)
    T = {k: c["tabs"][k].to(DEV) for k in KEYS}
    spec = ScoreSpec(model="transr" if p_norm == 1 else "transr_l2", ent=T["ent"], rel=T["rel"], dim=c["dr"],
                     norm_flag=nf, pred_kind=0, margin=0.0, dim_e=c["de"], transfer_matrix=T["transfer_matrix"])
    s = score_rows(spec, c["h"].to(DEV), c["r"].to(DEV), c["t"].to(DEV)).cpu().numpy()
    assert np.all(np.abs(a["score"].numpy() - s) <= 1e-4 * np.maximum(1.0, np.abs(s)))


# ---- 8. surfaces -----------------------------------------------------------------------------
def _strategy(c, loss, device, dtype=torch.float32):
    from openke.module.model import TransR
    from openke.module.strategy import NegativeSampling
    m = TransR(c["n_ent"], c["n_rel"], dim_e=c["de"], dim_r=c["dr"], p_norm=c["p_norm"], norm_flag=c["nf"])
    with torch.no_grad():
        for k, w in C.weights(m).items():
            w.copy_(c["tabs"][k])
    return NegativeSampling(model=m.to(device).to(dtype), loss=loss.to(device), batch_size=c["B"], regul_rate=c["regul"])


def _data(c, device, mode="normal"):
    return {"batch_h": c["h"].to(device), "batch_t": c["t"].to(device), "batch_r": c["r"].to(device), "mode": mode}


def _generic_loss(strategy, data):
    """The generic branch's value on the batch: scores through model(data), the loss module, the
    model's regularization (what NegativeSampling.forward did for TransR before the fused path)."""
    score = strategy.model(data)
    loss = strategy.loss(strategy._get_positive_score(score), strategy._get_negative_score(score))
    return loss + strategy.regul_rate * strategy.model.regularization(data)


def test_strategy_takes_the_fused_path():
    from mmre import transr_ns
    from openke.module.loss import MarginLoss
    c = C.case(1, True, 256, 200, 4, 3)
    st, eager = _strategy(c, MarginLoss(margin=4.0), DEV), _strategy(c, MarginLoss(margin=4.0), DEV)
    data = _data(c, DEV)
    n0 = transr_ns.calls
    loss = st(data)
    assert transr_ns.calls == n0 + 1
    want = _generic_loss(eager, data)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    loss.backward()
    want.backward()
    for (k, p), q in zip(C.weights(st.model).items(), C.weights(eager.model).values()):
        big = float(q.grad.abs().max())
        assert big > 0 and float((p.grad - q.grad).abs().max()) <= 1e-4 * big, k


def test_fused_and_generic_agree_on_the_small_dataset():
    """One sampler-made batch of tests/golden/data/small through both branches."""
    from mmre import transr_ns
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransR
    from openke.module.strategy import NegativeSampling
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    data = next(iter(tdl))
    data = {k: (torch.as_tensor(v).to(DEV) if k != "mode" else v) for k, v in data.items()}
    assert data["mode"] == "normal"
    torch.manual_seed(0)
    m = TransR(ent_tot=tdl.get_ent_tot(), rel_tot=tdl.get_rel_tot(), dim_e=40, dim_r=32, p_norm=1, norm_flag=True,
               rand_init=True).to(DEV)
    st = NegativeSampling(model=m, loss=MarginLoss(margin=4.0).to(DEV), batch_size=tdl.get_batch_size(), regul_rate=0.1)
    n0 = transr_ns.calls
    loss = st(data)
    assert transr_ns.calls == n0 + 1
    loss.backward()
    got = {k: w.grad.clone() for k, w in C.weights(m).items()}
    st.zero_grad()
    want = _generic_loss(st, data)
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    for k, w in C.weights(m).items():
        big = float(w.grad.abs().max())
        assert big > 0 and float((got[k] - w.grad).abs().max()) <= 1e-4 * big, k


@pytest.mark.parametrize("why", ("softplus", "head_batch", "float64", "cpu"))
def test_strategy_keeps_the_generic_branch(why):
    from mmre import transr_ns
    from openke.module.loss import MarginLoss, SoftplusLoss
    c = C.case(1, True, 256, 200, 4, 3)
    loss = SoftplusLoss() if why == "softplus" else MarginLoss(margin=4.0)
    dev = torch.device("cpu") if why == "cpu" else DEV
    st = _strategy(c, loss, dev, torch.float64 if why == "float64" else torch.float32)
    data = _data(c, dev, "head_batch" if why == "head_batch" else "normal")
    if why == "head_batch":  # a cross-sampling batch: B tails and relations, B (1 + K) heads
        data["batch_t"], data["batch_r"] = data["batch_t"][:c["B"]], data["batch_r"][:c["B"]]
    n0 = transr_ns.calls
    got = st(data)
    assert transr_ns.calls == n0
    want = _generic_loss(st, data)
    assert torch.equal(got.detach(), want.detach())


def test_trainer_runs_transr_fused():
    """The reference's examples/train_transr_FB15K237.py recipe (its second stage) on the small dataset."""
    from mmre import transr_ns
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss
    from openke.module.model import TransR
    from openke.module.strategy import NegativeSampling
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    torch.manual_seed(0)
    transr = TransR(ent_tot=tdl.get_ent_tot(), rel_tot=tdl.get_rel_tot(), dim_e=40, dim_r=32, p_norm=1, norm_flag=True,
                    rand_init=False)
    tabs = list(C.weights(transr).values())
    before = [p.detach().clone() for p in tabs]
    model = NegativeSampling(model=transr, loss=MarginLoss(margin=4.0), batch_size=tdl.get_batch_size())
    trainer = Trainer(model=model, data_loader=tdl, train_times=2, alpha=1.0, use_gpu=True)
    n0 = transr_ns.calls
    trainer.run()
    assert transr_ns.calls == n0 + 20 and trainer.used_one_call_step is False
    assert len(trainer.log) == 2 and trainer.log[1] < trainer.log[0]
    for b, p in zip(before, tabs):
        assert not torch.equal(b.to(p.device), p.detach())


def test_unsupported_shapes_raise_before_any_launch():
    from mmre._lib import MMREError
    from mmre.transr_ns import TRSpec, fused_ns_loss, supported
    assert supported(512, 512, 512) and supported(1, 512, 1) and supported(512, 1, 1)
    assert not supported(513, 7, 3) and not supported(7, 513, 3) and not supported(7, 7, 513) and not supported(7, 7, 0)
    for de, dr in ((513, 7), (7, 513)):
        ent = torch.zeros(5, de, device=DEV)
        rel = torch.zeros(2, dr, device=DEV)
        tm = torch.zeros(2, de * dr, device=DEV)
        ids = torch.zeros(8, dtype=torch.int64, device=DEV)
        with pytest.raises(MMREError):
            fused_ns_loss(TRSpec(1, de, dr), ent, rel, tm, ids, ids, ids, 2, 3, 1.0)


# ---- 9. the reference's own numbers ----------------------------------------------------------
def test_reference_fixture(golden):
    """tests/golden/transr_train.npz: the reference's TransR + MarginLoss + NegativeSampling in
    float64 (tests/golden/make_transr_train.py)."""
    from mmre.transr_ns import TRSpec, fused_ns_loss
    g = golden("transr_train")
    for name in [str(n) for n in g["names"]]:
        z = lambda k: g[f"{name}.{k}"]
        p_norm, nf, B, K = int(z("p_norm")), bool(z("norm_flag")), int(z("B")), int(z("K"))
        de, dr = int(z("dim_e")), int(z("dim_r"))
        w = lambda k: torch.from_numpy(g[f"d{de}_{dr}.{k}"])   # a width pair's four cases share tables and batch
        T = {k: w(k).to(DEV).requires_grad_(True) for k in KEYS}
        h, t, r = (w(k).to(DEV) for k in ("h", "t", "r"))
        loss, score = fused_ns_loss(TRSpec(p_norm, de, dr, nf), *(T[k] for k in KEYS), h, t, r, B, K,
                                    float(z("loss_margin")), None, float(z("regul")))
        loss.backward()
        rs = z("score")
        assert np.all(np.abs(score.cpu().numpy() - rs) <= 1e-4 * np.maximum(1.0, np.abs(rs))), name
        assert abs(float(loss.detach()) - float(z("loss"))) <= 1e-5 * abs(float(z("loss"))), name
        for k in KEYS:
            gw = z("grad_" + k)
            err = np.abs(T[k].grad.cpu().double().numpy() - gw).max()
            assert err <= 1e-4 * np.abs(gw).max(), (name, k, err)
