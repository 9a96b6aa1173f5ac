"""The negative-sampling training step at every width and K class: the shape, not the arithmetic,
selects the kernel instantiation (csrc/ns.hip: NC = 1 / 2 / 4 / 8 row elements per lane for dim <=
64 / 128 / 256 / 512, 16 / 32 on the rows path up to 2,048; the fused TransE kernel up to K = 32,
the generic slot kernel in chunks of 21 negatives, K <= 512 in LDS), so this file varies the shape:
both sides of every class boundary, widths below a wave, 1 to 4 positives (a workgroup holds 4),
and the shapes past the fused kernels, which take the rows path (mmre.ns.fused_supported).

Small synthetic tables (E 301, R 6: E + R is no multiple of the 4 table rows of an owner
workgroup), batches in the [pos | neg_1 | ... | neg_K] layout of tests/test_ns_losses_gpu.py. Every
case: scores, loss and every gradient table against float64 (oracle/ref_trainer for the margin
loss, tests/test_ns_losses_gpu.py::_reference for softplus / sigmoid), two runs bit-identical,
untouched table rows exactly zero, no NaN. Tolerances are the suite's: scores 1e-4 max(1, |s|), loss
1e-5 relative, gradients 1e-4 of the table's largest entry -- for L1 TransE with NO exempt row.

Seeds. A float32 run and a float64 reference may legitimately take different sides of a kink: the
L1 subgradient sign(x) at x = 0 and the hinge max(p - n, -m) at p - n = -m. Each case therefore
takes the first seed whose float64 reference ALONE stays clear of both -- no element x = (h + r) - t
of an L1 TransE row below the suite's 1e-7 (zero exempt rows) or within eight float32 roundings of
its operands (|x| < 8 * 2^-24 (|h| + |r| + |t|): the widths 1 and 7 hold elements near 8), no hinge
argument within 1e-5 max(1, |s|) of its kink (a hundred float32 roundings of a score) -- asserted
on the CPU before any GPU call. The expected number of such elements per case is below 1."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E, R = 301, 6
SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "small") + "/"

#           variant -> (model, norm_flag)
VARIANTS = {"transe_n": ("transe", True), "transe": ("transe", False), "transe_l2_n": ("transe_l2", True),
            "distmult": ("distmult", False), "complex": ("complex", False), "rotate": ("rotate", False)}
GENERIC = ("distmult", "complex", "rotate")
# loss margins that leave hinge terms on both sides of the kink at these tables' score spreads
MARGIN = {"transe": 1.0, "transe_l2": 0.05, "distmult": 3.0, "complex": 3.0, "rotate": 0.25}


def _tables(model, d, seed, n_ent=E, n_rel=R):
    """tests/test_ns_losses_gpu.py::_tables, per model, at any width."""
    g = torch.Generator().manual_seed(seed)
    u = lambda n, c, s: (torch.rand((n, c), generator=g) * 2 - 1) * s
    if model == "distmult":
        return {"ent": u(n_ent, d, 1.5), "rel": u(n_rel, d, 1.5)}
    if model == "complex":
        return {"ent": u(n_ent, d, 1.5), "ent_im": u(n_ent, d, 1.5), "rel": u(n_rel, d, 1.5),
                "rel_im": u(n_rel, d, 1.5)}
    if model == "rotate":
        return {"ent": u(n_ent, 2 * d, 8.0 / (2 * d)), "rel": u(n_rel, d, 8.0 / d)}
    return {"ent": u(n_ent, d, 8.0 / d), "rel": u(n_rel, d, 8.0 / d)}


def _batch(B, K, seed):
    """[pos | neg_1 | ... | neg_K] as tests/test_ns_losses_gpu.py::_batch: negative j corrupts the
    head (j even) or the tail (j odd); about 5 % of the negative rows are fully random; negative
    K // 2 of one positive is a copy of it."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda hi, n: torch.randint(0, hi, (n,), generator=g)
    h, t, r = ri(E, B), ri(E, B), ri(R, B)
    H, T, Rr = [h], [t], [r]
    for j in range(K):
        c = ri(E, B)
        H.append(c if j % 2 == 0 else h.clone())
        T.append(t.clone() if j % 2 == 0 else c)
        Rr.append(r.clone())
    h, t, r = torch.cat(H), torch.cat(T), torch.cat(Rr)
    rnd = torch.nonzero(torch.rand(B * K, generator=g) < 0.05).flatten() + B
    h[rnd], t[rnd], r[rnd] = ri(E, len(rnd)), ri(E, len(rnd)), ri(R, len(rnd))
    p = min(5, B - 1)
    row = p + (K // 2 + 1) * B
    h[row], t[row], r[row] = h[p], t[p], r[p]
    return h, t, r


def _spec(model, d, nf):
    from mmre.link import rotate_phase_denom
    from mmre.ns import NSSpec
    return NSSpec(model, d, norm_flag=nf, model_margin=6.0 if model == "rotate" else None,
                  phase_denom=rotate_phase_denom(6.0, 2.0, d) if model == "rotate" else 0.0)


def _reference(model, d, nf, tabs, h, t, r, B, kind, adv, regul, margin):
    """float64: loss, scores, gradients per table, and how far the reference stays from its kinks:
    (the smallest |x| - threshold of an L1 TransE element: clear when positive, the smallest
    |p - n + m| of a hinge argument, the fraction of hinge terms above their kink); inf / nan where
    there is no such kink."""
    import ref_trainer
    import test_ns_losses_gpu as losses
    if kind == "margin":
        T64 = {k: v.double().requires_grad_(True) for k, v in tabs.items()}
        if model in ("transe", "transe_l2"):
            loss, score = ref_trainer.transe_ns_loss(T64["ent"], T64["rel"], h, t, r, B, margin, norm_flag=nf,
                                                     p_norm=1 if model == "transe" else 2, adv_temperature=adv,
                                                     regul_rate=regul)
        else:
            loss, score = ref_trainer.model_ns_loss(model, T64, h, t, r, B, margin, adv, regul, model_margin=6.0)
        loss.backward()
        loss, score, grads = float(loss.detach()), score.detach().numpy(), {k: v.grad.numpy() for k, v in T64.items()}
    else:
        loss, score, grads, T64 = losses._reference(None, tabs, h, t, r, kind, adv, regul, B=B, model=(model, d, nf))
    x_min, hinge_min, active = np.inf, np.inf, np.nan
    if model == "transe":
        with torch.no_grad():
            nz = (lambda v: v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)) if nf else (lambda v: v)
            a, b, c = nz(T64["ent"][h]), nz(T64["rel"][r]), nz(T64["ent"][t])
            thr = (8 * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())).clamp_min(1e-7)
            x_min = float((((a + b) - c).abs() - thr).min())
    if kind == "margin":
        arg = score[:B][None, :] - score[B:].reshape(-1, B) + margin
        hinge_min, active = float(np.abs(arg).min()), float((arg > 0).mean())
    return loss, score, grads, (x_min, hinge_min, active)


@functools.lru_cache(maxsize=None)
def _case(variant, d, B, K, kind="margin", adv=None, regul=0.5):
    """Tables, batch and float64 reference of a case (made once, shared by the tests that use it):
    the first seed whose reference is clear of the kinks (module docstring)."""
    model, nf = VARIANTS[variant]
    margin = MARGIN[model]
    for seed in range(50, 90):
        tabs = _tables(model, d, seed)
        h, t, r = _batch(B, K, seed + 1000)
        ref = _reference(model, d, nf, tabs, h, t, r, B, kind, adv, regul, margin)
        x_min, hinge_min, active = ref[3]
        if x_min <= 0 or hinge_min < 1e-5 * max(1.0, np.abs(ref[1]).max()):
            continue
        if kind == "margin" and B * K >= 20 and not 0.0 < active < 1.0:
            continue  # hinge terms on both sides of the kink
        return dict(model=model, d=d, nf=nf, B=B, K=K, kind=kind, adv=adv, regul=regul, margin=margin, tabs=tabs,
                    h=h, t=t, r=r, ref=ref, seed=seed)
    raise AssertionError(f"no seed in 50..89 keeps the float64 reference of {variant} d {d} B {B} K {K} off its kinks")


def _run(c, lr=None, pass_optimizer=False):
    """Forward + backward on fresh device copies of the case's tables; with lr, an SGD over them
    steps afterwards (pass_optimizer: it is also given to fused_ns_loss as optimizer=)."""
    from mmre.ns import fused_ns_loss
    from mmre.optim import SGD
    T = {k: v.to(DEV).clone().requires_grad_(True) for k, v in c["tabs"].items()}
    opt = SGD(list(T.values()), lr=lr) if lr is not None else None
    loss, score = fused_ns_loss(_spec(c["model"], c["d"], c["nf"]), T["ent"], T["rel"], c["h"].to(DEV), c["t"].to(DEV),
                                c["r"].to(DEV), c["B"], c["K"], c["margin"], c["adv"], c["regul"],
                                ent_im=T.get("ent_im"), rel_im=T.get("rel_im"), loss=c["kind"],
                                optimizer=opt if pass_optimizer else None)
    out = dict(loss=loss.detach().cpu(), score=score.detach().cpu())
    loss.backward()
    out["grads"] = {k: v.grad.clone() for k, v in T.items()}
    if opt is not None:
        out["claimed"] = len(getattr(opt, "_fused_done", {}))  # tables whose step the backward says it applied
        opt.step()
        out["params"] = {k: v.detach().clone() for k, v in T.items()}
    torch.cuda.synchronize()
    return out


def _check(c, label=""):
    """What every case asserts; returns the first run."""
    ref_loss, rs, rg, (x_min, hinge_min, active) = c["ref"]
    assert x_min > 0 and hinge_min >= 1e-5 * max(1.0, np.abs(rs).max())  # before any GPU call: no exempt row
    a, b = _run(c), _run(c)
    serr = np.abs(a["score"].numpy() - rs).max()
    print(f"{label} seed {c['seed']}: loss {float(a['loss']):.9g} ref {ref_loss:.9g}; score err {serr:.3g} of "
          f"{np.abs(rs).max():.3g}; L1 clearance {x_min:.3g}, min hinge gap {hinge_min:.3g}, active {active:.2f}")
    touched = {"ent": np.zeros(E, bool), "rel": np.zeros(R, bool)}
    touched["ent"][c["h"].numpy()] = True
    touched["ent"][c["t"].numpy()] = True
    touched["rel"][c["r"].numpy()] = True
    for k in c["tabs"]:
        gw, gg = rg[k], a["grads"][k].cpu().double().numpy()
        err = np.abs(gg - gw).max()
        print(f"  grad {k}: err {err:.3g} of {np.abs(gw).max():.3g}")
    assert np.isfinite(float(a["loss"]))
    assert serr <= 1e-4 * max(1.0, np.abs(rs).max())
    assert abs(float(a["loss"]) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for k in c["tabs"]:
        gw, gg = rg[k], a["grads"][k].cpu().double().numpy()
        assert not np.isnan(gg).any(), k
        assert np.abs(gg - gw).max() <= 1e-4 * np.abs(gw).max(), (k, np.abs(gg - gw).max(), np.abs(gw).max())
        assert torch.equal(a["grads"][k], b["grads"][k]), k            # bit-reproducible
        assert not gg[~touched[k[:3]]].any(), k                         # rows outside the batch: exactly zero
    return a


# ---- (a) the width lattice -------------------------------------------------------------------
DIMS = (1, 7, 64, 65, 128, 129, 256, 257, 512)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_width_lattice_margin(variant, d):
    """Every NC class and both sides of each boundary, widths below a wave and odd; RotatE's entity
    rows are 2 d wide. TransE: k_ns_prepass + k_ns_transe_fused<NC, L2, true> + k_ns_row_owner<NC,
    L2>; the others k_ns_gen_forward / k_ns_gen_slots<NC, model> + k_ns_gen_owner<NC>."""
    _check(_case(variant, d, 13, 5), f"{variant} d {d}")


@pytest.mark.parametrize("d", (64, 128, 256, 512))
@pytest.mark.parametrize("variant", ["transe_n", "transe", "transe_l2_n"])
def test_width_classes_without_regularization(variant, d):
    """k_ns_transe_fused<NC, L2, REG = false>, once per NC class."""
    _check(_case(variant, d, 13, 5, regul=0.0), f"{variant} d {d} regul 0")


@pytest.mark.parametrize("d", (65, 128, 257))
@pytest.mark.parametrize("variant", GENERIC)
def test_width_lattice_softplus(variant, d):
    _check(_case(variant, d, 13, 5, kind="softplus", adv=0.5), f"{variant} d {d} softplus")


# ---- (b) K and B edges -------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,adv", [(5, 1, None), (5, 31, None), (5, 32, None), (5, 33, None), (5, 64, None),
                                     (5, 512, None), (1, 5, None), (3, 5, None), (4, 5, None), (5, 32, 1.0),
                                     (5, 33, 1.0)])
def test_transe_k_and_b_edges(B, K, adv):
    """K = 32 is the fused TransE kernel's last (NSW * NSF_MAXJ); 33 and beyond take the rows path
    (k_ns_transe_forward<2, false>, k_ns_row_coef, k_rows_slots<2>, k_ns_gen_owner<2>), 512 is the
    LDS limit; fewer positives than the 4 a workgroup holds."""
    from mmre.ns import fused_supported
    c = _case("transe_n", 65, B, K, adv=adv)
    assert fused_supported(_spec("transe", 65, True), K, 0) is (K <= 32)
    _check(c, f"transe_n d 65 B {B} K {K} adv {adv}")


@pytest.mark.parametrize("B,K", [(5, 1), (5, 21), (5, 22), (5, 43), (5, 512), (1, 22), (3, 22)])
@pytest.mark.parametrize("variant", ["distmult", "rotate"])
def test_generic_k_and_b_edges(variant, B, K):
    """The slot kernel's chunks of 21 negatives: one chunk, exactly one, one more, two and one more,
    and the 512 of the LDS limit."""
    _check(_case(variant, 129, B, K), f"{variant} d 129 B {B} K {K}")


# ---- (c) shapes beyond the fused kernels ---------------------------------------------------------
# the issue's: TransE margin (200, 33), (513, 5), (1024, 64); the generic models at 513 and 1024, K 64,
# margin and sigmoid with a temperature. Further: every k_ns_transe_forward<NC, L2> the rows path
# launches for TransE with K > 32 and the 2,048-wide (NC 32) rows instances.
BEYOND = ([("transe_n", 200, 33, "margin", None), ("transe_n", 513, 5, "margin", None),
           ("transe_n", 1024, 64, "margin", None)]
          + [(m, d, 64, kind, adv) for m in GENERIC for d in (513, 1024)
             for kind, adv in (("margin", None), ("sigmoid", 0.5))]
          + [("transe", 7, 33, "margin", None), ("transe_n", 512, 33, "margin", None),
             ("transe_l2_n", 65, 33, "margin", None), ("transe_l2_n", 200, 33, "margin", None),
             ("transe_l2_n", 512, 33, "margin", None), ("transe_n", 2048, 5, "margin", None),
             ("distmult", 2048, 5, "margin", None)])


@pytest.mark.parametrize("variant,d,K,kind,adv", BEYOND)
def test_shapes_beyond_the_fused_kernels(variant, d, K, kind, adv):
    """No fused kernel exists: the rows path serves them, with the optimizer's step its own --
    optimizer= claims no table, step() skips none, and the parameters are those of the run
    without optimizer=, bit for bit."""
    from mmre._lib import LOSS_KINDS
    from mmre.ns import fused_supported
    from mmre.optim import SGD
    c = _case(variant, d, 5, K, kind=kind, adv=adv)
    assert not fused_supported(_spec(c["model"], d, c["nf"]), K, LOSS_KINDS[kind])
    a = _check(c, f"{variant} d {d} K {K} {kind}")
    before = SGD.fallback_steps
    with_opt, without = _run(c, lr=0.7, pass_optimizer=True), _run(c, lr=0.7)
    assert SGD.fallback_steps == before
    assert with_opt["claimed"] == 0 and without["claimed"] == 0
    assert torch.equal(with_opt["loss"], a["loss"]) and torch.equal(with_opt["score"], a["score"])
    for k in c["tabs"]:
        assert torch.equal(with_opt["grads"][k], a["grads"][k]), k
        assert torch.equal(with_opt["params"][k], without["params"][k]), k
        assert not torch.equal(with_opt["params"][k].cpu(), c["tabs"][k]), k  # step() did not skip it


@pytest.mark.parametrize("variant", ["transe_n", "distmult"])
@pytest.mark.parametrize("d,K", [(2049, 5), (64, 513)])
def test_out_of_range_raises_in_the_forward(variant, d, K):
    """Past every path (dim > 2048, K > 512): MMREError from fused_ns_loss itself, never from
    backward(), and nothing written."""
    from mmre._lib import MMREError
    from mmre.ns import fused_ns_loss
    model, nf = VARIANTS[variant]
    B = 5
    tabs = _tables(model, d, 3)
    h, t, r = (x.to(DEV) for x in _batch(B, K, 4))
    T = {k: v.to(DEV).clone().requires_grad_(True) for k, v in tabs.items()}
    with pytest.raises(MMREError, match="unsupported shape"):
        fused_ns_loss(_spec(model, d, nf), T["ent"], T["rel"], h, t, r, B, K, 1.0, None, 0.5)
    with pytest.raises(MMREError, match="unsupported shape"), torch.no_grad():
        fused_ns_loss(_spec(model, d, nf), T["ent"], T["rel"], h, t, r, B, K, 1.0, None, 0.5)
    torch.cuda.synchronize()
    for k in tabs:
        assert torch.equal(T[k].detach().cpu(), tabs[k]) and T[k].grad is None, k


# ---- (d) the one-call step at small shapes -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_index():
    from mmre.data import OpenKEDataset, TrainIndex
    ds = OpenKEDataset(SMALL)
    return TrainIndex(ds.train[:, 0], ds.train[:, 1], ds.train[:, 2], ds.n_ent, ds.n_rel), ds.n_ent, ds.n_rel


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("variant,d,B,K", [("transe_n", 65, 13, 5), ("transe_n", 512, 5, 32), ("transe_n", 7, 3, 1),
                                           ("distmult", 129, 13, 22), ("complex", 129, 13, 22)])
def test_train_step_equals_the_autograd_path_at_small_shapes(variant, d, B, K, pipeline):
    """OpenKETrainStep against OpenKESampler.sample + fused_ns_loss(optimizer=) + backward +
    SGD.step over three steps: batches, loss, scores, gradients, parameters and seeds bit-identical
    (tests/test_ns_full_gpu.py holds this at B 2,721, K 25, d 200 alone)."""
    from mmre.ns import OpenKETrainStep, fused_ns_loss
    from mmre.optim import SGD
    from mmre.sampler import OpenKESampler
    idx, n_ent, n_rel = _small_index()
    model, nf = VARIANTS[variant]
    spec, margin, lr, regul = _spec(model, d, nf), MARGIN[model], 0.5, 0.25
    tabs = _tables(model, d, 7, n_ent, n_rel)
    ta = {n: v.to(DEV).clone().requires_grad_(True) for n, v in tabs.items()}
    tb = {n: v.to(DEV).clone().requires_grad_(True) for n, v in tabs.items()}
    sa, sb = OpenKESampler(idx, DEV, bern=True), OpenKESampler(idx, DEV, bern=True)
    opt = SGD(list(ta.values()), lr=lr)
    step = OpenKETrainStep(sb, spec, tb["ent"], tb["rel"], B, K, margin, lr, regul_rate=regul, pipeline=pipeline,
                           ent_im=tb.get("ent_im"), rel_im=tb.get("rel_im"))
    for i in range(3):
        ba = sa.sample(B, K)
        opt.zero_grad(set_to_none=True)
        la, sc_a = fused_ns_loss(spec, ta["ent"], ta["rel"], ba["batch_h"], ba["batch_t"], ba["batch_r"], B, K, margin,
                                 None, regul, optimizer=opt, ent_im=ta.get("ent_im"), rel_im=ta.get("rel_im"))
        la.backward()
        assert len(opt._fused_done) == len(ta)  # the in-pass step: these shapes have fused kernels
        opt.step()
        lb = step()
        torch.cuda.synchronize()
        for key in ("batch_h", "batch_t", "batch_r", "batch_y"):
            assert torch.equal(ba[key], step.batch[key]), (i, key)
        assert torch.isfinite(la) and torch.equal(la.detach().reshape(1), lb.reshape(1)), (i, float(la), float(lb))
        assert torch.equal(sc_a, step.score), i
        for n in tabs:
            assert torch.equal(ta[n].grad, tb[n].grad), (i, n)
            assert torch.equal(ta[n].detach(), tb[n].detach()), (i, n)
    for n in tabs:
        assert not torch.equal(ta[n].detach().cpu(), tabs[n]), n
    if pipeline:
        sa.sample(B, K)  # the prefetch drew batch 4
    assert torch.equal(sa._seeds_dev, sb._seeds_dev) and np.array_equal(sa.seeds, sb.seeds)


def test_train_step_refuses_an_unsupported_shape_when_built():
    from mmre.ns import OpenKETrainStep
    from mmre.sampler import OpenKESampler
    idx, n_ent, n_rel = _small_index()
    smp = OpenKESampler(idx, DEV, bern=True)
    for variant, d, K in (("transe_n", 65, 33), ("transe_n", 513, 5), ("rotate", 520, 64)):
        model, nf = VARIANTS[variant]
        T = {n: v.to(DEV).requires_grad_(True) for n, v in _tables(model, d, 7, n_ent, n_rel).items()}
        with pytest.raises(ValueError, match="no fused kernels"):
            OpenKETrainStep(smp, _spec(model, d, nf), T["ent"], T["rel"], 5, K, 1.0, 0.5)


# ---- (e) Trainer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ["transe", "rotate"])
def test_trainer_trains_past_the_fused_shapes(recipe):
    """neg_ent 64 (TransE: past the fused kernel's 32) and RotatE at dim 520 (past 512) in 'normal'
    mode: Trainer.run() stays on train_one_step, which trains through the rows path."""
    from mmre.optim import SGD
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import MarginLoss, SigmoidLoss
    from openke.module.model import RotatE, TransE
    from openke.module.strategy import NegativeSampling
    before = SGD.fallback_steps
    torch.manual_seed(0)
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=64, neg_rel=0)
    n_ent, n_rel = tdl.get_ent_tot(), tdl.get_rel_tot()
    if recipe == "transe":
        kg = TransE(ent_tot=n_ent, rel_tot=n_rel, dim=32, p_norm=1, norm_flag=True)
        model = NegativeSampling(model=kg, loss=MarginLoss(margin=5.0), batch_size=tdl.get_batch_size())
    else:
        kg = RotatE(ent_tot=n_ent, rel_tot=n_rel, dim=520, margin=6.0, epsilon=2.0)
        model = NegativeSampling(model=kg, loss=SigmoidLoss(adv_temperature=2), batch_size=tdl.get_batch_size(),
                                 regul_rate=0.0)
    trainer = Trainer(model=model, data_loader=tdl, train_times=5, alpha=0.5, use_gpu=True, opt_method="sgd")
    trainer.run()
    print(recipe, trainer.log)
    assert trainer.used_one_call_step is False
    assert isinstance(trainer.optimizer, SGD) and SGD.fallback_steps == before
    assert len(trainer.log) == 5 and np.isfinite(trainer.log).all()
    assert trainer.log[-1] < trainer.log[0]
