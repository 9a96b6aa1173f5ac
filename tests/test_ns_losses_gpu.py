"""SoftplusLoss / SigmoidLoss in the fused negative-sampling kernels (mmre.ns.fused_ns_loss(...,
loss=)): loss, scores and gradients against the reference's op sequence in float64 on small
synthetic tables (E 500, R 11, B 37 -- not a multiple of the 4 positives per workgroup -- and
K 1 or 70: more than one wave of negatives in every lane-strided loop and several 21-negative
chunks of the slot kernel). The float64 scores come from oracle/ref_trainer (its loss is not
used); the loss and the regularization are built here from SoftplusLoss.py:19-26 /
SigmoidLoss.py:19-26 with torch float64 ops. Tolerances are those of tests/test_ns_full_gpu.py:
scores 1e-4 max(1, |s|), loss 1e-5 relative, gradients 1e-4 of the table's largest entry (L1
TransE: on every table row no sign-ambiguous element touches, as there)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E, R, B = 500, 11, 37

#        name,        model,       d,   norm_flag
MODELS = {"distmult48": ("distmult", 48, False), "distmult200": ("distmult", 200, False),
          "complex200": ("complex", 200, False), "rotate512": ("rotate", 512, False),
          "transe200n": ("transe", 200, True), "transe_l2_48": ("transe_l2", 48, False)}
#          kind,      adv,  regul, K
CASES = [("softplus", None, 0.0, 70), ("sigmoid", 0.5, 1.0, 70), ("softplus", 0.5, 1.0, 1), ("sigmoid", None, 0.0, 1),
         ("softplus", 0.5, 0.0, 70)]


def _tables(name, seed=11, scale=1.0):
    model, d, _ = MODELS[name]
    g = torch.Generator().manual_seed(seed)
    u = lambda n, c, s: (torch.rand((n, c), generator=g) * 2 - 1) * s
    if model == "distmult":  # +-1.5: scores on both sides of the softplus threshold
        return {"ent": u(E, d, 1.5) * scale, "rel": u(R, d, 1.5) * scale}
    if model == "complex":
        return {"ent": u(E, d, 1.5), "ent_im": u(E, d, 1.5), "rel": u(R, d, 1.5), "rel_im": u(R, d, 1.5)}
    if model == "rotate":
        return {"ent": u(E, 2 * d, 8.0 / (2 * d)), "rel": u(R, d, 8.0 / d)}
    return {"ent": u(E, d, 8.0 / d), "rel": u(R, d, 8.0 / d)}


def _batch(K, seed=19, hub=False):  # seed 19: the distmult200 K 70 reference has positives beyond +-20
    """[pos | neg_1 | ... | neg_K]: negative j corrupts the head (j even) or the tail (j odd) of its
    positive; about 5 % of the negative rows are fully random (h, r, t); one is a copy of its positive."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda hi, n: torch.randint(0, hi, (n,), generator=g)
    h, t, r = ri(E, B), ri(E, B), ri(R, B)
    if hub:
        r[:] = 3
    H, T, Rr = [h], [t], [r]
    for j in range(K):
        c = ri(E, B)
        H.append(c if j % 2 == 0 else h.clone())
        T.append(t.clone() if j % 2 == 0 else c)
        Rr.append(r.clone())
    h, t, r = torch.cat(H), torch.cat(T), torch.cat(Rr)
    rnd = torch.nonzero(torch.rand(B * K, generator=g) < 0.05).flatten() + B
    if not hub:
        h[rnd], t[rnd], r[rnd] = ri(E, len(rnd)), ri(E, len(rnd)), ri(R, len(rnd))
    row = 5 + (K // 2 + 1) * B  # negative K // 2 of positive 5: a copy of it
    h[row], t[row], r[row] = h[5], t[5], r[5]
    return h, t, r


def _spec(name):
    from mmre.link import rotate_phase_denom
    from mmre.ns import NSSpec
    model, d, nf = MODELS[name]
    return NSSpec(model, d, norm_flag=nf, model_margin=6.0 if model == "rotate" else None,
                  phase_denom=rotate_phase_denom(6.0, 2.0, d) if model == "rotate" else 0.0)


def _reference(name, tabs, h, t, r, kind, adv, regul, B=B, model=None):
    """float64: (loss, scores, gradients per table, the float64 tables). B, model = (model, d,
    norm_flag): another batch size and model than this file's (tests/test_ns_shapes_gpu.py)."""
    import ref_trainer
    model, d, nf = model or MODELS[name]
    T64 = {k: v.double().requires_grad_(True) for k, v in tabs.items()}
    if model in ("transe", "transe_l2"):
        _, score = ref_trainer.transe_ns_loss(T64["ent"], T64["rel"], h, t, r, B, 0.0, norm_flag=nf,
                                              p_norm=1 if model == "transe" else 2, regul_rate=0)
    else:
        _, score = ref_trainer.model_ns_loss(model, T64, h, t, r, B, 0.0, None, 0, model_margin=6.0)
    p = score[:B].view(-1, B).permute(1, 0)
    n = score[B:].view(-1, B).permute(1, 0)
    w = torch.softmax(n * adv, dim=-1).detach() if adv is not None else None
    if kind == "softplus":  # SoftplusLoss.py:19-26
        c = torch.nn.Softplus()
        loss = (c(-p).mean() + ((w * c(n)).sum(dim=-1).mean() if adv is not None else c(n).mean())) / 2
    else:  # SigmoidLoss.py:19-26
        c = torch.nn.LogSigmoid()
        loss = -(c(p).mean() + ((w * c(-n)).sum(dim=-1).mean() if adv is not None else c(-n).mean())) / 2
    if regul != 0:  # Model.regularization: the mean of the gathered rows' mean squares
        if model == "complex":
            regs = [T64["ent"][h], T64["ent_im"][h], T64["ent"][t], T64["ent_im"][t], T64["rel"][r], T64["rel_im"][r]]
        else:
            regs = [T64["ent"][h], T64["ent"][t], T64["rel"][r]]
        loss = loss + regul * sum(torch.mean(x ** 2) for x in regs) / len(regs)
    loss.backward()
    return float(loss.detach()), score.detach().numpy(), {k: v.grad.numpy() for k, v in T64.items()}, T64


def _run(name, tabs, h, t, r, K, kind, adv, regul, upstream=1.0, **kw):
    from mmre.ns import fused_ns_loss
    T = {k: v.to(DEV).requires_grad_(True) for k, v in tabs.items()}
    loss, score = fused_ns_loss(_spec(name), T["ent"], T["rel"], h.to(DEV), t.to(DEV), r.to(DEV), B, K, 0.0, adv, regul,
                                ent_im=T.get("ent_im"), rel_im=T.get("rel_im"), **kw)
    (loss * upstream if upstream != 1.0 else loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), score.detach().cpu(), {k: v.grad.clone() for k, v in T.items()}


def _check(name, tabs, h, t, r, got, ref):
    loss, score, grads = got
    ref_loss, rs, rg, T64 = ref
    print(f"{name}: loss {float(loss):.9g} ref {ref_loss:.9g}; score err {np.abs(score.numpy() - rs).max():.3g} of "
          f"{np.abs(rs).max():.3g}")
    assert torch.isfinite(loss).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert np.abs(score.numpy() - rs).max() <= 1e-4 * max(1.0, np.abs(rs).max())
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    skip = {k: np.zeros(v.shape[0], bool) for k, v in tabs.items()}
    model, d, nf = MODELS[name]
    if model == "transe":  # L1: rows fed by a sign-ambiguous element (|x| < 1e-7), as tests/test_ns_full_gpu.py
        with torch.no_grad():
            nz = (lambda v: v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)) if nf else (lambda v: v)
            x = (nz(T64["ent"][h]) + nz(T64["rel"][r])) - nz(T64["ent"][t])
            amb = (x.abs() < 1e-7).any(1).numpy()
        skip["ent"][h.numpy()[amb]] = True
        skip["ent"][t.numpy()[amb]] = True
        skip["rel"][r.numpy()[amb]] = True
        assert skip["ent"].sum() <= 20
    for k in tabs:
        gw, gg = rg[k], grads[k].cpu().double().numpy()
        err = np.abs(gg - gw)[~skip[k]].max()
        print(f"  grad {k}: err {err:.3g} of {np.abs(gw).max():.3g}")
        assert err <= 1e-4 * np.abs(gw).max(), (k, err, np.abs(gw).max())


@pytest.mark.parametrize("kind,adv,regul,K", CASES)
@pytest.mark.parametrize("name", list(MODELS))
def test_loss_scores_gradients_match_float64(name, kind, adv, regul, K):
    tabs = _tables(name)
    h, t, r = _batch(K)
    ref = _reference(name, tabs, h, t, r, kind, adv, regul)
    if name == "distmult200" and K == 70:  # both softplus branches, the flat middle and a saturated positive
        rs = ref[1]
        assert (rs[B:] > 20).any() and (rs[B:] < -20).any() and (np.abs(rs[B:]) < 1).any() and (np.abs(rs[:B]) > 20).any()
    a = _run(name, tabs, h, t, r, K, kind, adv, regul, loss=kind)
    b = _run(name, tabs, h, t, r, K, kind, adv, regul, loss=kind)
    c = _run(name, tabs, h, t, r, K, kind, adv, regul, upstream=2.5, loss=kind)
    _check(name, tabs, h, t, r, a, ref)
    for k in tabs:
        assert torch.equal(a[2][k], b[2][k]), k        # bit-reproducible
        assert torch.equal(a[2][k] * 2.5, c[2][k]), k  # the upstream gradient scales exactly


@pytest.mark.parametrize("kind", ["softplus", "sigmoid"])
def test_no_overflow_at_scores_in_the_thousands(kind):
    name, K = "distmult200", 70
    tabs = _tables(name, scale=4.0)
    h, t, r = _batch(K)
    ref = _reference(name, tabs, h, t, r, kind, 0.5, 0.0)
    assert np.abs(ref[1]).max() > 1000
    _check(name, tabs, h, t, r, _run(name, tabs, h, t, r, K, kind, 0.5, 0.0, loss=kind), ref)
    ref = _reference(name, tabs, h, t, r, kind, None, 0.0)
    _check(name, tabs, h, t, r, _run(name, tabs, h, t, r, K, kind, None, 0.0, loss=kind), ref)


@pytest.mark.parametrize("name", ["distmult48", "complex200"])
def test_hub_relation_row(name):
    """All 37 positives share one relation, K 70: 37 * 71 slots in one bucket -- past the 64-slot
    bucket and the 512-slot LDS ordering, into the hub workgroups' repeated-minimum order."""
    K = 70
    tabs = _tables(name)
    h, t, r = _batch(K, hub=True)
    assert len(set(r.tolist())) == 1
    ref = _reference(name, tabs, h, t, r, "softplus", None, 1.0)
    a = _run(name, tabs, h, t, r, K, "softplus", None, 1.0, loss="softplus")
    b = _run(name, tabs, h, t, r, K, "softplus", None, 1.0, loss="softplus")
    _check(name, tabs, h, t, r, a, ref)
    for k in tabs:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("name", ["distmult200", "transe200n"])
def test_margin_is_unchanged(name):
    """loss="margin" is the call without the argument, bit for bit."""
    from mmre.ns import fused_ns_loss
    K = 25
    tabs = _tables(name)
    h, t, r = (x.to(DEV) for x in _batch(K))
    out = []
    for kw in ({}, {"loss": "margin"}):
        T = {k: v.to(DEV).requires_grad_(True) for k, v in tabs.items()}
        loss, score = fused_ns_loss(_spec(name), T["ent"], T["rel"], h, t, r, B, K, 3.0, 0.5, 0.25, **kw)
        loss.backward()
        out.append((loss.detach().clone(), score.clone(), {k: v.grad.clone() for k, v in T.items()}))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    for k in tabs:
        assert torch.equal(out[0][2][k], out[1][2][k]), k
