"""Cases of the TransH training tests (tests/test_transh_train_cpu.py, test_transh_train_gpu.py):
tables, batches, the float64 yardstick and the seed search that keeps it off its kinks.

The yardstick is float64 torch on the CPU through the repo's own model class: TransH._transfer and
TransH._calc (the reference's ops, TransH.py:52-93), MarginLoss and TransH.regularization, with
autograd for the gradients.

Kinks. A float32 run and a float64 reference may fall on different sides of sign(x) at x = 0 (L1)
and of the hinge max(p - n, -m). Each case takes the first seed in 50..89 whose float64 reference
ALONE meets three conditions (`clear`), asserted on the CPU before any GPU call:
  - every L1 element has |x| > max(1e-7, (d + 8) 2^-24 (|p^_h| + |r^| + |p^_t|)): each operand has
    been through a d-term dot product;
  - every hinge argument is at least 1e-5 max(1, |s|) from 0;
  - when B K >= 20, hinge terms lie on both sides (both_sides=False only for the case built to
    have no active hinge term at all: the regulariser's gradient on its own).
"""
import functools

import numpy as np
import torch

E, R = 301, 6
# loss margins that leave hinge terms on both sides at these tables' score spreads: (p_norm, norm_flag)
MARGIN = {(1, True): 1.0, (1, False): 0.25, (2, True): 0.05, (2, False): 0.02}
WIDTHS = (7, 64, 65, 128, 129, 200, 256, 257, 512)
COMBOS = ((1, True), (1, False), (2, True), (2, False))


def tables(d, seed, n_ent=E, n_rel=R):
    g = torch.Generator().manual_seed(seed)
    u = lambda n: (torch.rand((n, d), generator=g) * 2 - 1) * (8.0 / d)
    return {"ent": u(n_ent), "rel": u(n_rel), "norm": u(n_rel)}


def batch(B, K, seed, n_ent=E, n_rel=R, one_head=False):
    """[pos | neg_1 | ... | neg_K]: negative j corrupts the head (j even) or the tail (j odd); about
    5 % of the negative rows are fully random (their relation differs from their positive's when
    n_rel > 1); negative K // 2 of one positive is a copy of it. one_head: every positive has
    entity 3 as its head."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda hi, n: torch.randint(0, hi, (n,), generator=g)
    h, t, r = ri(n_ent, B), ri(n_ent, B), ri(n_rel, B)
    if one_head:
        h[:] = 3
    H, T, Rr = [h], [t], [r]
    for j in range(K):
        c = ri(n_ent, B)
        H.append(c if j % 2 == 0 else h.clone())
        T.append(t.clone() if j % 2 == 0 else c)
        Rr.append(r.clone())
    h, t, r = torch.cat(H), torch.cat(T), torch.cat(Rr)
    rnd = torch.nonzero(torch.rand(B * K, generator=g) < 0.05).flatten() + B
    h[rnd], t[rnd], r[rnd] = ri(n_ent, len(rnd)), ri(n_ent, len(rnd)), ri(n_rel, len(rnd))
    p = min(5, B - 1)
    row = p + (K // 2 + 1) * B
    h[row], t[row], r[row] = h[p], t[p], r[p]
    return h, t, r


def model64(tabs, p_norm, nf, model_margin=None):
    """The repo's TransH in float64 on the CPU, holding `tabs`."""
    from openke.module.model import TransH
    n_ent, d = tabs["ent"].shape
    m = TransH(n_ent, tabs["rel"].shape[0], dim=d, p_norm=p_norm, norm_flag=nf, margin=model_margin).double()
    with torch.no_grad():
        m.ent_embeddings.weight.copy_(tabs["ent"].double())
        m.rel_embeddings.weight.copy_(tabs["rel"].double())
        m.norm_vector.weight.copy_(tabs["norm"].double())
    return m


def reference(tabs, h, t, r, B, p_norm, nf, loss_margin, adv=None, regul=0.0, model_margin=None):
    """float64: (loss, scores, {ent, rel, norm: gradient}, (x_min, hinge_min, active)) -- the last
    three: the smallest |x| - threshold of an L1 element (clear when positive; inf for L2), the
    smallest |p - n + m| of a hinge argument, the fraction of hinge terms above their kink."""
    from openke.module.loss import MarginLoss
    m = model64(tabs, p_norm, nf, model_margin)
    data = {"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"}
    lossfn = MarginLoss(adv_temperature=adv, margin=loss_margin)
    score = m(data)
    p, n = score[:B].view(-1, B).permute(1, 0), score[B:].view(-1, B).permute(1, 0)
    # as NegativeSampling.forward adds them. (MarginLoss keeps its margin as a float32 tensor of one
    # element, so this last sum is rounded to float32 -- 6e-8 relative -- here as in the reference;
    # scores and gradients are float64 throughout.)
    loss = lossfn(p, n)
    if regul != 0:
        loss = loss + regul * m.regularization(data)
    loss = loss.reshape(())
    loss.backward()
    z = lambda w: (w.grad if w.grad is not None else torch.zeros_like(w)).numpy().copy()
    grads = {"ent": z(m.ent_embeddings.weight), "rel": z(m.rel_embeddings.weight), "norm": z(m.norm_vector.weight)}
    s = score.detach().numpy().copy()
    x_min = np.inf
    with torch.no_grad():
        if p_norm == 1:
            nz = (lambda v: torch.nn.functional.normalize(v, 2, -1)) if nf else (lambda v: v)
            w = m.norm_vector(r)
            a, b, c = nz(m._transfer(m.ent_embeddings(h), w)), nz(m.rel_embeddings(r)), nz(m._transfer(m.ent_embeddings(t), w))
            d = tabs["ent"].shape[1]
            thr = ((d + 8) * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())).clamp_min(1e-7)
            x_min = float((((a + b) - c).abs() - thr).min())
        lm = float(lossfn.margin.item())
    arg = s[:B][None, :] - s[B:].reshape(-1, B) + lm
    return float(loss.detach()), s, grads, (x_min, float(np.abs(arg).min()), float((arg > 0).mean()))


def clear(ref, B, K, both_sides=True):
    """The three conditions of the module docstring on a reference."""
    x_min, hinge_min, active = ref[3]
    if x_min <= 0 or hinge_min < 1e-5 * max(1.0, np.abs(ref[1]).max()):
        return False
    return not (both_sides and B * K >= 20 and not 0.0 < active < 1.0)


@functools.lru_cache(maxsize=None)
def case(p_norm, nf, d, B, K, adv=None, regul=0.5, model_margin=None, loss_margin=None, n_ent=E, n_rel=R,
         one_head=False, both_sides=True, zero_rows=False):
    """Tables, batch and float64 reference of a case, made once and shared (do not modify): the
    first seed in 50..89 whose reference is clear of the kinks. zero_rows: one entity row of the
    batch, one normal row and (norm_flag) one relation row are all zero (the 1e-12 clamps)."""
    lm = MARGIN[(p_norm, nf)] if loss_margin is None else loss_margin
    for seed in range(50, 90):
        tabs = tables(d, seed, n_ent, n_rel)
        h, t, r = batch(B, K, seed + 1000, n_ent, n_rel, one_head)
        if zero_rows:
            tabs["ent"][int(h[0])] = 0.0
            tabs["norm"][int(r[0])] = 0.0
            if nf:
                tabs["rel"][int(r[-1])] = 0.0
        ref = reference(tabs, h, t, r, B, p_norm, nf, lm, adv, regul, model_margin)
        if clear(ref, B, K, both_sides):
            return dict(p_norm=p_norm, nf=nf, d=d, B=B, K=K, adv=adv, regul=regul, model_margin=model_margin,
                        margin=lm, tabs=tabs, h=h, t=t, r=r, ref=ref, seed=seed, n_ent=n_ent, n_rel=n_rel)
    raise AssertionError(f"no seed in 50..89 keeps the float64 reference of p{p_norm} norm {nf} d {d} B {B} K {K} "
                         f"off its kinks")


# ---- the GPU file's cases, by test (the CPU file runs the seed search of every one) ----------
TH_SEG = 1024  # csrc/transh_train.hip: batch rows per relation-owner wave
CLASS_DIMS = (200, 7)
BATCH_CLASSES = ((1, 1), (5, 25), (3, 64), (2, 65),   # the issue's
                 (3, 2), (3, 4),                      # K + 1 = 3 / 5 rows over a positive's four waves (widths: 4)
                 (1, 512))                            # the largest K
HUB_SEG = ((512, 1), (205, 4), (683, 2))              # B (1 + K) = TH_SEG, TH_SEG + 1, 2 TH_SEG + 1; R = 1
HUB_HEAD = ((70, 3), (1100, 1))                       # one head in 70 / 1,100 positives: lists past 64 / past 1,024


def all_case_keys():
    """(args, kwargs) of every case the GPU file builds."""
    ks = []
    for pn, nf in COMBOS:
        for d in WIDTHS:
            ks.append(((pn, nf, d, 4, 3), {}))
        for d in CLASS_DIMS:
            for B, K in BATCH_CLASSES:
                ks.append(((pn, nf, d, B, K), {}))
        ks.append(((pn, nf, 65, 4, 3), dict(zero_rows=True)))
    for B, K in HUB_SEG:
        ks.append(((1, True, 7, B, K), dict(n_rel=1)))
    ks.append(((2, False, 200, 683, 2), dict(n_rel=1)))
    for B, K in HUB_HEAD:
        ks.append(((1, True, 7, B, K), dict(one_head=True)))
    ks.append(((2, True, 200, 70, 3), dict(one_head=True)))
    for pn, nf in ((1, True), (2, False)):
        ks.append(((pn, nf, 200, 5, 25), dict(model_margin=6.0)))
        ks.append(((pn, nf, 200, 5, 25), dict(adv=1.0)))
        ks.append(((pn, nf, 200, 5, 25), dict(regul=0.0)))
        ks.append(((pn, nf, 200, 5, 25), dict(loss_margin=-1000.0, both_sides=False)))
    return ks
