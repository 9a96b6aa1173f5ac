"""Cases of the TransD training tests (tests/test_transd_train_cpu.py, test_transd_train_gpu.py):
tables, batches, the float64 yardstick and the seed search that keeps it off its kinks. The batch
layout, the three conditions (`clear`) and the (p_norm, norm_flag) combos are TransH's
(tests/transh_train_cases.py), imported.

The yardstick is float64 torch on the CPU through the repo's own model class: TransD.forward (the
reference's ops, TransD.py:62-129), MarginLoss and TransD.regularization, with autograd for the
gradients.

Kinks: as for TransH, with the L1 element threshold
max(1e-7, (dim_e + dim_r + 8) 2^-24 (|u^_h| + |r^| + |u^_t|)): an operand has been through a
dim_e-term dot product and a dim_r-term norm.

Loss margins. TransD's u^ is always a unit vector, so the score spreads do not depend on the
tables' scale as TransH's do: 0.25 (L1) and 0.02 (L2) leave hinge terms on both sides at every
width pair below (the CPU test asserts it for every case with B K >= 20).
"""
import functools

import numpy as np
import torch

from transh_train_cases import COMBOS, TH_SEG, batch, clear  # noqa: F401

E, R = 301, 6
MARGIN = {(1, True): 0.25, (1, False): 0.25, (2, True): 0.02, (2, False): 0.02}
KEYS = ("ent", "ent_transfer", "rel", "rel_transfer")
# (dim_e, dim_r): each NC boundary (64, 128, 256) on either side, and the cut e[:dim_r]
WIDTHS = ((7, 7), (9, 7), (64, 64), (65, 64), (65, 65), (128, 128), (129, 128), (200, 200), (256, 200), (257, 256),
          (512, 512), (512, 65), (512, 7))


def tables(de, dr, seed, n_ent=E, n_rel=R):
    """Uniform +-8/d, d each table's own width (the draw of transh_train_cases.tables)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda n, d: (torch.rand((n, d), generator=g) * 2 - 1) * (8.0 / d)
    return {"ent": u(n_ent, de), "ent_transfer": u(n_ent, de), "rel": u(n_rel, dr), "rel_transfer": u(n_rel, dr)}


def model64(tabs, p_norm, nf, model_margin=None):
    """The repo's TransD in float64 on the CPU, holding `tabs`."""
    from openke.module.model import TransD
    (n_ent, de), (n_rel, dr) = tabs["ent"].shape, tabs["rel"].shape
    m = TransD(n_ent, n_rel, dim_e=de, dim_r=dr, p_norm=p_norm, norm_flag=nf, margin=model_margin).double()
    with torch.no_grad():
        m.ent_embeddings.weight.copy_(tabs["ent"].double())
        m.ent_transfer.weight.copy_(tabs["ent_transfer"].double())
        m.rel_embeddings.weight.copy_(tabs["rel"].double())
        m.rel_transfer.weight.copy_(tabs["rel_transfer"].double())
    return m


def weights(m):
    return {"ent": m.ent_embeddings.weight, "ent_transfer": m.ent_transfer.weight, "rel": m.rel_embeddings.weight,
            "rel_transfer": m.rel_transfer.weight}


def l1_clearance(m, h, t, r, nf):
    """The smallest |x| - threshold over the L1 elements of the rows (clear when positive)."""
    nz = (lambda v: torch.nn.functional.normalize(v, 2, -1)) if nf else (lambda v: v)
    rp = m.rel_transfer(r)
    a = nz(m._transfer(m.ent_embeddings(h), m.ent_transfer(h), rp))
    b = nz(m.rel_embeddings(r))
    c = nz(m._transfer(m.ent_embeddings(t), m.ent_transfer(t), rp))
    thr = ((m.dim_e + m.dim_r + 8) * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())).clamp_min(1e-7)
    return float((((a + b) - c).abs() - thr).min())


def reference(tabs, h, t, r, B, p_norm, nf, loss_margin, adv=None, regul=0.0, model_margin=None):
    """float64: (loss, scores, {table: gradient}, (x_min, hinge_min, active)), shaped as
    transh_train_cases.reference returns them."""
    from openke.module.loss import MarginLoss
    m = model64(tabs, p_norm, nf, model_margin)
    data = {"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"}
    lossfn = MarginLoss(adv_temperature=adv, margin=loss_margin)
    score = m(data)
    p, n = score[:B].view(-1, B).permute(1, 0), score[B:].view(-1, B).permute(1, 0)
    loss = lossfn(p, n)   # (its margin is a float32 tensor: this sum is rounded to float32, as in the reference)
    if regul != 0:
        loss = loss + regul * m.regularization(data)
    loss = loss.reshape(())
    loss.backward()
    grads = {k: (w.grad if w.grad is not None else torch.zeros_like(w)).numpy().copy() for k, w in weights(m).items()}
    s = score.detach().numpy().copy()
    with torch.no_grad():
        x_min = l1_clearance(m, h, t, r, nf) if p_norm == 1 else np.inf
        lm = float(lossfn.margin.item())
    arg = s[:B][None, :] - s[B:].reshape(-1, B) + lm
    return float(loss.detach()), s, grads, (x_min, float(np.abs(arg).min()), float((arg > 0).mean()))


@functools.lru_cache(maxsize=None)
def case(p_norm, nf, de, dr, B, K, adv=None, regul=0.5, model_margin=None, loss_margin=None, n_ent=E, n_rel=R,
         one_head=False, both_sides=True, zero_rows=False):
    """Tables, batch and float64 reference of a case, made once and shared (do not modify): the
    first seed in 50..89 whose reference is clear of the kinks. zero_rows: one batch entity's `ent`
    row is zero (u = 0), another's `ent_transfer` row (s = 0), one relation's `rel_transfer` row
    (u = e[:dim_r]) and, under norm_flag, one `rel` row."""
    lm = MARGIN[(p_norm, nf)] if loss_margin is None else loss_margin
    for seed in range(50, 90):
        tabs = tables(de, dr, seed, n_ent, n_rel)
        h, t, r = batch(B, K, seed + 1000, n_ent, n_rel, one_head)
        if zero_rows:
            other = next(int(x) for x in torch.cat([t, h]) if int(x) != int(h[0]))
            tabs["ent"][int(h[0])] = 0.0
            tabs["ent_transfer"][other] = 0.0
            tabs["rel_transfer"][int(r[0])] = 0.0
            if nf:
                tabs["rel"][int(r[-1])] = 0.0
        ref = reference(tabs, h, t, r, B, p_norm, nf, lm, adv, regul, model_margin)
        if clear(ref, B, K, both_sides):
            return dict(p_norm=p_norm, nf=nf, de=de, dr=dr, B=B, K=K, adv=adv, regul=regul, model_margin=model_margin,
                        margin=lm, tabs=tabs, h=h, t=t, r=r, ref=ref, seed=seed, n_ent=n_ent, n_rel=n_rel)
    raise AssertionError(f"no seed in 50..89 keeps the float64 reference of p{p_norm} norm {nf} d ({de}, {dr}) B {B} "
                         f"K {K} off its kinks")


# ---- the GPU file's cases, by test (the CPU file runs the seed search of every one) ----------
CLASS_DIMS = ((200, 200), (9, 7))
BATCH_CLASSES = ((1, 1), (5, 25), (3, 64), (2, 65), (3, 2), (3, 4), (1, 512))
HUB_SEG = ((512, 1), (205, 4), (683, 2))              # B (1 + K) = TH_SEG, TH_SEG + 1, 2 TH_SEG + 1; R = 1
HUB_HEAD = ((70, 3), (1100, 1))                       # one head in 70 / 1,100 positives: lists past 64 / past 1,024
CLAMP_DIMS = (72, 65)
OPTION_COMBOS = ((1, True), (2, False))


def all_case_keys():
    """(args, kwargs) of every case the GPU file builds."""
    ks = []
    for pn, nf in COMBOS:
        for de, dr in WIDTHS:
            ks.append(((pn, nf, de, dr, 4, 3), {}))
        for de, dr in CLASS_DIMS:
            for B, K in BATCH_CLASSES:
                ks.append(((pn, nf, de, dr, B, K), {}))
        ks.append(((pn, nf) + CLAMP_DIMS + (4, 3), dict(zero_rows=True)))
    for B, K in HUB_SEG:
        ks.append(((1, True, 9, 7, B, K), dict(n_rel=1)))
    ks.append(((2, False, 200, 200, 683, 2), dict(n_rel=1)))
    for B, K in HUB_HEAD:
        ks.append(((1, True, 9, 7, B, K), dict(one_head=True)))
    ks.append(((2, True, 200, 200, 70, 3), dict(one_head=True)))
    for pn, nf in OPTION_COMBOS:
        ks.append(((pn, nf, 200, 200, 5, 25), dict(model_margin=6.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(adv=1.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(regul=0.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(loss_margin=-1000.0, both_sides=False)))
    return ks
