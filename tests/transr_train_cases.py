"""Cases of the TransR training tests (tests/test_transr_train_cpu.py, test_transr_train_gpu.py):
tables, batches, the float64 yardstick and the seed search that keeps it off its kinks. The batch
layout, the three conditions (`clear`) and the (p_norm, norm_flag) combos are TransH's
(tests/transh_train_cases.py), imported.

The yardstick is float64 torch on the CPU through the repo's own model class: TransR.forward (the
reference's ops, TransR.py:37-85), MarginLoss and TransR.regularization (the squared one), with
autograd for the gradients.

Kinks: as for TransH, with the L1 element threshold
max(1e-7, (dim_e + dim_r + 8) 2^-24 (|p_h| + |r^| + |p_t|)): an operand has been through a
dim_e-term dot product and a dim_r-term norm.

Tables: ent uniform +-8/dim_e, rel uniform +-8/dim_r, transfer_matrix uniform +-sqrt(3/dim_e) --
general matrices (an identity hides transpositions), scaled so that a projection keeps its
entity's size; one separate case has the model's identity initialisation. Loss margins 0.25 (L1)
and 0.02 (L2) leave hinge terms on both sides at every case with B K >= 20 (the CPU test asserts
it).
"""
import functools

import numpy as np
import torch

from transh_train_cases import COMBOS, TH_SEG, batch, clear  # noqa: F401

E, R = 301, 6
MARGIN = {(1, True): 0.25, (1, False): 0.25, (2, True): 0.02, (2, False): 0.02}
KEYS = ("ent", "rel", "transfer_matrix")
# csrc/transh_train.hip, the TransR part
TR_TM = 32        # slots per MFMA row tile (k_trt_gemm)
TR_ISEG = 1024    # slots one k_trt_rank workgroup ranks
TR_DSEG = 1024    # slots one k_trt_dmat workgroup sums
TH_REGL_LIST = 16 * 64  # list entries k_trt_owner orders in registers (TH_REGL lanes' worth)
# (dim_e, dim_r): the MFMA's K and N steps (2, 32), the K block (32), the column chunk (128) and the
# row kernels' NC boundaries on either side, in either order
WIDTHS = ((7, 7), (9, 7), (7, 9), (33, 31), (64, 64), (65, 64), (64, 65), (200, 200), (256, 200), (200, 256),
          (512, 512), (512, 7), (7, 512))


def tables(de, dr, seed, n_ent=E, n_rel=R, identity=False):
    g = torch.Generator().manual_seed(seed)
    u = lambda n, d, a: (torch.rand((n, d), generator=g) * 2 - 1) * a
    tabs = {"ent": u(n_ent, de, 8.0 / de), "rel": u(n_rel, dr, 8.0 / dr),
            "transfer_matrix": u(n_rel, de * dr, (3.0 / de) ** 0.5)}
    if identity:  # TransR.__init__ without rand_init
        eye = torch.zeros(de, dr)
        for i in range(min(de, dr)):
            eye[i][i] = 1
        tabs["transfer_matrix"][:] = eye.view(de * dr)
    return tabs


def model64(tabs, de, dr, p_norm, nf, model_margin=None):
    """The repo's TransR in float64 on the CPU, holding `tabs`."""
    from openke.module.model import TransR
    m = TransR(tabs["ent"].shape[0], tabs["rel"].shape[0], dim_e=de, dim_r=dr, p_norm=p_norm, norm_flag=nf,
               margin=model_margin).double()
    with torch.no_grad():
        for k, w in weights(m).items():
            w.copy_(tabs[k].double())
    return m


def weights(m):
    return {"ent": m.ent_embeddings.weight, "rel": m.rel_embeddings.weight, "transfer_matrix": m.transfer_matrix.weight}


def l1_clearance(m, h, t, r, nf):
    """The smallest |x| - threshold over the L1 elements of the rows (clear when positive)."""
    nz = (lambda v: torch.nn.functional.normalize(v, 2, -1)) if nf else (lambda v: v)
    M = m.transfer_matrix(r)
    a = nz(m._transfer(m.ent_embeddings(h), M))
    b = nz(m.rel_embeddings(r))
    c = nz(m._transfer(m.ent_embeddings(t), M))
    thr = ((m.dim_e + m.dim_r + 8) * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())).clamp_min(1e-7)
    return float((((a + b) - c).abs() - thr).min())


def reference(tabs, de, dr, h, t, r, B, p_norm, nf, loss_margin, adv=None, regul=0.0, model_margin=None):
    """float64: (loss, scores, {table: gradient}, (x_min, hinge_min, active)), shaped as
    transh_train_cases.reference returns them."""
    from openke.module.loss import MarginLoss
    m = model64(tabs, de, dr, p_norm, nf, model_margin)
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


def live_slots(h, t, r, B):
    """Projection slots the kernels keep for a batch: two per positive, and a negative's head
    (tail) where it does not share (entity, relation) with its positive's."""
    h, t, r = (x.numpy() for x in (h, t, r))
    b = np.arange(len(h)) % B
    neg = np.arange(len(h)) >= B
    return int((~(neg & (r == r[b]) & (h == h[b]))).sum() + (~(neg & (r == r[b]) & (t == t[b]))).sum())


@functools.lru_cache(maxsize=None)
def case(p_norm, nf, de, dr, B, K, adv=None, regul=0.5, model_margin=None, loss_margin=None, n_ent=E, n_rel=R,
         one_head=False, both_sides=True, zero_rows=False, identity=False):
    """Tables, batch and float64 reference of a case, made once and shared (do not modify): the
    first seed in 50..89 whose reference is clear of the kinks. zero_rows: one batch entity's `ent`
    row is zero (m = 0), one relation's matrix is all zero (every projection by it is 0) and,
    under norm_flag, one `rel` row."""
    lm = MARGIN[(p_norm, nf)] if loss_margin is None else loss_margin
    for seed in range(50, 90):
        tabs = tables(de, dr, seed, n_ent, n_rel, identity)
        h, t, r = batch(B, K, seed + 1000, n_ent, n_rel, one_head)
        if zero_rows:
            tabs["ent"][int(h[0])] = 0.0
            tabs["transfer_matrix"][int(r[0])] = 0.0
            if nf:
                tabs["rel"][int(r[-1])] = 0.0
        ref = reference(tabs, de, dr, h, t, r, B, p_norm, nf, lm, adv, regul, model_margin)
        if clear(ref, B, K, both_sides):
            return dict(p_norm=p_norm, nf=nf, de=de, dr=dr, B=B, K=K, adv=adv, regul=regul, model_margin=model_margin,
                        margin=lm, tabs=tabs, h=h, t=t, r=r, ref=ref, seed=seed, n_ent=n_ent, n_rel=n_rel,
                        slots=live_slots(h, t, r, B))
    raise AssertionError(f"no seed in 50..89 keeps the float64 reference of p{p_norm} norm {nf} d ({de}, {dr}) B {B} "
                         f"K {K} off its kinks")


# ---- the GPU file's cases, by test (the CPU file runs the seed search of every one) ----------
CLASS_DIMS = ((200, 200), (9, 7))
BATCH_CLASSES = ((1, 1), (5, 25), (3, 64), (2, 65), (3, 2), (1, 512))
L1_WIDE = ((12, 7), (20, 9))                          # L1 at (200, 200) past a row tile per relation
MULTI_TILE = (40, 31)                                 # several row tiles per relation: L2 at (200, 200), L1 at (9, 7)
# one relation owns every slot, at (9, 7) L1. Live slots: about B (2 + K). The first three are past
# TR_ISEG = TR_DSEG = 1,024 slots (two and three segments); the last three around TR_TM = 32 (two and
# three row tiles); HUB_EDGE below straddles each constant closely.
HUB_SEG = ((512, 1), (205, 4), (683, 2), (16, 1), (11, 2), (13, 4))
HUB_SEG_WIDE = ((683, 2), (205, 4))                   # at (200, 200) L2
HUB_HEAD = ((70, 3), (1100, 1))                       # one head in 70 / 1,100 positives: lists past 64 / past TH_REGL_LIST
# one-relation batches with K = 1 on either side of TR_TM and of TR_DSEG = TR_ISEG: 32, 35, 1,023 and
# 1,026 live slots at the seeds the search takes (the GPU test asserts the counts)
HUB_EDGE = ((11, 1), (12, 1), (335, 1), (336, 1))
CLAMP_DIMS = (72, 65)
OPTION_COMBOS = ((1, True), (2, False))
IDENTITY = (1, True, 200, 200, 4, 3)


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
    for B, K in L1_WIDE:
        ks.append(((1, True, 200, 200, B, K), {}))
    ks.append(((2, True, 200, 200) + MULTI_TILE, {}))
    ks.append(((1, True, 9, 7) + MULTI_TILE, {}))
    for B, K in HUB_SEG + HUB_EDGE:
        ks.append(((1, True, 9, 7, B, K), dict(n_rel=1)))
    for B, K in HUB_SEG_WIDE:
        ks.append(((2, False, 200, 200, B, K), dict(n_rel=1)))
    for B, K in HUB_HEAD:
        ks.append(((1, True, 9, 7, B, K), dict(one_head=True)))
    ks.append(((2, True, 200, 200, 70, 3), dict(one_head=True)))
    ks.append((IDENTITY, dict(identity=True)))
    for pn, nf in OPTION_COMBOS:
        ks.append(((pn, nf, 200, 200, 5, 25), dict(model_margin=6.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(adv=1.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(regul=0.0)))
        ks.append(((pn, nf, 200, 200, 5, 25), dict(loss_margin=-1000.0, both_sides=False)))
    return ks
