"""Times the paths that run the row-wise score chain (csrc/row_chain.h) outside relation prediction,
at the FB15K237 id space (E = 14,541, R = 237), between two device events:

  tc_complex_d*               mmre_tc_scores (k_tc_score), ComplEx, 200,000 pairs of rows
  ns_transe*_rows_d*          fused_ns_loss without gradients (k_ns_transe_forward), B 16,384, K 25
  ns_*_generic_d1024          the same at dim 1,024 (k_ns_forward: row_score), B 2,721, K 25
  ns_complex_fused_forward_d* mmre_ns_fused_forward alone (k_ns_gen_forward), B 16,384, K 25

d = 64, 128, 200, 512 are the four instances (NC 1, 2, 4, 8). Each of the 5 repetitions times 20
warmed-up calls. Prints one JSON line: case -> ms per call of every repetition. The library is the
one MMRE_LIB names, else the tree's, so two builds can alternate in one session
(profiles/row_chain). No CPU path."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "multimodal-relation-extrapolation_amd"))
import numpy as np
import torch

from mmre import _lib
from mmre.link import ScoreSpec
from mmre.ns import NSSpec, fused_ns_loss
from mmre.tripleclass import classification_scores

DEV = torch.device("cuda:0")
E, R = 14541, 237
REPS, ITERS, WARM = 5, 20, 3
rng = np.random.default_rng(0)
u = lambda *s: torch.from_numpy(rng.uniform(-0.5, 0.5, s).astype(np.float32)).to(DEV)
ids = lambda n, hi: torch.from_numpy(rng.integers(0, hi, n)).to(DEV)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS)
    return out


def batch(B, K):
    """OpenKE-shaped rows: each negative replaces its positive's head or tail."""
    h, t, r = ids(B, E), ids(B, E), ids(B, R)
    H, T = h.repeat(1 + K).clone(), t.repeat(1 + K).clone()
    neg = ids(B * K, E)
    coin = torch.from_numpy(rng.integers(0, 2, B * K).astype(bool)).to(DEV)
    H[B:] = torch.where(coin, neg, H[B:])
    T[B:] = torch.where(coin, T[B:], neg)
    return H, T, r.repeat(1 + K)


res = {"lib": _lib.lib_identity()}
# k_tc_score, ComplEx, every NC
N = 200000
ph, pr, pt, nh, nt = ids(N, E), ids(N, R), ids(N, E), ids(N, E), ids(N, E)
nt = torch.where(torch.arange(N, device=DEV) % 2 == 0, pt, nt)
nh = torch.where(torch.arange(N, device=DEV) % 2 == 1, ph, nh)
for d in (64, 128, 200, 512):
    sp = ScoreSpec(model="complex", ent=u(E, d), rel=u(R, d), dim=d, ent_im=u(E, d), rel_im=u(R, d), pred_kind=2)
    res["tc_complex_d%d" % d] = timed(lambda: classification_scores(sp, ph, pr, pt, nh, nt))
# k_ns_transe_forward (no gradient wanted), L1 with norm_flag at every NC and L2 at d 200
B, K = 16384, 25
H, T, Rr = batch(B, K)
for model, d in (("transe", 64), ("transe", 128), ("transe", 200), ("transe", 512), ("transe_l2", 200)):
    ns = NSSpec(model, d, norm_flag=True)
    ent, rel = u(E, d), u(R, d)
    with torch.no_grad():
        res["ns_%s_rows_d%d" % (model, d)] = timed(lambda: fused_ns_loss(ns, ent, rel, H, T, Rr, B, K, 5.0))
# k_ns_forward (the generic path: dim > 512), TransE and ComplEx
B2, K2 = 2721, 25
H2, T2, R2 = batch(B2, K2)
for model, d in (("transe", 1024), ("complex", 1024)):
    ns = NSSpec(model, d, norm_flag=model == "transe")
    ent, rel = u(E, d), u(R, d)
    im = dict(ent_im=u(E, d), rel_im=u(R, d)) if model == "complex" else {}
    with torch.no_grad():
        res["ns_%s_generic_d%d" % (model, d)] = timed(
            lambda: fused_ns_loss(ns, ent, rel, H2, T2, R2, B2, K2, 5.0, **im))
# k_ns_gen_forward, ComplEx, every NC: the fused forward alone, between the events around its call
for d in (64, 128, 200, 512):
    ns = NSSpec("complex", d)
    tabs = [u(E, d).requires_grad_(True), u(R, d).requires_grad_(True), u(E, d).requires_grad_(True),
            u(R, d).requires_grad_(True)]
    ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
    one = lambda: fused_ns_loss(ns, tabs[0], tabs[1], H, T, Rr, B, K, 5.0, ent_im=tabs[2], rel_im=tabs[3], events=ev)
    for _ in range(WARM):
        one()
    out = []
    for _ in range(REPS):
        acc = 0.0
        for _ in range(ITERS):
            one()
            ev[1].synchronize()
            acc += ev[0].elapsed_time(ev[1])
        out.append(acc / ITERS)
    res["ns_complex_fused_forward_d%d" % d] = out
print(json.dumps(res))
