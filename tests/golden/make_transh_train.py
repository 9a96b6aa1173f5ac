"""make_transh_train.py -- TransH training fixtures from the REFERENCE itself.

Runs only in the build container (needs /root/reference), on the CPU; never on the GPU box.
Nothing from the reference travels: only the numbers written to tests/golden/transh_train.npz.

What is executed from the reference: its OpenKE TransH (openke/module/model/TransH.py), MarginLoss
(openke/module/loss/MarginLoss.py) and NegativeSampling (openke/module/strategy/
NegativeSampling.py), in float64 on the CPU: NegativeSampling(TransH, MarginLoss(m),
regul_rate=0.5).forward(batch).backward().

Cases: E 61, R 5, B 4, K 3 at d 40 and d 72, both p-norms and both norm_flag values (8 cases; the
loss margins of tests/transh_train_cases.py). The tables (float32 values, computed on in float64)
and the batch are drawn as tests/transh_train_cases.py draws them and shared by the four cases of a
width, which keeps the file small. Seeds are checked, not assumed: per width the generator walks
seeds from 50 and keeps the first at which the reference's own float64 numbers of all four cases
meet the kink rule of tests/transh_train_cases.py (every L1 element clear of 0 by
max(1e-7, (d + 8) 2^-24 (|p^_h| + |r^| + |p^_t|)), every hinge argument 1e-5 max(1, |s|) from 0).

Written per case `name`: name.{p_norm, norm_flag, d, B, K, loss_margin, regul, loss, score,
grad_ent, grad_rel, grad_norm}; per width: d<d>.{ent, rel, norm, h, t, r, seed}; names.

Usage:  python tests/golden/make_transh_train.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "OpenKE"))

import transh_train_cases as C  # noqa: E402  (tables, batch, the kink rule: nothing of the repo's model code)

N_ENT, N_REL, B, K, REGUL = 61, 5, 4, 3, 0.5
DIMS = (40, 72)


def reference_case(tabs, h, t, r, p_norm, nf):
    """The reference's numbers of one case, shaped as transh_train_cases.reference returns them."""
    from openke.module.loss import MarginLoss
    from openke.module.model import TransH
    from openke.module.strategy import NegativeSampling
    d = tabs["ent"].shape[1]
    m = TransH(N_ENT, N_REL, dim=d, p_norm=p_norm, norm_flag=nf).double()
    with torch.no_grad():
        m.ent_embeddings.weight.copy_(tabs["ent"].double())
        m.rel_embeddings.weight.copy_(tabs["rel"].double())
        m.norm_vector.weight.copy_(tabs["norm"].double())
    lossfn = MarginLoss(margin=C.MARGIN[(p_norm, nf)])
    st = NegativeSampling(model=m, loss=lossfn, batch_size=B, regul_rate=REGUL)
    data = {"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"}
    loss = st(data).reshape(())
    loss.backward()
    grads = {"ent": m.ent_embeddings.weight.grad.numpy().copy(), "rel": m.rel_embeddings.weight.grad.numpy().copy(),
             "norm": m.norm_vector.weight.grad.numpy().copy()}
    with torch.no_grad():
        s = m(data).numpy().copy()
        x_min = np.inf
        if p_norm == 1:
            nz = (lambda v: F.normalize(v, 2, -1)) if nf else (lambda v: v)
            w = m.norm_vector(r)
            a, b, c = nz(m._transfer(m.ent_embeddings(h), w)), nz(m.rel_embeddings(r)), nz(m._transfer(m.ent_embeddings(t), w))
            thr = ((d + 8) * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())).clamp_min(1e-7)
            x_min = float((((a + b) - c).abs() - thr).min())
        lm = float(lossfn.margin.item())
    arg = s[:B][None, :] - s[B:].reshape(-1, B) + lm
    return float(loss.detach()), s, grads, (x_min, float(np.abs(arg).min()), float((arg > 0).mean())), lm


def main():
    res, names = {}, []
    for d in DIMS:
        for seed in range(50, 90):
            tabs = C.tables(d, seed, N_ENT, N_REL)
            h, t, r = C.batch(B, K, seed + 1000, N_ENT, N_REL)
            refs = {(pn, nf): reference_case(tabs, h, t, r, pn, nf) for pn, nf in C.COMBOS}
            if all(C.clear(ref, B, K) for ref in refs.values()):
                break
        else:
            raise AssertionError(f"d {d}: no seed in 50..89 keeps all four cases off their kinks")
        print(f"d {d}: seed {seed}")
        for k, v in tabs.items():
            assert v.dtype == torch.float32
            res[f"d{d}.{k}"] = v.numpy()
        res[f"d{d}.h"], res[f"d{d}.t"], res[f"d{d}.r"] = h.numpy(), t.numpy(), r.numpy()
        res[f"d{d}.seed"] = np.int64(seed)
        for (pn, nf), (loss, s, grads, _, lm) in refs.items():
            name = f"l{pn}_{'norm' if nf else 'raw'}_d{d}"
            names.append(name)
            res.update({f"{name}.p_norm": np.int64(pn), f"{name}.norm_flag": np.int64(nf), f"{name}.d": np.int64(d),
                        f"{name}.B": np.int64(B), f"{name}.K": np.int64(K), f"{name}.loss_margin": np.float64(lm),
                        f"{name}.regul": np.float64(REGUL), f"{name}.loss": np.float64(loss), f"{name}.score": s})
            for k, g in grads.items():
                res[f"{name}.grad_{k}"] = g
    res["names"] = np.array(names)
    out = os.path.join(HERE, "transh_train.npz")
    np.savez_compressed(out, **res)
    size = os.path.getsize(out)
    assert size < 200 * 1024, size
    print(f"transh training fixture: {len(names)} cases, {size} bytes")


if __name__ == "__main__":
    main()
