"""make_transr_train.py -- TransR training fixtures from the REFERENCE itself.

Runs only in the build container (needs /root/reference), on the CPU; never on the GPU box.
Nothing from the reference travels: only the numbers written to tests/golden/transr_train.npz.

What is executed from the reference: its OpenKE TransR (openke/module/model/TransR.py), MarginLoss
(openke/module/loss/MarginLoss.py) and NegativeSampling (openke/module/strategy/
NegativeSampling.py), in float64 on the CPU: NegativeSampling(TransR, MarginLoss(m),
regul_rate=0.5).forward(batch).backward().

Cases: E 61, R 5, B 4, K 3 at (dim_e, dim_r) = (40, 24) and (24, 40), both p-norms and both
norm_flag values (8 cases; the loss margins of tests/transr_train_cases.py). The tables (float32
values, computed on in float64) and the batch are drawn as tests/transr_train_cases.py draws them
and shared by the four cases of a width pair. Seeds are checked, not assumed: per width pair the
generator walks seeds from 50 and keeps the first at which the reference's own float64 numbers of
all four cases meet the kink rule of tests/transr_train_cases.py.

Written per case `name`: name.{p_norm, norm_flag, dim_e, dim_r, B, K, loss_margin, regul, loss,
score, grad_ent, grad_rel, grad_transfer_matrix}; per width pair:
d<dim_e>_<dim_r>.{ent, rel, transfer_matrix, h, t, r, seed}; names.

Usage:  python tests/golden/make_transr_train.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "OpenKE"))

import transr_train_cases as C  # noqa: E402  (tables, batch, the kink rule: nothing of the repo's model code runs)

N_ENT, N_REL, B, K, REGUL = 61, 5, 4, 3, 0.5
DIMS = ((40, 24), (24, 40))


def reference_case(tabs, h, t, r, p_norm, nf):
    """The reference's numbers of one case, shaped as transr_train_cases.reference returns them."""
    from openke.module.loss import MarginLoss
    from openke.module.model import TransR
    from openke.module.strategy import NegativeSampling
    de, dr = tabs["ent"].shape[1], tabs["rel"].shape[1]
    m = TransR(N_ENT, N_REL, dim_e=de, dim_r=dr, p_norm=p_norm, norm_flag=nf).double()
    assert sys.modules[TransR.__module__].__file__.startswith(REF)   # the reference's class, not the repo's
    with torch.no_grad():
        for k, w in C.weights(m).items():
            w.copy_(tabs[k].double())
    lossfn = MarginLoss(margin=C.MARGIN[(p_norm, nf)])
    st = NegativeSampling(model=m, loss=lossfn, batch_size=B, regul_rate=REGUL)
    data = {"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"}
    loss = st(data).reshape(())
    loss.backward()
    grads = {k: w.grad.numpy().copy() for k, w in C.weights(m).items()}
    with torch.no_grad():
        s = m(data).numpy().copy()
        x_min = C.l1_clearance(m, h, t, r, nf) if p_norm == 1 else np.inf
        lm = float(lossfn.margin.item())
    arg = s[:B][None, :] - s[B:].reshape(-1, B) + lm
    return float(loss.detach()), s, grads, (x_min, float(np.abs(arg).min()), float((arg > 0).mean())), lm


def main():
    res, names = {}, []
    for de, dr in DIMS:
        for seed in range(50, 90):
            tabs = C.tables(de, dr, seed, N_ENT, N_REL)
            h, t, r = C.batch(B, K, seed + 1000, N_ENT, N_REL)
            refs = {(pn, nf): reference_case(tabs, h, t, r, pn, nf) for pn, nf in C.COMBOS}
            if all(C.clear(ref, B, K) for ref in refs.values()):
                break
        else:
            raise AssertionError(f"d ({de}, {dr}): no seed in 50..89 keeps all four cases off their kinks")
        print(f"d ({de}, {dr}): seed {seed}")
        pre = f"d{de}_{dr}"
        for k, v in tabs.items():
            assert v.dtype == torch.float32
            res[f"{pre}.{k}"] = v.numpy()
        res[f"{pre}.h"], res[f"{pre}.t"], res[f"{pre}.r"] = h.numpy(), t.numpy(), r.numpy()
        res[f"{pre}.seed"] = np.int64(seed)
        for (pn, nf), (loss, s, grads, _, lm) in refs.items():
            name = f"l{pn}_{'norm' if nf else 'raw'}_d{de}_{dr}"
            names.append(name)
            res.update({f"{name}.p_norm": np.int64(pn), f"{name}.norm_flag": np.int64(nf), f"{name}.dim_e": np.int64(de),
                        f"{name}.dim_r": np.int64(dr), f"{name}.B": np.int64(B), f"{name}.K": np.int64(K),
                        f"{name}.loss_margin": np.float64(lm), f"{name}.regul": np.float64(REGUL),
                        f"{name}.loss": np.float64(loss), f"{name}.score": s})
            for k, g in grads.items():
                res[f"{name}.grad_{k}"] = g
    res["names"] = np.array(names)
    out = os.path.join(HERE, "transr_train.npz")
    np.savez_compressed(out, **res)
    size = os.path.getsize(out)
    assert size < 200 * 1024, size
    print(f"TransR training fixture: {len(names)} cases, {size} bytes")


if __name__ == "__main__":
    main()
