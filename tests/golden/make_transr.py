"""make_transr.py -- TransR link-prediction fixtures from the REFERENCE itself.

Runs only in the build container (needs /root/reference and oracle/_ref/Base.so), on the CPU;
never on the GPU box. Nothing from the reference travels: only the numbers written to
tests/golden/transr_small.npz.

The method is tests/golden/make_transh.py's, unchanged (its Tester loop, its screen, its three
conditions and their constants NEAR, REL and MAX_SEEDS are imported from it): the reference's
OpenKE TransR (openke/module/model/TransR.py) under the reference Tester loop (Tester.py:70-91)
with its Base.so on tests/golden/data/small (E = 257, R = 13, 150 test triples), for four
configurations and type_constrain 0 / 1. For each configuration seeds are walked from SEED0 and
the first one is kept for which
  1. in the reference's own scores no candidate other than the truth lies within
     NEAR * max(1, |truth|) of its query's truth (screened from predict before the Base.so loop,
     asserted again on the loop's scores);
  2. the restatement of DESIGN.md §3 (tests/transr_restate.py) deviates from the reference by at
     most REL relative on every score;
  3. the restatement's counts equal Base.so's on all 300 queries, with and without type
     constraints.

One configuration's INPUTS are widened, nothing else: l1_nonorm_margin_tall takes the reference's
constructor at its seed (rand_init=True: xavier matrices) and multiplies transfer_matrix by
MATRIX_SCALE = 8 before anything is evaluated. As xavier leaves them, a projected entity (std 0.019
per element) is a tenth of a relation element (std 0.20), and without norm_flag nothing rescales
it: a query's 257 scores span 0.6 around |truth| = 6.8, condition 1's window catches a neighbour in
14 - 30 of the 300 queries of every seed, and none of 4,000 seeds (343 .. 4342) met it. Times 8
(exact in float32) the projection is of the relation's size (0.15 against 0.20) and a seed has
about four such queries, as TransH's fixture does. Condition 1 is a condition on the inputs; the
screen, the three conditions, NEAR, REL, MAX_SEEDS and the Tester loop are make_transh.py's as
they stand, and the scaled matrices are what the fixture stores and every test loads.

Usage:  python tests/golden/make_transr.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_transh import (DATA, MAX_SEEDS, N_PRED, NEAR, REF, REL, base_setup, load_base, near_truth,  # noqa: E402
                         reference_run, restated_counts, screen)

import transr_restate as R  # noqa: E402

SEED0 = 300
CONFIGS = [
    ("l1_norm", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=True)),
    ("l2_norm_wide", dict(dim_e=40, dim_r=24, p_norm=2, norm_flag=True, rand_init=True)),
    ("l1_nonorm_margin_tall", dict(dim_e=24, dim_r=40, p_norm=1, norm_flag=False, rand_init=True, margin=5.0)),
    ("l1_identity", dict(dim_e=32, dim_r=32, p_norm=1, norm_flag=True, rand_init=False)),
]
TABLES = ("ent_embeddings", "rel_embeddings", "transfer_matrix")
MATRIX_SCALE = {"l1_nonorm_margin_tall": 8.0}   # (the module docstring says why; every other configuration: 1)


def import_transr():
    sys.path.insert(0, os.path.join(REF, "OpenKE"))
    from openke.module.model import TransR  # noqa: E402
    return TransR


def try_seed(lib, TransR, ds, index, kw, seed, scale=1.0):
    """The fixture of one configuration at one seed, or the reason the seed is refused."""
    E, T = ds.n_ent, len(ds.test)
    torch.manual_seed(seed)
    model = TransR(ent_tot=E, rel_tot=ds.n_rel, **kw)
    if scale != 1.0:
        model.transfer_matrix.weight.data *= scale
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    why = screen(model, ds)
    if why is not None:
        return None, why
    out = {}
    for tc in (0, 1):
        preds, counts, (qh, qr, qt), metrics = reference_run(lib, model, E, T, tc)
        out[f"tc{tc}_head_counts"], out[f"tc{tc}_tail_counts"] = counts["head"], counts["tail"]
        out[f"tc{tc}_metrics"] = metrics
    tabs = [sd[f"{k}.weight"] for k in TABLES]
    margin = kw.get("margin")
    worst = 0.0
    for side, head in (("head", True), ("tail", False)):
        ref = preds[side]
        truth = qh if head else qt
        assert not near_truth(ref, truth), "the Tester loop's scores are the screened ones"  # condition 1
        ours = R.sweep_scores(*tabs, qh, qr, qt, np.full(T, 0 if head else 1), kw["p_norm"], kw["norm_flag"], margin)
        dev = float((np.abs(ours.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)).max())
        worst = max(worst, dev)
        if dev > REL:                                                        # condition 2
            return None, f"restatement {dev:.3g} relative off the reference ({side} batch)"
        mine = restated_counts(ours, qh, qr, qt, head, ds, index)
        # Base.so fills the constrained ranks only under type_constrain (Test.h:88-98)
        if not (np.array_equal(mine[:2].T, out[f"tc0_{side}_counts"][:, :2])
                and np.array_equal(mine.T, out[f"tc1_{side}_counts"])):      # condition 3
            return None, f"restated {side}-batch counts differ from the reference's"
        out[f"pred_{side}"] = ref[:N_PRED].copy()
    out.update(qh=qh, qr=qr, qt=qt, seed=np.int64(seed), restate_rel_dev=np.float64(worst),
               matrix_scale=np.float64(scale))
    for k, v in sd.items():
        out[k] = v
    out.setdefault("margin", np.full(1, np.nan, np.float32))  # (the state dict's own, where the model has one)
    return out, None


def main():
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    path = os.path.join(DATA, "small")
    lib = load_base()
    base_setup(lib, path)
    TransR = import_transr()
    ds = OpenKEDataset(path)
    index = FilterIndex(*ds.all_triples(), ds.n_ent, ds.n_rel)
    res = {"E": ds.n_ent, "R": ds.n_rel, "T": len(ds.test), "near": np.float64(NEAR), "rel": np.float64(REL)}
    seed = SEED0
    for name, kw in CONFIGS:
        for _ in range(MAX_SEEDS):
            fx, why = try_seed(lib, TransR, ds, index, kw, seed, MATRIX_SCALE.get(name, 1.0))
            seed += 1
            if fx is not None:
                break
            if not why.endswith("of a truth"):  # (a near tie refuses most seeds)
                print(f"{name}: seed {seed - 1} refused: {why}")
        assert fx is not None, f"{name}: no seed in {MAX_SEEDS} meets the three conditions"
        print(f"{name}: seed {int(fx['seed'])}, restatement within {float(fx['restate_rel_dev']):.3g} relative")
        for k, v in fx.items():
            res[f"{name}.{k}"] = v
    np.savez_compressed(os.path.join(HERE, "transr_small.npz"), **res)
    print("transr fixture: small")


if __name__ == "__main__":
    main()
