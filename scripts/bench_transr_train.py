"""Times one training step of the reference's TransR recipe (OpenKE examples/train_transr_FB15K237.py:
NegativeSampling(TransR, MarginLoss(4.0)), SGD alpha 1.0, neg 25, dim_e = dim_r = 200, L1,
norm_flag, rand_init matrices) at the project's training shape (the C2 id space, B = 2,721), three
ways in one process, as scripts/bench_transd_train.py does for TransD:

  eager      NegativeSampling's generic branch (model(data) through torch ops -- one gathered
             dim_e x dim_r matrix per batch row -- the loss module), backward through autograd,
             mmre.optim.SGD.step: the step before the fused path
  fused      mmre.transr_ns.fused_ns_loss through NegativeSampling, backward, step
  fused+sgd  the same with the optimizer's step applied in the gradient's owner pass

TransD's fused+sgd step at (200, 200) runs beside them as a reference point, all alternating inside
every repetition. Before timing, the loss of eager and fused on the same batch and the same tables
is compared to 1e-5 relative. --only PATH runs that path alone (for a kernel trace); --batch halves
B for all legs where the eager leg's gathered matrices (B (1 + K) dim_e dim_r floats, several
times over) do not fit.

Prints one JSON line (per path: median, min, max and every repetition in ms per step; the parity
check; whether the slowest repetition of fused and of fused+sgd beats the fastest eager one; the
ratio to TransD's fused+sgd step; the live projection slots and the GEMMs' FLOP of one batch) and
writes it to --out. There is no CPU path: without a GPU the script fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_transh_train import PATHS  # noqa: E402


def slot_stats(h, t, r, B, R, de, dr):
    """The projection slots of one batch by the rule of csrc/transh_train.hip's TransR part: two per
    positive, a negative's where it does not share (entity, relation) with its positive's."""
    import numpy as np
    h, t, r = (x.cpu().numpy() for x in (h, t, r))
    b = np.arange(len(h)) % B
    neg = np.arange(len(h)) >= B
    live_h, live_t = ~(neg & (r == r[b]) & (h == h[b])), ~(neg & (r == r[b]) & (t == t[b]))
    per_rel = np.bincount(r[live_h], minlength=R) + np.bincount(r[live_t], minlength=R)
    n = int(per_rel.sum())
    return {"rows": int(len(h)), "live_slots": n, "relations_in_batch": int((per_rel > 0).sum()),
            "largest_relation_slots": int(per_rel.max()), "row_tiles_of_32": int(((per_rel + 31) // 32).sum()),
            "flop_per_gemm": 2 * n * de * dr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=PATHS, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=2721)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_transr_train: no GPU (there is no CPU path)")
    from mmre import _lib, transd_ns, transr_ns
    from mmre.data import TrainIndex
    from mmre.optim import SGD
    from mmre.sampler import OpenKESampler
    from mmre.workloads import zs_workload
    from openke.module.loss import MarginLoss
    from openke.module.model import TransD, TransR
    from openke.module.strategy import NegativeSampling
    dev = torch.device("cuda:0")
    B, K, de, dr, lr, margin = a.batch, 25, 200, 200, 1.0, 4.0
    w = zs_workload("FB15K-237-ZS", "transe", 200)
    E, R = int(w["n_ent"]), int(w["n_rel"])
    idx = TrainIndex(w["filter_h"], w["filter_t"], w["filter_r"], E, R)
    smp = OpenKESampler(idx, dev, bern=True)
    ring = []
    for _ in range(a.batches):
        b = smp.sample(B, K)
        ring.append({"batch_h": b["batch_h"].clone(), "batch_t": b["batch_t"].clone(), "batch_r": b["batch_r"].clone(),
                     "mode": "normal"})

    def build(path, model="transr"):
        torch.manual_seed(0)
        if model == "transd":
            kg = TransD(ent_tot=E, rel_tot=R, dim_e=de, dim_r=dr, p_norm=1, norm_flag=True).to(dev)
        else:
            kg = TransR(ent_tot=E, rel_tot=R, dim_e=de, dim_r=dr, p_norm=1, norm_flag=True, rand_init=True).to(dev)
        st = NegativeSampling(model=kg, loss=MarginLoss(margin=margin).to(dev), batch_size=B)
        if path == "eager":
            st._transr_fused = lambda data, mode: None  # the generic branch, as for any model without a fused path
        opt = SGD(st.parameters(), lr=lr)
        if path == "fused+sgd":
            st.fuse_optimizer(opt)
        state = {"i": 0}

        def one():
            data = ring[state["i"] % len(ring)]
            state["i"] += 1
            opt.zero_grad()
            loss = st(data)
            loss.backward()
            opt.step()
            return loss
        return st, one

    result = {"shape": {"n_ent": E, "n_rel": R, "batch": B, "neg": K, "dim_e": de, "dim_r": dr, "p_norm": 1,
                        "norm_flag": True, "rand_init": True, "loss": "margin", "loss_margin": margin,
                        "optimizer": "sgd", "lr": lr},
              "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    # parity: the two branches' loss on the same batch and tables
    if a.only is None:
        with torch.no_grad():
            le = float(build("eager")[0](ring[0]))
            n0 = transr_ns.calls
            lf = float(build("fused")[0](ring[0]))
        assert transr_ns.calls == n0 + 1, "the fused path did not run"
        result["parity"] = {"eager_loss": le, "fused_loss": lf, "relative": abs(le - lf) / abs(le)}
        assert abs(le - lf) <= 1e-5 * abs(le), result["parity"]
        torch.cuda.empty_cache()

    jobs = [(a.only, "transr")] if a.only else [(p, "transr") for p in PATHS] + [("fused+sgd", "transd")]
    name = lambda p, model: p if model == "transr" else "transd " + p
    runners = {}
    for p, model in jobs:
        mod = transr_ns if model == "transr" else transd_ns
        n0 = mod.calls
        one = build(p, model)[1]
        for _ in range(a.warmup):
            last = one()
        torch.cuda.synchronize()
        assert (mod.calls - n0 == a.warmup) == (p != "eager"), (p, model)
        runners[name(p, model)] = (one, float(last.detach()))
    times = {n: [] for n in runners}
    for _ in range(a.reps):  # the paths alternate within every repetition
        for n, (one, _) in runners.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                one()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.steps)
    result["paths"] = {n: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v),
                           "ms_per_step_max": max(v), "ms_per_step": v, "loss_after_warmup": runners[n][1]}
                       for n, v in times.items()}
    ok = True
    med = lambda n: statistics.median(times[n])
    if "eager" in times:
        for f in ("fused", "fused+sgd"):
            beats = max(times[f]) < min(times["eager"])
            ok = ok and beats
            result["slowest_%s_beats_fastest_eager" % f.replace("+", "_")] = beats
            result["eager_over_%s_median" % f.replace("+", "_")] = med("eager") / med(f)
        result["fused_sgd_over_transd_fused_sgd_median"] = med("fused+sgd") / med("transd fused+sgd")
    result["slots"] = slot_stats(ring[0]["batch_h"], ring[0]["batch_t"], ring[0]["batch_r"], B, R, de, dr)
    result["peak_memory_bytes"] = int(torch.cuda.max_memory_allocated())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("bench_transr_train: a fused path is not faster than eager")


if __name__ == "__main__":
    main()
