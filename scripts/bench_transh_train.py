"""Times one training step of the reference's TransH recipe (OpenKE examples/train_transh_FB15K237.py:
NegativeSampling(TransH, MarginLoss(4.0)), SGD, neg 25, d 200, L1, norm_flag) at the project's
training shape (the C2 id space, B = 2,721; SGD lr 0.5), three ways in one process:

  eager      NegativeSampling's generic branch (model(data) through torch ops, the loss module),
             backward through autograd, mmre.optim.SGD.step: the step before the fused path
  fused      mmre.transh_ns.fused_ns_loss through NegativeSampling, backward, step
  fused+sgd  the same with the optimizer's step applied in the gradient's owner pass

Batches are drawn once from mmre.sampler.OpenKESampler (--batches of them, cycled), so a step is
the loss, the backward and the update, not the sampler. The paths alternate inside every
repetition; each repetition times --steps warmed-up steps of a path between two device events on
the launch stream. Before timing, the loss of eager and fused on the same batch and the same
tables is compared to 1e-5 relative. --only PATH runs a single path (for a kernel trace).

Prints one JSON line (per path: median, min, max and every repetition in ms per step; the parity
check; whether the slowest fused+sgd repetition beats the fastest eager one) and writes it to
--out. Also reports, from the shapes and one batch, what the gradient's kernels move: records per
table and their bytes, the gathered rows, the tables written, and the longest and the median
contribution list of each table. There is no CPU path: without a GPU the script fails."""
import argparse
import json
import os
import statistics
import sys

HBM_PEAK = 8.0e12  # B/s, MI355X
PATHS = ("eager", "fused", "fused+sgd")


def record_stats(h, t, r, B, K, E, R, d):
    """The records of one batch by the rule of csrc/transh_train.hip (regul_rate 0, every hinge
    term active: the most a step writes): a positive's four summed rows, and a negative's row
    wherever it differs from its positive's."""
    import numpy as np
    h, t, r = (x.cpu().numpy() for x in (h, t, r))
    ph, pt, pr = (np.tile(x[:B], K) for x in (h, t, r))
    nh, nt, nr = h[B:], t[B:], r[B:]
    same_r = nr == pr
    ent_keys = np.concatenate([h[:B], t[:B], nh[~(same_r & (nh == ph))], nt[~(same_r & (nt == pt))]])
    rel_keys = np.concatenate([r[:B], nr[~same_r]])
    out = {}
    for name, keys, n in (("ent", ent_keys, E), ("rel", rel_keys, R), ("norm", rel_keys, R)):
        c = np.bincount(keys, minlength=n)
        c = c[c > 0]
        out[name] = {"records": int(len(keys)), "rows_with_records": int(len(c)), "longest_list": int(c.max()),
                     "median_list": float(np.median(c))}
    n_rec = sum(v["records"] for v in out.values())
    N = B * (1 + K)
    gathered = (4 * B + len(ent_keys) - 2 * B + 2 * int((~same_r).sum())) * d * 4 + 3 * 8 * N
    out["bytes"] = {
        "forward": gathered + 4 * N,
        "records": gathered + 4 * N + n_rec * d * 4 + 12 * N,
        "owner": n_rec * d * 4 + (E + 2 * R) * d * 4 + 8 * out["ent"]["records"],
        "records_written": n_rec * d * 4,
        "unsummed_records_would_be": 4 * N * d * 4,
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=PATHS, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_transh_train: no GPU (there is no CPU path)")
    from mmre import _lib, transh_ns
    from mmre.data import TrainIndex
    from mmre.optim import SGD
    from mmre.sampler import OpenKESampler
    from mmre.workloads import zs_workload
    from openke.module.loss import MarginLoss
    from openke.module.model import TransH
    from openke.module.strategy import NegativeSampling
    dev = torch.device("cuda:0")
    B, K, d, lr, margin = 2721, 25, 200, 0.5, 4.0
    w = zs_workload("FB15K-237-ZS", "transe", d)
    E, R = int(w["n_ent"]), int(w["n_rel"])
    idx = TrainIndex(w["filter_h"], w["filter_t"], w["filter_r"], E, R)
    smp = OpenKESampler(idx, dev, bern=True)
    ring = []
    for _ in range(a.batches):
        b = smp.sample(B, K)
        ring.append({"batch_h": b["batch_h"].clone(), "batch_t": b["batch_t"].clone(), "batch_r": b["batch_r"].clone(),
                     "mode": "normal"})
    paths = [a.only] if a.only else list(PATHS)

    def build(path):
        torch.manual_seed(0)
        kg = TransH(ent_tot=E, rel_tot=R, dim=d, p_norm=1, norm_flag=True).to(dev)
        st = NegativeSampling(model=kg, loss=MarginLoss(margin=margin).to(dev), batch_size=B)
        if path == "eager":
            st._transh_fused = lambda data, mode: None  # the generic branch, as for any model without a fused path
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

    result = {"shape": {"n_ent": E, "n_rel": R, "batch": B, "neg": K, "dim": d, "p_norm": 1, "norm_flag": True,
                        "loss": "margin", "loss_margin": margin, "optimizer": "sgd", "lr": lr},
              "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    # parity: the two branches' loss on the same batch and tables
    with torch.no_grad():
        le = float(build("eager")[0](ring[0]))
        n0 = transh_ns.calls
        lf = float(build("fused")[0](ring[0]))
    assert transh_ns.calls == n0 + 1, "the fused path did not run"
    result["parity"] = {"eager_loss": le, "fused_loss": lf, "relative": abs(le - lf) / abs(le)}
    assert abs(le - lf) <= 1e-5 * abs(le), result["parity"]

    runners = {}
    for p in paths:
        n0 = transh_ns.calls
        one = build(p)[1]
        for _ in range(a.warmup):
            last = one()
        torch.cuda.synchronize()
        assert (transh_ns.calls - n0 == a.warmup) == (p != "eager"), p
        runners[p] = (one, float(last.detach()))
    times = {p: [] for p in paths}
    for _ in range(a.reps):  # the paths alternate within every repetition
        for p in paths:
            one = runners[p][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                one()
            e1.record()
            e1.synchronize()
            times[p].append(e0.elapsed_time(e1) / a.steps)
    result["paths"] = {p: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v),
                           "ms_per_step_max": max(v), "ms_per_step": v, "loss_after_warmup": runners[p][1]}
                       for p, v in times.items()}
    if "eager" in times and "fused+sgd" in times:
        result["slowest_fused_sgd_beats_fastest_eager"] = max(times["fused+sgd"]) < min(times["eager"])
        result["eager_over_fused_sgd_median"] = (statistics.median(times["eager"])
                                                 / statistics.median(times["fused+sgd"]))
    result["gradient_traffic"] = record_stats(ring[0]["batch_h"], ring[0]["batch_t"], ring[0]["batch_r"], B, K, E, R, d)
    result["hbm_peak_bytes_per_s"] = HBM_PEAK
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if "slowest_fused_sgd_beats_fastest_eager" in result and not result["slowest_fused_sgd_beats_fastest_eager"]:
        sys.exit("bench_transh_train: fused+sgd is not faster than eager")


if __name__ == "__main__":
    main()
