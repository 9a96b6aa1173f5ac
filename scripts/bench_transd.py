"""Times the fused TransD link-prediction evaluation at the C2 shape (FB15K-237-ZS: every test
triple in both modes against every entity, dim_e = dim_r = 200, L1, norm_flag, seeded xavier tables
and the bench's synthetic filter set) and, in the same process and alternating with it inside every
repetition, the yardstick: the TransH evaluation of the same queries on the same plan. The sweep
kernel is the same code on the same shapes, so a difference is the prologue's.

  transd   TransDSweep.run: prologue (s, the (-s, N) table), truth / filter pass, sweep, finalize
  transh   TransHSweep.run: prologue ((a, n) table), truth / filter pass, sweep, finalize

Each repetition times `--iters` warmed-up calls of a path between two device events on the launch
stream; the JSON line has the median, min and max per evaluation and whether TransD's median lies
inside TransH's min - max. The kernels one by one (k_td_s, k_td_an against k_th_an,
k_td_relations, the shared ones) are read from a kernel trace of this script (rocprofv3
--kernel-trace --stats, a run of its own). Reads nothing outside the repository. No CPU path."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dim", type=int, default=200, help="dim_r (and TransH's dim)")
    ap.add_argument("--dim-e", type=int, default=None, help="dim_e >= dim (default: dim)")
    ap.add_argument("--n-test", type=int, default=None, help="only the first n test triples")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dim_e = a.dim if a.dim_e is None else a.dim_e
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_transd: no GPU (there is no CPU path)")
    from mmre import _lib
    from mmre.link import FilterIndex, ScoreSpec
    from mmre.transd import TransDSweep
    from mmre.transh import TransHSweep, plan_tiles
    from mmre.workloads import xavier, zs_workload
    dev = torch.device("cuda:0")
    w = zs_workload("FB15K-237-ZS", "transe", a.dim, n_test=a.n_test)
    E, R = w["n_ent"], w["n_rel"]
    g = torch.Generator().manual_seed(1)
    nv = xavier(R, a.dim, g)                       # TransH's normals double as TransD's rel_transfer
    ept = xavier(E, dim_e, g)
    ent_d = w["ent"] if dim_e == a.dim else torch.cat([w["ent"], xavier(E, dim_e - a.dim, g)], 1)
    ent, rel, nv, ept, ent_d = (x.to(dev) for x in (w["ent"], w["rel"], nv, ept, ent_d))
    index = FilterIndex(w["filter_h"], w["filter_r"], w["filter_t"], E, R)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n = len(w["test_h"])
    qh, qr, qt = (np.concatenate([x, x]).astype(np.int64) for x in (w["test_h"], w["test_r"], w["test_t"]))
    qm = np.concatenate([np.zeros(n, np.int8), np.ones(n, np.int8)])
    groups = tuple(to(x) for x in index.groups(qh, qr, qt, qm))
    q = tuple(to(x) for x in (qh, qr, qt, qm))
    plan = plan_tiles(qr)

    td = TransDSweep(ScoreSpec(model="transd", ent=ent_d, rel=rel, dim=a.dim, norm_flag=True, pred_kind=0,
                               ent_transfer=ept, rel_transfer=nv, dim_e=dim_e))
    th = TransHSweep(ScoreSpec(model="transh", ent=ent, rel=rel, dim=a.dim, norm_flag=True, pred_kind=0, norm_vec=nv))
    bd, bh = {}, {}
    paths = {"transd": lambda: td.run(*q, filt=groups, buffers=bd, plan=plan),
             "transh": lambda: th.run(*q, filt=groups, buffers=bh, plan=plan)}
    with torch.no_grad():
        for p in paths.values():
            for _ in range(a.warmup):
                p()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, p in paths.items():   # the two alternate inside every repetition
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    p()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.iters)
    out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in times.items()}
    result = {"shape": {"entities": E, "relations": R, "dim_e": dim_e, "dim_r": a.dim, "queries": 2 * n},
              "tiles": int(len(plan["tiles"])), "relations_used": int(len(plan["used"])), "padding": plan["padding"],
              "iters": a.iters, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0), **out,
              "transd_over_transh": out["transd"]["median"] / out["transh"]["median"],
              "transd_median_inside_transh_range": out["transh"]["min"] <= out["transd"]["median"] <= out["transh"]["max"],
              # (two models: the sums differ; they show that both evaluations ran to the end)
              "raw_count_sums": {"transd": int(bd["counts"][0].sum()), "transh": int(bh["counts"][0].sum())}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
