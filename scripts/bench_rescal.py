"""Times the fused RESCAL link-prediction evaluation at FB15K237's shape (E = 14,541, R = 237,
20,466 test triples in both modes against every entity; random triples and seeded xavier tables,
no filter, no type masks) and, in the same process and alternating with it inside every repetition,
two yardsticks:

  rescal    RescalSweep.run: the k-major entity copy, the MFMA plane of every used relation, the
            query gather, the truth pass, the sweep with a per-tile entity operand, finalize
  distmult  LinkSweep.run of a DistMult model at the same Q, E and d with the exact f32 MFMA sweep
            (the split-bf16 filter switched off): the same arithmetic with one entity operand; its
            sweep kernel alone is also timed between two events (LinkSweep's sweep_events)
  eager     the Tester loop a user has with only the model class: per test triple and side one
            predict from forward()'s torch ops over all entities and its copy to the host
            (Tester.py:70-91 without Base.so's ranking). Run on the first --eager-n triples; the loop
            is one independent iteration per triple, so the JSON also carries the figure scaled to
            all of them, marked as scaled

Each repetition times `--iters` warmed-up calls of a path between two device events on the launch
stream; the JSON line has the median, min and max per evaluation, the plan's padding and the
workspace bytes at this dim (all relations used, and 29). The kernels one by one (k_rs_planes,
k_rs_queries, k_rs_scores, k_sweep_rescal against k_sweep_mfma) are read from a kernel trace of
this script (rocprofv3 --kernel-trace --stats, a run of its own). Reads nothing outside the
repository. No CPU path."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--entities", type=int, default=14541)
    ap.add_argument("--relations", type=int, default=237)
    ap.add_argument("--n-test", type=int, default=20466)
    ap.add_argument("--eager-n", type=int, default=1024, help="test triples the eager loop runs (0: skip it)")
    ap.add_argument("--only", default=None, help="comma-separated paths of rescal,distmult")
    ap.add_argument("--check", type=int, default=32, help="queries recounted from k_rescal_rows' scores")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rescal: no GPU (there is no CPU path)")
    from mmre import _lib
    from mmre.link import LinkSweep, ScoreSpec
    from mmre.rescal import RescalSweep, plan_keys, score_rows
    from mmre.workloads import xavier
    from openke.module.model import RESCAL
    dev = torch.device("cuda:0")
    d, E, R, n = a.dim, a.entities, a.relations, a.n_test
    g = torch.Generator().manual_seed(1)
    ent, mats, rel = xavier(E, d, g).to(dev), xavier(R, d * d, g).to(dev), xavier(R, d, g).to(dev)
    rng = np.random.default_rng(0)
    th, tr, tt = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    qh, qr, qt = (np.concatenate([x, x]).astype(np.int64) for x in (th, tr, tt))
    qm = np.concatenate([np.zeros(n, np.int8), np.ones(n, np.int8)])
    q = tuple(to(x) for x in (qh, qr, qt, qm))
    plan = plan_keys(qr, qm)

    rs = RescalSweep(ScoreSpec(model="rescal", ent=ent, rel=None, dim=d, pred_kind=0, rel_matrices=mats))
    dm = LinkSweep(ScoreSpec(model="distmult", ent=ent, rel=rel, dim=d, pred_kind=2))
    dm.mfma_filter = False                          # the exact f32 MFMA sweep (mmre_link_sweep)
    br, bd = {}, dm.alloc_queries(2 * n)
    sweep_ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    dm_sweep = []

    def distmult():
        dm.run(*q, buffers=bd, sweep_events=sweep_ev)

    paths = {"rescal": lambda: rs.run(*q, buffers=br, plan=plan), "distmult": distmult}
    if a.only:
        paths = {k: paths[k] for k in a.only.split(",")}
    with torch.no_grad():
        for p in paths.values():
            for _ in range(a.warmup):
                p()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, p in paths.items():   # the paths alternate inside every repetition
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    p()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.iters)
                if k == "distmult":
                    dm_sweep.append(sweep_ev[0].elapsed_time(sweep_ev[1]))   # the repetition's last call
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    out = {k: stat(v) for k, v in times.items()}
    if dm_sweep:
        out["distmult_sweep_kernel"] = stat(dm_sweep)
    ws = _lib.lib().mmre_rescal_workspace
    n_tiles, n_used = int(len(plan["tiles"])), int(len(plan["used"]))
    result = {"shape": {"entities": E, "relations": R, "dim": d, "queries": 2 * n}, "tiles": n_tiles,
              "relations_used": n_used, "padding": plan["padding"], "distmult_tiles": -(-2 * n // 128),
              "iters": a.iters, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0), **out,
              "planes_flop": 2 * n_used * (-(-E // 128) * 128) * d * d,
              "workspace_bytes": int(ws(E, R, d, n_tiles, n_used, 0)),
              "workspace_bytes_29_used": int(ws(E, R, d, n_tiles, 29, 0))}
    if "rescal" in out and a.check > 0:
        # an independent count for a sample of queries: k_rescal_rows (from the raw tables, no plane,
        # no sweep) scores every entity for the query, the host counts those below the truth
        pick = rng.choice(2 * n, a.check, replace=False)
        ids = torch.arange(E, device=dev)
        bad = 0
        for i in pick:
            head = qm[i] == 0
            anchor = torch.full((E,), int(qt[i] if head else qh[i]), device=dev)
            sc = score_rows(rs.spec, ids if head else anchor, torch.full((E,), int(qr[i]), device=dev),
                            anchor if head else ids)
            want = int((sc < sc[int(qh[i] if head else qt[i])]).sum())
            bad += int(want != int(br["counts"][0, i]))
        result["check"] = {"queries": int(a.check), "fused_raw_counts_differing_from_rows_kernel": bad}
    if a.eager_n > 0:
        model = RESCAL(ent_tot=E, rel_tot=R, dim=d).to(dev)
        with torch.no_grad():
            model.ent_embeddings.weight.copy_(ent)
            model.rel_matrices.weight.copy_(mats)
        ids = torch.arange(E, device=dev)
        m = min(a.eager_n, n)
        hs, rs_, ts = (to(x[:m].astype(np.int64)) for x in (th, tr, tt))

        def eager_loop():
            with torch.no_grad():
                for i in range(m):
                    for side in ("head_batch", "tail_batch"):
                        data = {"batch_h": ids if side == "head_batch" else hs[i:i + 1],
                                "batch_t": hs[i:i + 1] * 0 + ts[i] if side == "head_batch" else ids,
                                "batch_r": rs_[i:i + 1], "mode": side}
                        (-model(data)).cpu().numpy()     # RESCAL.py:44-46, as the reference's predict

        eager_loop()                                     # warm-up
        runs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eager_loop()
            runs.append((time.perf_counter() - t0) * 1e3)
        result["eager"] = {"triples": m, "ms": stat(runs), "ms_per_query": statistics.median(runs) / (2 * m),
                           "ms_scaled_to_all_triples": statistics.median(runs) * n / m}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
