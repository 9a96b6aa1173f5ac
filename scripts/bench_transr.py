"""Times the fused TransR link-prediction evaluation at the C2 shape (FB15K-237-ZS: every test
triple in both modes against every entity, dim_e = dim_r = 200, L1, norm_flag, seeded xavier tables
with rand_init matrices, and the bench's synthetic filter set) and, in the same process and
alternating with it inside every repetition, two yardsticks on the same queries, plan and filter
groups:

  transr   TransRSweep.run: r_hat, the MFMA projection of every used relation, the query gather,
           the truth / filter pass, the sweep over the planes, finalize
  transh   TransHSweep.run: the sweep whose geometry TransR's shares (it stages one raw plane and
           projects per element; TransR stages 29 projected planes as they are)
  eager    the best torch does with the parent commit's tools: per used relation
           P = F.normalize(ent @ M_r), the query vectors, torch.cdist(q, P, p=1), and the four rank
           counts by comparison against the truth score (raw and, through the filter lists, filtered)

Each repetition times `--iters` warmed-up calls of a path between two device events on the launch
stream; the JSON line has the median, min and max per evaluation, TransR's workspace, and the
condition: the slowest TransR repetition against the fastest eager one. The kernels one by one
(k_tr_project and its rate, k_sweep_transr against k_sweep_transh) are read from a kernel trace of
this script (rocprofv3 --kernel-trace --stats, a run of its own). Reads nothing outside the
repository. No CPU path."""
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
    ap.add_argument("--dim", type=int, default=200, help="dim_e = dim_r (and TransH's dim)")
    ap.add_argument("--n-test", type=int, default=None, help="only the first n test triples")
    ap.add_argument("--only", default=None, help="comma-separated paths (default: all three)")
    ap.add_argument("--check", type=int, default=64, help="queries recounted from k_transr_rows' scores")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit("bench_transr: no GPU (there is no CPU path)")
    from mmre import _lib
    from mmre.link import FilterIndex, ScoreSpec
    from mmre.transh import TransHSweep, plan_tiles
    from mmre.transr import TransRSweep
    from mmre.workloads import xavier, zs_workload
    dev = torch.device("cuda:0")
    d = a.dim
    w = zs_workload("FB15K-237-ZS", "transe", d, n_test=a.n_test)
    E, R = w["n_ent"], w["n_rel"]
    g = torch.Generator().manual_seed(1)
    nv = xavier(R, d, g)
    tm = xavier(R, d * d, g)                       # rand_init=True (TransR.py:31)
    ent, rel, nv, tm = (x.to(dev) for x in (w["ent"], w["rel"], nv, tm))
    index = FilterIndex(w["filter_h"], w["filter_r"], w["filter_t"], E, R)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n = len(w["test_h"])
    qh, qr, qt = (np.concatenate([x, x]).astype(np.int64) for x in (w["test_h"], w["test_r"], w["test_t"]))
    qm = np.concatenate([np.zeros(n, np.int8), np.ones(n, np.int8)])
    groups = tuple(to(x) for x in index.groups(qh, qr, qt, qm))
    q = tuple(to(x) for x in (qh, qr, qt, qm))
    plan = plan_tiles(qr)

    tr = TransRSweep(ScoreSpec(model="transr", ent=ent, rel=rel, dim=d, norm_flag=True, pred_kind=0, dim_e=d,
                               transfer_matrix=tm))
    th = TransHSweep(ScoreSpec(model="transh", ent=ent, rel=rel, dim=d, norm_flag=True, pred_kind=0, norm_vec=nv))
    br, bh = {}, {}

    # the eager leg's host-side plan, made once (as the fused paths' plan and filter groups are):
    # per used relation its queries, and the filter lists flattened to (query row, entity) pairs
    off, ids = index.filters(qh, qr, qt, qm)
    cnt = np.diff(off)
    by_rel = []
    for r in plan["used"]:
        sel = np.nonzero(qr == r)[0]
        rows = np.repeat(np.arange(len(sel)), cnt[sel])
        cols = np.concatenate([ids[off[i]:off[i + 1]] for i in sel]) if len(sel) else np.zeros(0, np.int64)
        head = qm[sel] == 0
        by_rel.append((int(r), to(sel), to(np.where(head, qt[sel], qh[sel])), to(np.where(head, qh[sel], qt[sel])),
                       to(head), to(rows.astype(np.int64)), to(cols.astype(np.int64))))
    e_raw = torch.zeros(2 * n, dtype=torch.int64, device=dev)
    e_filt = torch.zeros(2 * n, dtype=torch.int64, device=dev)

    CDIST_ROWS = 1024

    def eager():
        r_hat = F.normalize(rel, 2, -1)
        for r, sel, anchor, truth, head, rows, cols in by_rel:
            P = F.normalize(ent @ tm[r].view(d, d), 2, -1)                    # (E, d)
            pa = P[anchor]
            qv = torch.where(head[:, None], pa - r_hat[r], pa + r_hat[r])     # s = |q - p(e)|_1 in both modes
            # (n_r, E), in blocks of CDIST_ROWS query rows: cdist launches one workgroup per pair, and
            # a relation with more rows than that overruns the launch's thread count -- its scores
            # came back wrong without an error
            s = torch.cat([torch.cdist(qv[i:i + CDIST_ROWS], P, p=1) for i in range(0, len(sel), CDIST_ROWS)])
            t = s.gather(1, truth[:, None])
            beat = s < t
            raw = beat.sum(1)
            known = torch.zeros(len(sel), dtype=torch.int64, device=dev)
            known.index_add_(0, rows, (beat[rows, cols] & (cols != truth[rows])).to(torch.int64))
            e_raw[sel] = raw
            e_filt[sel] = raw - known

    paths = {"transr": lambda: tr.run(*q, filt=groups, buffers=br, plan=plan),
             "transh": lambda: th.run(*q, filt=groups, buffers=bh, plan=plan),
             "eager": eager}
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
    out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in times.items()}
    n_used, e_pad = int(len(plan["used"])), -(-E // 128) * 128
    result = {"shape": {"entities": E, "relations": R, "dim_e": d, "dim_r": d, "queries": 2 * n},
              "tiles": int(len(plan["tiles"])), "relations_used": n_used, "padding": plan["padding"],
              "iters": a.iters, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0), **out,
              "projection_flop": 2 * n_used * e_pad * d * d,
              "transr_workspace_bytes": int(_lib.lib().mmre_transr_workspace(E, R, d, d, len(plan["tiles"]), n_used,
                                                                             int(groups[3].shape[0])))}
    if "transr" in out and "eager" in out:
        result["condition_slowest_transr_below_fastest_eager"] = out["transr"]["max"] < out["eager"]["min"]
        # the eager counts agree with the fused ones except where a float rounding flips a comparison
        c = br["counts"]
        result["eager_vs_transr_raw_counts_differing"] = int((c[0].to(torch.int64) != e_raw).sum())
        result["eager_vs_transr_filtered_counts_differing"] = int((c[1].to(torch.int64) != e_filt).sum())
        dr = (c[0].to(torch.int64) - e_raw).abs()
        result["eager_vs_transr_raw_count_abs_difference"] = {"max": int(dr.max()), "mean": float(dr.double().mean()),
                                                              "mean_raw_count": float(e_raw.double().mean())}
    if "transr" in out and a.check > 0:
        # an independent count for a sample of queries: k_transr_rows (from the raw tables, no plane,
        # no sweep) scores every entity for the query, the host counts those below the truth
        from mmre.transr import score_rows
        rng = np.random.default_rng(0)
        pick = rng.choice(2 * n, a.check, replace=False)
        ids = torch.arange(E, device=dev)
        bad_fused, bad_eager = 0, 0
        for i in pick:
            head = qm[i] == 0
            anchor = torch.full((E,), int(qt[i] if head else qh[i]), device=dev)
            rr = torch.full((E,), int(qr[i]), device=dev)
            sc = score_rows(tr.spec, ids if head else anchor, rr, anchor if head else ids,
                            mode="head_batch" if head else "tail_batch")
            tv = sc[int(qh[i] if head else qt[i])]
            want = int((sc < tv).sum())
            bad_fused += int(want != int(br["counts"][0, i]))
            if "eager" in out:
                bad_eager += int(want != int(e_raw[i]))
        result["check"] = {"queries": int(a.check), "fused_raw_counts_differing_from_rows_kernel": bad_fused,
                           "eager_raw_counts_differing_from_rows_kernel": bad_eager if "eager" in out else None}
    if "transr" in out and "transh" in out:
        result["transr_over_transh"] = out["transr"]["median"] / out["transh"]["median"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
