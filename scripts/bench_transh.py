"""Times the fused TransH link-prediction evaluation at the C2 shape (FB15K-237-ZS: every test
triple in both modes against every entity, d = 200, L1, norm_flag, seeded xavier tables and the
bench's synthetic filter set) and, in the same process and alternating with it, the yardstick: the
TransE evaluation of the same queries through the exact f32 sweep (MMRE_L1_FILTER=0).

  transh        TransHSweep.run: prologue ((a, n) table), truth / filter pass, sweep, finalize
  transe_f32    LinkSweep.run with the integer filter off: prepare, truth / filter pass, f32 sweep
  transe_sweep  the f32 sweep kernel alone (LinkSweep's sweep_events)

Each repetition times `--iters` warmed-up calls of a path between two device events on the launch
stream; the JSON line has the median, min and max per evaluation, the plan's padding factor
P = padded query rows / Q and the ratio transh / (P * transe_sweep) against the target 1.15. The
TransH sweep kernel alone is read from a kernel trace of this script (rocprofv3 --kernel-trace
--stats, a run of its own). Two extreme plans are timed too: all queries of one relation (P ~ 1)
and one query per tile (one query per relation, P = 128). Reads nothing outside the repository.
No CPU path."""
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
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--n-test", type=int, default=None, help="only the first n test triples")
    ap.add_argument("--no-extremes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["MMRE_L1_FILTER"] = "0"   # the yardstick is the exact f32 sweep (read when LinkSweep is made)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_transh: no GPU (there is no CPU path)")
    from mmre import _lib
    from mmre.link import FilterIndex, LinkSweep, ScoreSpec
    from mmre.transh import TransHSweep, plan_tiles
    from mmre.workloads import xavier, zs_workload
    dev = torch.device("cuda:0")
    w = zs_workload("FB15K-237-ZS", "transe", a.dim, n_test=a.n_test)
    E, R = w["n_ent"], w["n_rel"]
    nv = xavier(R, a.dim, torch.Generator().manual_seed(1))
    ent, rel, nv = (x.to(dev) for x in (w["ent"], w["rel"], nv))
    index = FilterIndex(w["filter_h"], w["filter_r"], w["filter_t"], E, R)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def queries(h, r, t, both=True):
        """Head-batch and (both) tail-batch queries of the triples, as the Tester's evaluation makes them."""
        n = len(h)
        rep = 2 if both else 1
        qh, qr, qt = (np.concatenate([x] * rep).astype(np.int64) for x in (h, r, t))
        qm = np.concatenate([np.zeros(n, np.int8), np.ones(n, np.int8)])[:rep * n]
        groups = tuple(to(x) for x in index.groups(qh, qr, qt, qm))
        return dict(n=rep * n, host_qr=qr, dev=tuple(to(x) for x in (qh, qr, qt, qm)), groups=groups)

    sp_h = ScoreSpec(model="transh", ent=ent, rel=rel, dim=a.dim, norm_flag=True, pred_kind=0, norm_vec=nv)
    sp_e = ScoreSpec(model="transe", ent=ent, rel=rel, dim=a.dim, norm_flag=True, pred_kind=0)
    th, te = TransHSweep(sp_h), LinkSweep(sp_e)

    def timed(paths):
        """{name: ms per call} lists over the repetitions, the paths alternating within each."""
        with torch.no_grad():
            for p in paths.values():
                for _ in range(a.warmup):
                    p()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for _ in range(a.reps):
                for k, p in paths.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        p()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.iters)
        return times

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    def measure(q):
        plan = plan_tiles(q["host_qr"])
        bh, be = {}, te.alloc_queries(q["n"])
        sweep_ms = []

        def transe():
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            te.run(*q["dev"], filt=q["groups"], buffers=be, sweep_events=ev)
            sweep_ms.append(ev)

        t = timed({"transh": lambda: th.run(*q["dev"], filt=q["groups"], buffers=bh, plan=plan), "transe_f32": transe})
        torch.cuda.synchronize()
        sw = [x.elapsed_time(y) for x, y in sweep_ms[a.warmup:]]
        out = {k: summary(v) for k, v in t.items()}
        out["transe_sweep"] = summary(sw)
        out.update(queries=q["n"], tiles=int(len(plan["tiles"])), relations_used=int(len(plan["used"])),
                   padding=plan["padding"])
        out["transh_over_transe_f32"] = out["transh"]["median"] / out["transe_f32"]["median"]
        out["transh_over_P_transe_sweep"] = out["transh"]["median"] / (plan["padding"] * out["transe_sweep"]["median"])
        return out

    result = {"shape": {"entities": E, "relations": R, "dim": a.dim}, "iters": a.iters, "warmup": a.warmup,
              "reps": a.reps, "target_ratio": 1.15, "lib": _lib.lib_identity(), "torch": torch.__version__,
              "device": torch.cuda.get_device_name(0)}
    result["c2"] = measure(queries(w["test_h"], w["test_r"], w["test_t"]))
    if not a.no_extremes:
        n = len(w["test_h"])
        result["one_relation"] = measure(queries(w["test_h"], np.zeros(n, np.int64), w["test_t"]))
        first = np.unique(w["test_r"], return_index=True)[1]            # one test triple per relation
        result["one_query_per_tile"] = measure(queries(w["test_h"][first], w["test_r"][first], w["test_t"][first],
                                                               both=False))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
