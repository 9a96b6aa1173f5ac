"""Times triple classification at the FB15K237 shape (N = 20,466 test triples, E = 14,541,
R = 237, d = 200) for TransE (L1, norm_flag) and RotatE, tables and test list from mmre.workloads:

  fused     mmre_tc_evaluate into preallocated buffers: negatives, both prediction arrays and the
            threshold search enqueued by one call; and each stage alone through its own entry
            (mmre_tc_negatives, mmre_tc_scores, mmre_tc_threshold), between two device events
  composed  the same task from what the code before this feature had: mmre.ns.score_rows on the 2N
            rows (positives, then the same negatives, which that code could not draw: they are not
            timed), the copy of the 2N scores to the host, and the reference's threshold loop
            (Tester.py:93-112) restated in numpy (argsort, cumulative sums, argmax). Wall clock
            around a synchronised call, since two of its three parts run on the host.
  search    mmre_tc_threshold alone on random scores at 2N = 40,932 and at 2N = 120,000

Each repetition times `--iters` warmed-up calls. Prints one JSON line (median, min, max in ms)
and writes it to --out. Reads nothing outside the repository. No CPU path."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "multimodal-relation-extrapolation_amd"))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tripleclass_time: no GPU (there is no CPU path)")
    from mmre import _lib
    from mmre._lib import call, ptr, stream_ptr
    from mmre.data import TrainIndex
    from mmre.ns import NSSpec, score_rows
    from mmre.sampler import glibc_seeds
    from mmre.tripleclass import INDEX_KEYS, _model_args, device_index
    from mmre.workloads import FB15K237_TRAIN, workload_spec, zs_workload
    dev = torch.device("cuda:0")
    st = stream_ptr(dev)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    state = int(glibc_seeds(1)[0])

    def timed(fn, wall=False):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            if wall:
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3 / a.iters)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1) / a.iters)
        return {"median": statistics.median(out), "min": min(out), "max": max(out), "all": out}

    def reference_loop(score, ans):
        """get_best_threshlod without the Python loop: the same walk as array operations."""
        order = np.argsort(score)
        a_sorted = ans[order]
        cur = np.cumsum(a_sorted)
        total = float(len(score))
        res = (2.0 * cur + (total - cur[-1]) - np.arange(1, len(score) + 1)) / total
        i = int(np.argmax(res))
        return score[order][i], res[i]

    result = {"iters": a.iters, "warmup": a.warmup, "reps": a.reps, "lib": _lib.lib_identity(),
              "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "models": {}, "search": {}}
    for model in ("transe", "rotate"):
        w = zs_workload("FB15K-237-ZS", model, dim=a.dim)
        if model == "transe":
            w["norm_flag"] = True
        sp = workload_spec(w, dev)
        E, R, d = w["n_ent"], w["n_rel"], a.dim
        n_train = FB15K237_TRAIN
        index = TrainIndex(w["filter_h"][:n_train], w["filter_t"][:n_train], w["filter_r"][:n_train], E, R)
        D = device_index(index, dev)
        h, r, t = (to(w[k]) for k in ("test_h", "test_r", "test_t"))
        n = int(h.shape[0])
        neg_h, neg_t = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
        pos, neg = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        nbytes = int(_lib.lib().mmre_tc_threshold_workspace(n, n))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        c = lambda x: None if x is None else x.detach().contiguous().float()
        margs = _model_args(sp, c(sp.ent), c(sp.rel), c(sp.ent_im), c(sp.rel_im))
        iargs = tuple(ptr(D[k]) for k in INDEX_KEYS)
        paths = {
            "evaluate": lambda: call("mmre_tc_evaluate", *margs, *iargs, index.train_total, ptr(h), ptr(r), ptr(t), n,
                                     state, 0, 0.0, ptr(neg_h), ptr(neg_t), ptr(pos), ptr(neg), ptr(out), ptr(work),
                                     nbytes, st),
            "negatives": lambda: call("mmre_tc_negatives", *iargs, index.train_total, E, ptr(h), ptr(r), ptr(t), n,
                                      state, ptr(neg_h), ptr(neg_t), st),
            "scores": lambda: call("mmre_tc_scores", *margs, ptr(h), ptr(r), ptr(t), ptr(neg_h), None, ptr(neg_t), n,
                                   ptr(pos), ptr(neg), st),
            "threshold": lambda: call("mmre_tc_threshold", ptr(pos), n, ptr(neg), n, 0, 0.0, ptr(out), ptr(work),
                                      nbytes, st),
        }
        ms = {k: timed(p) for k, p in paths.items()}
        o = out.cpu().numpy()
        fused_thr = float(np.array([int(o[0])], np.uint32).view(np.float32)[0])
        # the composed path, on the same rows
        ns = (NSSpec("rotate", d, model_margin=w["margin"], phase_denom=sp.phase_denom) if model == "rotate"
              else NSSpec("transe", d, norm_flag=True))
        xh, xt, xr = torch.cat([h, neg_h]), torch.cat([t, neg_t]), torch.cat([r, r])
        ans = np.concatenate([np.ones(n, np.int64), np.zeros(n, np.int64)])
        last = {}

        def composed():
            with torch.no_grad():
                s = score_rows(ns, sp.ent, sp.rel, xh, xt, xr)
                s = -s if model == "rotate" else s
            last["thr"], last["acc"] = reference_loop(s.cpu().numpy(), ans)

        def rows_only():
            with torch.no_grad():
                score_rows(ns, sp.ent, sp.rel, xh, xt, xr)

        ms["composed_wall"] = timed(composed, wall=True)
        ms["evaluate_wall"] = timed(lambda: (paths["evaluate"](), out.cpu()), wall=True)
        ms["composed_score_rows"] = timed(rows_only)
        acc = float(_lib.lib().mmre_tc_accuracy(int(o[1]), int(o[2]), n, n))
        result["models"][model] = {"shape": {"n": n, "entities": E, "relations": R, "dim": d}, "ms": ms,
                                   "fused": {"threshold": fused_thr, "accuracy": acc, "n_nan": int(o[3])},
                                   "composed": {"threshold": float(last["thr"]), "accuracy": float(last["acc"])},
                                   "composed_over_fused_wall": ms["composed_wall"]["median"] /
                                   ms["evaluate_wall"]["median"]}
    rng = np.random.default_rng(0)
    for total in (40932, 120000):
        n = total // 2
        pos, neg = to(rng.normal(0.0, 1.0, n).astype(np.float32)), to(rng.normal(0.5, 1.0, n).astype(np.float32))
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        nbytes = int(_lib.lib().mmre_tc_threshold_workspace(n, n))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        fn = lambda: call("mmre_tc_threshold", ptr(pos), n, ptr(neg), n, 0, 0.0, ptr(out), ptr(work), nbytes, st)
        result["search"][str(total)] = dict(timed(fn), pairs=total * total)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
