"""make_tripleclass.py -- triple-classification fixtures from the REFERENCE itself.

Runs only in the build container (needs /root/reference and oracle/_ref/Base.so), on the CPU;
never on the GPU box. Nothing from the reference travels: only the numbers written to
tests/golden/tripleclass_{small,dense}.npz, for the datasets data/small and data/relpred.

What is executed from the reference: getTestBatch of its Base.so (Test.h:393-422) twice in a row
from a fresh randReset, with thread 0's state (next_random[0]) read before and after each call; its
OpenKE models' predict (TransE.py, DistMult.py, ComplEx.py, RotatE.py) on the positive and the
negative rows; and its own Tester.get_best_threshlod / run_triple_classification (Tester.py:93-151)
on those scores. The Tester is made with __new__ (its __init__ wants release/Base.so), with a
loader object that yields the batch once.

Per file:
  state0, state1, state2            thread 0's state before the first call and after each call
  pos_h/r/t, neg1_h/t, neg2_h/t     getTestBatch's output of the two calls (nr == pr, asserted)
  coin1, coin2                      per triple: True when the tail was replaced (kept entity: h)
  mask1, mask2                      per triple: the kept entity never occurs on that side of a train
                                    triple, where Corrupt.h reads trainHead[-1] / trainTail[-1]
  per configuration c of make_relpred.CONFIGS: the tables (c.<state_dict key>), c_pos, c_neg (the
  model's predict on the first batch), c_neg2 (on the second batch's negatives), c_best =
  (threshlod, res_mx) and c_run = (acc, threshlod) of the reference's Tester, c_run_given = acc of
  its run_triple_classification(threshlod).

Asserted here: at most 5 % of a dataset's test-triple sides are out of range. The 2N reference
scores of a configuration are NOT all distinct on these datasets: getNegTest filters against train
only, so a negative can be another test triple (2 such rows in `small`, 4 in `relpred`, counted in
repeated_rows), and TransE scores every row with h == t by its relation alone (c_ties counts the
scores that repeat another). What is asserted instead is what distinctness was for: the reference's
walk gives the same (threshlod, res_mx) with the positives first and with the negatives first
inside every group of equal scores, and that is its own result -- so its unstable argsort does not
matter and its result is the one any correct search gives. The model seed of a configuration is
the first of 700 + i, 800 + i, ... at which that holds (c_seed).

Usage:  python tests/golden/make_tripleclass.py
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import DATA, REF, base_setup, import_openke, load_base, seeds_now  # noqa: E402
from make_relpred import CONFIGS  # noqa: E402

MASK = (1 << 64) - 1


def lcg_next(s):
    return (s * 25214903917 + 11) & MASK


def read_train(path):
    with open(os.path.join(path, "train2id.txt")) as f:
        n = int(f.readline())
        a = np.array([list(map(int, f.readline().split())) for _ in range(n)], np.int64)
    return a[:, 0], a[:, 1]          # heads, tails ("h t r" lines)


def coins_and_mask(state, h, t, train_heads, train_tails):
    """The coin of every triple (two draws each) and whether the kept entity is absent."""
    hs, ts = set(train_heads.tolist()), set(train_tails.tolist())
    coin, mask = np.zeros(len(h), bool), np.zeros(len(h), bool)
    for i in range(len(h)):
        state = lcg_next(state)
        coin[i] = state % 1000 < 500
        mask[i] = (int(h[i]) not in hs) if coin[i] else (int(t[i]) not in ts)
        state = lcg_next(state)
    return coin, mask, state


def walk(score, ans, positives_first):
    """Tester.py:93-112 with the order inside a group of equal scores fixed."""
    order = np.lexsort((-ans if positives_first else ans, score))
    total, cur, false = float(len(score)), 0.0, float(len(score)) - float(np.sum(ans))
    res_mx, thr = 0.0, None
    for index, j in enumerate(order):
        if ans[j] == 1:
            cur += 1.0
        res_current = (2 * cur + false - index - 1) / total
        if res_current > res_mx:
            res_mx, thr = res_current, np.float64(score[j])
    return thr, res_mx


class OnceLoader:
    def __init__(self, batch):
        self.batch = batch

    def set_sampling_mode(self, mode):
        assert mode == "classification"

    def __iter__(self):
        yield self.batch


def reference_tester(lib, model, batch):
    sys.path.insert(0, os.path.join(REF, "OpenKE"))
    from openke.config.Tester import Tester
    t = Tester.__new__(Tester)
    t.lib, t.model, t.data_loader, t.use_gpu = lib, model, OnceLoader(batch), False
    return t


def tripleclass_fixture(lib, ok, path, tag):
    base_setup(lib, path)
    lib.getTestBatch.argtypes = [ctypes.c_void_p] * 6
    E, R, T = lib.getEntityTotal(), lib.getRelationTotal(), lib.getTestTotal()
    th, tt = read_train(path)
    res = {"E": E, "R": R, "T": T}
    res["state0"] = np.uint64(seeds_now(lib, 1)[0])
    state = int(res["state0"])
    for call in (1, 2):
        a = [np.zeros(T, np.int64) for _ in range(6)]
        lib.getTestBatch(*[x.ctypes.data for x in a])
        ph, pt, pr, nh, nt, nr = a
        assert np.array_equal(nr, pr)
        coin, mask, state = coins_and_mask(state, ph, pt, th, tt)
        after = int(seeds_now(lib, 1)[0])
        assert after == state, "two draws per test triple"
        assert np.array_equal(nh[coin], ph[coin]) and np.array_equal(nt[~coin], pt[~coin])
        res[f"state{call}"] = np.uint64(after)
        res[f"neg{call}_h"], res[f"neg{call}_t"] = nh, nt
        res[f"coin{call}"], res[f"mask{call}"] = coin, mask
        if call == 1:
            res["pos_h"], res["pos_r"], res["pos_t"] = ph, pr, pt
    hs, ts = set(th.tolist()), set(tt.tolist())
    out_sides = sum(int(h) not in hs for h in res["pos_h"]) + sum(int(t) not in ts for t in res["pos_t"])
    print(f"{tag}: {out_sides} of {2 * T} test-triple sides out of range, "
          f"{int(res['mask1'].sum())} / {int(res['mask2'].sum())} chosen in the two batches")
    assert out_sides * 20 <= 2 * T
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    rows = np.concatenate([np.stack([res["pos_h"], res["pos_r"], res["pos_t"]], 1),
                           np.stack([res["neg1_h"], res["pos_r"], res["neg1_t"]], 1)])
    n_same = 2 * T - len(np.unique(rows, axis=0))
    print(f"{tag}: {n_same} rows of the first batch repeat another row (a negative that is a test triple)")
    res["repeated_rows"] = np.int64(n_same)
    pos = {"batch_h": res["pos_h"], "batch_t": res["pos_t"], "batch_r": res["pos_r"], "mode": "normal"}
    neg = {"batch_h": res["neg1_h"], "batch_t": res["neg1_t"], "batch_r": res["pos_r"], "mode": "normal"}
    ans = np.concatenate([np.ones(T, np.int64), np.zeros(T, np.int64)])
    for i, (name, cfg) in enumerate(CONFIGS):
        # the first seed at which equal scores do not decide the reference's result: its walk gives
        # the same answer with the positives first and with the negatives first inside every group
        for seed in range(700 + i, 700 + i + 2000, 100):
            torch.manual_seed(seed)
            model = ok[cfg["cls"]](ent_tot=E, rel_tot=R, **cfg["kw"])
            pred = lambda d: np.ascontiguousarray(
                model.predict({k: (to(v) if k != "mode" else v) for k, v in d.items()}), dtype=np.float32)
            sp, sn = pred(pos), pred(neg)
            both = np.concatenate([sp, sn])
            assert np.all(np.isfinite(both))
            if walk(both, ans, True) == walk(both, ans, False):
                break
        else:
            raise AssertionError(f"{tag}/{name}: the ties matter at every seed")
        res[f"{name}_ties"] = np.int64(2 * T - len(np.unique(both)))
        sn2 = pred(dict(neg, batch_h=res["neg2_h"], batch_t=res["neg2_t"]))
        res[f"{name}_seed"] = np.int64(seed)
        tester = reference_tester(lib, model, [pos, neg])
        thr, res_mx = tester.get_best_threshlod(both, ans)
        assert walk(both, ans, True) == walk(both, ans, False) == (thr, res_mx), f"{tag}/{name}: the ties matter"
        acc, thr_run = tester.run_triple_classification()
        acc_given, thr_given = tester.run_triple_classification(threshlod=thr_run)
        assert thr_given == thr_run == thr
        res[f"{name}_pos"], res[f"{name}_neg"], res[f"{name}_neg2"] = sp, sn, sn2
        res[f"{name}_best"] = np.array([thr, res_mx], np.float64)
        res[f"{name}_run"] = np.array([acc, thr_run], np.float64)
        res[f"{name}_run_given"] = np.float64(acc_given)
        for k, v in model.state_dict().items():
            res[f"{name}.{k}"] = v.detach().numpy().copy()
        print(f"  {name}: threshlod {thr:.6g} res_mx {res_mx:.6f} acc {acc:.6f}")
    np.savez_compressed(os.path.join(HERE, f"tripleclass_{tag}.npz"), **res)
    print("tripleclass fixture", tag, "E", E, "R", R, "T", T)


def main():
    lib = load_base()
    ok = import_openke()
    tripleclass_fixture(lib, ok, os.path.join(DATA, "small"), "small")
    tripleclass_fixture(lib, ok, os.path.join(DATA, "relpred"), "dense")


if __name__ == "__main__":
    main()
