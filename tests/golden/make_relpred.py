"""make_relpred.py -- relation-prediction fixtures from the REFERENCE itself.

Runs only in the build container (needs /root/reference and oracle/_ref/Base.so), on the CPU;
never on the GPU box. Nothing from the reference travels: only the numbers written to
tests/golden/relpred_{small,dense}.npz and the synthetic dataset tests/golden/data/relpred/.

What is executed from the reference: its OpenKE models' predict (TransE.py, DistMult.py,
ComplEx.py, RotatE.py) on the rows getRelBatch fills, and getRelBatch / testRel /
test_relation_prediction of its Base.so (Test.h:55-62, :194-228, :329-354). The per-triple raw
and filtered counts are the deltas of the float globals rel_rank / rel_filter_rank around each
testRel; the ten metric globals are read after test_relation_prediction.

initTest does not reset the rel_* globals (Test.h:29 declares shadowing locals), so they are
zeroed here before every configuration.

The dense dataset (E = 48, R = 70: the relations cross one wave's 64) draws its triples from a
small pool of (h, t) pairs, 1 to 12 relations each, so that most test triples have known
competing relations -- the `small` and `medium` sets have at most two relations per pair.

Usage:  python tests/golden/make_relpred.py
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
from make_golden import DATA, base_setup, import_openke, load_base  # noqa: E402

REL_GLOBALS = ["rel_filter_reci_rank", "rel_filter_rank", "rel_filter_tot", "rel3_filter_tot", "rel1_filter_tot",
               "rel_reci_rank", "rel_rank", "rel_tot", "rel3_tot", "rel1_tot"]  # {mrr,mr,hit10,hit3,hit1} x {filter,raw}
CONFIGS = [
    ("transe", dict(cls="TransE", kw=dict(dim=32, p_norm=1, norm_flag=True))),
    ("transe_nonorm_margin", dict(cls="TransE", kw=dict(dim=32, p_norm=1, norm_flag=False, margin=5.0))),
    ("transe_l2", dict(cls="TransE", kw=dict(dim=32, p_norm=2, norm_flag=True))),
    ("distmult", dict(cls="DistMult", kw=dict(dim=32))),
    ("complex", dict(cls="ComplEx", kw=dict(dim=24))),
    ("rotate", dict(cls="RotatE", kw=dict(dim=16, margin=6.0, epsilon=2.0))),
]
NEAR_REL = 1e-5


def write_dense_dataset(path, n_ent=48, n_rel=70, n_train=1500, n_valid=60, n_test=120, seed=5):
    """OpenKE-format dataset (first line = count, then `h t r`) whose (h, t) pairs carry 1..12
    relations each."""
    rng = np.random.default_rng(seed)
    os.makedirs(path, exist_ok=True)
    total = n_train + n_valid + n_test
    pairs, out = set(), []
    while len(out) < total:
        h, t = int(rng.integers(n_ent)), int(rng.integers(n_ent))
        if (h, t) in pairs:
            continue
        pairs.add((h, t))
        for r in rng.choice(n_rel, size=int(rng.integers(1, 13)), replace=False):
            out.append((h, t, int(r)))
    out = np.array(out[:total], np.int64)
    rng.shuffle(out)
    splits = {"train2id.txt": out[:n_train], "valid2id.txt": out[n_train:n_train + n_valid],
              "test2id.txt": out[n_train + n_valid:]}
    for name, arr in splits.items():
        with open(os.path.join(path, name), "w") as f:
            f.write(f"{len(arr)}\n")
            for h, t, r in arr:
                f.write(f"{h} {t} {r}\n")
    for name, n, tag in (("entity2id.txt", n_ent, "e"), ("relation2id.txt", n_rel, "r")):
        with open(os.path.join(path, name), "w") as f:
            f.write(f"{n}\n")
            for i in range(n):
                f.write(f"{tag}{i}\t{i}\n")
    with open(os.path.join(path, "type_constrain.txt"), "w") as f:  # Reader.h:266-317
        f.write(f"{n_rel}\n")
        for r in range(n_rel):
            for col in (0, 1):
                ids = sorted(set(out[out[:, 2] == r][:, col].tolist()))
                f.write(f"{r}\t{len(ids)}\t" + "\t".join(map(str, ids)) + "\n")
    # how hard the filter works: test triples whose pair has another known relation
    cnt = {}
    for h, t, _ in out:
        cnt[(h, t)] = cnt.get((h, t), 0) + 1
    per = np.array([cnt[(h, t)] for h, t, _ in splits["test2id.txt"]])
    print(f"dense dataset: {len(pairs)} pairs, relations per pair 1..{max(cnt.values())}, "
          f"{int((per > 1).sum())} of {len(per)} test triples with a known competing relation")
    assert (per > 1).sum() * 2 >= len(per)


def fset(lib, name, v=0.0):
    ctypes.c_float.in_dll(lib, name).value = v


def fget(lib, name):
    return ctypes.c_float.in_dll(lib, name).value


def relpred_fixture(lib, ok, path, tag):
    base_setup(lib, path)
    lib.getRelBatch.argtypes = [ctypes.c_void_p] * 3
    lib.testRel.argtypes = [ctypes.c_void_p]
    R, T = lib.getRelationTotal(), lib.getTestTotal()
    ph, pt, pr = (np.zeros(R, np.int64) for _ in range(3))
    res = {"E": lib.getEntityTotal(), "R": R, "T": T, "near_rel": np.float64(NEAR_REL)}
    for i, (name, cfg) in enumerate(CONFIGS):
        torch.manual_seed(500 + i)
        model = ok[cfg["cls"]](ent_tot=lib.getEntityTotal(), rel_tot=R, **cfg["kw"])
        for g in REL_GLOBALS:  # initTest leaves them (Test.h:29)
            fset(lib, g)
        lib.initTest()
        q, preds, counts = [], [], []
        for _ in range(T):
            lib.getRelBatch(ph.ctypes.data, pt.ctypes.data, pr.ctypes.data)
            assert np.array_equal(pr, np.arange(R))
            data = {"batch_h": torch.from_numpy(ph.copy()), "batch_t": torch.from_numpy(pt.copy()),
                    "batch_r": torch.from_numpy(pr.copy()), "mode": "normal"}
            s = np.ascontiguousarray(model.predict(data), dtype=np.float32)
            before = [fget(lib, "rel_rank"), fget(lib, "rel_filter_rank")]
            lib.testRel(s.ctypes.data)
            after = [fget(lib, "rel_rank"), fget(lib, "rel_filter_rank")]
            counts.append([int(round(a - b)) - 1 for a, b in zip(after, before)])
            q.append((int(ph[0]), int(pt[0])))
            preds.append(s)
        lib.test_relation_prediction()
        res[f"{name}_pred"] = np.stack(preds)
        res[f"{name}_counts"] = np.array(counts, np.int64).T.copy()          # (2, T): raw, filt
        res[f"{name}_metrics"] = np.array([fget(lib, g) for g in REL_GLOBALS], np.float32)
        for k, v in model.state_dict().items():
            res[f"{name}.{k}"] = v.detach().numpy().copy()
        res["qh"] = np.array([a for a, _ in q], np.int64)
        res["qt"] = np.array([b for _, b in q], np.int64)
    np.savez_compressed(os.path.join(HERE, f"relpred_{tag}.npz"), **res)
    print("relpred fixture", tag, "R", R, "T", T)


def main():
    write_dense_dataset(os.path.join(DATA, "relpred"))
    lib = load_base()
    ok = import_openke()
    relpred_fixture(lib, ok, os.path.join(DATA, "small"), "small")
    relpred_fixture(lib, ok, os.path.join(DATA, "relpred"), "dense")


if __name__ == "__main__":
    main()
