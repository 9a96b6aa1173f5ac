"""Triple classification on the GPU: the negatives (mmre_tc_negatives, libmmre_base's getTestBatch,
TestDataLoader('classification')), the fused predictions (mmre_tc_scores), the sort-free threshold
search (mmre_tc_threshold), the one-call evaluation and the Tester entries.

Exactness: negatives are compared with array_equal against Base.so's own output (fixtures of
tests/golden/make_tripleclass.py) wherever Base.so's is defined, and against the Python restatement
of Corrupt.h (tests/tc_restate.py, itself held to Base.so in test_tripleclass_cpu.py) where it is
not; predictions are bit-equal to mmre.ns.score_rows plus the model's transform; the search is
compared with `==` against the reference Tester's result on the reference's scores and against
the restated rule on synthetic arrays. Only the predictions against the reference's torch carry a
tolerance: 1e-4 x max(1, |ref|), the bound DESIGN.md §3 records for the canonical arithmetic."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG
from tc_restate import accuracy, counts_at, neg_test, search
from test_relpred_gpu import E, _fixture_tables, _random_tables, _same_bits, _specs, _to

pytestmark = pytest.mark.gpu

CONFIGS = ["transe", "transe_nonorm_margin", "transe_l2", "distmult", "complex", "rotate"]
DATASETS = {"tripleclass_small": "small", "tripleclass_dense": "relpred"}
# (d, N): d below one wave (idle lanes), one wave's multiple or not, the 1 / 2 / 4 / 8-chunk kernels,
# the largest; N = 1, fewer than one workgroup's waves, many workgroups with a ragged last one
SHAPES = [(24, 1), (32, 3), (100, 150), (200, 3), (512, 150), (24, 150)]
R = 13


def _dataset(fixture):
    from mmre.data import OpenKEDataset, TrainIndex
    d = OpenKEDataset(os.path.join(GOLDEN, "data", DATASETS[fixture]))
    return d, TrainIndex(d.train[:, 0], d.train[:, 1], d.train[:, 2], d.n_ent, d.n_rel)


def _expected_negatives(g, index, call):
    """Base.so's batch `call`, with the rule of the absent entity on the masked triples."""
    state = int(g["state0"]) if call == 1 else int(g["state1"])
    nh, nt, _, absent, after = neg_test(index, g["pos_h"], g["pos_r"], g["pos_t"], state)
    mask = g[f"mask{call}"]
    assert np.array_equal(absent, mask) and after == int(g[f"state{call}"])
    eh, et = g[f"neg{call}_h"].copy(), g[f"neg{call}_t"].copy()
    eh[mask], et[mask] = nh[mask], nt[mask]
    return eh, et


# ------------------------------------------------------------------------ negatives ----
@pytest.mark.parametrize("fixture", list(DATASETS))
def test_engine_negatives_equal_base_so(golden, fixture):
    from mmre.tripleclass import advance_state, classification_negatives
    g = golden(fixture)
    d, index = _dataset(fixture)
    h, r, t = d.test_list()
    state = int(g["state0"])
    for call in (1, 2):
        nh, nt = classification_negatives(index, h, r, t, state, device="cuda:0")
        eh, et = _expected_negatives(g, index, call)
        assert np.array_equal(nh.cpu().numpy(), eh) and np.array_equal(nt.cpu().numpy(), et)
        state = advance_state(state, len(h))
        assert state == int(g[f"state{call}"])


@pytest.mark.parametrize("fixture", list(DATASETS))
def test_loader_negatives_equal_base_so(golden, fixture):
    from openke.data import TestDataLoader
    g = golden(fixture)
    _, index = _dataset(fixture)
    dl = TestDataLoader(os.path.join(GOLDEN, "data", DATASETS[fixture]) + "/", "classification")
    if fixture == "tripleclass_small":
        assert dl.get_seed_state() == int(g["state0"])      # the default: a fresh randReset
    dl.set_seed_state(int(g["state0"]))
    for call in (1, 2):
        batches = list(dl)
        assert len(batches) == 1 and len(batches[0]) == 2
        pos, neg = batches[0]
        eh, et = _expected_negatives(g, index, call)
        for b in (pos, neg):
            assert b["mode"] == "normal" and all(b[k].dtype == np.int64 for k in ("batch_h", "batch_t", "batch_r"))
        assert np.array_equal(pos["batch_h"], g["pos_h"]) and np.array_equal(pos["batch_t"], g["pos_t"])
        assert np.array_equal(pos["batch_r"], g["pos_r"]) and np.array_equal(neg["batch_r"], g["pos_r"])
        assert np.array_equal(neg["batch_h"], eh) and np.array_equal(neg["batch_t"], et)
        assert dl.get_seed_state() == int(g[f"state{call}"])
    dl.set_sampling_mode("link")                             # 'link' still iterates as before
    first = next(iter(dl))
    assert [b["mode"] for b in first] == ["head_batch", "tail_batch"] and len(dl) == dl.testTotal
    assert first[0]["batch_h"].shape == (dl.entTotal,) and int(first[0]["batch_t"][0]) == int(g["pos_t"][0])


def _base(ds, state0):
    """libmmre_base with `ds` imported and work thread 0 reseeded to state0: the process's rand()
    stream restarted and advanced to the draw that equals it."""
    import ctypes
    from mmre import base
    from mmre.sampler import glibc_seeds
    skip = next(k for k in range(8) if int(glibc_seeds(1, skip=k)[0]) == state0)
    L = base.load()
    L.mmre_base_clear_error()
    L.setInPath((os.path.join(GOLDEN, "data", ds) + "/").encode())
    L.setWorkThreads(1)
    L.importTrainFiles()
    L.importTestFiles()
    libc = ctypes.CDLL(None)
    libc.srand(1)
    for _ in range(skip):
        libc.rand()
    L.randReset()
    return L


@pytest.mark.parametrize("fixture", list(DATASETS))
def test_base_abi_get_test_batch_equals_base_so(golden, fixture):
    from mmre import base
    g = golden(fixture)
    _, index = _dataset(fixture)
    L = _base(DATASETS[fixture], int(g["state0"]))
    T = L.getTestTotal()
    assert T == int(g["T"])
    for call in (1, 2):                                      # the second call: thread 0's state advanced
        a = [np.full(T, 7, np.int64) for _ in range(6)]
        L.getTestBatch(*[x.ctypes.data for x in a])
        assert base.last_error() == (0, "")
        ph, pt, pr, nh, nt, nr = a
        eh, et = _expected_negatives(g, index, call)
        assert np.array_equal(ph, g["pos_h"]) and np.array_equal(pt, g["pos_t"]) and np.array_equal(pr, g["pos_r"])
        assert np.array_equal(nr, pr) and np.array_equal(nh, eh) and np.array_equal(nt, et)


def test_tiny_dataset_pins_the_quirks():
    """E = 6, ten train triples: a test head that is no train head, a test tail that is no train
    tail, and a relation below, between and above the kept entity's relations, on both sides."""
    from mmre.data import TrainIndex
    from mmre.tripleclass import classification_negatives
    train = np.array([(0, 1, 1), (0, 1, 2), (0, 3, 4), (1, 2, 0), (1, 2, 3), (2, 0, 4), (2, 4, 1), (2, 4, 3),
                      (3, 1, 0), (5, 2, 1)], np.int64)                       # (h, r, t)
    index = TrainIndex(train[:, 0], train[:, 2], train[:, 1], 6, 5)
    assert index.rig_head[4] < index.lef_head[4] and index.rig_tail[5] < index.lef_tail[5]
    # head 0 has relations {1, 3}; tail 1 has {1, 2, 4}; tail 0 has {1, 2}
    cases = [(0, 0, 1), (0, 2, 1), (0, 4, 0), (0, 1, 0), (0, 3, 1), (4, 1, 1), (4, 0, 0), (0, 2, 5), (1, 3, 5),
             (2, 3, 1), (3, 4, 0), (4, 2, 5), (2, 0, 1)]
    test = np.array(cases * 4, np.int64)
    h, r, t = test[:, 0], test[:, 1], test[:, 2]
    seen = set()
    for state in (1804289383, 846930886, 5, (1 << 63) + 12345):
        nh, nt = classification_negatives(index, h, r, t, state, device="cuda:0")
        eh, et, coin, absent, _ = neg_test(index, h, r, t, state)
        assert np.array_equal(nh.cpu().numpy(), eh) and np.array_equal(nt.cpu().numpy(), et), state
        # (an empty block between two rows whose values descend shifts a draw of E - 1 to E, as in
        # the reference: such a negative is out of range and scores NaN)
        assert np.all((eh >= 0) & (eh <= 6) & (et >= 0) & (et <= 6))
        for i in range(len(h)):
            rels = sorted(set(train[train[:, 0] == h[i], 1]) if coin[i] else set(train[train[:, 2] == t[i], 1]))
            kind = ("absent" if absent[i] else "below" if r[i] < rels[0] else "above" if r[i] > rels[-1]
                    else "present" if r[i] in rels else "between")
            seen.add((bool(coin[i]), kind))
    assert seen == {(c, k) for c in (True, False) for k in ("absent", "below", "between", "above", "present")}, seen


# ---------------------------------------------------------------------- predictions ----
def _tc_scores(sp, ph, pr, pt, nh, nt, nr=None):
    from mmre.tripleclass import classification_scores
    pos, neg = classification_scores(sp, ph, pr, pt, nh, nt, neg_r=nr)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), neg.cpu().numpy()


def _predict(sp, ns, tr, h, r, t):
    from mmre.ns import score_rows
    with torch.no_grad():
        s = tr(score_rows(ns, sp.ent, sp.rel, _to(h), _to(t), _to(r), ent_im=sp.ent_im, rel_im=sp.rel_im))
    return s.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_N%d" % s)
@pytest.mark.parametrize("config", CONFIGS)
def test_scores_bit_equal_to_predict(config, shape):
    d, N = shape
    sp, ns, tr = _specs(config, *_random_tables(config, R, d, seed=1000 + d))
    rng = np.random.default_rng(N + d)
    ph, pt, pr = rng.integers(0, E, N), rng.integers(0, E, N), rng.integers(0, R, N)
    side = rng.integers(0, 2, N).astype(bool)                 # which entity the negative replaces
    nh = np.where(side, rng.integers(0, E, N), ph)
    nt = np.where(side, pt, rng.integers(0, E, N))
    pos, neg = _tc_scores(sp, ph, pr, pt, nh, nt)
    assert _same_bits(pos, _predict(sp, ns, tr, ph, pr, pt))
    assert _same_bits(neg, _predict(sp, ns, tr, nh, pr, nt))
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(neg))
    # negatives that share nothing with their positive, relation included
    nh2, nt2, nr2 = rng.integers(0, E, N), rng.integers(0, E, N), rng.integers(0, R, N)
    pos2, neg2 = _tc_scores(sp, ph, pr, pt, nh2, nt2, nr2)
    assert _same_bits(pos2, pos) and _same_bits(neg2, _predict(sp, ns, tr, nh2, nr2, nt2))


@pytest.mark.parametrize("config", CONFIGS)
def test_out_of_range_ids_score_nan_and_read_nothing(config):
    d, N = 40, 12
    sp, ns, tr = _specs(config, *_random_tables(config, R, d, seed=5))
    rng = np.random.default_rng(9)
    ph, pt, pr = rng.integers(0, E, N), rng.integers(0, E, N), rng.integers(0, R, N)
    nh, nt = ph.copy(), rng.integers(0, E, N)
    ph[0], pt[1], pr[2] = -1, E, R                             # positives out of range (row 2: both rows)
    nh[0] = 3                                                  # ... its negative is still scored
    nh[3], nt[4] = E + 7, -5                                   # negatives out of range
    ph[5], nt[5] = 1 << 40, -(1 << 40)                         # both
    pos, neg = _tc_scores(sp, ph, pr, pt, nh, nt)
    bad_p = np.isin(np.arange(N), [0, 1, 2, 5])
    bad_n = np.isin(np.arange(N), [2, 3, 4, 5])
    assert np.all(np.isnan(pos[bad_p])) and np.all(np.isnan(neg[bad_n]))
    ok = ~bad_p
    assert _same_bits(pos[ok], _predict(sp, ns, tr, ph[ok], pr[ok], pt[ok]))
    ok = ~bad_n
    assert _same_bits(neg[ok], _predict(sp, ns, tr, nh[ok], pr[ok], nt[ok]))


@pytest.mark.parametrize("fixture", list(DATASETS))
@pytest.mark.parametrize("config", CONFIGS)
def test_scores_against_the_reference_predict(golden, fixture, config):
    g = golden(fixture)
    sp, _, _ = _specs(config, *_fixture_tables(g, config))
    pos, neg = _tc_scores(sp, g["pos_h"], g["pos_r"], g["pos_t"], g["neg1_h"], g["neg1_t"])
    _, neg2 = _tc_scores(sp, g["pos_h"], g["pos_r"], g["pos_t"], g["neg2_h"], g["neg2_t"])
    for got, name in ((pos, "pos"), (neg, "neg"), (neg2, "neg2")):
        ref = g[f"{config}_{name}"].astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{fixture}/{config}/{name}: max err {err.max():.3g}, max err / max(1, |ref|) "
              f"{(err / np.maximum(1.0, np.abs(ref))).max():.3g}")
        assert np.all(err <= 1e-4 * np.maximum(1.0, np.abs(ref))), float(err.max())


# --------------------------------------------------------------------------- search ----
def _gpu_search(pos, neg):
    from mmre.tripleclass import best_threshold
    res = best_threshold(np.asarray(pos, np.float32), np.asarray(neg, np.float32))
    return res["threshold"], res["P"], res["A"], res["n_nan"], res["accuracy"]


def _same_result(got, exp, n_pos, n_neg):
    thr, P, A, n_nan, acc = got
    ethr, eP, eA, enan = exp
    assert (thr == ethr or (thr != thr and ethr != ethr)) and (P, A, n_nan) == (eP, eA, enan), (got, exp)
    if n_pos + n_neg:
        assert acc == accuracy(eP, eA, n_pos, n_neg)


@pytest.mark.parametrize("fixture", list(DATASETS))
@pytest.mark.parametrize("config", CONFIGS)
def test_search_on_reference_scores_equals_the_reference_tester(golden, fixture, config):
    from mmre.tripleclass import accuracy_at
    from openke.config import Tester
    g = golden(fixture)
    pos, neg = g[f"{config}_pos"], g[f"{config}_neg"]
    T = len(pos)
    ref_thr, res_mx = g[f"{config}_best"]
    thr, P, A, n_nan, acc = _gpu_search(pos, neg)
    assert thr == ref_thr and acc == res_mx and n_nan == 0, (thr, ref_thr, acc, res_mx)
    score = np.concatenate([pos, neg])
    ans = np.concatenate([np.ones(T, np.int64), np.zeros(T, np.int64)])
    perm = np.random.default_rng(1).permutation(2 * T)        # generic in `ans`: any interleaving
    t2, mx2 = Tester().get_best_threshlod(score[perm], ans[perm])
    assert t2 == ref_thr and mx2 == res_mx
    run_acc, run_thr = g[f"{config}_run"]
    at = accuracy_at(pos, neg, thr)
    assert run_thr == ref_thr and at["accuracy"] == run_acc == float(g[f"{config}_run_given"])
    assert (at["P"], at["A"]) == (P, A)


def _synthetic(case):
    rng = np.random.default_rng(sum(case) if isinstance(case, tuple) else zlib.crc32(case.encode()))
    f = lambda a: np.asarray(a, np.float32)
    if isinstance(case, tuple):
        return f(rng.normal(0.0, 1.0, case[0])), f(rng.normal(0.4, 1.0, case[1]))
    if case == "mixed_ties":          # few distinct values: every group mixes both labels
        return f(rng.integers(-3, 4, 300) * 0.5), f(rng.integers(-2, 5, 280) * 0.5)
    if case == "equal_maxima":        # 2 P - A is 1 at -1 and again at 2: the smaller wins
        return f([-1.0, 1.0, 2.0]), f([0.0, 1.5])
    if case == "zeros":               # -0 and +0 are one group, reported as +0
        return f([-0.0, 0.0, 0.0, 5.0]), f([-0.0, 3.0, 1.0])
    if case == "infs":
        return f([-np.inf, 0.5, np.inf, -np.inf]), f([np.inf, -np.inf, 0.25, np.inf])
    if case == "nans":
        p, n = f(rng.normal(0, 1, 70)), f(rng.normal(0.3, 1, 90))
        p[[0, 13, 69]], n[[5, 64]] = np.nan, np.nan
        return p, n
    if case == "all_nan":
        return f([np.nan, np.nan]), f([np.nan])
    if case == "separable":           # all positives above all negatives: the worst order for `<=`
        return f(rng.uniform(2.0, 3.0, 130)), f(rng.uniform(-1.0, 1.0, 140))
    if case == "separable_below":     # all positives below all negatives: accuracy 1
        return f(rng.uniform(-3.0, -2.0, 130)), f(rng.uniform(-1.0, 1.0, 140))
    raise KeyError(case)


# (20000, 21000): 41 workgroups of candidates x 21 chunks of the score stream, two LDS tiles each
SEARCH_CASES = [(1, 1), (1, 0), (0, 1), (63, 65), (64, 64), (257, 1031), (20000, 21000), "mixed_ties",
                "equal_maxima", "zeros", "infs", "nans", "all_nan", "separable", "separable_below"]


@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "%dx%d" % c if isinstance(c, tuple) else c)
def test_search_equals_the_restated_rule(case):
    from mmre.tripleclass import accuracy_at
    pos, neg = _synthetic(case)
    exp = search(pos, neg)
    got = _gpu_search(pos, neg)
    _same_result(got, exp, len(pos), len(neg))
    again = _gpu_search(pos, neg)                             # identical from run to run
    assert np.array_equal(np.array(got), np.array(again), equal_nan=True), (got, again)
    if case == "equal_maxima":
        assert got[0] == -1.0 and (got[1], got[2]) == (1, 1)
    if case == "zeros":
        assert got[0] == 0.0 and not np.signbit(np.float32(got[0])) and (got[1], got[2]) == (3, 4)
    if case == "separable_below":
        assert got[4] == 1.0
    if case == "all_nan":
        assert got[0] != got[0] and got[1:4] == (0, 0, 3)
    # a given threshold: below every score, above every score, equal to a (tied) score, NaN
    finite = np.concatenate([pos, neg])
    finite = finite[np.isfinite(finite)]
    thrs = [-np.inf, np.inf, float("nan")]
    if len(finite):
        thrs += [float(finite.min()) - 1.0, float(finite.max()) + 1.0, float(np.sort(finite)[len(finite) // 2])]
    for thr in thrs:
        at = accuracy_at(pos, neg, thr)
        P, A, n_nan = counts_at(pos, neg, thr)
        assert (at["P"], at["A"], at["n_nan"]) == (P, A, n_nan), (thr, at)
        assert at["accuracy"] == accuracy(P, A, len(pos), len(neg))
    if len(finite) and case != "infs":                        # no score above the threshold: A = all non-NaN
        at = accuracy_at(pos, neg, float(finite.max()) + 1.0)
        assert at["A"] == len(finite) and at["P"] == int(np.isfinite(pos).sum())


# -------------------------------------------------------------------------- surface ----
@pytest.mark.parametrize("cls,kw", [("TransE", dict(dim=32, p_norm=1, norm_flag=True)),
                                     ("RotatE", dict(dim=16, margin=6.0, epsilon=2.0))])
def test_tester_run_triple_classification(golden, cls, kw):
    import openke.module.model as models
    from mmre.tripleclass import evaluate_triple_classification
    from openke.config import Tester
    from openke.data import TestDataLoader
    g = golden("tripleclass_small")
    path = os.path.join(GOLDEN, "data", "small") + "/"
    torch.manual_seed(21)
    dl = TestDataLoader(path, "link")
    model = getattr(models, cls)(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), **kw)
    tester = Tester(model=model, data_loader=dl, use_gpu=True)
    state0 = dl.get_seed_state()
    acc, thr = tester.run_triple_classification()             # NotImplementedError before this feature
    last = tester.last
    T = dl.testTotal
    assert dl.get_seed_state() == int(g["state1"]) and state0 == int(g["state0"])
    _, index = _dataset("tripleclass_small")
    eh, et = _expected_negatives(g, index, 1)
    assert np.array_equal(last["neg_h"], eh) and np.array_equal(last["neg_t"], et)
    # the engine's result from the same state
    res = evaluate_triple_classification(model.score_spec(), dl.test_h, dl.test_r, dl.test_t, dl.train_index(),
                                         state0)
    assert (acc, thr) == (res["accuracy"], res["threshold"])
    assert _same_bits(res["pos_scores"], last["pos_scores"]) and _same_bits(res["neg_scores"], last["neg_scores"])
    # the scores are model.predict's on the loader's rows
    pred = lambda h, t: model.predict({"batch_h": h, "batch_t": t, "batch_r": dl.test_r, "mode": "normal"})
    assert _same_bits(last["pos_scores"], np.asarray(pred(dl.test_h, dl.test_t), np.float32))
    assert _same_bits(last["neg_scores"], np.asarray(pred(eh, et), np.float32))
    # ... and the result is the restated rule on them
    ethr, eP, eA, enan = search(last["pos_scores"], last["neg_scores"])
    assert thr == ethr and (last["P"], last["A"], last["n_nan"]) == (eP, eA, enan)
    assert acc == accuracy(eP, eA, T, T)
    t2, mx2 = tester.get_best_threshlod(np.concatenate([last["pos_scores"], last["neg_scores"]]),
                                        np.concatenate([np.ones(T), np.zeros(T)]))
    assert (t2, mx2) == (thr, acc)
    # a given threshold: the same accuracy (on the same negatives: the state set back)
    dl.set_seed_state(state0)
    acc2, thr2 = tester.run_triple_classification(threshlod=thr)
    assert (acc2, thr2) == (acc, thr) and dl.get_seed_state() == int(g["state1"])
    # 'link' afterwards still iterates as before
    dl.set_sampling_mode("link")
    first = next(iter(dl))
    assert [b["mode"] for b in first] == ["head_batch", "tail_batch"]


def test_get_test_batch_before_import_train_files_latches():
    """In a fresh process (the library's state is global): getTestBatch without importTrainFiles is
    refused before any GPU work, the error is latched and the six outputs are poisoned with -1."""
    so = os.path.join(PKG, "mmre", "lib", "libmmre_base.so")
    code = (
        "import ctypes, numpy as np, torch\n"
        "L = ctypes.CDLL(%r)\n"
        "L.setInPath.argtypes = [ctypes.c_char_p]\n"
        "L.getTestBatch.argtypes = [ctypes.c_void_p] * 6\n"
        "L.getTestTotal.restype = ctypes.c_int64\n"
        "L.mmre_base_last_error.argtypes = [ctypes.c_char_p, ctypes.c_int]\n"
        "L.mmre_base_set_error_mode(1)\n"
        "L.setInPath(%r)\n"
        "L.importTestFiles()\n"
        "L.randReset()\n"
        "T = L.getTestTotal()\n"
        "a = [np.full(T, 7, np.int64) for _ in range(6)]\n"
        "L.getTestBatch(*[x.ctypes.data for x in a])\n"
        "buf = ctypes.create_string_buffer(256)\n"
        "code = L.mmre_base_last_error(buf, 256)\n"
        "print('RESULT', T, code, all(bool(np.all(x == -1)) for x in a), buf.value.decode())\n"
        % (so, (os.path.join(GOLDEN, "data", "small") + "/").encode()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = next(l for l in r.stdout.splitlines() if l.startswith("RESULT"))
    assert line.startswith("RESULT 150 1 True") and "importTrainFiles" in line, line
