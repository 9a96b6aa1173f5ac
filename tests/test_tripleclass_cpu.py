"""Triple classification, host side (no GPU): the Python restatements the GPU tests compare
against are themselves checked against the reference here (fixtures of
tests/golden/make_tripleclass.py: Base.so's getTestBatch, the reference models' predict and the
reference Tester's get_best_threshlod / run_triple_classification); the error codes of every
mmre_tc_* entry for arguments it refuses before any launch; the declarations and exports."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (the library binds to torch's HIP runtime)

from conftest import GOLDEN, PKG, REPO
from tc_restate import accuracy, counts_at, neg_test, search

CONFIGS = ["transe", "transe_nonorm_margin", "transe_l2", "distmult", "complex", "rotate"]
DATASETS = {"tripleclass_small": "small", "tripleclass_dense": "relpred"}
ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4

_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, aligned, never dereferenced


# ----------------------------------------------------------------- the restatements ----
@pytest.mark.parametrize("fixture", list(DATASETS))
@pytest.mark.parametrize("config", CONFIGS)
def test_restated_search_equals_the_reference_tester(golden, fixture, config):
    g = golden(fixture)
    pos, neg = g[f"{config}_pos"], g[f"{config}_neg"]
    T = int(g["T"])
    assert pos.dtype == np.float32 and pos.shape == neg.shape == (T,)
    thr, P, A, n_nan = search(pos, neg)
    ref_thr, res_mx = g[f"{config}_best"]
    assert n_nan == 0
    assert thr == ref_thr and accuracy(P, A, T, T) == res_mx, (thr, ref_thr, accuracy(P, A, T, T), res_mx)
    acc, run_thr = g[f"{config}_run"]
    assert run_thr == ref_thr
    assert accuracy(*counts_at(pos, neg, thr)[:2], T, T) == acc == float(g[f"{config}_run_given"])
    assert counts_at(pos, neg, thr)[:2] == (P, A)


@pytest.mark.parametrize("fixture", list(DATASETS))
def test_restated_negatives_equal_base_so(golden, fixture):
    from mmre.data import OpenKEDataset, TrainIndex
    g = golden(fixture)
    d = OpenKEDataset(os.path.join(GOLDEN, "data", DATASETS[fixture]))
    h, r, t = d.test_list()
    assert np.array_equal(h, g["pos_h"]) and np.array_equal(r, g["pos_r"]) and np.array_equal(t, g["pos_t"])
    index = TrainIndex(d.train[:, 0], d.train[:, 1], d.train[:, 2], d.n_ent, d.n_rel)
    state = int(g["state0"])
    for call in (1, 2):
        nh, nt, coin, absent, state = neg_test(index, h, r, t, state)
        mask = g[f"mask{call}"]
        assert np.array_equal(coin, g[f"coin{call}"]) and np.array_equal(absent, mask)
        assert state == int(g[f"state{call}"])
        assert np.array_equal(nh[~mask], g[f"neg{call}_h"][~mask])
        assert np.array_equal(nt[~mask], g[f"neg{call}_t"][~mask])
        assert np.all((nh >= 0) & (nh < d.n_ent) & (nt >= 0) & (nt < d.n_ent))
    assert int(g["mask1"].sum() + g["mask2"].sum()) <= 0.05 * 2 * len(h)
    if fixture == "tripleclass_small":
        assert g["mask1"].sum() == 1                       # the rule of the absent entity is exercised
        from mmre.sampler import glibc_seeds
        assert int(glibc_seeds(1)[0]) == int(g["state0"])  # a fresh randReset: the loader's default


def test_state_advance_is_two_draws_per_triple(golden):
    from mmre import _lib
    g = golden("tripleclass_small")
    L = _lib.lib()
    T = int(g["T"])
    assert L.mmre_tc_advance(int(g["state0"]), T) == int(g["state1"])
    assert L.mmre_tc_advance(int(g["state1"]), T) == int(g["state2"])
    assert L.mmre_tc_advance(12345, 0) == 12345
    from mmre.tripleclass import advance_state
    assert advance_state(int(g["state0"]), 2 * T) == int(g["state2"])


def test_accuracy_is_the_python_float():
    from mmre import _lib
    L = _lib.lib()
    for P, A, n_pos, n_neg in ((3, 5, 7, 11), (0, 0, 1, 1), (150, 201, 150, 150), (20466, 30000, 20466, 20466),
                               (1, 1, 1, 0)):
        assert L.mmre_tc_accuracy(P, A, n_pos, n_neg) == accuracy(P, A, n_pos, n_neg)
    assert np.isnan(L.mmre_tc_accuracy(0, 0, 0, 0))


# ----------------------------------------------------------------- the error contract ----
NEG = ("head_hrt", "tail_hrt", "lef_head", "rig_head", "lef_tail", "rig_tail", "train_total", "n_ent", "test_h",
       "test_r", "test_t", "n", "state", "neg_h", "neg_t", "stream")
SCORES = ("model", "norm_flag", "pred_kind", "margin", "ent", "ent_im", "rel", "rel_im", "n_ent", "n_rel", "dim",
          "phase_denom", "pos_h", "pos_r", "pos_t", "neg_h", "neg_r", "neg_t", "n", "pos_scores", "neg_scores", "stream")
THRESHOLD = ("pos_scores", "n_pos", "neg_scores", "n_neg", "have_threshold", "threshold", "out", "work", "work_bytes",
             "stream")
EVALUATE = SCORES[:12] + NEG[:7] + ("test_h", "test_r", "test_t", "n", "state", "have_threshold", "threshold",
                                    "neg_h", "neg_t", "pos_scores", "neg_scores", "out", "work", "work_bytes", "stream")
PARAMS = {"negatives": NEG, "scores": SCORES, "threshold": THRESHOLD, "evaluate": EVALUATE}
SCALARS = dict(model=0, norm_flag=1, pred_kind=0, margin=0.0, n_ent=40, n_rel=5, dim=16, phase_denom=0.0, n=9,
               train_total=100, state=7, n_pos=9, n_neg=9, have_threshold=0, threshold=0.0, work_bytes=1 << 40,
               stream=None)
OPTIONAL = {"ent_im", "rel_im", "neg_r"}


def run(name, **over):
    """Return code of mmre_tc_`name` at arguments it would accept, changed by `over`."""
    from mmre import _lib
    a = {p: (SCALARS[p] if p in SCALARS else (None if p in OPTIONAL else fake())) for p in PARAMS[name]}
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    return getattr(_lib.lib(), "mmre_tc_" + name)(*[a[p] for p in PARAMS[name]])


def test_signatures_cover_the_tables_above():
    from mmre import _lib
    for name, params in PARAMS.items():
        assert len(_lib.SIGNATURES["mmre_tc_" + name][1]) == len(params), name


@pytest.mark.parametrize("name", ["scores", "evaluate"])
def test_score_arguments(name):
    assert run(name, model=-1) == MODEL and run(name, model=5) == MODEL
    assert run(name, dim=513) == SHAPE and run(name, dim=0) == ARG and run(name, dim=-4) == ARG
    assert run(name, pred_kind=-1) == ARG and run(name, pred_kind=5) == ARG
    for p in ("ent", "rel", "pos_scores", "neg_scores", "neg_h", "neg_t"):
        assert run(name, **{p: None}) == ARG, p
    for p in (("pos_h", "pos_r", "pos_t") if name == "scores" else ("test_h", "test_r", "test_t")):
        assert run(name, **{p: None}) == ARG, p
    assert run(name, n=-1) == ARG and run(name, n_ent=0) == ARG and run(name, n_rel=0) == ARG
    assert run(name, n=1 << 31) == SHAPE
    assert run(name, model=3) == ARG                              # ComplEx without its imaginary tables
    assert run(name, model=3, ent_im=fake()) == ARG
    assert run(name, model=4) == ARG                              # RotatE without its phase scale
    assert run(name, model=4, phase_denom=float("nan")) == ARG
    assert run(name, model=9, dim=513, ent=None) == MODEL         # the model answers first, then the shape
    assert run(name, dim=513, ent=None) == SHAPE


@pytest.mark.parametrize("name", ["negatives", "evaluate"])
def test_negatives_arguments(name):
    for p in NEG[:6] + ("test_h", "test_r", "test_t", "neg_h", "neg_t"):
        assert run(name, **{p: None}) == ARG, p
    assert run(name, train_total=0) == ARG and run(name, train_total=-3) == ARG
    assert run(name, n_ent=2) == ARG                              # the absent-entity modulus is n_ent - 2
    assert run(name, n=-1) == ARG
    assert run(name, n=1 << 31) == SHAPE


@pytest.mark.parametrize("name", ["threshold", "evaluate"])
def test_threshold_arguments(name):
    from mmre import _lib
    L = _lib.lib()
    assert L.mmre_tc_threshold_workspace(9, 9) == 16 + 8 * 18
    assert L.mmre_tc_threshold_workspace(20466, 20466) == 16 + 8 * 40932
    assert L.mmre_tc_threshold_workspace(-1, 3) < 0 and L.mmre_tc_threshold_workspace((1 << 30) + 1, 0) < 0
    need = L.mmre_tc_threshold_workspace(9, 9)
    assert run(name, out=None) == ARG
    assert run(name, work=None) == ARG                            # a search needs its workspace
    assert run(name, work_bytes=need - 1) == WORKSPACE and run(name, work_bytes=0) == WORKSPACE
    if name == "threshold":
        assert run(name, n_pos=-1) == ARG and run(name, n_neg=-1) == ARG
        assert run(name, pos_scores=None) == ARG and run(name, neg_scores=None) == ARG
        assert run(name, n_pos=(1 << 30) + 1) == SHAPE and run(name, n_pos=1 << 29, n_neg=(1 << 29) + 1) == SHAPE
        assert run(name, n_pos=0, n_neg=0) == 0 and run(name, n_pos=0, n_neg=0, out=None, work=None) == 0


def test_n_zero_is_a_no_op():
    """Nothing is launched (the pointers are fakes): every entry returns MMRE_OK for an empty set."""
    assert run("negatives", n=0) == 0 and run("negatives", n=0, test_h=None, neg_h=None) == 0
    assert run("scores", n=0) == 0 and run("scores", n=0, pos_h=None, pos_scores=None) == 0
    assert run("evaluate", n=0) == 0 and run("evaluate", n=0, test_h=None, out=None, work=None) == 0
    assert run("negatives", n=0, n_ent=2) == ARG and run("scores", n=0, model=7) == MODEL   # still checked


# ------------------------------------------------------------ declarations and surface ----
def _header(name):
    txt = open(os.path.join(REPO, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_declare_and_libraries_export():
    hip = ctypes.CDLL(os.path.join(PKG, "mmre", "lib", "libmmre_hip.so"))
    names = ("mmre_tc_negatives", "mmre_tc_advance", "mmre_tc_scores", "mmre_tc_threshold_workspace",
             "mmre_tc_threshold", "mmre_tc_accuracy", "mmre_tc_evaluate")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, _header("mmre.h")), n
        assert hasattr(hip, n), n
    base = ctypes.CDLL(os.path.join(PKG, "mmre", "lib", "libmmre_base.so"))
    for n in ("getNegTest", "getTestBatch"):
        assert re.search(r"\bvoid\s+%s\s*\(" % n, _header("mmre_base.h")), n
        assert hasattr(base, n), n
    from mmre import _lib, base as mbase
    assert set(names) <= set(_lib.SIGNATURES)
    assert {"getNegTest", "getTestBatch"} <= set(mbase.SIGNATURES)


def test_the_not_implemented_notes_are_gone():
    for rel in ("include/mmre_base.h", "multimodal-relation-extrapolation_amd/csrc/base_compat.hip",
                "multimodal-relation-extrapolation_amd/openke/config/Tester.py",
                "multimodal-relation-extrapolation_amd/openke/data/TestDataLoader.py"):
        txt = open(os.path.join(REPO, rel)).read()
        assert "Not exported" not in txt and "not exported" not in txt and "NotImplementedError" not in txt, rel


def test_surface_has_the_reference_names():
    from openke.config import Tester
    from openke.data import TestDataLoader
    import mmre.tripleclass as tc
    for n in ("get_best_threshlod", "run_triple_classification"):
        assert callable(getattr(Tester, n)), n
    for n in ("classification_negatives", "best_threshold", "accuracy_at", "evaluate_triple_classification"):
        assert callable(getattr(tc, n)), n
    dl = TestDataLoader(os.path.join(GOLDEN, "data", "small") + "/", "link")
    assert len(dl) == dl.testTotal
    dl.set_sampling_mode("classification")
    assert len(dl) == dl.testTotal                # as upstream OpenKE's loader: the mode does not change it
    dl.set_seed_state(99)
    assert dl.get_seed_state() == 99
    dl.set_sampling_mode("nonsense")
    with pytest.raises(ValueError):
        next(iter(dl))
