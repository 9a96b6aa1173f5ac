"""Relation prediction, host side (no GPU): the C declarations and exports, the known-relation
index, the Test.h metric reduction against the reference's own globals (fixtures made by
tests/golden/make_relpred.py from the reference's Base.so: getRelBatch -> predict -> testRel ->
test_relation_prediction), and the Tester entry."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO

CONFIGS = ["transe", "transe_nonorm_margin", "transe_l2", "distmult", "complex", "rotate"]
FIXTURES = ["relpred_small", "relpred_dense"]
DATASETS = {"relpred_small": "small", "relpred_dense": "relpred"}


def _header(name):
    txt = open(os.path.join(REPO, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_declare_and_libraries_export():
    hip = ctypes.CDLL(os.path.join(PKG, "mmre", "lib", "libmmre_hip.so"))
    for n in ("mmre_rel_workspace", "mmre_rel_evaluate", "mmre_rel_metrics"):
        assert re.search(r"\b%s\s*\(" % n, _header("mmre.h")), n
        assert hasattr(hip, n), n
    base = ctypes.CDLL(os.path.join(PKG, "mmre", "lib", "libmmre_base.so"))
    for n in ("getRelBatch", "testRel", "test_relation_prediction", "mmre_base_get_rel_metrics"):
        assert re.search(r"\bvoid\s+%s\s*\(" % n, _header("mmre_base.h")), n
        assert hasattr(base, n), n
    from mmre import _lib, base as mbase
    assert {"mmre_rel_workspace", "mmre_rel_evaluate", "mmre_rel_metrics"} <= set(_lib.SIGNATURES)
    assert {"getRelBatch", "testRel", "test_relation_prediction", "mmre_base_get_rel_metrics"} <= set(mbase.SIGNATURES)
    # the workspace formula the header states
    L = _lib.lib()
    assert L.mmre_rel_workspace(0, 237, 200) == 237 * 200 * 4
    assert L.mmre_rel_workspace(4, 237, 200) == 2 * 237 * 200 * 4
    assert L.mmre_rel_workspace(2, 237, 200) == 0 and L.mmre_rel_workspace(3, 5, 512) == 0
    assert L.mmre_rel_workspace(0, 5, 513) < 0 and L.mmre_rel_workspace(7, 5, 8) < 0


@pytest.mark.parametrize("ds", ["small", "relpred"])
def test_relation_filters_match_brute_force(ds):
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    d = OpenKEDataset(os.path.join(GOLDEN, "data", ds))
    h, r, t = d.all_triples()
    index = FilterIndex(h, r, t, d.n_ent, d.n_rel)
    known = {}
    for a, b, c in zip(h.tolist(), r.tolist(), t.tolist()):
        known.setdefault((a, c), set()).add(b)
    th, tr, tt = d.test_list()
    absent = next((a, b) for a in range(d.n_ent) for b in range(d.n_ent) if (a, b) not in known)
    alone = [(a, b) for (a, b), s in known.items() if len(s) == 1]
    assert alone, "no pair with a single relation"
    qh = np.r_[th, absent[0], alone[0][0], th[:5]]       # + an unknown pair, a lone pair, repeats
    qt = np.r_[tt, absent[1], alone[0][1], tt[:5]]
    off, ids = index.relation_filters(qh, qt)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and off.shape == (len(qh) + 1,) and off[0] == 0
    assert off[-1] == len(ids)
    for i, (a, b) in enumerate(zip(qh.tolist(), qt.tolist())):
        got = ids[off[i]:off[i + 1]].tolist()
        assert got == sorted(known.get((a, b), ())), (i, a, b)
    n = len(th)
    assert off[n + 1] == off[n]                                             # the unknown pair: empty list
    assert ids[off[n + 1]:off[n + 2]].tolist() == sorted(known[alone[0]])   # its own relation only
    # every test triple's list holds its own relation (test triples are known)
    assert all(tr[i] in ids[off[i]:off[i + 1]] for i in range(n))
    if ds == "relpred":  # the dense set is dense: most test pairs have a competing known relation
        assert (np.diff(off[:n + 1]) > 1).sum() * 2 >= n
    # the existing filters are untouched by the lazily built order
    o2, i2 = FilterIndex(h, r, t, d.n_ent, d.n_rel).filters(th, tr, tt, np.zeros(n, np.int8))
    o1, i1 = index.filters(th, tr, tt, np.zeros(n, np.int8))
    assert np.array_equal(o1, o2) and np.array_equal(i1, i2)
    e_off, e_ids = index.relation_filters(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert e_off.tolist() == [0] and len(e_ids) == 0


def _metrics_vec(m):
    from mmre.link import METRIC_NAMES
    return np.array([m[g][k] for g in ("filter", "raw") for k in METRIC_NAMES], np.float32)


@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("config", CONFIGS)
def test_rel_metrics_bit_equal_to_reference_globals(golden, fixture, config):
    from mmre.link import rel_metrics
    g = golden(fixture)
    counts = g[f"{config}_counts"].astype(np.int32)                 # (2, T) raw, filt
    assert counts.shape == (2, int(g["T"])) and np.all(counts[1] <= counts[0]) and np.all(counts >= 0)
    got = _metrics_vec(rel_metrics(counts))
    exp = g[f"{config}_metrics"]
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (got, exp)
    # a strided view: the two columns as rows of a wider table
    wide = np.full((2, counts.shape[1] + 7), 99, np.int32)
    wide[:, 3:3 + counts.shape[1]] = counts
    got = _metrics_vec(rel_metrics(wide[:, 3:3 + counts.shape[1]]))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_rel_metrics_single_query_and_arguments():
    from mmre._lib import MMREError
    from mmre.link import rel_metrics
    m = rel_metrics(np.array([[4], [2]], np.int32))
    assert m["raw"] == dict(mrr=float(np.float32(1.0 / 5.0)), mr=5.0, hit10=1.0, hit3=0.0, hit1=0.0)
    assert m["filter"] == dict(mrr=float(np.float32(1.0 / 3.0)), mr=3.0, hit10=1.0, hit3=1.0, hit1=0.0)
    m = rel_metrics(np.array([[0], [0]], np.int64))
    assert m["raw"] == m["filter"] == dict(mrr=1.0, mr=1.0, hit10=1.0, hit3=1.0, hit1=1.0)
    with pytest.raises(MMREError):
        rel_metrics(np.zeros((2, 0), np.int32))
    with pytest.raises(ValueError):
        rel_metrics(np.zeros((4, 3), np.int32))


def test_fixture_contents(golden):
    """What the GPU tests rely on: testList order, predictions per relation, a worked filter."""
    from mmre.data import OpenKEDataset
    for fixture in FIXTURES:
        g = golden(fixture)
        d = OpenKEDataset(os.path.join(GOLDEN, "data", DATASETS[fixture]))
        h, r, t = d.test_list()
        assert np.array_equal(g["qh"], h) and np.array_equal(g["qt"], t)
        assert int(g["R"]) == d.n_rel and float(g["near_rel"]) == 1e-5
        for c in CONFIGS:
            p = g[f"{c}_pred"]
            assert p.shape == (len(h), d.n_rel) and p.dtype == np.float32
            raw = ((p < p[np.arange(len(h)), r][:, None]) & (np.arange(d.n_rel)[None] != r[:, None])).sum(1)
            assert np.array_equal(raw, g[f"{c}_counts"][0])
    dense = golden("relpred_dense")
    assert int(dense["R"]) == 70 and int(dense["E"]) == 48
    assert any((dense[f"{c}_counts"][0] != dense[f"{c}_counts"][1]).sum() >= 30 for c in CONFIGS)


def test_tester_has_relation_prediction():
    from openke.config import Tester
    assert callable(getattr(Tester, "run_relation_prediction"))
