"""Relation prediction on the GPU: the fused all-relation sweep (mmre_rel_evaluate), the Base ABI
loop (getRelBatch -> testRel -> test_relation_prediction) and the Tester entry.

Exactness: a prediction of the sweep is, bit for bit, model.predict's for the row (h, j, t)
(mmre.ns.score_rows + the model's transform), so scores are compared with array_equal and the
counts are exact integers. Against the reference (fixtures of tests/golden/make_relpred.py, its
CPU models and Base.so) the method is test_ref_fixture_gpu.py's: the only entries whose side of
Test.h's strict `<` may differ are those within near_rel x max|row| of the truth, and the
reference counts are moved by exactly those whose side differs in the GPU's own scores."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CONFIGS = ["transe", "transe_nonorm_margin", "transe_l2", "distmult", "complex", "rotate"]
DATASETS = {"relpred_small": "small", "relpred_dense": "relpred"}
# (R, d, Q): R = 1, below / at / across one wave of relations, several waves; d below one wave
# (idle lanes), one wave's multiple or not, the 1 / 2 / 4 / 8-chunk kernels, the largest; Q = 1,
# fewer than one workgroup's waves, many workgroups with a ragged last one
SHAPES = [(1, 24, 1), (13, 32, 3), (64, 100, 150), (65, 200, 3), (257, 512, 3), (70, 24, 150)]
E = 40


def _dev():
    return torch.device("cuda:0")


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _specs(config, ent, rel, ent_im=None, rel_im=None, margin=None, eps=2.0):
    """(ScoreSpec, NSSpec, predict's transform of forward's score) for a fixture configuration."""
    from mmre.link import ScoreSpec, rotate_phase_denom
    from mmre.ns import NSSpec
    f = lambda a: None if a is None else _to(np.asarray(a, np.float32))
    d = rel.shape[1]
    if config.startswith("transe"):
        model = "transe_l2" if config == "transe_l2" else "transe"
        norm = config != "transe_nonorm_margin"
        m = 5.0 if config == "transe_nonorm_margin" else None
        m = margin if margin is not None else m
        sp = ScoreSpec(model=model, ent=f(ent), rel=f(rel), dim=d, norm_flag=norm, pred_kind=1 if m is not None else 0,
                       margin=float(m or 0.0))
        ns = NSSpec(model, d, norm_flag=norm, model_margin=m)
        tr = (lambda s: m - s) if m is not None else (lambda s: s)
    elif config == "distmult":
        sp = ScoreSpec(model="distmult", ent=f(ent), rel=f(rel), dim=d, pred_kind=2)
        ns, tr = NSSpec("distmult", d), (lambda s: -s)
    elif config == "complex":
        sp = ScoreSpec(model="complex", ent=f(ent), rel=f(rel), dim=d, ent_im=f(ent_im), rel_im=f(rel_im), pred_kind=2)
        ns, tr = NSSpec("complex", d), (lambda s: -s)
    else:
        m = 6.0 if margin is None else margin
        pd = rotate_phase_denom(m, eps, d)
        sp = ScoreSpec(model="rotate", ent=f(ent), rel=f(rel), dim=d, pred_kind=3, margin=m, phase_denom=pd)
        ns, tr = NSSpec("rotate", d, model_margin=m, phase_denom=pd), (lambda s: -s)
    return sp, ns, tr


def _random_tables(config, n_rel, d, seed):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-0.5, 0.5, s).astype(np.float32)
    if config == "complex":
        return u(E, d), u(n_rel, d), u(E, d), u(n_rel, d)
    if config == "rotate":
        return u(E, 2 * d), rng.uniform(-0.3, 0.3, (n_rel, d)).astype(np.float32), None, None
    return u(E, d), u(n_rel, d), None, None


def _predict_rows(sp, ns, tr, qh, qt, n_rel):
    """model.predict on the expanded rows (h, j, t), j = 0..R-1 of every query: (Q, R)."""
    from mmre.ns import score_rows
    Q = len(qh)
    h = _to(np.repeat(qh, n_rel))
    t = _to(np.repeat(qt, n_rel))
    r = _to(np.tile(np.arange(n_rel, dtype=np.int64), Q))
    with torch.no_grad():
        s = tr(score_rows(ns, sp.ent, sp.rel, h, t, r, ent_im=sp.ent_im, rel_im=sp.rel_im))
    return s.reshape(Q, n_rel).cpu().numpy()


def _expected_counts(scores, qr, off=None, ids=None):
    """Test.h:200-213 on a (Q, R) score matrix; a list's invalid ids and the truth are ignored."""
    Q, R = scores.shape
    raw, filt = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    for i in range(Q):
        better = scores[i] < scores[i, qr[i]]            # False for NaN on either side
        better[qr[i]] = False
        raw[i] = filt[i] = better.sum()
        if off is not None:
            lst = {int(j) for j in ids[off[i]:off[i + 1]] if 0 <= j < R}
            filt[i] -= sum(bool(better[j]) for j in lst)
    return np.stack([raw, filt])


def _sweep(sp, qh, qr, qt, filt=None, scores=True):
    from mmre.link import relation_sweep
    f = None if filt is None else (_to(filt[0]), _to(filt[1]))
    res = relation_sweep(sp, _to(qh), _to(qr), _to(qt), filt=f, return_scores=scores)
    torch.cuda.synchronize()
    return (res["counts"].cpu().numpy(), res["truth"].cpu().numpy(),
            None if res["scores"] is None else res["scores"].cpu().numpy())


def _same_bits(a, b):
    """Bit-equal floats; a NaN matches a NaN (its payload is not part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _random_lists(rng, Q, R, qr):
    """Per-query lists of distinct relations, some holding the truth, some empty."""
    off, ids = [0], []
    for i in range(Q):
        k = int(rng.integers(0, min(R, 9) + 1))
        lst = rng.choice(R, size=k, replace=False).tolist()
        if i % 3 == 0 and qr[i] not in lst:
            lst.append(int(qr[i]))
        ids += sorted(lst)
        off.append(len(ids))
    return np.array(off, np.int64), np.array(ids, np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d_d%d_Q%d" % s)
@pytest.mark.parametrize("config", CONFIGS)
def test_scores_bit_equal_to_predict_and_counts_exact(config, shape):
    R, d, Q = shape
    sp, ns, tr = _specs(config, *_random_tables(config, R, d, seed=R * 1000 + d))
    rng = np.random.default_rng(Q + R)
    qh, qt, qr = rng.integers(0, E, Q), rng.integers(0, E, Q), rng.integers(0, R, Q)
    off, ids = _random_lists(rng, Q, R, qr)
    counts, truth, scores = _sweep(sp, qh, qr, qt, (off, ids))
    ref = _predict_rows(sp, ns, tr, qh, qt, R)
    assert scores.shape == (Q, R)
    assert np.array_equal(scores.view(np.uint32), ref.view(np.uint32)), float(np.abs(scores - ref).max())
    assert np.array_equal(truth.view(np.uint32), ref[np.arange(Q), qr].view(np.uint32))
    assert np.array_equal(counts, _expected_counts(scores, qr, off, ids))
    if R == 1:
        assert not counts.any()
    # count-only, and without a filter: the filtered column is the raw one
    c2, t2, s2 = _sweep(sp, qh, qr, qt, (off, ids), scores=False)
    assert s2 is None and np.array_equal(c2, counts) and np.array_equal(t2.view(np.uint32), truth.view(np.uint32))
    c3, _, _ = _sweep(sp, qh, qr, qt, None, scores=False)
    assert np.array_equal(c3[0], counts[0]) and np.array_equal(c3[1], counts[0])


@pytest.mark.parametrize("config", CONFIGS)
def test_counts_exact_on_adversarial_rows(config):
    """Ties, NaN, the truth in its own list, listed relations that lose, repeated pairs."""
    R, d, Q = 70, 40, 12
    ent, rel, ent_im, rel_im = _random_tables(config, R, d, seed=77)
    true_r, copy_r, nan_r = 5, 66, 30
    rel[copy_r] = rel[true_r]                      # a bitwise copy of the true relation's row
    if rel_im is not None:
        rel_im[copy_r] = rel_im[true_r]
    rel[nan_r, 3] = np.nan                         # never counted
    sp, ns, tr = _specs(config, ent, rel, ent_im, rel_im)
    rng = np.random.default_rng(3)
    qh, qt = rng.integers(0, E, Q), rng.integers(0, E, Q)
    qh[6:] = qh[:6]                                # every pair twice ...
    qt[6:] = qt[:6]
    qr = np.full(Q, true_r, np.int64)
    qr[9:] = rng.integers(0, R, 3)                 # ... some with another truth
    qr[11] = nan_r                                 # a NaN truth: nothing is below it
    counts0, truth0, scores0 = _sweep(sp, qh, qr, qt)
    assert np.array_equal(scores0[:, copy_r].view(np.uint32), scores0[:, true_r].view(np.uint32))
    assert np.all(np.isnan(scores0[:, nan_r])) and np.isnan(truth0[11]) and not counts0[:, 11].any()
    assert np.isfinite(np.delete(scores0, nan_r, axis=1)).all()
    off, ids = [0], []
    for i in range(Q):
        order = np.argsort(np.where(np.isnan(scores0[i]), np.inf, scores0[i]), kind="stable")
        win = [int(j) for j in order if scores0[i, j] < scores0[i, qr[i]]][:3]         # beat the truth
        lose = [int(j) for j in order[::-1] if not scores0[i, j] < scores0[i, qr[i]] and j != qr[i]][:2]
        lst = set(win + lose + [int(qr[i]), copy_r, nan_r])
        if i % 4 == 0:
            lst = {int(qr[i])}                     # only its own relation
        if i % 4 == 1:
            lst |= {-1, R, R + 5}                  # ids outside the table: ignored
        ids += sorted(lst)
        off.append(len(ids))
    off, ids = np.array(off, np.int64), np.array(ids, np.int32)
    counts, truth, scores = _sweep(sp, qh, qr, qt, (off, ids))
    assert _same_bits(scores, scores0)
    exp = _expected_counts(scores, qr, off, ids)
    assert np.array_equal(counts, exp), (counts, exp)
    assert np.array_equal(counts[0], counts0[0]) and (counts[1] < counts[0]).any()
    assert np.array_equal(counts[0, :3], counts[0, 6:9])           # the repeated pairs (lists differ)
    c2, t2, _ = _sweep(sp, qh, qr, qt, (off, ids), scores=False)
    assert np.array_equal(c2, counts) and _same_bits(t2, truth)
    ref = _predict_rows(sp, ns, tr, qh, qt, R)
    assert _same_bits(scores, ref)


def _fixture_tables(g, name):
    if name == "complex":
        return (g[f"{name}.ent_re_embeddings.weight"], g[f"{name}.rel_re_embeddings.weight"],
                g[f"{name}.ent_im_embeddings.weight"], g[f"{name}.rel_im_embeddings.weight"])
    return g[f"{name}.ent_embeddings.weight"], g[f"{name}.rel_embeddings.weight"], None, None


def _dataset(fixture):
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    d = OpenKEDataset(os.path.join(GOLDEN, "data", DATASETS[fixture]))
    return d, FilterIndex(*d.all_triples(), d.n_ent, d.n_rel)


@pytest.mark.parametrize("fixture", list(DATASETS))
@pytest.mark.parametrize("config", CONFIGS)
def test_reference_parity(golden, fixture, config):
    from mmre.link import evaluate_relation_prediction
    g = golden(fixture)
    d, index = _dataset(fixture)
    h, r, t = d.test_list()
    T, R = len(h), d.n_rel
    sp, _, _ = _specs(config, *_fixture_tables(g, config))
    metrics, counts, gs = evaluate_relation_prediction(sp, h, r, t, index=index, return_scores=True)
    ref = g[f"{config}_pred"].astype(np.float64)
    rows = np.arange(T)
    r_truth, g_truth = ref[rows, r], gs[rows, r].astype(np.float64)
    err_t = np.abs(g_truth - r_truth)
    print(f"{fixture}/{config}: max truth err {err_t.max():.3g}")
    assert np.all(err_t <= 1e-4 * np.maximum(1.0, np.abs(r_truth))), float(err_t.max())
    window = float(g["near_rel"]) * np.abs(ref).max(axis=1)
    err = np.abs(gs.astype(np.float64) - ref).max(axis=1)
    print(f"{fixture}/{config}: max err / window {float((err / window).max()):.3g}")
    assert np.all(err <= 0.25 * window), float((err / window).max())
    # the reference's counts, moved by the near entries whose side differs in the GPU's own scores
    near = np.abs(ref - r_truth[:, None]) <= window[:, None]
    near[rows, r] = False
    flip = ((gs < gs[rows, r][:, None]).astype(np.int64) - (ref < r_truth[:, None]).astype(np.int64)) * near
    known = np.zeros((T, R), bool)
    off, ids = index.relation_filters(h, t)
    known[np.repeat(rows, np.diff(off)), ids] = True
    ref_c = g[f"{config}_counts"]
    d_raw, d_filt = flip.sum(1), (flip * ~known).sum(1)
    assert np.array_equal(counts[0], ref_c[0] + d_raw) and np.array_equal(counts[1], ref_c[1] + d_filt)
    moved = int((d_raw != 0).sum() + (d_filt != 0).sum())
    print(f"{fixture}/{config}: {int(near.sum())} near entries, {moved} counts moved, "
          f"{int((ref_c[0] != ref_c[1]).sum())} of {T} triples filtered")
    if moved == 0:
        from mmre.link import METRIC_NAMES
        got = np.array([metrics[k][m] for k in ("filter", "raw") for m in METRIC_NAMES], np.float32)
        assert np.array_equal(got.view(np.uint32), g[f"{config}_metrics"].view(np.uint32)), (got, g[f"{config}_metrics"])


def _base(ds):
    from mmre import base
    L = base.load()
    L.mmre_base_clear_error()
    L.setInPath((os.path.join(GOLDEN, "data", ds) + "/").encode())
    L.importTrainFiles()
    L.importTestFiles()
    return L


def _abi_loop(L, preds, check=None):
    """getRelBatch -> (given predictions) -> testRel per test triple, test_relation_prediction."""
    R, T = L.getRelationTotal(), L.getTestTotal()
    ph, pt, pr = (np.zeros(R, np.int64) for _ in range(3))
    L.initTest()
    for i in range(T):
        L.getRelBatch(ph.ctypes.data, pt.ctypes.data, pr.ctypes.data)
        if check is not None:
            check(i, ph, pt, pr)
        s = np.ascontiguousarray(preds(i, ph, pt, pr), np.float32)
        L.testRel(s.ctypes.data)
    L.test_relation_prediction()
    out = np.zeros(10, np.float32)
    L.mmre_base_get_rel_metrics(out.ctypes.data)
    return out


@pytest.mark.parametrize("fixture", list(DATASETS))
def test_base_abi_loop_bit_exact(golden, fixture):
    from mmre import base
    g = golden(fixture)
    # the type lists of a dataset with fewer relations, loaded earlier in the process, must not be
    # indexed by this one's relations (no importTypeFiles below: relation prediction has no types)
    _base("small").importTypeFiles()
    L = _base(DATASETS[fixture])
    R, T = L.getRelationTotal(), L.getTestTotal()
    assert (R, T) == (int(g["R"]), int(g["T"]))

    def check(i, ph, pt, pr):
        assert np.all(ph == g["qh"][i]) and np.all(pt == g["qt"][i]) and np.array_equal(pr, np.arange(R))
        a, b, c = (np.zeros(R, np.int64) for _ in range(3))
        L.getRelBatch(a.ctypes.data, b.ctypes.data, c.ctypes.data)     # lastRel did not advance
        assert np.array_equal(a, ph) and np.array_equal(b, pt) and np.array_equal(c, pr)

    for config in CONFIGS:
        pred = g[f"{config}_pred"]
        got = _abi_loop(L, lambda i, *_: pred[i], check if config == CONFIGS[0] else None)
        exp = g[f"{config}_metrics"]
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (config, got, exp)
    # initTest starts the sums over (the reference's does not, Test.h:29): a second pass is identical
    again = _abi_loop(L, lambda i, *_: g[f"{CONFIGS[-1]}_pred"][i])
    assert np.array_equal(again.view(np.uint32), g[f"{CONFIGS[-1]}_metrics"].view(np.uint32))
    assert base.last_error() == (0, "")
    # one testRel past the last test triple: latched before any GPU work, outputs poisoned
    s = np.zeros(R, np.float32)
    L.testRel(s.ctypes.data)
    code, msg = base.last_error()
    assert code == 1 and "out of range" in msg
    ph, pt, pr = (np.full(R, 7, np.int64) for _ in range(3))
    L.getRelBatch(ph.ctypes.data, pt.ctypes.data, pr.ctypes.data)
    assert np.all(ph == -1) and np.all(pt == -1) and np.all(pr == -1)
    out = np.zeros(10, np.float32)
    L.mmre_base_get_rel_metrics(out.ctypes.data)
    assert np.all(np.isnan(out))
    L.mmre_base_clear_error()
    L.mmre_base_get_rel_metrics(out.ctypes.data)
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32))
    L.initTest()
    L.getRelBatch(ph.ctypes.data, pt.ctypes.data, pr.ctypes.data)   # and the library works again
    assert base.last_error()[0] == 0 and ph[0] == g["qh"][0]


@pytest.mark.parametrize("cls,kw", [("TransE", dict(dim=32, p_norm=1, norm_flag=True)),
                                     ("RotatE", dict(dim=16, margin=6.0, epsilon=2.0))])
def test_tester_equals_the_predict_testrel_loop(cls, kw, capsys):
    """Tester.run_relation_prediction (one fused evaluation) == model.predict(getRelBatch rows) ->
    testRel per test triple through libmmre_base, same model."""
    import openke.module.model as models
    from openke.config import Tester
    from openke.data import TestDataLoader
    path = os.path.join(GOLDEN, "data", "small") + "/"
    torch.manual_seed(11)
    dl = TestDataLoader(path, "link")
    model = getattr(models, cls)(ent_tot=dl.get_ent_tot(), rel_tot=dl.get_rel_tot(), **kw)
    tester = Tester(model=model, data_loader=dl, use_gpu=True)
    got = tester.run_relation_prediction()
    printed = capsys.readouterr().out
    assert "averaged(raw):" in printed and "averaged(filter):" in printed
    assert tester.last["counts"].shape == (2, dl.testTotal)
    L = _base("small")
    loop = _abi_loop(L, lambda i, ph, pt, pr: model.predict({"batch_h": ph, "batch_t": pt, "batch_r": pr,
                                                             "mode": "normal"}))
    assert np.array_equal(np.array(got, np.float32).view(np.uint32), loop[:5].view(np.uint32)), (got, loop)
    m = tester.last["metrics"]
    from mmre.link import METRIC_NAMES
    raw = np.array([m["raw"][k] for k in METRIC_NAMES], np.float32)
    assert np.array_equal(raw.view(np.uint32), loop[5:].view(np.uint32))


def test_error_contract():
    """Bad calls are refused before any launch; nothing faults."""
    from mmre._lib import lib, stream_ptr
    L = lib()
    dev = _dev()
    E_, R, d, Q = 8, 5, 16, 3
    ent = torch.zeros((E_, 1026), dtype=torch.float32, device=dev)
    rel = torch.zeros((R, 513), dtype=torch.float32, device=dev)
    q = torch.zeros(Q, dtype=torch.int64, device=dev)
    counts = torch.full((2, Q), -7, dtype=torch.int32, device=dev)
    truth = torch.full((Q,), -7.0, dtype=torch.float32, device=dev)
    work = torch.empty(2 * R * 513 * 4, dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = stream_ptr(dev)

    def run(model=0, dim=d, ent_=ent, rel_=rel, ent_im=None, rel_im=None, n_query=Q, off=None, ids=None, kind=0,
            work_bytes=work.numel(), qh=q, phase=0.0, n_rel=R):
        return L.mmre_rel_evaluate(model, 1, kind, 0.0, p(ent_), p(ent_im), p(rel_), p(rel_im), E_, n_rel, dim, phase,
                                   p(qh), p(q), p(q), n_query, p(off), p(ids), p(counts), p(truth), None, p(work),
                                   work_bytes, st)

    assert run(dim=513) == 3                      # MMRE_ERR_SHAPE
    assert run(ent_=None) == 1 and run(rel_=None) == 1      # MMRE_ERR_ARG
    assert run(model=3) == 1                      # ComplEx without imaginary tables
    assert run(model=9) == 2                      # MMRE_ERR_MODEL
    assert run(kind=5) == 1 and run(n_query=-1) == 1 and run(n_rel=0) == 1 and run(dim=0) == 1
    assert run(off=q) == 1                        # offsets without ids
    assert run(model=4, phase=0.0) == 1           # RotatE without its phase scale
    assert run(qh=None) == 1
    assert run(work_bytes=R * d * 4 - 1) == 4     # MMRE_ERR_WORKSPACE
    assert run(n_query=0) == 0 and run(n_query=0, qh=None) == 0
    torch.cuda.synchronize()
    assert torch.all(counts == -7) and torch.all(truth == -7.0)      # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.all(counts == 0) and torch.all(truth == 0.0)
