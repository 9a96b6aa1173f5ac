"""k_heavy_rows, the exact kernel of the per-query route (mmre_link_evaluate_l1q): the
routed queries' pairs are scored with the canonical chain, a thread per entity column and QB routed
queries per workgroup, and counted into the raw column. Counts must equal the same call with the
route off (MMRE_L1_HEAVY=0), the exact path (MMRE_L1_FILTER=0) and a float32 restatement of the
chain in numpy, bit for bit -- no tolerance anywhere.

MMRE_L1_HEAVY=1 lets the route act at these sizes, MMRE_L1_BITS=8 keeps the 8-bit codes,
MMRE_L1_HEAVY_MIN=0 flags every query and MMRE_L1_HEAVY_CAP sets the routed count: the first `cap`
queries in query order. The small tables (TE - 1 .. 2 TE + 3 entities) hold 40 queries: their
routed list stores 32 ids at most, enough for QB + 1; 129 routed queries need the list of a larger
table (E = 2,100, the existing route tests' size)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_eval_grouped_gpu import _eval, _same
from test_eval_heavy_gpu import _env, _run
from test_link_gpu import _spec_from

pytestmark = pytest.mark.gpu
TE, QB = 128, 16  # csrc/link.hip: HR_TE entity columns and HR_QB routed queries per workgroup
R = 5
TIED = (0, QB - 1, QB)  # queries whose truth row has three exact copies (the first, the last of the
                        # first block, the only one of the second block at QB + 1 routed)


def _case(n_ent, d, n_query, seed=5):
    """Random tables and queries (distinct anchor and truth); for the queries of TIED the truth's
    row is copied onto three other entity ids, whose scores then equal the threshold bit for bit."""
    rng = np.random.default_rng(seed + 1000 * n_ent + d)
    er = 8.0 / (2 * d)
    ent = rng.uniform(-er, er, (n_ent, d)).astype(np.float32)
    rel = rng.uniform(-er, er, (R, d)).astype(np.float32)
    mode = rng.integers(0, 2, n_query)
    r = rng.integers(0, R, n_query)
    anchor = rng.integers(0, n_ent, n_query)
    truth = (anchor + 1 + rng.integers(0, n_ent - 1, n_query)) % n_ent
    free = np.setdiff1d(np.arange(n_ent), np.r_[anchor, truth])
    copies = rng.permutation(free)[:3 * len(TIED)].reshape(len(TIED), 3)
    for t, c in zip(TIED, copies):
        ent[c] = ent[truth[t]]
    qh, qt = np.where(mode == 0, truth, anchor), np.where(mode == 0, anchor, truth)
    q = (qh.astype(np.int64), r.astype(np.int64), qt.astype(np.int64), mode.astype(np.int8))
    return ent, rel, q, truth, copies


def _chain_counts(ent, rel, q, e0=0, e1=None):
    """Raw counts by the canonical chain in float32 (acc = acc + |q[k] - e[k]|, k ascending, from
    0): entities of [e0, e1) strictly below the truth's score, the truth left out. No row norm."""
    qh, qr, qt, qm = q
    e1 = ent.shape[0] if e1 is None else e1
    head = (qm == 0)[:, None]
    vec = np.where(head, -(rel[qr] - ent[qt]), ent[qh] + rel[qr]).astype(np.float32)
    truth = np.where(qm == 0, qh, qt)
    acc = np.zeros((len(qh), ent.shape[0]), np.float32)
    for k in range(ent.shape[1]):
        acc = acc + np.abs(vec[:, k, None] - ent[None, :, k])
    th = acc[np.arange(len(qh)), truth]
    ids = np.arange(ent.shape[0])
    better = (acc < th[:, None]) & (ids[None, :] != truth[:, None]) & (ids[None, :] >= e0) & (ids[None, :] < e1)
    return better.sum(1), acc, th


def _filt(ent, rel, q, spec, entity_range=None):
    from mmre.link import FilterIndex, group_args
    rng = np.random.default_rng(7)
    n = ent.shape[0]
    fh, fr, ft = rng.integers(0, n, 3 * n), rng.integers(0, R, 3 * n), rng.integers(0, n, 3 * n)
    index = FilterIndex(np.r_[fh, q[0]], np.r_[fr, q[1]], np.r_[ft, q[2]], n, R)
    kw = {} if entity_range is None else dict(entity_range=entity_range)
    return index.groups(*q, **kw, **group_args(spec))


_REF = {}


def _reference(n_ent, d, n_query):
    """The case, its spec and filter groups, and its oracles, computed once per shape: the same call
    with the route off, the exact path's counts, the float32 chain's raw counts."""
    key = (n_ent, d, n_query)
    if key not in _REF:
        ent, rel, q, truth, copies = _case(n_ent, d, n_query)
        spec = _spec_from("transe", ent, rel, dim=d, norm=False)
        with pytest.MonkeyPatch.context() as mp:
            _env(mp, heavy="0", cap="8")
            filt = _filt(ent, rel, q, spec)
            off = _run(spec, q, filt, mp)
            mp.setenv("MMRE_L1_FILTER", "0")
            f32 = _eval(spec, q, _filt(ent, rel, q, spec), True, mp)
        raw, acc, th = _chain_counts(ent, rel, q)
        for t, c in zip(TIED, copies):  # the copies tie with the threshold bit for bit
            assert (acc[t, c].view(np.uint32) == th[t].view(np.uint32)).all()
        assert off["route"] == dict(flagged=0, routed=0, sample=0, threshold=0)
        assert f32["st"] is None and np.array_equal(off["counts"], f32["counts"])
        assert np.array_equal(off["counts"][0], raw)
        _REF[key] = dict(ent=ent, rel=rel, q=q, truth=truth, spec=spec, filt=filt, off=off, raw=raw)
    return _REF[key]


@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("n_ent", [TE - 1, TE, TE + 1, 2 * TE + 3])
@pytest.mark.parametrize("routed", [0, 1, QB - 1, QB, QB + 1])
def test_small_tables(monkeypatch, routed, n_ent, d):
    """Every routed count around a query block at every entity count around an entity tile: the
    padding columns up to e_pad never count, a tie with the threshold never counts, the truth is
    skipped. Routed 0 (a flag threshold no count reaches: the kernel runs on an empty list) leaves
    the counts as the code sweeps wrote them."""
    ref = _reference(n_ent, d, 40)
    if routed:
        _env(monkeypatch, cap="8", hmin=0, hcap=routed)
    else:
        _env(monkeypatch, cap="8", hmin=10 ** 6)
    on = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch)
    assert on["route"]["routed"] == routed and np.array_equal(on["ids"], np.arange(routed)), on["route"]
    assert on["st"]["bits"] == 8 and not on["st"]["fallback"] and on["st"]["guarded"] == 0
    print("raw counts of the routed queries:", on["counts"][0][:routed], "expected:", ref["raw"][:routed])
    assert np.array_equal(on["counts"][0], ref["raw"])
    assert np.array_equal(on["counts"], ref["off"]["counts"])
    if routed == 0:
        _same(on, ref["off"])


@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("hcap,want", [(128, 128), (129, 129), (200, 129)])
def test_129_flagged(monkeypatch, d, hcap, want):
    """129 flagged queries (eight query blocks and one query) with the list's cap below, at and
    above them, over 16 whole entity tiles and one of 52 columns."""
    ref = _reference(2100, d, 129)
    _env(monkeypatch, cap="8", hmin=0, hcap=hcap)
    on = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch)
    assert on["route"] == dict(flagged=129, routed=want, sample=256, threshold=0), on["route"]
    assert np.array_equal(on["ids"], np.arange(want)) and on["st"]["guarded"] == 0
    assert np.array_equal(on["counts"][0], ref["raw"])
    assert np.array_equal(on["counts"], ref["off"]["counts"])


@pytest.mark.parametrize("d", [24, 200])
def test_entity_slices(monkeypatch, d):
    """Two entity slices, the second from a tile boundary (e_begin = TE) to the table's end: every
    routed query's truth is inside one slice and outside the other; each part equals the chain's
    counts of its slice and the same part with the route off, and the parts sum to the whole call's."""
    n_ent = 2 * TE + 3
    ref = _reference(n_ent, d, 40)
    routed = QB + 1
    assert (ref["truth"][:routed] < TE).any() and (ref["truth"][:routed] >= TE).any()
    _env(monkeypatch, cap="8", hmin=0, hcap=routed)
    whole = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch)
    total = np.zeros_like(whole["counts"])
    for er in ((0, TE), (TE, n_ent)):
        filt = _filt(ref["ent"], ref["rel"], ref["q"], ref["spec"], entity_range=er)
        _env(monkeypatch, cap="8", hmin=0, hcap=routed)
        part = _run(ref["spec"], ref["q"], filt, monkeypatch, entity_range=er)
        _env(monkeypatch, heavy="0", cap="8")
        off = _run(ref["spec"], ref["q"], filt, monkeypatch, entity_range=er)
        assert part["route"]["routed"] == routed and part["st"]["guarded"] == 0
        assert np.array_equal(part["counts"][0], _chain_counts(ref["ent"], ref["rel"], ref["q"], *er)[0]), er
        assert np.array_equal(part["counts"], off["counts"]), er
        total += part["counts"]
    assert np.array_equal(total, whole["counts"]) and np.array_equal(total, ref["off"]["counts"])


def test_repeats_and_graph_replays(monkeypatch):
    """Two calls, and two calls plus three graph replays over poisoned counts, give the table of one
    call: the kernel leaves no state behind."""
    ref = _reference(2 * TE + 3, 24, 40)
    _env(monkeypatch, cap="8", hmin=0, hcap=QB + 1)
    once = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch)
    twice = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch, reps=2)
    replayed = _run(ref["spec"], ref["q"], ref["filt"], monkeypatch, reps=2, graph=True)
    for r in (twice, replayed):
        _same(once, r)
        assert r["route"] == once["route"] and np.array_equal(r["ids"], once["ids"])
    assert once["route"]["routed"] == QB + 1 and np.array_equal(once["counts"], ref["off"]["counts"])
