"""The grouped sweep of the fused TransE L1 evaluation (mmre_link_evaluate_l1q): the integer
filter's SAD chains run once per sweep ROW -- a filter group, whose members share the query vector
(mode, r, anchor) -- and the rank epilogue compares every pair against each member's thresholds.

Bar: everything the call leaves in HBM bit-identical to the separate entry points
(MMRE_FUSED_EVAL=0: one sweep per query), counts equal to the oracle's Test.h restatement, the
same undecided-pair record -- for every partition that meets the contract (each group shares its
key): any cap, any group order, groups larger than the slot capacity, one group of everything.

Shapes: E = 2,100 (16 whole entity tiles + one of 52 columns), d = 40 (two K stages: dynamic
scheduling live), ~340 queries over 40 keys with group sizes 1, 2, cap - 1, cap, cap + 1, 64, 65,
130; fully duplicated (h, r, t) queries; every member's truth is a listed entity of its fellow
members; tables with exact copies of truth rows (exact ties must not count)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_sweep_filters_gpu import _adversarial
from test_link_gpu import _spec_from

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP = 8  # mmre.link.FUSED_MAX_GROUP: the sweep's member slots per row
E, D = 2100, 40
SIZES = [1, 2, CAP - 1, CAP, CAP + 1, 64, 65, 130] + [1] * 20 + [3, 4, 5, 6, 2, 2, 3, 1, 1, 1, 1, 1]


@pytest.fixture(autouse=True, params=["8", None], ids=["cap8", "capauto"])
def _slot_cap(request, monkeypatch):
    """MMRE_GROUP_CAP=8: every row takes up to the full eight member slots. Unset: the call's own
    choice, which at these sizes (fewer units than resident workgroups) is the ungrouped sweep."""
    if request.param is None:
        monkeypatch.delenv("MMRE_GROUP_CAP", raising=False)
    else:
        monkeypatch.setenv("MMRE_GROUP_CAP", request.param)


def _workload():
    """Adversarial tables; the queries resampled into 40 keys of the sizes above. A key is an
    original query's (mode, r, anchor); its first member is that query (its truth row has exact
    copies and near copies in the table), the others draw their truths from the tied truths and
    from random entities; key 5's members are all one (h, r, t)."""
    ent, rel, oh, orr, ot, om = _adversarial(E=E, d=D, Q=300, seed=3, model="transe", huge=False)
    rng = np.random.default_rng(11)
    tied = np.array([oh[i] if om[i] == 0 else ot[i] for i in range(0, 300, 3)])
    qh, qr, qt, qm = [], [], [], []
    seen = set()
    src = iter(range(0, 300, 3))
    for k, n in enumerate(SIZES):
        i = next(j for j in src if (om[j], orr[j], ot[j] if om[j] == 0 else oh[j]) not in seen)
        head = om[i] == 0
        anchor = ot[i] if head else oh[i]
        seen.add((om[i], orr[i], anchor))
        truths = np.r_[oh[i] if head else ot[i], np.where(rng.random(n - 1) < 0.5, rng.choice(tied, n - 1),
                                                           rng.integers(0, E, n - 1))]
        if k == 5:
            truths[:] = truths[0]  # 64 fully duplicated queries
        for tr in truths:
            qh.append(tr if head else anchor)
            qt.append(anchor if head else tr)
            qr.append(orr[i])
            qm.append(om[i])
    p = rng.permutation(len(qh))
    qh, qr, qt = (np.asarray(x, np.int64)[p] for x in (qh, qr, qt))
    return ent, rel, qh, qr, qt, np.asarray(qm, np.int8)[p]


def _index(qh, qr, qt, n_rel, seed=7):
    from mmre.link import FilterIndex
    rng = np.random.default_rng(seed)
    fh, fr, ft = rng.integers(0, E, 3 * E), rng.integers(0, n_rel, 3 * E), rng.integers(0, E, 3 * E)
    fh, fr, ft = np.r_[fh, qh], np.r_[fr, qr], np.r_[ft, qt]
    return FilterIndex(fh, fr, ft, E, n_rel), (fh, fr, ft)


def _reorder(filt, perm):
    """The same groups in another order (group g of the result = group perm[g])."""
    gqo, gq, off, ids, entry_q = filt
    perm = np.asarray(perm)
    sz, ln = np.diff(gqo)[perm], np.diff(off)[perm]
    n_gqo, n_off = np.r_[0, np.cumsum(sz)].astype(np.int64), np.r_[0, np.cumsum(ln)].astype(np.int64)
    qsrc = np.repeat(gqo[:-1][perm] - n_gqo[:-1], sz) + np.arange(n_gqo[-1])
    lsrc = np.repeat(off[:-1][perm] - n_off[:-1], ln) + np.arange(n_off[-1])
    return n_gqo, gq[qsrc], n_off, ids[lsrc.astype(np.int64)], entry_q[lsrc.astype(np.int64)]


def _eval(spec, q, filt, fused, monkeypatch, entity_range=None, reps=1, graph=False, und=False):
    from mmre.link import LinkSweep
    qh, qr, qt, qm = q
    monkeypatch.setenv("MMRE_FUSED_EVAL", "1" if fused else "0")
    to = lambda a, dt=np.int64: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    dfilt = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in filt)
    sw = LinkSweep(spec)
    bufs = sw.alloc_queries(len(qh))
    args = (to(qh), to(qr), to(qt), to(qm, np.int8))
    und_q = torch.full((len(qh),), -1, dtype=torch.int32, device=DEV) if und else None
    for _ in range(reps):
        sw.run(*args, filt=dfilt, buffers=bufs, entity_range=entity_range, undecided_q=und_q)
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sw.run(*args, filt=dfilt, buffers=bufs, entity_range=entity_range)
        for _ in range(3):
            bufs["counts"].fill_(-7)
            g.replay()
    torch.cuda.synchronize()
    n = len(qh)
    cp = lambda t: t.cpu().numpy().copy()
    out = {"counts": cp(bufs["counts"]), "truth": cp(bufs["truth"]), "q_km": cp(bufs["q_km"]),
           "q_rows": cp(bufs["q_rows"][:n]), "q_true": cp(bufs["q_true"][:n]), "ent_km": cp(sw.ent_km),
           "ent_rows": cp(sw.ent_rows), "st": sw.l1q_stats(bufs), "und_q": cp(und_q) if und else None}
    monkeypatch.delenv("MMRE_FUSED_EVAL")
    return out


def _same(a, b):
    for k in ("counts", "truth", "q_km", "q_rows", "q_true", "ent_km", "ent_rows"):
        x, y = a[k], b[k]
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y), k
    sa, sb = a["st"], b["st"]
    assert sa["bits"] == sb["bits"] and sa["fallback"] == sb["fallback"], (sa, sb)
    assert sa["undecided"] == sb["undecided"], (sa, sb)
    assert sa["guarded"] == 0 and sb["guarded"] == 0


def _setbits(monkeypatch, bits):
    if bits is None:
        monkeypatch.delenv("MMRE_L1_BITS", raising=False)
    else:
        monkeypatch.setenv("MMRE_L1_BITS", bits)


@pytest.fixture(scope="module")
def work():
    ent, rel, qh, qr, qt, qm = _workload()
    index, trip = _index(qh, qr, qt, rel.shape[0])
    return dict(ent=ent, rel=rel, q=(qh, qr, qt, qm), index=index, trip=trip)


def test_workload_has_the_group_sizes(work):
    qh, qr, qt, qm = work["q"]
    gqo = work["index"].groups(qh, qr, qt, qm, max_group=len(qh))[0]
    sizes = np.diff(gqo)
    assert sorted(sizes.tolist()) == sorted(SIZES) and sizes.max() > 128
    assert {1, 2, CAP - 1, CAP, CAP + 1, 64, 65} <= set(sizes.tolist())
    key = qm.astype(np.int64) * 10 ** 9 + qh * 10 ** 5 + qt + qr * 10 ** 12
    assert len(np.unique(key)) <= len(qh) - 63  # the fully duplicated (h, r, t) queries


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("bits", [None, "8", "16"])
def test_grouped_equals_separate_and_oracle(oracle_mod, monkeypatch, work, norm, bits):
    from mmre.link import group_args
    _setbits(monkeypatch, bits)
    qh, qr, qt, qm = work["q"]
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=norm)
    filt = work["index"].groups(qh, qr, qt, qm, **group_args(spec))
    assert np.diff(filt[0]).max() == CAP
    fused = _eval(spec, work["q"], filt, True, monkeypatch, reps=2)
    sep = _eval(spec, work["q"], filt, False, monkeypatch)
    _same(fused, sep)
    hrt = oracle_mod.sorted_hrt(*work["trip"])
    for mode_id, mode in ((0, "head_batch"), (1, "tail_batch")):
        sel = qm == mode_id
        o_pred = oracle_mod.link_predict("transe", mode, work["ent"], work["rel"], qh[sel], qr[sel], qt[sel],
                                         norm_flag=norm)
        o_c = oracle_mod.test_rank(mode, o_pred, qh[sel], qr[sel], qt[sel], hrt)
        assert np.array_equal(fused["counts"][:2, sel].T, o_c[:, :2])


@pytest.mark.parametrize("bits", ["8", "16"])
def test_partition_independence(monkeypatch, work, bits):
    """max_group 1 (a row per query: the ungrouped sweep), 3, the cap, 64 and one group per key
    (both past the slot capacity: the native side cuts them), each with its groups by descending
    size, reversed and shuffled: identical counts, undecided totals and per-query counters."""
    _setbits(monkeypatch, bits)
    qh, qr, qt, qm = work["q"]
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=True)
    rng = np.random.default_rng(5)
    ref = None
    for mg in (1, 3, CAP, 64, len(qh)):
        base = work["index"].groups(qh, qr, qt, qm, max_group=mg, order="size")
        ng = len(base[0]) - 1
        for perm in (np.arange(ng), np.arange(ng)[::-1], rng.permutation(ng)):
            r = _eval(spec, work["q"], _reorder(base, perm), True, monkeypatch, und=True)
            assert r["st"]["guarded"] == 0 and r["st"]["bits"] == int(bits)
            assert r["und_q"].sum() == r["st"]["undecided"]
            if ref is None:
                ref = r
                continue
            assert np.array_equal(r["counts"], ref["counts"]), (mg, perm[:4])
            assert r["st"]["undecided"] == ref["st"]["undecided"], (mg, r["st"], ref["st"])
            assert np.array_equal(r["und_q"], ref["und_q"]), mg
    sep = _eval(spec, work["q"], work["index"].groups(qh, qr, qt, qm), False, monkeypatch)
    assert np.array_equal(sep["counts"], ref["counts"]) and sep["st"]["undecided"] == ref["st"]["undecided"]


def _random_case(n_keys, per_key, seed, extra=0):
    """n_keys keys x per_key members (+ extra single-member keys) on the adversarial tables."""
    ent, rel, oh, orr, ot, om = _adversarial(E=E, d=D, Q=300, seed=3, model="transe", huge=False)
    rng = np.random.default_rng(seed)
    R = rel.shape[0]
    keys = rng.permutation(2 * R * E)[:n_keys + extra]  # distinct (mode, r, anchor)
    reps = np.r_[np.full(n_keys, per_key), np.ones(extra, np.int64)].astype(np.int64)
    k = np.repeat(keys, reps)
    mode, r, anchor = k // (R * E), (k // E) % R, k % E
    truth = rng.integers(0, E, len(k))
    qh, qt = np.where(mode == 0, truth, anchor), np.where(mode == 0, anchor, truth)
    return ent, rel, (qh.astype(np.int64), r.astype(np.int64), qt.astype(np.int64), mode.astype(np.int8))


@pytest.mark.parametrize("case", ["five", "one_key", "rows128", "rows129", "q256_cap1", "q257_cap1"])
def test_edges(monkeypatch, case):
    """n_query = 5 (one tile, mostly padding rows); one key for all 200 queries; the row count an
    exact multiple of 128 and one more, with two members per row and with a row per query."""
    from mmre.link import group_args
    _setbits(monkeypatch, "8")
    n_keys, per_key, extra, mg = {"five": (2, 2, 1, None), "one_key": (1, 200, 0, 200), "rows128": (128, 2, 0, None),
                                  "rows129": (128, 2, 1, None), "q256_cap1": (128, 2, 0, 1),
                                  "q257_cap1": (128, 2, 1, 1)}[case]
    ent, rel, q = _random_case(n_keys, per_key, seed=21, extra=extra)
    index, _ = _index(q[0], q[1], q[2], rel.shape[0])
    spec = _spec_from("transe", ent, rel, dim=D, norm=True)
    kw = group_args(spec) if mg is None else dict(max_group=mg, order="size")
    filt = index.groups(*q, **kw)
    if case in ("rows128", "q256_cap1"):
        assert len(filt[0]) - 1 == (128 if mg is None else 256)
    fused = _eval(spec, q, filt, True, monkeypatch)
    sep = _eval(spec, q, filt, False, monkeypatch)
    _same(fused, sep)


def test_slices_repeats_and_graph_replays(monkeypatch, work):
    """Three entity slices sum to the whole table; three calls and three hipGraph replays over
    poisoned counts give the same table (the LDS accumulators, work counters and tickets reset)."""
    from mmre.link import group_args
    _setbits(monkeypatch, "8")
    qh, qr, qt, qm = work["q"]
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=True)
    once = _eval(spec, work["q"], work["index"].groups(qh, qr, qt, qm, **group_args(spec)), True, monkeypatch)
    again = _eval(spec, work["q"], work["index"].groups(qh, qr, qt, qm, **group_args(spec)), True, monkeypatch,
                  reps=3, graph=True)
    _same(once, again)
    total = np.zeros_like(once["counts"])
    for er in ((0, 768), (768, 1536), (1536, E)):
        filt = work["index"].groups(qh, qr, qt, qm, entity_range=er, **group_args(spec))
        part = _eval(spec, work["q"], filt, True, monkeypatch, entity_range=er)
        sep = _eval(spec, work["q"], filt, False, monkeypatch, entity_range=er)
        assert np.array_equal(part["counts"], sep["counts"]) and part["st"]["undecided"] == sep["st"]["undecided"]
        total += part["counts"]
    assert np.array_equal(total, once["counts"])
