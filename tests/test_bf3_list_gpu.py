"""The split-bf16 filter's list of undecided pairs (csrc/link.hip: bf3_list, k_bf3_rescore,
k_bf3_stats) between empty and overflowing, and the type-constrained VALU sweep's 16-bit counters.

The list has 64 per-workgroup segments and a shared half; a full segment's appends go to the
shared half, a full shared half raises the flag that gates the device-side fallback to the exact
f32 sweep. These tests size the list (MMRE_BF3_CAP) from the per-segment append counters of a run
at the default capacity, so that segments fill while the shared half holds (the middle), so that
the shared half is exactly full, and so that it is one pair short -- on the whole table, on entity
slices, on the wide sweep and on the lock-step windows. The workspace is decoded by its documented
layout (the comment above BF3_HDR): the flag at word 1, the segment capacity at word 4, the
counters at words 64 + 32 s, the pairs from byte BF3_HDR.

Bar: raw / filtered counts bit-equal to the run at the default capacity, to the score-storing exact
sweep and to the oracle's Test.h restatement (an independent f32 restatement of the canonical
chain; the tables are built from exact ties, so no float64 reference could be the bar); the listed
pairs the same multiset at every capacity, and a superset of the exact ties.

The counters: expected counts in numpy float64 from a table whose scores lie >= 0.05 from
every threshold (f32 rounding of these sums: < 1e-5)."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from test_sweep_filters_gpu import _adversarial_dot, _run, _spec_from

pytestmark = pytest.mark.gpu

BF3_SEGS = 64
BF3_SEG_W0 = 64
BF3_HDR = 4 * (BF3_SEG_W0 + 32 * (BF3_SEGS + 1))
SLICES = ((0, 768), (768, 1664), (1664, None))
SWEEPS = [None, "256", "128"]  # the 128 x 128 sweep, the wide sweep at query tile 256 / 128


@functools.lru_cache(maxsize=None)
def _case(model, seed, E, Q):
    """The adversarial table (nonfinite rows: the bursts of one workgroup the shared half exists
    for), its exact sweep with stored scores and the oracle's counts: computed once, shared."""
    import oracle
    import torch
    from mmre.link import FilterIndex
    oracle.build()
    ent, rel, ent_im, rel_im, qh, qr, qt, qm = _adversarial_dot(model, E=E, seed=seed, nonfinite=True, Q=Q)
    R, d = rel.shape
    rng = np.random.default_rng(seed + 10)
    fh, fr, ft = rng.integers(0, E, 3 * E), rng.integers(0, R, 3 * E), rng.integers(0, E, 3 * E)
    fh, fr, ft = np.concatenate([fh, qh]), np.concatenate([fr, qr]), np.concatenate([ft, qt])
    index = FilterIndex(fh, fr, ft, E, R)
    spec = _spec_from(model, ent, rel, ent_im, rel_im, dim=d)
    exact = _run(spec, qh, qr, qt, qm, index=index, scores=True)
    dev = spec.ent.device
    tq = lambda a, dt=np.int64: torch.from_numpy(np.asarray(a, dt)).to(dev)
    hrt = oracle.sorted_hrt(fh, fr, ft)
    o_counts = np.zeros((2, Q), np.int32)
    for mode_id, mode in ((0, "head_batch"), (1, "tail_batch")):
        sel = qm == mode_id
        o_pred = oracle.link_predict(model, mode, ent, rel, qh[sel], qr[sel], qt[sel], ent_im=ent_im, rel_im=rel_im)
        o_counts[:, sel] = oracle.test_rank(mode, o_pred, qh[sel], qr[sel], qt[sel], hrt)[:, :2].T
    assert np.array_equal(exact["counts"][:2], o_counts)
    # the pairs whose exact f32 score equals their query's truth score (the truth pair among them)
    ties = np.argwhere(exact["scores"] == exact["truth"][:, None])
    assert len(ties) > Q  # the construction has exact ties beyond the truths themselves
    return SimpleNamespace(model=model, E=E, Q=Q, index=index, spec=spec, q=(qh, qr, qt, qm),
                           args=(tq(qh), tq(qr), tq(qt), tq(qm, np.int8)), counts=o_counts,
                           exact=exact["counts"][:2].copy(), ties={(int(q), int(e)) for q, e in ties})


def _select(monkeypatch, wide, blocked=None):
    monkeypatch.setenv("MMRE_BF3_WIDE", "1" if wide else "0")
    if wide:
        monkeypatch.setenv("MMRE_BF3_QT", wide)
    if blocked is None:
        monkeypatch.delenv("MMRE_BF3_BLOCKED", raising=False)
    else:
        monkeypatch.setenv("MMRE_BF3_BLOCKED", "1" if blocked else "0")


def _decode(wk):
    """The list header of the workspace tensor by the documented layout: (flag, segment capacity,
    the 64 segment counters, the shared half's counter)."""
    import torch
    hdr = wk[:BF3_HDR].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    c = hdr[BF3_SEG_W0 + 32 * np.arange(BF3_SEGS + 1)]
    return int(hdr[1]), int(hdr[4]), c[:BF3_SEGS].copy(), int(c[BF3_SEGS])


def _listed(wk):
    """The pairs the list holds (a run that did not overflow): the first min(c_s, seg_cap) slots of
    each segment, then the shared half's appends from pair 64 seg_cap on. Rows (query, entity),
    sorted."""
    import torch
    flag, seg_cap, c, shared = _decode(wk)
    assert flag == 0
    n = BF3_SEGS * seg_cap + shared
    pairs = wk[BF3_HDR:BF3_HDR + 8 * n].view(torch.int32).cpu().numpy().reshape(n, 2)
    keep = [pairs[s * seg_cap:s * seg_cap + min(int(c[s]), seg_cap)] for s in range(BF3_SEGS)]
    keep.append(pairs[BF3_SEGS * seg_cap:])
    out = np.concatenate(keep)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def _bf3(case, monkeypatch, cap=None, entity_range=None, raw=None):
    """One split-bf16 run at list capacity `cap` (None: the default); raw: MMRE_BF3_RAW."""
    import torch
    from mmre.link import LinkSweep
    if cap is None:
        monkeypatch.delenv("MMRE_BF3_CAP", raising=False)
    else:
        monkeypatch.setenv("MMRE_BF3_CAP", str(cap))
    if raw is None:
        monkeypatch.delenv("MMRE_BF3_RAW", raising=False)
    else:
        monkeypatch.setenv("MMRE_BF3_RAW", "1" if raw else "0")
    sw = LinkSweep(case.spec)
    bufs = sw.alloc_queries(case.Q)
    dev = case.spec.ent.device
    filt = tuple(torch.from_numpy(a).to(dev) for a in case.index.groups(*case.q, entity_range=entity_range))
    res = sw.run(*case.args, filt=filt, buffers=bufs, entity_range=entity_range)
    torch.cuda.synchronize()
    st = sw.bf3_stats(bufs)
    assert st is not None
    flag, seg_cap, c, shared = _decode(bufs["bf3_work"])
    assert st["fallback"] == bool(flag) and st["spilled"] == shared, (st, flag, shared)
    if case.model == "distmult":  # d = 48: the raw rows are split directly unless MMRE_BF3_RAW=0
        assert bufs["bf3_raw"] == (raw is not False)
    return SimpleNamespace(counts=res["counts"].cpu().numpy().copy(), st=st, seg_cap=seg_cap, c=c,
                           work=bufs["bf3_work"])


def _spill(c, k):
    return int(np.maximum(0, c - k).sum())


def _mid_k(c):
    """The smallest segment capacity k >= 1 whose overflow the shared half of MMRE_BF3_CAP = 128 k
    (64 k pairs) still holds."""
    k = 1
    while _spill(c, k) > BF3_SEGS * k:
        k += 1
    return k


def _shared_size(cap):
    return cap - BF3_SEGS * (cap // (2 * BF3_SEGS))


def _boundary_caps(c):
    """(cap*, cap-): the first capacity whose shared half is exactly full, and the largest one
    below it whose shared half is one pair short. A host-side search over the counters."""
    top = 2 * BF3_SEGS * (int(c.max()) + 1)
    sp = [_spill(c, k) for k in range(int(c.max()) + 2)]
    full = next(cap for cap in range(1, top + 1) if _shared_size(cap) == sp[cap // (2 * BF3_SEGS)])
    short = max(cap for cap in range(1, full) if _shared_size(cap) == sp[cap // (2 * BF3_SEGS)] - 1)
    return full, short


def _baseline(case, monkeypatch, path, entity_range=None, raw=None, twice=True):
    """The run at the default capacity; its counters are the same on a second run (the bf3 grids
    give every workgroup a static unit range)."""
    base = _bf3(case, monkeypatch, entity_range=entity_range, raw=raw)
    assert not base.st["fallback"], base.st
    assert (base.st["wide"], base.st["blocked"]) == path, base.st
    assert base.st["undecided"] == int(np.minimum(base.c, base.seg_cap).sum()) + base.st["spilled"], base.st
    if twice:
        again = _bf3(case, monkeypatch, entity_range=entity_range, raw=raw)
        assert np.array_equal(again.c, base.c)
        assert np.array_equal(again.counts, base.counts)
    return base


def _check_mid(case, monkeypatch, base, path, entity_range=None, raw=None):
    """Segments full, shared half not: MMRE_BF3_CAP = 128 k for the smallest k the shared half can
    back. Nothing is lost, nothing is listed or rescored twice, the counts do not move."""
    k = _mid_k(base.c)
    spill = _spill(base.c, k)
    assert k < base.c.max() and spill > 0, (k, base.c)  # conditions on the inputs
    mid = _bf3(case, monkeypatch, cap=2 * BF3_SEGS * k, entity_range=entity_range, raw=raw)
    print(f"{case.model} {path} slice {entity_range}: U = {base.st['undecided']}, max c_s = {base.c.max()}, "
          f"k = {k}, spill = {spill} of {BF3_SEGS * k}")
    assert not mid.st["fallback"], mid.st
    assert (mid.st["wide"], mid.st["blocked"]) == path, mid.st
    assert mid.seg_cap == k
    assert mid.st["spilled"] == spill, (mid.st, spill)
    assert mid.st["undecided"] == base.st["undecided"], (mid.st, base.st)
    assert np.array_equal(mid.c, base.c)
    want, got = _listed(base.work), _listed(mid.work)
    assert len(np.unique(want, axis=0)) == len(want) == base.st["undecided"]
    assert np.array_equal(got, want)
    assert np.array_equal(mid.counts, base.counts)
    return mid


@pytest.mark.parametrize("wide", SWEEPS)
@pytest.mark.parametrize("model,seed", [("distmult", 0), ("complex", 0)])
def test_list_between_empty_and_full(monkeypatch, model, seed, wide):
    """The list at the middle capacity and at the exact boundary of the shared half; every
    exact tie is in the list."""
    _select(monkeypatch, wide)
    case = _case(model, seed, 2300, 500 if wide == "256" else 300)
    path = (int(wide or 0), False)
    base = _baseline(case, monkeypatch, path)
    assert np.array_equal(base.counts[:2], case.exact)
    assert np.array_equal(base.counts[:2], case.counts)
    listed = {(int(q), int(e)) for q, e in _listed(base.work)}
    missing = case.ties - listed
    assert not missing, sorted(missing)[:10]
    mid = _check_mid(case, monkeypatch, base, path)
    assert np.array_equal(mid.counts[:2], case.exact) and np.array_equal(mid.counts[:2], case.counts)
    # the exact boundary: the shared half holds cap - 64 floor(cap / 128) pairs
    full, short = _boundary_caps(base.c)
    print(f"{model} {path}: cap* = {full} (shared half {_shared_size(full)}), one short at {short}")
    at = _bf3(case, monkeypatch, cap=full)
    assert not at.st["fallback"], at.st
    assert at.st["spilled"] == _shared_size(full) == _spill(base.c, full // (2 * BF3_SEGS)), at.st
    assert at.st["undecided"] == base.st["undecided"]
    assert np.array_equal(_listed(at.work), _listed(base.work))
    assert np.array_equal(at.counts, base.counts)
    assert np.array_equal(at.counts[:2], case.exact) and np.array_equal(at.counts[:2], case.counts)
    below = _bf3(case, monkeypatch, cap=short)
    assert _shared_size(short) == _spill(base.c, short // (2 * BF3_SEGS)) - 1
    assert below.st["fallback"], below.st
    assert np.array_equal(below.counts, base.counts)
    assert np.array_equal(below.counts[:2], case.exact) and np.array_equal(below.counts[:2], case.counts)


def _check_fallback_slices(case, monkeypatch, base, path_of, slices, raw=None):
    """MMRE_BF3_CAP=64: no segment, a shared half of 64 pairs -- every slice overflows and takes
    the gated exact sweep; the slices' counts sum to the whole table's."""
    total = np.zeros_like(base.counts)
    for e0, e1 in slices:
        r = _bf3(case, monkeypatch, cap=64, entity_range=(e0, e1 or case.E), raw=raw)
        assert r.st["fallback"], (e0, e1, r.st)
        assert (r.st["wide"], r.st["blocked"]) == path_of((e0, e1 or case.E)), r.st
        total += r.counts
    assert np.array_equal(total[:2], base.counts[:2])


@pytest.mark.parametrize("wide", SWEEPS)
@pytest.mark.parametrize("model,raw", [("distmult", True), ("distmult", False), ("complex", None)])
def test_fallback_and_spill_on_entity_slices(monkeypatch, model, raw, wide):
    """Entity slices (e_begin > 0: every rank but the first under entity sharding) through
    the overflow fallback -- DistMult's raw-row path writes the fallback's k-major planes at
    d_ent_km + e_begin -- and through the middle capacity, recomputed per slice."""
    _select(monkeypatch, wide)
    case = _case(model, 0, 2300, 500 if wide == "256" else 300)
    path = (int(wide or 0), False)
    base = _baseline(case, monkeypatch, path, raw=raw, twice=False)
    assert np.array_equal(base.counts[:2], case.exact)
    _check_fallback_slices(case, monkeypatch, base, lambda s: path, SLICES, raw=raw)
    total = np.zeros_like(base.counts)
    for e0, e1 in SLICES:
        rng_ = (e0, e1 or case.E)
        sbase = _baseline(case, monkeypatch, path, entity_range=rng_, raw=raw, twice=False)
        total += _check_mid(case, monkeypatch, sbase, path, entity_range=rng_, raw=raw).counts
    assert np.array_equal(total[:2], base.counts[:2])


@pytest.mark.parametrize("wide", ["256", None])
@pytest.mark.parametrize("model", ["distmult", "complex"])
def test_lockstep_windows_spill_and_fallback(monkeypatch, model, wide):
    """The lock-step windows (MMRE_BF3_BLOCKED=1: BlockMap), on the wide sweep and on the
    128 x 128 one: the middle capacity, and the overflow fallback on the whole table and on two
    slices (18 / 19 tiles of 128, 9 / 10 wide tiles: the windows engage on each)."""
    _select(monkeypatch, wide, blocked=True)
    case = _case(model, 3, 4700, 512)
    path = (int(wide or 0), True)
    base = _baseline(case, monkeypatch, path)
    assert np.array_equal(base.counts[:2], case.exact) and np.array_equal(base.counts[:2], case.counts)
    assert not case.ties - {(int(q), int(e)) for q, e in _listed(base.work)}
    _check_mid(case, monkeypatch, base, path)
    _check_fallback_slices(case, monkeypatch, base, lambda s: path, ((0, None),))
    _check_fallback_slices(case, monkeypatch, base, lambda s: path, ((0, 2304), (2304, None)))


@pytest.mark.parametrize("model", ["distmult", "complex"])
def test_lockstep_windows_off_when_unset(monkeypatch, model):
    """MMRE_BF3_BLOCKED is read per call: unset, the 4,700-entity table of
    test_wide_sweep_lockstep_windows (planes far below 64 MB) sweeps contiguous ranges, whatever an
    earlier call of the process ran with; set, the windows engage; unset again, they do not."""
    case = _case(model, 3, 4700, 512)
    for blocked in (None, True, None, False):
        _select(monkeypatch, "256", blocked=blocked)
        r = _bf3(case, monkeypatch)
        assert r.st["wide"] == 256 and r.st["blocked"] == bool(blocked), (blocked, r.st)
        assert not r.st["fallback"] and np.array_equal(r.counts[:2], case.exact)


# --------------------------------------------- the type-constrained sweep's 16-bit counters ---
TC_TILES = 8200          # entity tiles of 128: one workgroup that sweeps them all adds up to 8 per
TC_E = TC_TILES * 128    # unit to a 16-bit counter -- 65,600 > 65,535
TC_Q = 128               # one query tile


def _tc_table():
    """TransE L1, d = 4, one relation. Every row but the 128 truth rows lies within 0.04 (L1) of
    c = (1, 1, 1, 1); query q's truth row is c + (2 + 0.1 q) e_0. The anchor is a bulk row, so every
    bulk row scores <= 0.14 against a truth score >= 1.9, and truth row q' scores 0.1 (q' - q)
    from truth row q: the scores lie >= 0.05 from every threshold (asserted by the reference)."""
    rng = np.random.default_rng(7)
    ent = (1.0 + rng.uniform(-0.01, 0.01, (TC_E, 4))).astype(np.float32)
    rel = np.array([[0.01, -0.02, 0.0, 0.03]], np.float32)
    ids = rng.choice(TC_E, 2 * TC_Q, replace=False)
    truth, anchor = ids[:TC_Q], ids[TC_Q:]
    ent[truth] = 1.0
    ent[truth, 0] = (3.0 + 0.1 * np.arange(TC_Q)).astype(np.float32)
    qm = (np.arange(TC_Q) % 2).astype(np.int8)           # 0: head batch (the truth is h), 1: tail batch
    qh, qt = np.where(qm == 0, truth, anchor), np.where(qm == 0, anchor, truth)
    qr = np.zeros(TC_Q, np.int64)
    # known triples: the queries and, per query, three bulk entities in the truth's place
    known = rng.choice(TC_E, (TC_Q, 3))
    fh = np.concatenate([qh] + [np.where(qm == 0, known[:, j], qh) for j in range(3)])
    ft = np.concatenate([qt] + [np.where(qm == 0, qt, known[:, j]) for j in range(3)])
    return ent, rel, qh, qr, qt, qm, fh, np.zeros(len(fh), np.int64), ft, known


@functools.lru_cache(maxsize=None)
def _tc_expected():
    """Raw / filtered / type-constrained counts in numpy float64 (Test.h's rule: strictly smaller
    than the truth's score, the truth itself skipped, known entities taken off the filtered
    count; the type lists hold every entity, so the constrained counts equal the plain ones)."""
    ent, rel, qh, qr, qt, qm, fh, fr, ft, known = _tc_table()
    e64 = np.ascontiguousarray(ent.astype(np.float64).T)              # (4, E)
    r64 = rel[0].astype(np.float64)
    truth = np.where(qm == 0, qh, qt)
    anchor = np.where(qm == 0, qt, qh)
    # head batch: |e + r - t|, tail batch: |h + r - e| = |e - (h + r)|
    off = np.where((qm == 0)[:, None], ent[anchor].astype(np.float64) - r64, ent[anchor].astype(np.float64) + r64)
    raw = np.zeros(TC_Q, np.int64)
    filt = np.zeros(TC_Q, np.int64)
    gap, lowest = np.inf, 1 << 30
    for q0 in range(0, TC_Q, 16):
        s = np.zeros((16, TC_E))
        for k in range(4):
            s += np.abs(e64[k][None, :] - off[q0:q0 + 16, k][:, None])
        rows = np.arange(16)
        t = s[rows, truth[q0:q0 + 16]].copy()
        s[rows, truth[q0:q0 + 16]] = np.inf                          # the truth itself is skipped
        gap = min(gap, float(np.abs(s - t[:, None]).min()))
        better = s < t[:, None]
        raw[q0:q0 + 16] = better.sum(1)
        # a thread's counter of a query row sums its 8 columns (4 te + j, 64 + 4 te + j) of every unit
        lowest = min(lowest, int(better.reshape(16, TC_TILES, 2, 16, 4).sum((1, 2, 4)).min()))
        for i in range(16):
            lst = np.unique(known[q0 + i])
            filt[q0 + i] = raw[q0 + i] - int(better[i, lst[lst != truth[q0 + i]]].sum())
    assert gap >= 0.05, gap
    assert lowest > 65535, lowest  # every 16-bit counter of the one workgroup wraps unless it is flushed
    return np.stack([raw, filt, raw, filt]).astype(np.int32)


def _tc_counts():
    """One type-constrained count-only run on the table (whichever sweep the environment selects)."""
    from mmre.link import FilterIndex
    ent, rel, qh, qr, qt, qm, fh, fr, ft, _ = _tc_table()
    every = [np.arange(TC_E)]
    index = FilterIndex(fh, fr, ft, TC_E, 1, every, every)
    spec = _spec_from("transe", ent, rel, norm=False, dim=4)
    out = _run(spec, qh, qr, qt, qm, index=index, tc=True, scores=False)
    return out["counts"], out["l1q"]


def _tc_child():
    counts, st = _tc_counts()
    print("RESULT " + json.dumps({"counts": counts.tolist(), "l1q": st}))


@pytest.mark.parametrize("l1_filter", ["0", "1"])
def test_tc_counters_one_workgroup_owns_the_query_tile(l1_filter):
    """A grid that is no multiple of 8 has one XCD group (n_groups == 1): MMRE_SWEEP_GRID=1 leaves
    all 8,200 units of the one query tile to one workgroup. Its 16-bit LDS counters must be flushed
    on the way: the f32 type-constrained sweep (MMRE_L1_FILTER=0) and the integer filter's. The
    grid knob is read once per process, so each sweep runs in a fresh child."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MMRE_SWEEP_GRID="1", MMRE_FUSED_EVAL="0", MMRE_L1_FILTER=l1_filter)
    env.pop("MMRE_L1_BITS", None)
    code = "import sys; sys.path[:0] = %r; import test_bf3_list_gpu as t; t._tc_child()" % ([here] + sys.path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    st = res["l1q"]
    if l1_filter == "1":  # the integer sweep itself counted (no f32 fallback)
        assert st is not None and not st["fallback"], st
    else:
        assert st is None
    got, want = np.asarray(res["counts"], np.int32), _tc_expected()
    print(f"MMRE_L1_FILTER={l1_filter}: raw count of query 0 {got[0, 0]} (expected {want[0, 0]}), l1q {st}")
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(0))[:10]


def test_tc_counters_default_grid(monkeypatch):
    """The control: the default grid (a multiple of 8: n_groups == 8, 1,025 units of the query
    tile per group) holds the same counts, with the integer filter and without."""
    for l1_filter in ("1", "0"):
        monkeypatch.setenv("MMRE_L1_FILTER", l1_filter)
        monkeypatch.setenv("MMRE_FUSED_EVAL", "0")
        monkeypatch.delenv("MMRE_L1_BITS", raising=False)
        counts, st = _tc_counts()
        assert (st is None) == (l1_filter == "0") and not (st and st["fallback"]), st
        assert np.array_equal(counts, _tc_expected())
