"""The per-query route of the fused TransE L1 evaluation (mmre_link_evaluate_l1q): a
query whose 8-bit band holds a large share of the entities is left out of the code sweep and counted
by an exact f32 sweep of its own. Counts must not move; only where a query is counted does.

Tables (E = 2,100: 16 whole entity tiles and one of 52 columns; d = 40; 640 queries) hold two
kinds of query. Kind A: the truth's row is the query vector plus tiny noise, so the threshold is
near 0 and no sampled pair is inside the band. Kind B: the truth is a random entity of the middle
fifth by score, mid-table, where the scores are densest. A float64 emulation of the 8-bit band (the codes, the error sums and
offsets of the tight bound, the integer thresholds) on the sampled columns fixes the expected routed
set from the inputs: every kind-B query at least twice the flag threshold, every kind-A query 0.
MMRE_L1_HEAVY=1 lets the route act at this size (the call's own rule keeps small evaluations off
it); MMRE_L1_BITS=8 keeps the code-width probe from choosing the 16-bit codes, which it does on
tables with this many mid-table truths (the last test)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_eval_grouped_gpu import _eval, _index, _random_case, _same
from test_link_gpu import _spec_from
from test_sweep_filters_gpu import _adversarial

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E, D, R = 2100, 40, 6
# (members, of them kind A) per key: more than eight members; a full row of kind B; a mixed row;
# a short mixed row; then single-member keys
# (640 queries, 32 of kind B: inside the routed list's cap of a sixteenth of the queries, 40)
KEYS = [(13, 6), (8, 0), (8, 4), (5, 2)] + [(1, 1)] * 596 + [(1, 0)] * 10
FLAG_MIN = 26  # ceil(0.10 x 256 sampled columns): L1Q_HEAVY_FRAC of the sample


def ab_workload(seed=0):
    """ent, rel, (qh, qr, qt, qm), is_b. Kind-A truths are entities of their own outside the sampled
    columns, never anchors; their rows are overwritten with the query vector plus noise."""
    from mmre.link import l1q_heavy_sample
    rng = np.random.default_rng(seed)
    er = 8.0 / (2 * D)
    ent = rng.uniform(-er, er, (E, D)).astype(np.float32)
    rel = rng.uniform(-er, er, (R, D)).astype(np.float32)
    n_a = sum(a for _, a in KEYS)
    sampled = set(l1q_heavy_sample(E).tolist())
    pool = rng.permutation([e for e in range(E) if e not in sampled])
    a_truth, anchors = pool[:n_a], pool[n_a:n_a + len(KEYS)]
    # one large value (an entity nobody samples, anchors on or ranks as a truth) sets the code step:
    # four times the step the other values alone would give, so the band of a mid-table truth is wide
    ent[pool[n_a + len(KEYS)], 0] = 8 * er
    ordinary = np.setdiff1d(np.arange(E), np.r_[a_truth, pool[n_a + len(KEYS)]])
    qh, qr, qt, qm, is_b = [], [], [], [], []
    ai = 0
    for k, (n, na) in enumerate(KEYS):
        mode, r, anchor = int(rng.integers(0, 2)), int(rng.integers(0, R)), int(anchors[k])
        vec = ent[anchor] - rel[r] if mode == 0 else ent[anchor] + rel[r]  # head batch: |e + r - t|
        for m in range(n):
            if m < na:
                tr = int(a_truth[ai])
                ai += 1
                ent[tr] = vec + rng.uniform(-1e-6, 1e-6, D).astype(np.float32)
            else:  # mid-table: a random one of the middle fifth of the ordinary entities by score
                cand = ordinary[ordinary != anchor]
                by_score = cand[np.argsort(np.abs(ent[cand].astype(np.float64) - vec).sum(1), kind="stable")]
                tr = int(rng.choice(by_score[2 * len(cand) // 5:3 * len(cand) // 5]))
            qh.append(tr if mode == 0 else anchor)
            qt.append(anchor if mode == 0 else tr)
            qr.append(r)
            qm.append(mode)
            is_b.append(m >= na)
    p = rng.permutation(len(qh))
    f = lambda x, dt=np.int64: np.asarray(x, dt)[p]
    return ent, rel, (f(qh), f(qr), f(qt), f(qm, np.int8)), f(is_b, bool)


def band_counts(ent, rel, q, cols):
    """Per query, the sampled columns inside its 8-bit band (its truth left out): float64
    restatement of k_eval_quant_list's codes and tight bound and of l1_int_thresholds, whole table,
    no row normalisation."""
    qh, qr, qt, qm = q
    kt = ent.shape[1]
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    vec = np.where((qm == 0)[:, None], e64[qt] - r64[qr], e64[qh] + r64[qr]).astype(np.float32).astype(np.float64)
    truth = np.where(qm == 0, qh, qt)
    th = np.abs(vec - e64[truth]).sum(1)
    m = max(np.abs(vec).max(), np.abs(e64).max())
    delta = 2.0 * m / 255.0
    l1f = (kt + 4) * 2.0 ** -23 * (1 + 2.0 ** -8)

    def quant(x):
        code = np.rint(np.clip((x + m) * (255.0 / (2.0 * m)), 0, 255))
        return code, 1.01 * np.abs(x - (code * delta - m)).sum(1) + kt * 2.0 ** -20 * m

    cq, eb_q = quant(vec)
    ce, eb_e = quant(np.r_[e64, np.zeros((1, kt))])  # (the last row: a padding column of the last tile)
    off = np.ceil(eb_e / (delta * (1 - l1f)) * (1 + 2.0 ** -17))
    o_max = off.max()
    x = (th - eb_q) / (delta * (1 + l1f)) * (1 - 2.0 ** -18)
    y = (th + eb_q) / (delta * (1 - l1f)) * (1 + 2.0 ** -18)
    ts = np.where(x > 0, np.floor(x), 0.0)
    to = np.where(y > 0, np.ceil(y) + 2 * o_max, 0.0)
    acc = np.abs(cq[:, None, :] - ce[cols][None, :, :]).sum(2) + off[cols][None, :]
    inside = (acc >= ts[:, None]) & (acc < to[:, None]) & (cols[None, :] != truth[:, None])
    return inside.sum(1)


@pytest.fixture(scope="module")
def work():
    ent, rel, q, is_b = ab_workload()
    index, trip = _index(q[0], q[1], q[2], R)
    return dict(ent=ent, rel=rel, q=q, is_b=is_b, index=index, trip=trip)


def _env(monkeypatch, heavy="1", bits="8", cap=None, hmin=None, hcap=None):
    for k, v in (("MMRE_L1_HEAVY", heavy), ("MMRE_L1_BITS", bits), ("MMRE_GROUP_CAP", cap),
                 ("MMRE_L1_HEAVY_MIN", hmin), ("MMRE_L1_HEAVY_CAP", hcap)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(spec, q, filt, monkeypatch, **kw):
    """_eval (the grouped tests') plus the route's record and routed ids of the same buffers."""
    from mmre.link import LinkSweep
    seen = {}
    real = LinkSweep.l1q_stats

    def spy(self, bufs):
        seen["route"] = self.l1q_route_stats(bufs)
        seen["ids"] = self.l1q_routed(bufs)
        return real(self, bufs)

    monkeypatch.setattr(LinkSweep, "l1q_stats", spy)
    out = _eval(spec, q, filt, True, monkeypatch, **kw)
    monkeypatch.setattr(LinkSweep, "l1q_stats", real)
    out.update(seen)
    return out


def _groups(work, spec, **kw):
    from mmre.link import group_args
    return work["index"].groups(*work["q"], **(kw or group_args(spec)))


def test_inputs_fix_the_routed_set(work):
    from mmre.link import l1q_heavy_sample
    cols = l1q_heavy_sample(E)
    assert len(cols) == 256
    n = band_counts(work["ent"], work["rel"], work["q"], cols)
    b = work["is_b"]
    print("kind B sampled band:", n[b].min(), n[b].max(), "kind A:", n[~b].max())
    assert b.sum() == sum(m - a for m, a in KEYS) and (n[b] >= 2 * FLAG_MIN).all() and (n[~b] == 0).all()


@pytest.mark.parametrize("cap", ["8", None], ids=["grouped", "ungrouped"])
def test_base(oracle_mod, monkeypatch, work, cap):
    """Kind B routed, kind A not; counts equal to route-off, the f32 sweep and the oracle."""
    qh, qr, qt, qm = work["q"]
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    filt = _groups(work, spec)
    _env(monkeypatch, cap=cap)
    on = _run(spec, work["q"], filt, monkeypatch, und=True)
    _env(monkeypatch, heavy="0", cap=cap)
    off = _run(spec, work["q"], filt, monkeypatch, und=True)
    n_b = int(work["is_b"].sum())
    assert on["route"] == dict(flagged=n_b, routed=n_b, sample=256, threshold=FLAG_MIN), on["route"]
    assert np.array_equal(on["ids"], np.flatnonzero(work["is_b"]))
    assert off["route"] == dict(flagged=0, routed=0, sample=0, threshold=0) and len(off["ids"]) == 0
    assert np.array_equal(on["counts"], off["counts"])
    assert on["st"]["guarded"] == 0 and on["st"]["bits"] == 8 and not on["st"]["fallback"]
    assert on["st"]["undecided"] < off["st"]["undecided"], (on["st"], off["st"])
    # a routed query's entry is its f32 row's cost in rescored pairs: ceil(4.3 x 2,100 / 90)
    assert (on["und_q"][work["is_b"]] == 101).all()
    assert np.array_equal(on["und_q"][~work["is_b"]], off["und_q"][~work["is_b"]])
    assert on["und_q"][~work["is_b"]].sum() == on["st"]["undecided"]
    monkeypatch.setenv("MMRE_L1_FILTER", "0")
    f32 = _eval(spec, work["q"], _groups(work, spec), True, monkeypatch)
    monkeypatch.delenv("MMRE_L1_FILTER")
    assert f32["st"] is None and np.array_equal(on["counts"], f32["counts"])
    hrt = oracle_mod.sorted_hrt(*work["trip"])
    for mode_id, mode in ((0, "head_batch"), (1, "tail_batch")):
        sel = qm == mode_id
        o_pred = oracle_mod.link_predict("transe", mode, work["ent"], work["rel"], qh[sel], qr[sel], qt[sel],
                                         norm_flag=False)
        o_c = oracle_mod.test_rank(mode, o_pred, qh[sel], qr[sel], qt[sel], hrt)
        assert np.array_equal(on["counts"][:2, sel].T, o_c[:, :2])


@pytest.mark.parametrize("hcap,want", [(1, 1), (128, 128), (129, 129), (200, 129)])
def test_everything_flagged(monkeypatch, work, hcap, want):
    """MMRE_L1_HEAVY_MIN=0 flags every query; the cap below, at and above the 129 flagged: 1, 128
    (one whole tile of the indexed sweep), 129 routed -- the first ones in query order, twice alike."""
    q = tuple(a[:129] for a in work["q"])
    index, _ = _index(q[0], q[1], q[2], R)
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    from mmre.link import group_args
    filt = index.groups(*q, **group_args(spec))
    _env(monkeypatch, heavy="0", cap="8")
    off = _run(spec, q, filt, monkeypatch)
    _env(monkeypatch, cap="8", hmin=0, hcap=hcap)
    one = _run(spec, q, filt, monkeypatch, und=True)
    two = _run(spec, q, filt, monkeypatch, und=True, reps=2)
    for r in (one, two):
        assert r["route"] == dict(flagged=129, routed=want, sample=256, threshold=0), r["route"]
        assert np.array_equal(r["ids"], np.arange(want))
        assert np.array_equal(r["counts"], off["counts"]) and r["st"]["guarded"] == 0
    assert one["st"] == two["st"] and np.array_equal(one["und_q"], two["und_q"])
    if want == 129:
        assert one["st"]["undecided"] == 0


def test_nothing_flagged(monkeypatch, work):
    """A threshold no count reaches: the whole record equals route-off."""
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    filt = _groups(work, spec)
    _env(monkeypatch, cap="8", hmin=10 ** 6)
    on = _run(spec, work["q"], filt, monkeypatch, und=True)
    _env(monkeypatch, heavy="0", cap="8")
    off = _run(spec, work["q"], filt, monkeypatch, und=True)
    _same(on, off)
    assert on["route"] == dict(flagged=0, routed=0, sample=256, threshold=10 ** 6)
    assert np.array_equal(on["und_q"], off["und_q"]) and on["st"] == off["st"]


def test_grouped_rows(monkeypatch, work):
    """Eight member slots: the 13-member key spans two rows, one row is all kind B (every slot
    emptied), two rows mix the kinds. Counts equal the ungrouped run's, route on and off."""
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    filt = _groups(work, spec)
    sizes = np.diff(filt[0])
    assert sizes.max() == 8 and (sizes == 8).sum() >= 3 and 5 in sizes
    b_of = work["is_b"][filt[1]]
    rows = [b_of[a:b] for a, b in zip(filt[0][:-1], filt[0][1:]) if b - a > 1]
    assert any(r.all() for r in rows) and any(r.any() and not r.all() for r in rows)
    _env(monkeypatch, cap="8")
    grouped = _run(spec, work["q"], filt, monkeypatch, und=True)
    _env(monkeypatch, cap=None)
    flat = _run(spec, work["q"], _groups(work, spec, max_group=1, order="size"), monkeypatch, und=True)
    assert np.array_equal(grouped["counts"], flat["counts"])
    assert grouped["route"] == flat["route"] and np.array_equal(grouped["ids"], flat["ids"])
    assert grouped["st"]["undecided"] == flat["st"]["undecided"] and np.array_equal(grouped["und_q"], flat["und_q"])


@pytest.mark.parametrize("huge", [False, True])
@pytest.mark.parametrize("hmin", [0, 3])
def test_adversarial_tables(monkeypatch, huge, hmin):
    """Exact ties, one-ulp copies, zero and subnormal rows (huge: a 3e19 row and a NaN -- a
    non-finite code step, every pair rescored; NaN truths) with the route forced: counts equal to
    the separate path's, whichever queries the route takes."""
    from mmre.link import group_args
    ent, rel, qh, qr, qt, qm = _adversarial(E=E, d=D, Q=300, seed=2 if huge else 3, model="transe", huge=huge)
    if huge:
        qt[5], qm[5] = int(np.flatnonzero(np.isnan(ent).any(1))[0]), 1  # a NaN truth
    q = (qh.astype(np.int64), qr.astype(np.int64), qt.astype(np.int64), qm.astype(np.int8))
    index, _ = _index(q[0], q[1], q[2], rel.shape[0])
    spec = _spec_from("transe", ent, rel, dim=D, norm=True)
    filt = index.groups(*q, **group_args(spec))
    for cap in ("8", None):
        _env(monkeypatch, cap=cap, hmin=hmin, hcap=150)
        on = _run(spec, q, filt, monkeypatch)
        _env(monkeypatch, heavy="0", cap=cap)
        sep = _eval(spec, q, filt, False, monkeypatch)
        assert np.array_equal(on["counts"], sep["counts"]), cap
        assert on["st"]["guarded"] == 0 and on["route"]["routed"] <= 150
        if hmin == 0 and not on["st"]["fallback"]:
            assert on["route"]["routed"] == 150 and np.array_equal(on["ids"], np.arange(150))


def test_slices_repeats_and_graph_replays(monkeypatch, work):
    """Three entity slices (each with its own sample) sum to the whole table; three calls and three
    graph replays over poisoned counts give the same table and the same record."""
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    _env(monkeypatch, cap="8")
    once = _run(spec, work["q"], _groups(work, spec), monkeypatch)
    again = _run(spec, work["q"], _groups(work, spec), monkeypatch, reps=3, graph=True)
    _same(once, again)
    assert once["route"] == again["route"] and np.array_equal(once["ids"], again["ids"])
    assert once["route"]["routed"] == work["is_b"].sum()
    from mmre.link import group_args
    total = np.zeros_like(once["counts"])
    for er in ((0, 768), (768, 1536), (1536, E)):
        filt = work["index"].groups(*work["q"], entity_range=er, **group_args(spec))
        part = _run(spec, work["q"], filt, monkeypatch, entity_range=er)
        assert part["st"]["guarded"] == 0 and part["route"]["sample"] == 256
        total += part["counts"]
    assert np.array_equal(total, once["counts"])


def test_sixteen_bit_codes_keep_the_route_inert(monkeypatch, work):
    """MMRE_L1_BITS=16, and the probe's own choice of the 16-bit codes on this table (a twentieth of
    its queries are mid-table): nothing routed, the record equal to route-off."""
    spec = _spec_from("transe", work["ent"], work["rel"], dim=D, norm=False)
    filt = _groups(work, spec)
    for bits in ("16", None):
        _env(monkeypatch, bits=bits, cap="8")
        on = _run(spec, work["q"], filt, monkeypatch, und=True)
        _env(monkeypatch, heavy="0", bits=bits, cap="8")
        off = _run(spec, work["q"], filt, monkeypatch, und=True)
        assert on["st"]["bits"] == 16, bits
        assert on["route"] == dict(flagged=0, routed=0, sample=0, threshold=0), on["route"]
        _same(on, off)
        assert on["st"] == off["st"] and np.array_equal(on["und_q"], off["und_q"])
