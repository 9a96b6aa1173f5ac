"""Row-tile-affine claims of the grouped sweep (mmre_link_evaluate_l1q): a workgroup
takes the next unclaimed unit of its own row tile in its XCD group and moves, to the lowest row
tile that still has a unit, only when that tile is exhausted -- one claim counter per (group, row
tile) and one hint per group, zeroed by the call's first kernel.

Bar: everything the call leaves in HBM bit-identical to the separate entry points
(MMRE_FUSED_EVAL=0) and to the sequential counter (MMRE_SWEEP_AFFINE=0), the same undecided-pair
record, no guarded pair -- at every grid that makes workgroups claim, and over graph replays (the
counters are zeroed inside the call). A dropped or doubled unit shows only if the unit holds a
counted pair, so every (row tile, entity tile) block of a case is first shown, from the oracle's
scores, to hold a pair that beats its member's truth. The counters themselves are read back: after
an affine run every group's hint stands at the row tiles' count and every tile's counter is at
least its units -- the affine claims ran, and ran to the end.

Shapes: d = 40 (two K stages: dynamic scheduling live), cap 8, 700 keys of 1-8 members = 700 rows
= 6 row tiles (the last of 60 rows), ~1,900 queries; E = 2,100 (17 entity tiles: m = 2 per group
and one leftover tile, whose 6 units are shared out over the groups) and E = 900 (8 tiles: m = 1,
no leftover, the last group's tile of 4 columns). Grids (MMRE_SWEEP_GRID; the default gives a
workgroup per unit, which claims nothing further): 8 (one workgroup per group walks every tile),
16, 24, 3 (no multiple of 8: one group owns every entity tile) and the default. Xavier-initialised
tables: truths rank mid-table."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_eval_grouped_gpu import _eval, _same
from test_link_gpu import _spec_from

pytestmark = pytest.mark.gpu
CAP, D, TILE = 8, 40, 128
N_KEYS, R = 700, 6
SIZES = np.resize([1, 2, 3, 4, 1, 2, 8, 1], N_KEYS)
_CASES: dict = {}
_REFS: dict = {}


def _case(E):
    """Tables, queries, groups (a row each, by descending size) and the oracle's score rows."""
    from mmre.link import FilterIndex
    if E in _CASES:
        return _CASES[E]
    rng = np.random.default_rng(100 + E)
    lim = lambda n: np.sqrt(6.0 / (n + D))
    ent = rng.uniform(-lim(E), lim(E), (E, D)).astype(np.float32)
    rel = rng.uniform(-lim(R), lim(R), (R, D)).astype(np.float32)
    keys = rng.permutation(2 * R * E)[:N_KEYS]  # distinct (mode, r, anchor)
    k = np.repeat(keys, SIZES)
    mode, r, anchor = k // (R * E), (k // E) % R, k % E
    truth = rng.integers(0, E, len(k))
    p = rng.permutation(len(k))
    q = tuple(np.ascontiguousarray(x[p]) for x in (np.where(mode == 0, truth, anchor).astype(np.int64),
                                                    r.astype(np.int64),
                                                    np.where(mode == 0, anchor, truth).astype(np.int64),
                                                    mode.astype(np.int8)))
    # known triples: random ones and the queries' own
    known = [np.r_[rng.integers(0, n, 3 * E), x] for n, x in ((E, q[0]), (R, q[1]), (E, q[2]))]
    index = FilterIndex(*known, E, R)
    filt = index.groups(*q, max_group=CAP, order="size")
    _CASES[E] = dict(ent=ent, rel=rel, q=q, filt=filt)
    return _CASES[E]


def _assert_every_block_counts(oracle_mod, case, E):
    """Every (row tile, entity tile) block holds a pair that beats its member's truth."""
    qh, qr, qt, qm = case["q"]
    gqo, gq = case["filt"][0], case["filt"][1]
    assert np.diff(gqo).max() == CAP and len(gqo) - 1 == N_KEYS  # a sweep row per group, in group order
    n_qt, n_et = -(-N_KEYS // TILE), -(-E // TILE)
    assert n_qt == 6
    beats = np.zeros((len(qh), E), bool)
    for mode_id, mode in ((0, "head_batch"), (1, "tail_batch")):
        sel = np.flatnonzero(qm == mode_id)
        s = oracle_mod.link_predict("transe", mode, case["ent"], case["rel"], qh[sel], qr[sel], qt[sel],
                                    norm_flag=True)
        tr = (qh if mode_id == 0 else qt)[sel]
        b = s < s[np.arange(len(sel)), tr][:, None]
        b[np.arange(len(sel)), tr] = False
        beats[sel] = b
    for t in range(n_qt):
        members = gq[gqo[t * TILE]:gqo[min((t + 1) * TILE, N_KEYS)]]
        per_col = beats[members].any(axis=0)
        for e in range(n_et):
            assert per_col[e * TILE:(e + 1) * TILE].any(), (t, e)


def _claim_counters(sw_bufs, dim, e_pad, q_pad):
    """The claim counters of the last affine run, (8 groups, stride): column 0 the group's hint,
    column 1 + t row tile t's claims -- the last words of the row map's row_cnt, which sits before
    row_of_q (q_pad words) and tile_m (a word per query tile, padded to 256 B) at the workspace's
    end (link.hip: eval_layout, l1q_affine_stride)."""
    from mmre import _lib
    total = int(_lib.lib().mmre_link_evaluate_l1q_workspace(dim, e_pad, q_pad))
    stride = (1 + q_pad // TILE + 31) // 32 * 32
    end = total - (4 * (q_pad // TILE) + 255) // 256 * 256 - 4 * q_pad
    wk = sw_bufs["l1q_work"]
    return wk[end - 4 * 8 * stride:end].cpu().numpy().view(np.uint32).reshape(8, stride).astype(np.int64)


def _eval_keep(spec, case, monkeypatch, **kw):
    """_eval, and the claim counters its last run left."""
    from mmre.link import LinkSweep
    kept = {}
    orig = LinkSweep.alloc_queries

    def alloc(self, n):
        kept["b"], kept["sw"] = orig(self, n), self
        return kept["b"]

    monkeypatch.setattr(LinkSweep, "alloc_queries", alloc)
    out = _eval(spec, case["q"], case["filt"], True, monkeypatch, **kw)
    monkeypatch.setattr(LinkSweep, "alloc_queries", orig)
    out["claims"] = _claim_counters(kept["b"], D, kept["sw"].e_pad, kept["b"]["q_pad"])
    return out


def _units(E, grid, n_qt):
    """Per XCD group, the units of every row tile (UnitMap: m main units, then the tile's run of the
    group's share of the leftover units)."""
    n_et = -(-E // TILE)
    ng = 8 if grid % 8 == 0 and n_et >= 8 else 1
    m, r = n_et // ng, n_et % ng
    out = np.full((ng, n_qt), m, np.int64)
    for g in range(ng):
        lo0, lo1 = n_qt * r * g // ng, n_qt * r * (g + 1) // ng
        for t in range(n_qt):
            out[g, t] += max(0, min(lo1, (t + 1) * r) - max(lo0, t * r))
    assert out.sum() == n_qt * n_et
    return out


def _reference(oracle_mod, E, bits, monkeypatch):
    """The separate entry points' result and the sequential counter's at the default grid, once per
    (E, bits) -- and before any test sets MMRE_SWEEP_GRID."""
    monkeypatch.setenv("MMRE_GROUP_CAP", str(CAP))
    monkeypatch.setenv("MMRE_L1_BITS", bits)
    monkeypatch.delenv("MMRE_SWEEP_GRID", raising=False)
    monkeypatch.delenv("MMRE_SWEEP_AFFINE", raising=False)
    monkeypatch.delenv("MMRE_SWEEP_CHUNK", raising=False)
    case = _case(E)
    spec = _spec_from("transe", case["ent"], case["rel"], dim=D, norm=True)
    if (E, bits) not in _REFS:
        if not case.get("checked"):
            _assert_every_block_counts(oracle_mod, case, E)
            case["checked"] = True
        _REFS[(E, bits)] = _eval(spec, case["q"], case["filt"], False, monkeypatch)
        assert _REFS[(E, bits)]["st"]["bits"] == int(bits)
    return case, spec, _REFS[(E, bits)]


def _check(oracle_mod, monkeypatch, E, grid, bits, **kw):
    case, spec, sep = _reference(oracle_mod, E, bits, monkeypatch)
    if grid is not None:
        monkeypatch.setenv("MMRE_SWEEP_GRID", str(grid))
    monkeypatch.setenv("MMRE_SWEEP_AFFINE", "0")
    seq = _eval(spec, case["q"], case["filt"], True, monkeypatch)
    monkeypatch.delenv("MMRE_SWEEP_AFFINE")
    aff = _eval_keep(spec, case, monkeypatch, **kw)
    _same(aff, sep)
    _same(aff, seq)
    # the claims ran, and to the end: every tile's counter holds at least its units (each failed
    # claim adds one more), every group's hint stands at the row tiles' count
    n_qt = 6
    units = _units(E, grid if grid is not None else 8 * n_qt * (-(-E // TILE)), n_qt)
    claims = aff["claims"]
    for g in range(units.shape[0]):
        assert claims[g, 0] == n_qt, (g, claims[g, :1 + n_qt])
        assert (claims[g, 1:1 + n_qt] >= units[g]).all(), (g, claims[g, 1:1 + n_qt], units[g])
        # at most one failed claim per workgroup and tile on the way out
        wgs = max(1, (grid or 0) // units.shape[0]) if grid is not None else None
        if wgs is not None:
            assert (claims[g, 1:1 + n_qt] <= units[g] + 2 * wgs).all(), (g, claims[g, 1:1 + n_qt], units[g])
    assert (claims[units.shape[0]:, :1 + n_qt] == 0).all()


@pytest.mark.parametrize("grid", [8, 16, 24, 3, None])
@pytest.mark.parametrize("E", [2100, 900])
def test_affine_claims_equal_sequential_and_separate(oracle_mod, monkeypatch, E, grid):
    _check(oracle_mod, monkeypatch, E, grid, "8")


@pytest.mark.parametrize("grid", [8, 24])
def test_affine_claims_16_bit_codes(oracle_mod, monkeypatch, grid):
    _check(oracle_mod, monkeypatch, 2100, grid, "16")


def test_affine_claims_over_graph_replays(oracle_mod, monkeypatch):
    """Three calls, then three replays of the captured call over poisoned counts: the counters are
    zeroed inside the call, by a kernel node of the graph."""
    _check(oracle_mod, monkeypatch, 2100, 16, "8", reps=3, graph=True)
