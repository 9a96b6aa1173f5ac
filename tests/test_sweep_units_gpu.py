"""The TransH / TransD / TransR sweeps (k_sweep_transh, k_sweep_transr) where a workgroup sweeps
SEVERAL units: the loader moving to the next unit a stage ahead, the double-buffered query-tile
metadata and type words, the per-row counts kept in LDS until the query tile is left, the tile's
relation / (a, n) columns / plane / w_hat / type row changing under a running workgroup, the
XCD-grouped unit map and its leftover branch. The other synthetic cases of these families are 30
units on a grid of 30 workgroups: one unit each, one group.

No launcher hook: the grid is the production one. plan_tiles(qr, tile=t) makes query tiles of at
most t live rows (the kernels pad the rest), so a few thousand queries are a few thousand query
tiles, and the Python mirror of the unit map (tests/test_sweep_units_cpu.py) says, from the
device's CU count, what the grid then does -- asserted before anything is launched.

    A  E = 2200 (18 entity tiles: 8 XCD groups own 2 each and share 2 leftover ones), ~16 x CUs
       query tiles of 1..3 rows over 256 relations: >= 4 units per workgroup
    B  E = 300 (3 entity tiles, one group), ~85 x CUs query tiles of one row: >= 4 units per workgroup
    C  E = 1100 (9 entity tiles: 8 groups own 1 each and share 1), the 751-query mix in 10 full
       tiles: 160 workgroups for 90 units, so some own nothing; the leftover branch at one unit

The yardstick is the numpy restatement (sweep_scores + rank_counts); counts and truth bit-equal."""
import numpy as np
import pytest
import torch

import test_sweep_units_cpu as U
import transd_restate as RD
import transh_restate as RH
import transr_restate as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COPY, ZERO_E, ZERO_EP, SRC = 5, 7, 9, 11            # hand-placed entity rows (COPY copies SRC); LAST = E - 1
NARROW = {"transh": 6, "transd": (7, 5), "transr": (5, 4)}        # kp = 8: one K stage per unit
WIDE = {"transh": 20, "transd": (20, 20), "transr": (12, 20)}     # kp = 24: three stages
FAMILIES = ("transh", "transd", "transr")


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------ queries ---
def make_queries(E, n_rel, per_rel, seed, known_per_query=4):
    """Queries (both modes mixed, the caller's order not by relation), known triples that hit
    them and random type lists, after the make_case functions of tests/test_trans{h,d,r}_gpu.py.
    The zero entity, the copied entity with its source and the last entity stand as truth and as
    anchor under the first three relations that have eight queries: `special` (the tables make
    the first two of them special relations)."""
    rng = np.random.default_rng(seed)
    per_rel = np.asarray(per_rel, np.int64)
    qr = np.repeat(np.arange(n_rel), per_rel)
    n = len(qr)
    last = E - 1
    qh, qt = rng.integers(0, E, n), rng.integers(0, E, n)
    qm = rng.integers(0, 2, n).astype(np.int8)
    special = [int(r) for r in np.nonzero(per_rel >= 8)[0][:3]]
    assert len(special) == 3
    for r in special:
        i = int(np.nonzero(qr == r)[0][0])
        qh[i], qm[i] = ZERO_E, 0                                     # the zero entity as truth
        qt[i + 1], qm[i + 1] = ZERO_E, 0                             # ... and as the anchor
        qt[i + 2], qm[i + 2] = last, 1                               # truth E - 1 (tail side)
        qh[i + 3], qm[i + 3] = last, 0                               # truth E - 1 (head side)
        qt[i + 4], qm[i + 4] = last, 0                               # E - 1 as the anchor
        qt[i + 5], qm[i + 5] = SRC, 1                                # COPY ties with this truth
        qt[i + 6], qm[i + 6] = COPY, 1
        qh[i + 7], qm[i + 7] = COPY, 1                               # ... and as the anchor
    order = rng.permutation(n)
    qh, qr, qt, qm = qh[order], qr[order].astype(np.int64), qt[order], qm[order]
    kn = known_per_query * n
    kh, kr, kt = rng.integers(0, E, kn), rng.integers(0, n_rel, kn), rng.integers(0, E, kn)
    # half of the known triples share a query's (h, r) or (r, t), so the filter lists are not empty
    pick = rng.integers(0, n, kn // 2)
    kh[:kn // 4], kr[:kn // 4] = qh[pick[:kn // 4]], qr[pick[:kn // 4]]
    kr[kn // 4:kn // 2], kt[kn // 4:kn // 2] = qr[pick[kn // 4:]], qt[pick[kn // 4:]]
    kh, kr, kt = (np.concatenate([a, b]) for a, b in ((kh, qh), (kr, qr), (kt, qt)))
    types = np.zeros((2, n_rel, E), bool)                            # [head side / tail side][relation][entity]
    for side in range(2):
        for r in range(n_rel):
            types[side, r, rng.choice(E, int(rng.integers(20, E)), replace=False)] = True
    return dict(E=E, n_rel=n_rel, qh=qh, qr=qr, qt=qt, qm=qm, known=(kh, kr, kt), types=types, special=special)


def index_queries(s, filt):
    """The filter index, its device groups and masks and the host lists the restatement counts with."""
    from mmre.link import FilterIndex
    lists = [[np.nonzero(row)[0] for row in s["types"][side]] for side in range(2)]
    idx = FilterIndex(*s["known"], s["E"], s["n_rel"], *lists)
    s["masks"] = tuple(to(m) for m in idx.type_masks())
    s["lists"] = None
    if filt:
        s["groups"] = tuple(to(a) for a in idx.groups(s["qh"], s["qr"], s["qt"], s["qm"]))
        off, ids = idx.filters(s["qh"], s["qr"], s["qt"], s["qm"])
        s["lists"] = [ids[off[i]:off[i + 1]] for i in range(len(s["qh"]))]
        assert np.diff(off).min() >= 1 and np.diff(off).max() >= 2
    s["allowed"] = s["types"][np.where(s["qm"] == 0, 0, 1), s["qr"]]
    s["truth_id"] = np.where(s["qm"] == 0, s["qh"], s["qt"])
    s["dev"] = {k: to(s[k]) for k in ("qh", "qr", "qt", "qm")}
    return s


# ------------------------------------------------------------------------------- tables ---
def make_tables(fam, dims, s):
    """One family's tables for the query set s: the zero entity, the copied entity; the first
    special relation with the zero normal / zero transfer row / zero matrix, the second with a zero
    relation vector (TransR: and the identity matrix)."""
    f = np.float32
    E, n_rel = s["E"], s["n_rel"]
    ra, rb = s["special"][:2]
    rng = np.random.default_rng(1000 + 31 * FAMILIES.index(fam) + 7 * int(np.sum(dims)) + E)
    u = lambda *shape: rng.uniform(-0.5, 0.5, shape).astype(f)
    if fam == "transh":
        T = dict(ent=u(E, dims), rel=u(n_rel, dims), nv=u(n_rel, dims))
        T["nv"][ra] = 0.0                                            # w_hat = 0: no projection
    elif fam == "transd":
        de, dr = dims
        T = dict(ent=u(E, de), ept=u(E, de), rel=u(n_rel, dr), rpt=u(n_rel, dr))
        T["rpt"][ra] = 0.0                                           # u = e under this relation
        T["ept"][ZERO_EP] = 0.0                                      # s = 0
        T["ept"][COPY] = T["ept"][SRC]
    else:
        de, dr = dims
        T = dict(ent=u(E, de), rel=u(n_rel, dr), tm=u(n_rel, de, dr))
        T["tm"][ra] = 0.0                                            # every entity projects to 0: all tie
        T["tm"][rb] = 0.0
        T["tm"][rb][np.arange(min(de, dr)), np.arange(min(de, dr))] = 1.0
        T["tm"] = T["tm"].reshape(n_rel, de * dr)
    T["rel"][rb] = 0.0
    T["ent"][ZERO_E] = 0.0
    T["ent"][COPY] = T["ent"][SRC]
    T["dev"] = {k: to(v) for k, v in T.items()}
    return T


def spec_of(fam, T, p_norm, norm_flag, margin):
    from mmre.link import ScoreSpec
    d = T["dev"]
    kw = dict(model=fam if p_norm == 1 else fam + "_l2", ent=d["ent"], rel=d["rel"], dim=d["rel"].shape[1],
              norm_flag=norm_flag, pred_kind=0 if margin is None else 1, margin=margin or 0.0)
    if fam == "transh":
        kw.update(norm_vec=d["nv"])
    elif fam == "transd":
        kw.update(ent_transfer=d["ept"], rel_transfer=d["rpt"], dim_e=d["ent"].shape[1])
    else:
        kw.update(transfer_matrix=d["tm"], dim_e=d["ent"].shape[1])
    return ScoreSpec(**kw)


def sweep_of(fam, spec):
    from mmre.transd import TransDSweep
    from mmre.transh import TransHSweep
    from mmre.transr import TransRSweep
    return {"transh": TransHSweep, "transd": TransDSweep, "transr": TransRSweep}[fam](spec)


def restate(fam, T, q, p_norm, norm_flag):
    """The restatement's (Q, E) scores without a margin (predict's m - (m - s) is applied on top)."""
    if fam == "transh":
        return RH.sweep_scores(T["ent"], T["rel"], T["nv"], *q, p_norm, norm_flag, None)
    if fam == "transd":
        return RD.sweep_scores(T["ent"], T["ept"], T["rel"], T["rpt"], *q, p_norm, norm_flag, None)
    return RR.sweep_scores(T["ent"], T["rel"], T["tm"], *q, p_norm, norm_flag, None)


_shapes, _tables, _scores = {}, {}, {}


def tables(shape, fam, dims, s):
    key = (shape, fam, dims)
    if key not in _tables:
        _tables[key] = make_tables(fam, dims, s)
    return _tables[key]


def wanted(shape, fam, dims, s, T, p_norm, norm_flag, margin):
    """(scores, counts) of the restatement; the margin-free scores of the latest configuration are
    kept (consecutive parameters share them), never changed."""
    key = (shape, fam, dims, p_norm, norm_flag)
    if _scores.get("key") != key:
        _scores.clear()
        _scores.update(key=key, s=restate(fam, T, (s["qh"], s["qr"], s["qt"], s["qm"]), p_norm, norm_flag))
    want_s = RH.pred(_scores["s"], margin)
    return want_s, RH.rank_counts(want_s, s["truth_id"], s["lists"], s["allowed"])


def run(sw, s, plan, filt=True, masks=True, sel=None):
    d = s["dev"] if sel is None else {k: v[to(sel)] for k, v in s["dev"].items()}
    res = sw.run(d["qh"], d["qr"], d["qt"], d["qm"], filt=s["groups"] if filt else None,
                 type_masks=s["masks"] if masks else None, plan=plan)
    return res["counts"].cpu().numpy(), res["truth"].cpu().numpy()


# ------------------------------------------------------------------------------ shape A ---
A_E, A_REL = 2200, 259
A_ABSENT = (0, 100, 258)                            # relations of the table without a query
A_THREES = (3, 11, 19)                              # r % 24 in here: tiles of three rows, else one row


def a_tile_of(r):
    return 3 if r % 24 in A_THREES else 1


def shape_a():
    """256 relations with queries, `per` (16 at 256 CUs) or a few more each: the smallest `per`
    at which every XCD group has 4 units for each of its 8 x CUs workgroups."""
    if "A" not in _shapes:
        n_et = -(-A_E // U.TE)
        per = 16
        while True:
            per_rel = np.array([0 if r in A_ABSENT else per + (A_THREES.index(r % 24) if r % 24 in A_THREES else 0)
                                for r in range(A_REL)])
            n_qt = int(sum(-(-c // a_tile_of(r)) for r, c in enumerate(per_rel)))
            if min(U.UnitMap(g, 8, n_qt, n_et).count for g in range(8)) >= 4 * 8 * cus():
                break
            per += 1
        s = index_queries(make_queries(A_E, A_REL, per_rel, seed=41), filt=True)
        s["plan"] = U.mixed_plan(s["qr"], {r: 3 for r in range(A_REL) if a_tile_of(r) == 3})
        assert len(s["plan"]["tiles"]) == n_qt
        s["per"] = per
        _shapes["A"] = s
    return _shapes["A"]


def check_grid_a(s):
    """The arithmetic that makes shape A mean something, from the device's CU count."""
    n_cu = cus()
    n_qt, n_et = len(s["plan"]["tiles"]), -(-A_E // U.TE)
    assert n_et == 18 and set(s["plan"]["tiles"][:, 2].tolist()) == {1, 2, 3}
    assert sorted(set(range(A_REL)) - set(s["plan"]["used"].tolist())) == list(A_ABSENT)
    # the relation changes every `per` tiles at the most (16 at 256 CUs)
    assert np.diff(np.nonzero(np.diff(s["plan"]["tiles"][:, 0]))[0]).max() == s["per"]
    assert U.sweep_units(n_qt, n_et) >= 64 * n_cu                     # the grid is 16 x resident, not the unit count
    units = []
    for per in (1, 2, 3, 4):                                          # whatever the occupancy: at most 4 per CU
        g, n_groups = U.launch_grid(n_qt, n_et, per * n_cu)
        assert g == 16 * per * n_cu and n_groups == 8
        um = U.UnitMap(0, 8, n_qt, n_et)
        assert (um.m, um.r) == (2, 2)
        units.append(min(U.UnitMap(grp, 8, n_qt, n_et).count for grp in range(8)) // (g // 8))
    assert U.busiest_count(n_qt, n_et, 8) / (8 * n_cu) >= 4 and min(units) >= 4
    visits, per_wg, crossing, leftover = U.walk(n_qt, n_et, 64 * n_cu, 8)
    assert np.all(visits == 1) and per_wg.min() >= 4 and crossing > 32 * n_cu and leftover == 2 * n_qt
    return per_wg


def check_a(fam, dims, p_norm, norm_flag, margin):
    from mmre.transh import plan_tiles
    s = shape_a()
    per_wg = check_grid_a(s)
    T = tables("A", fam, dims, s)
    want_s, want = wanted("A", fam, dims, s, T, p_norm, norm_flag, margin)
    Q = len(s["qh"])
    sw = sweep_of(fam, spec_of(fam, T, p_norm, norm_flag, margin))
    got, truth = run(sw, s, s["plan"])
    print(f"A {fam} {dims} p{p_norm} norm {norm_flag} margin {margin}: {len(s['plan']['tiles'])} query tiles, "
          f"{per_wg.min()}..{per_wg.max()} units per workgroup, counts differing "
          f"{int((got != want).any(0).sum())} of {Q} queries, truth differing "
          f"{int((truth != want_s[np.arange(Q), s['truth_id']]).sum())}")
    assert np.array_equal(got, want)
    assert np.array_equal(truth, want_s[np.arange(Q), s["truth_id"]])
    assert want[0].max() > 1000 and (want[1] < want[0]).any() and (want[3] < want[2]).any()
    # two runs give the same bits
    again, truth2 = run(sw, s, s["plan"])
    assert np.array_equal(again, got) and np.array_equal(truth2, truth)
    # raw: no filter, no type masks
    raw, _ = run(sw, s, s["plan"], filt=False, masks=False)
    assert np.array_equal(raw[0], want[0]) and np.array_equal(raw[1], want[0]) and not raw[2:].any()
    # the padded rows count nothing: full 128-row tiles give the same counts
    full, _ = run(sw, s, plan_tiles(s["qr"]))
    assert np.array_equal(full, got)
    # a relation without a query leaves the others' counts as they were: every 16th relation dropped
    keep = np.nonzero(s["qr"] % 16 != 7)[0]
    sub_plan = U.mixed_plan(s["qr"][keep], {r: 3 for r in range(A_REL) if a_tile_of(r) == 3})
    assert len(sub_plan["used"]) < len(s["plan"]["used"])
    sub, sub_truth = run(sw, s, sub_plan, filt=False, masks=False, sel=keep)
    assert np.array_equal(sub[0], want[0][keep]) and np.array_equal(sub_truth, truth[keep])


CONFIGS = [(1, True, None), (1, True, 5.0), (2, False, None), (2, False, 5.0)]   # consecutive ones share scores


@pytest.mark.parametrize("p_norm,norm_flag,margin", CONFIGS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_grouped_several_units_per_workgroup_one_stage(fam, p_norm, norm_flag, margin):
    check_a(fam, NARROW[fam], p_norm, norm_flag, margin)


@pytest.mark.parametrize("fam", FAMILIES)
def test_grouped_several_units_per_workgroup_three_stages(fam):
    check_a(fam, WIDE[fam], 1, True, None)


# ------------------------------------------------------------------------------ shape B ---
B_E, B_REL = 300, 512
B_ABSENT = (0, 200, 511)


def shape_b():
    if "B" not in _shapes:
        n_q = -(-4 * 64 * cus() // 3)                                 # 3 * tiles / (64 * CUs) >= 4
        used = B_REL - len(B_ABSENT)
        per_rel, j = np.zeros(B_REL, np.int64), 0
        for r in range(B_REL):
            if r not in B_ABSENT:
                per_rel[r] = n_q // used + (j < n_q % used)
                j += 1
        s = index_queries(make_queries(B_E, B_REL, per_rel, seed=43), filt=False)
        from mmre.transh import plan_tiles
        s["plan"] = plan_tiles(s["qr"], tile=1)
        _shapes["B"] = s
    return _shapes["B"]


@pytest.mark.parametrize("fam", ["transh", "transr"])
def test_one_group_several_units_per_workgroup(fam):
    from mmre.transh import plan_tiles
    s = shape_b()
    n_cu = cus()
    n_qt, n_et = len(s["plan"]["tiles"]), 3
    assert n_qt == len(s["qh"]) and 3 * n_qt / (64 * n_cu) >= 4
    for per in (1, 2, 3, 4):
        g, n_groups = U.launch_grid(n_qt, n_et, per * n_cu)
        assert g == 16 * per * n_cu and n_groups == 1 and 3 * n_qt // g >= 4
    visits, per_wg, crossing, leftover = U.walk(n_qt, n_et, 64 * n_cu, 1)
    assert np.all(visits == 1) and per_wg.min() >= 4 and crossing == 64 * n_cu and leftover == 0
    dims, (p_norm, norm_flag, margin) = NARROW[fam], (1, True, None)
    T = tables("B", fam, dims, s)
    want_s, want = wanted("B", fam, dims, s, T, p_norm, norm_flag, margin)
    Q = len(s["qh"])
    sw = sweep_of(fam, spec_of(fam, T, p_norm, norm_flag, margin))
    got, truth = run(sw, s, s["plan"], filt=False)
    print(f"B {fam} {dims}: {n_qt} query tiles, {per_wg.min()}..{per_wg.max()} units per workgroup, counts differing "
          f"{int((got != want).any(0).sum())} of {Q} queries")
    # no filter: the filtered columns are the raw ones
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[3], got[2])
    assert np.array_equal(truth, want_s[np.arange(Q), s["truth_id"]])
    assert (want[2] < want[0]).any() and want[0].max() > 200
    again, truth2 = run(sw, s, s["plan"], filt=False)
    assert np.array_equal(again, got) and np.array_equal(truth2, truth)
    # the padded rows count nothing: full 128-row tiles give the same counts
    full, _ = run(sw, s, plan_tiles(s["qr"]), filt=False)
    assert np.array_equal(full, got)
    # a relation without a query leaves the others' counts as they were
    keep = np.nonzero(s["qr"] % 16 != 7)[0]
    sub, _ = run(sw, s, plan_tiles(s["qr"][keep], tile=1), filt=False, sel=keep)
    assert np.array_equal(sub, got[:, keep])


# ------------------------------------------------------------------------------ shape C ---
C_E, C_REL = 1100, 8
C_PER_REL = [0, 1, 127, 128, 129, 300, 2, 64]       # the 751-query mix of the other synthetic cases


def shape_c():
    if "C" not in _shapes:
        from mmre.transh import plan_tiles
        s = index_queries(make_queries(C_E, C_REL, C_PER_REL, seed=47), filt=True)
        s["plan"] = plan_tiles(s["qr"])
        _shapes["C"] = s
    return _shapes["C"]


@pytest.mark.parametrize("fam", FAMILIES)
def test_grouped_fewer_units_than_workgroups(fam):
    s = shape_c()
    n_cu = cus()
    n_qt, n_et = len(s["plan"]["tiles"]), -(-C_E // U.TE)
    assert (n_qt, n_et) == (10, 9)
    g, n_groups = U.launch_grid(n_qt, n_et, n_cu)                     # the unit count, whatever the occupancy
    assert (g, n_groups) == (160, 8) == U.launch_grid(n_qt, n_et, 4 * n_cu) and g % 8 == 0
    um = U.UnitMap(0, 8, n_qt, n_et)
    assert (um.m, um.r) == (1, 1)
    visits, per_wg, crossing, leftover = U.walk(n_qt, n_et, g, n_groups)
    assert np.all(visits == 1) and (per_wg == 0).sum() == 70 and per_wg.max() == 1 and leftover == 10
    dims, (p_norm, norm_flag, margin) = WIDE[fam], (1, True, None)
    T = tables("C", fam, dims, s)
    want_s, want = wanted("C", fam, dims, s, T, p_norm, norm_flag, margin)
    Q = len(s["qh"])
    sw = sweep_of(fam, spec_of(fam, T, p_norm, norm_flag, margin))
    got, truth = run(sw, s, s["plan"])
    print(f"C {fam} {dims}: counts differing {int((got != want).any(0).sum())} of {Q} queries")
    assert np.array_equal(got, want)
    assert np.array_equal(truth, want_s[np.arange(Q), s["truth_id"]])
    again, truth2 = run(sw, s, s["plan"])
    assert np.array_equal(again, got) and np.array_equal(truth2, truth)
    raw, _ = run(sw, s, s["plan"], filt=False, masks=False)
    assert np.array_equal(raw[0], want[0]) and np.array_equal(raw[1], want[0]) and not raw[2:].any()
    # padded rows (relations 1, 6 and 7 fill 1, 2 and 64 rows of their tiles) and the absent
    # relation 0 count nothing: without relation 5's 300 queries the others keep their counts
    keep = np.nonzero(s["qr"] != 5)[0]
    from mmre.transh import plan_tiles
    sub, _ = run(sw, s, plan_tiles(s["qr"][keep]), filt=False, masks=False, sel=keep)
    assert np.array_equal(sub[0], want[0][keep])
