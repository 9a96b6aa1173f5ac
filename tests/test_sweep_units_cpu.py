"""The unit map of the TransH / TransD / TransR sweeps without a GPU: a Python mirror of what
th_launch_sweep / tr_launch_sweep and the head of k_sweep_transh / k_sweep_transr compute
(link_common.h: sweep_units, xcd_groups, UnitMap; transh.hip: THUnitMap, the same map), walked for
every workgroup of a grid. tests/test_sweep_units_gpu.py takes its shapes' arithmetic from here:
how many units a workgroup sweeps, how many XCD groups there are, whether the leftover branch of
the map runs. Also the plans of short query tiles those shapes are made of."""
import numpy as np
import pytest

from test_transh_cpu import check_plan

TQ = TE = 128


# --------------------------------------------------------------------------- the mirror ---
def sweep_units(n_qt, n_et):
    """link_common.h sweep_units: the units of the busiest XCD group times 8, or all units."""
    return 8 * n_qt * ((n_et + 7) // 8) if n_et >= 8 else n_qt * n_et


def xcd_groups(g, n_et):
    """link_common.h xcd_groups, of a grid of g workgroups."""
    return 8 if (g % 8 == 0 and n_et >= 8) else 1


def launch_grid(n_qt, n_et, resident):
    """th_launch_sweep / tr_launch_sweep: (workgroups, n_groups) for `resident` resident
    workgroups (resident_groups: CUs x min(occupancy, 4), so at most 4 x CUs)."""
    g = 16 * resident
    units = sweep_units(n_qt, n_et)
    if units < g:
        g = units if units > 0 else 1
    return g, xcd_groups(g, n_et)


class UnitMap:
    """THUnitMap / UnitMap (query-tile major) of XCD group `grp`."""

    def __init__(self, grp, n_groups, n_qt, n_et):
        self.m = n_et // n_groups
        self.r = n_et - self.m * n_groups
        self.ex0 = grp * self.m
        self.el0 = self.m * n_groups
        self.n_main = n_qt * self.m
        left = n_qt * self.r
        self.lo0 = left * grp // n_groups
        self.count = self.n_main + left * (grp + 1) // n_groups - self.lo0

    def at(self, i):
        """Unit i (< count) -> (query tile, entity tile, taken from the leftover tiles?)."""
        if i < self.n_main:
            return i // self.m, self.ex0 + i % self.m, False
        j = self.lo0 + (i - self.n_main)
        return j // self.r, self.el0 + j % self.r, True


def workgroup_ranges(n_qt, n_et, g, n_groups):
    """[(grp, u0, u1)] of every workgroup of the grid, as the sweep kernels' first lines."""
    per_grp = g // n_groups
    out = []
    for b in range(g):
        grp, gmem = b % n_groups, b // n_groups
        count = UnitMap(grp, n_groups, n_qt, n_et).count
        out.append((grp, gmem * count // per_grp, (gmem + 1) * count // per_grp))
    return out


def busiest_count(n_qt, n_et, n_groups):
    return max(UnitMap(grp, n_groups, n_qt, n_et).count for grp in range(n_groups))


def walk(n_qt, n_et, g, n_groups):
    """Every workgroup's units: visits (n_qt, n_et) int, units per workgroup, workgroups that
    cross a query-tile boundary, units taken through the leftover branch."""
    visits = np.zeros((n_qt, n_et), np.int64)
    maps = [UnitMap(grp, n_groups, n_qt, n_et) for grp in range(n_groups)]
    per_wg, crossing, leftover = [], 0, 0
    for grp, u0, u1 in workgroup_ranges(n_qt, n_et, g, n_groups):
        assert 0 <= u0 <= u1 <= maps[grp].count
        tiles = set()
        for i in range(u0, u1):
            qt, et, left = maps[grp].at(i)
            assert 0 <= qt < n_qt and 0 <= et < n_et
            visits[qt, et] += 1
            tiles.add(qt)
            leftover += left
        per_wg.append(u1 - u0)
        crossing += len(tiles) > 1
    return visits, np.array(per_wg), crossing, leftover


def mixed_plan(qr, tile_of_rel, default=1):
    """A plan whose relation r has query tiles of at most tile_of_rel.get(r, default) rows: the
    tiles of plan_tiles(qr, tile=t) for every t in use, a relation's rows taken from its own t.
    The permutation and the used relations do not depend on t. padding: against full 128-row tiles."""
    from mmre.transh import plan_tiles
    qr = np.asarray(qr, np.int64)
    plans = {t: plan_tiles(qr, tile=t) for t in sorted({default, *tile_of_rel.values()})}
    base = plans[default]
    parts = []
    for r in base["used"]:
        t = plans[tile_of_rel.get(int(r), default)]["tiles"]
        parts.append(t[t[:, 0] == r])
    tiles = np.ascontiguousarray(np.concatenate(parts).astype(np.int32).reshape(-1, 3))
    return dict(perm=base["perm"], tiles=tiles, used=base["used"], padding=float(len(tiles) * TQ / max(len(qr), 1)))


# ----------------------------------------------------------------------------- the tests ---
# (n_qt, n_et, resident workgroups): the existing suite's shape (one unit per workgroup, one group);
# shapes A, B and C of tests/test_sweep_units_gpu.py at 256 CUs x 4; A and B on a smaller device;
# a grid that is no multiple of 8 with n_et >= 8; n_et = 8 and 16 (no leftover tile), 7 and 15;
# more workgroups than the busiest group's share; one query tile; one unit.
SHAPES = [(10, 3, 1024), (3776, 18, 1024), (21846, 3, 1024), (10, 9, 1024), (1200, 18, 304), (3000, 3, 120),
          (37, 9, 5), (50, 8, 2), (40, 16, 16), (33, 7, 3), (21, 15, 8), (3, 23, 1024), (1, 9, 1024), (1, 1, 1024),
          (129, 18, 1)]


@pytest.mark.parametrize("n_qt,n_et,resident", SHAPES)
def test_every_unit_is_swept_exactly_once(n_qt, n_et, resident):
    g, n_groups = launch_grid(n_qt, n_et, resident)
    assert 1 <= g <= 16 * resident and g % n_groups == 0
    visits, per_wg, crossing, leftover = walk(n_qt, n_et, g, n_groups)
    assert np.all(visits == 1)
    assert per_wg.sum() == n_qt * n_et
    # the static ranges are even: two workgroups of one group differ by at most one unit
    for grp in range(n_groups):
        mine = per_wg[grp::n_groups]
        assert mine.max() - mine.min() <= 1
        assert mine.sum() == UnitMap(grp, n_groups, n_qt, n_et).count
    m, r = n_et // n_groups, n_et % n_groups
    assert leftover == n_qt * r and (n_groups == 1) == (m == n_et)


def test_the_shapes_of_the_gpu_file():
    """What tests/test_sweep_units_gpu.py asserts from the device's CU count, at 256 CUs."""
    cus = 256
    # the existing synthetic cases: 30 units, 30 workgroups of one unit each, one group
    g, n_groups = launch_grid(10, 3, 4 * cus)
    assert (g, n_groups) == (30, 1)
    assert walk(10, 3, g, n_groups)[1].tolist() == [1] * 30
    # A: 8 groups of 2 whole entity tiles and a share of 2 leftover ones; >= 4 units per workgroup
    g, n_groups = launch_grid(3776, 18, 4 * cus)
    assert (g, n_groups) == (64 * cus, 8)
    assert busiest_count(3776, 18, 8) >= 4 * 8 * cus
    visits, per_wg, crossing, leftover = walk(3776, 18, g, n_groups)
    assert per_wg.min() >= 4 and crossing > g // 2 and leftover == 2 * 3776
    # B: one group, >= 4 units per workgroup
    g, n_groups = launch_grid(21846, 3, 4 * cus)
    assert (g, n_groups) == (64 * cus, 1)
    assert walk(21846, 3, g, n_groups)[1].min() >= 4
    # C: 160 workgroups in 8 groups of 20 for 11 or 12 units each: some own nothing
    g, n_groups = launch_grid(10, 9, 4 * cus)
    assert (g, n_groups) == (160, 8)
    visits, per_wg, crossing, leftover = walk(10, 9, g, n_groups)
    assert set(per_wg.tolist()) == {0, 1} and (per_wg == 0).sum() == 160 - 90 and leftover == 10
    # a smaller grid only gives a workgroup more units
    for resident in (cus, 2 * cus, 3 * cus):
        g, n_groups = launch_grid(3776, 18, resident)
        assert n_groups == 8 and busiest_count(3776, 18, 8) * n_groups // g >= 4


def test_short_tile_plans():
    from mmre.transh import plan_tiles
    rng = np.random.default_rng(5)
    counts = [0, 1, 2, 3, 4, 16, 17, 0, 7]
    qr = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    for tile in (1, 3):
        plan = plan_tiles(qr, tile=tile)
        check_plan(qr, plan, tile=tile)
        assert plan["tiles"][:, 2].max() == tile and plan["padding"] == len(plan["tiles"]) * tile / len(qr)
    assert len(plan_tiles(qr, tile=1)["tiles"]) == len(qr)
    three = plan_tiles(qr, tile=3)["tiles"]
    assert three[three[:, 0] == 5][:, 2].tolist() == [3, 3, 3, 3, 3, 1]
    assert three[three[:, 0] == 6][:, 2].tolist() == [3, 3, 3, 3, 3, 2]
    # the mixed plan: relation 5 and 6 in threes, every other relation one row per tile
    mixed = mixed_plan(qr, {5: 3, 6: 3})
    perm, tiles = mixed["perm"], mixed["tiles"]
    assert tiles.dtype == np.int32 and np.array_equal(perm, plan_tiles(qr)["perm"])
    covered = np.zeros(len(qr), int)
    for rel, first, rows in tiles:
        assert 1 <= rows <= (3 if rel in (5, 6) else 1)
        assert np.all(qr[perm[first:first + rows]] == rel)
        covered[first:first + rows] += 1
    assert np.all(covered == 1)
    assert np.all(np.diff(tiles[:, 0]) >= 0) and np.all(np.diff(tiles[:, 1]) > 0)   # a relation's tiles consecutive
    assert len(tiles) == 1 + 2 + 3 + 4 + 6 + 6 + 7 and mixed["used"].tolist() == [1, 2, 3, 4, 5, 6, 8]
