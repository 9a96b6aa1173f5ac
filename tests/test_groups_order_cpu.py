"""FilterIndex.groups(order="size"): the group order of the fused TransE evaluation's grouped
sweep (a group is one sweep row; a 128-row tile costs its largest group). Still a partition of the
queries whose shared list equals every member's own filter list, sizes non-increasing, max_group
respected; the default order is unchanged."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.mark.parametrize("max_group", [1, 3, 8, 64])
def test_size_ordered_groups_are_a_partition(max_group):
    from mmre.data import OpenKEDataset
    from mmre.link import FilterIndex
    d = OpenKEDataset(os.path.join(GOLDEN, "data", "medium"))
    idx = FilterIndex(*d.all_triples(), d.n_ent, d.n_rel)
    h, r, t = d.test_list()
    n = len(h)
    qh, qr, qt = (np.concatenate([x, x]) for x in (h, r, t))
    qm = np.r_[np.zeros(n, np.int8), np.ones(n, np.int8)]
    off, ids = idx.filters(qh, qr, qt, qm)
    gqo, gq, goff, gids, entry_q = idx.groups(qh, qr, qt, qm, max_group=max_group, order="size")
    sizes = np.diff(gqo)
    assert gqo[0] == 0 and gqo[-1] == 2 * n and sizes.min() >= 1 and sizes.max() <= max_group
    assert np.all(np.diff(sizes) <= 0)
    assert gq.dtype == np.int32 and np.array_equal(np.sort(gq), np.arange(2 * n))
    assert len(goff) == len(gqo) and goff[-1] == len(gids) == len(entry_q)
    for g in range(len(gqo) - 1):
        members = gq[gqo[g]:gqo[g + 1]]
        lst = gids[goff[g]:goff[g + 1]].tolist()
        m0 = members[0]
        assert np.all(entry_q[goff[g]:goff[g + 1]] == m0)
        for q in members:
            assert qm[q] == qm[m0] and qr[q] == qr[m0]
            assert (qt[q] == qt[m0]) if qm[q] == 0 else (qh[q] == qh[m0])
            assert ids[off[q]:off[q + 1]].tolist() == lst
    # the same groups as the default order, only rearranged
    k_gqo, k_gq = idx.groups(qh, qr, qt, qm, max_group=max_group)[:2]
    as_sets = lambda o, m: sorted(tuple(m[o[g]:o[g + 1]].tolist()) for g in range(len(o) - 1))
    assert as_sets(gqo, gq) == as_sets(k_gqo, k_gq)


def test_unknown_order_is_refused():
    from mmre.link import FilterIndex
    idx = FilterIndex(np.array([0]), np.array([0]), np.array([1]), 2, 1)
    with pytest.raises(ValueError):
        idx.groups(np.array([0]), np.array([0]), np.array([1]), np.array([0], np.int8), order="heavy")
