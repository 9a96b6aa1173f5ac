"""The per-query route of the fused TransE L1 evaluation, what holds without a
device: its storage lives in a workspace region that is dead by the time it is written, so no
workspace grows; that region holds a routed list of at least one query for every shape of the
workspace table; the statistics entry point refuses bad arguments before it launches anything; the
sampled columns restated in Python are the documented four windows."""
import numpy as np
import torch  # noqa: F401  (the library binds to torch's HIP runtime)

from test_link_abi_cpu import WORKSPACES, fake

ARG = 1


def test_workspaces_did_not_grow():
    from mmre import _lib
    L = _lib.lib()
    for (dim, e_pad, q_pad), want in WORKSPACES.items():
        assert L.mmre_link_l1q_workspace(dim, e_pad, q_pad) == want[0]
        assert L.mmre_link_evaluate_l1q_workspace(dim, e_pad, q_pad) == want[1]


def test_route_cap_at_least_one_and_at_most_a_sixteenth():
    from mmre import _lib
    L = _lib.lib()
    for dim, e_pad, q_pad in WORKSPACES:
        for n_query in {1, 15, 16, 17, q_pad - 127, q_pad}:
            cap = L.mmre_link_l1q_route_cap(dim, e_pad, q_pad, n_query)
            assert 1 <= cap <= max(1, n_query // 16), (dim, e_pad, q_pad, n_query, cap)
    # the storage bound acts where the queries dwarf the table: K1's region is 8 bytes per block of
    # 16 entity rows / 8 queries, the flag bytes take q_pad of it
    assert L.mmre_link_l1q_route_cap(7, 128, 1048576, 1048576) == 64
    assert L.mmre_link_l1q_route_cap(200, 14336, 35200, 35192) == 1824
    for bad in ((0, 128, 128, 1), (8, 0, 128, 1), (8, 128, 0, 1), (8, 128, 128, 0), (8, 128, 128, 129),
                (8, 100, 128, 1), (8, 128, 100, 1)):
        assert L.mmre_link_l1q_route_cap(*bad) == 0, bad


def test_route_stats_refusals():
    from mmre import _lib
    L = _lib.lib()
    assert L.mmre_link_l1q_route_stats(None, 1 << 20, fake(), None) == ARG
    assert L.mmre_link_l1q_route_stats(fake(), 1 << 20, None, None) == ARG
    assert L.mmre_link_l1q_route_stats(fake(), 0, fake(), None) == ARG
    assert L.mmre_link_l1q_route_stats(fake(), 8191, fake(), None) == ARG  # the header is 8 KB
    assert len(_lib.SIGNATURES["mmre_link_l1q_route_stats"][1]) == 4


def test_sample_columns():
    from mmre.link import l1q_heavy_sample
    c = l1q_heavy_sample(2100)
    assert len(c) == 256 and len(np.unique(c)) == 256
    starts = c[::64]
    assert starts.tolist() == [0, 676, 1356, 2036] and (np.diff(c.reshape(4, 64), axis=1) == 1).all()
    assert c.max() == 2099
    # slices shorter than a window or than the four of them: cut at the end, repeats kept
    assert l1q_heavy_sample(52).tolist() == list(range(52)) * 4
    c = l1q_heavy_sample(128)
    assert len(c) == 256 and c[::64].tolist() == [0, 20, 40, 64] and c.max() == 127
    c = l1q_heavy_sample(14208)
    assert len(c) == 256 and c[::64].tolist() == [0, 4712, 9428, 14144]
