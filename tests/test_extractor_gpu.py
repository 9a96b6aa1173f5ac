"""GPU parity of the ZSL Extractor path (csrc/extractor.hip) against the oracle's torch-fp32
restatement of zsl_module.py:47-110 / 666-706 (oracle/zsl_extractor.py; parity unpinned by
reference fixtures, see its header). Tolerance 1e-4 on vectors and matching scores (fp32 MFMA,
reassociated sums); cosine scores 1e-5; ranks exact wherever the true candidate's score is not
within 1e-5 of another candidate's (near ties are screened and counted, not hidden)."""
import numpy as np
import pytest
import torch

from zsl_synth import candidates, embeddings, init_extractor, make_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _pair(dim, seed=0, max_nb=50, bias_scale=0.1, **kw):
    import zsl_extractor as ox
    from module.zsl_module import Extractor, ZSLGraph
    g = make_graph(seed=seed, **kw)
    ent, rel = embeddings(g, dim, seed=seed + 1)
    G = ZSLGraph(g["rel2id"], g["ent2id"], g["train_tasks"], g["test_tasks"], ent, rel, max_neighbor=max_nb)
    ref = ox.ExtractorRef(dim, G.num_symbols, G.symbol2vec)
    init_extractor(ref, seed=seed + 2, bias_scale=bias_scale)
    ex = Extractor(dim, G.num_symbols, G.symbol2vec)
    ex.load_state_dict(ref.state_dict(), strict=True)
    ex = ex.to(DEV).eval()
    return g, G, ref, ex


def _pairs(g, G, n, seed):
    rng = np.random.default_rng(seed)
    ents = [e for e in g["ent2id"] if e != "OOV"]
    a = rng.choice(len(ents), n)
    b = rng.choice(len(ents), n)
    q = np.array([[G.symbol2id[ents[i]], G.symbol2id[ents[j]]] for i, j in zip(a, b)], np.int64)
    return q, [g["ent2id"][ents[i]] for i in a], [g["ent2id"][ents[j]] for j in b]


@pytest.mark.parametrize("dim", [64, 100, 128, 200, 256])
def test_extractor_forward_matches_oracle(dim):
    import zsl_extractor as ox
    g, G, ref, ex = _pair(dim, seed=dim)
    q, ql, qr = _pairs(g, G, 77, 1)       # ragged: 77 rows = 4 full waves + a partial one
    s, sl, sr = _pairs(g, G, 5, 2)
    qm = ox.get_meta(G.connections, dict(enumerate(G.e1_degrees)), ql, qr)
    sm = ox.get_meta(G.connections, dict(enumerate(G.e1_degrees)), sl, sr)
    rq, rs = ref(torch.from_numpy(q), torch.from_numpy(s), qm, sm)
    to = lambda m: tuple(x.to(DEV) for x in m)
    gq, gs = ex(torch.from_numpy(q).to(DEV), torch.from_numpy(s).to(DEV), to(qm), to(sm))
    torch.cuda.synchronize()
    assert gq.shape == rq.shape and gs.shape == rs.shape
    assert (gq.cpu() - rq).abs().max().item() <= 1e-4
    assert (gs.cpu() - rs).abs().max().item() <= 1e-4 * max(1.0, rs.abs().max().item())


def test_extractor_single_query_squeezes_to_scalar():
    import zsl_extractor as ox
    g, G, ref, ex = _pair(200, seed=5)
    q, ql, qr = _pairs(g, G, 1, 3)
    m = ox.get_meta(G.connections, dict(enumerate(G.e1_degrees)), ql, qr)
    rq, rs = ref(torch.from_numpy(q), torch.from_numpy(q), m, m)
    gq, gs = ex(torch.from_numpy(q).to(DEV), torch.from_numpy(q).to(DEV), tuple(x.to(DEV) for x in m),
                tuple(x.to(DEV) for x in m))
    assert gs.dim() == 0 and rs.dim() == 0
    assert abs(gs.item() - rs.item()) <= 1e-4 * max(1.0, abs(rs.item()))


@pytest.mark.parametrize("bias_scale", [0.1, 0.0])
def test_isolated_nodes_follow_reference_division(bias_scale):
    """deg = 0: the reference divides the neighbour sum by zero (zsl_module.py:57); tanh(+-inf)
    = +-1 with a non-zero gcn bias, NaN (0/0) with the zero bias of weights_init."""
    import zsl_extractor as ox
    g, G, ref, ex = _pair(200, seed=9, bias_scale=bias_scale)
    iso = [i for i in range(len(G.e1_degrees)) if G.e1_degrees[i] == 0]
    assert iso
    busy = int(np.argmax(G.e1_degrees))
    ql, qr = [iso[0], busy, iso[-1], busy], [busy, iso[0], iso[0], busy]  # the last row stays finite
    q = np.array([[G.ent_sym[a], G.ent_sym[b]] for a, b in zip(ql, qr)], np.int64)
    m = ox.get_meta(G.connections, dict(enumerate(G.e1_degrees)), ql, qr)
    rq, _ = ref(torch.from_numpy(q), torch.from_numpy(q), m, m)
    gq, _ = ex(torch.from_numpy(q).to(DEV), torch.from_numpy(q).to(DEV), tuple(x.to(DEV) for x in m),
               tuple(x.to(DEV) for x in m))
    a, b = gq.cpu(), rq
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    fin = ~torch.isnan(b)
    assert (a[fin] - b[fin]).abs().max().item() <= 1e-4
    assert (bias_scale == 0.0) == bool(torch.isnan(b).any())


def test_support_encoder_matches_torch():
    from module.submodule import SupportEncoder
    torch.manual_seed(0)
    se = SupportEncoder(200, 400)
    with torch.no_grad():
        se.proj1.bias.normal_(0, 0.1)
        se.proj2.bias.normal_(0, 0.1)
        se.layer_norm.weight.normal_(1, 0.1)
        se.layer_norm.bias.normal_(0, 0.1)
    x = torch.randn(3, 37, 200)
    ref = se.layer_norm(se.proj2(torch.relu(se.proj1(x))) + x).detach()
    se = se.to(DEV).eval()
    out = se(x.to(DEV))
    assert out.shape == x.shape
    assert (out.cpu() - ref).abs().max().item() <= 1e-4


@pytest.mark.parametrize("dim,max_nb", [(200, 50), (100, 10)])
def test_zsl_eval_ranks_match_oracle(dim, max_nb):
    import zsl_extractor as ox
    from module.zsl_module import ZSLEvaluator
    g, G, ref, ex = _pair(dim, seed=11, max_nb=max_nb, n_ent=400, n_test=90)
    cands = candidates(g, n_cand=60, seed=3)
    gen = torch.Generator().manual_seed(4)
    # generated relation vectors share a direction per relation (as a trained generator's do),
    # which spreads the candidates' mean cosines over ~0.1 instead of ~0.02
    rel_vecs = {r: torch.randn(dim, generator=gen) + 0.5 * torch.randn((20, dim), generator=gen) for r in cands}
    ev = ZSLEvaluator(ex, G, device=DEV)
    (ranks, scores), _ = ev.rank({r: v.to(DEV) for r, v in rel_vecs.items()}, cands, return_scores=True)
    torch.cuda.synchronize()
    ranks, scores = ranks.cpu().numpy(), scores.cpu().numpy()
    o_ranks, o_scores = ox.zsl_eval_ranks(ref, G.symbol2id, g["ent2id"], G.connections,
                                          dict(enumerate(G.e1_degrees)), {r: v.numpy() for r, v in rel_vecs.items()},
                                          cands)
    flat = np.concatenate(o_scores)
    assert len(ranks) == len(o_ranks) and len(scores) == len(flat)
    err = np.abs(scores - flat).max()
    assert err <= 1e-5
    tie = max(4 * err, 1e-6)  # near-tie screen: within 4x the observed GPU-vs-oracle score error
    pos, screened = 0, 0
    for i, s in enumerate(o_scores):
        near = np.abs(s[1:] - s[0]) <= tie
        if near.any():
            screened += 1
        else:
            assert ranks[i] == o_ranks[i], (i, ranks[i], o_ranks[i])
        pos += len(s)
    assert screened <= len(o_scores) // 20
    assert (ranks >= 1).all() and (ranks <= np.array([len(s) for s in o_scores])).all()


def test_rank_desc_edge_cases():
    from mmre.extractor import rank_desc
    s = torch.tensor([0.5, 0.1, 0.9, 0.5, 0.3, 0.7, 0.2], device=DEV)
    off = torch.tensor([0, 4, 4, 5, 7], device=DEV)  # one empty list, one singleton
    r = rank_desc(s, off).cpu().tolist()
    assert r == [2, 0, 1, 1]
    # lists longer than one workgroup
    x = torch.rand(5000, generator=torch.Generator().manual_seed(0))
    off = torch.tensor([0, 1000, 5000])
    r = rank_desc(x.to(DEV), off.to(DEV)).cpu().tolist()
    assert r == [1 + int((x[1:1000] > x[0]).sum()), 1 + int((x[1001:] > x[1000]).sum())]


def test_rank_desc_above_grid_cap():
    """16,389 queries against the 16,384-workgroup grid cap: the first five workgroups take a
    second query. Lists of 0-3 entries, the last one empty, one NaN score (never greater)."""
    from mmre.extractor import rank_desc
    rng = np.random.default_rng(5)
    Q = 16389
    lens = rng.integers(0, 4, Q)
    lens[-1] = 0
    lens[:5], lens[16384:16388] = [3, 0, 2, 1, 3], [0, 3, 3, 2]  # q and q + 16384 differ
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s = rng.random(int(off[-1])).astype(np.float32)
    s[off[16385] + 1] = np.nan
    want = np.zeros(Q, np.int64)
    for q in np.flatnonzero(lens):
        a, b = off[q], off[q + 1]
        with np.errstate(invalid="ignore"):
            want[q] = 1 + int((s[a + 1:b] > s[a]).sum())
    r = rank_desc(torch.from_numpy(s).to(DEV), torch.from_numpy(off).to(DEV)).cpu().numpy()
    assert np.array_equal(r, want)
    assert want[-1] == 0 and len(set(want[16384:].tolist())) > 1
