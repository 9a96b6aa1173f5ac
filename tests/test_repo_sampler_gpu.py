"""The repo's per-edge filtered sampler (k_sampler_repo, csrc/sampler.hip) at its edges.

Reference: the allowed sets, by brute force with Python sets from the whole triples (independent
of the sampler's CSR and binary searches), and the reference's rule for the distribution
(module/NegativeSampling.py:321-375): uniform over the allowed local nodes, a fair head/tail split.
Contract under test: layout [pos | neg_1 | ... | neg_k], heads corrupted first, a filtered node
never emitted while an allowed one exists, same-side negatives of a positive distinct while that
side has enough allowed nodes, otherwise every allowed node used once before any repeats."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _known(whole):
    """(global t, r) -> known global heads ; (global h, r) -> known global tails."""
    kh, kt = {}, {}
    for h, r, t in zip(*(np.asarray(x).tolist() for x in whole)):
        kh.setdefault((t, r), set()).add(h)
        kt.setdefault((h, r), set()).add(t)
    return kh, kt


def _sample(sampler, eh, et, er, neg, n_local, l2g):
    ei, ety = sampler.sample(torch.from_numpy(np.stack([eh, et])).to(DEV), torch.from_numpy(er).to(DEV), neg, n_local,
                             None if l2g is None else torch.from_numpy(l2g).to(DEV))
    torch.cuda.synchronize()
    return ei.cpu().numpy(), ety.cpu().numpy()


def _check(ei, ety, eh, et, er, neg, n_local, l2g, filt, whole, in_whole=None):
    """Every invariant of one sampled batch. Returns per positive (head negatives, tail negatives)."""
    B = len(er)
    g = (lambda x: int(x)) if l2g is None else (lambda x: int(l2g[x]))
    kh, kt = _known(whole)
    assert ei.shape == (2, B * (1 + neg)) and ety.shape == (B * (1 + neg),)
    assert ei.dtype == np.int64 and ety.dtype == np.int64
    assert np.array_equal(ei[0, :B], eh) and np.array_equal(ei[1, :B], et)  # the positives lead
    assert np.array_equal(ety, np.tile(er, 1 + neg))                        # relation copied
    assert ei.min() >= 0 and ei.max() < n_local
    out = []
    for b in range(B):
        h, t, r = int(eh[b]), int(et[b]), int(er[b])
        h2 = ei[0, b + B * np.arange(1, neg + 1)]
        t2 = ei[1, b + B * np.arange(1, neg + 1)]
        assert np.all((h2 == h) | (t2 == t)), b                              # never both sides
        bad_h = {x for x in range(n_local) if g(x) in kh.get((g(t), r), ())} if filt else set()
        bad_t = {x for x in range(n_local) if g(x) in kt.get((g(h), r), ())} if filt else set()
        if filt and (in_whole is None or in_whole[b]):
            assert h in bad_h and t in bad_t
            assert np.all((h2 != h) ^ (t2 != t)), b                         # exactly one side corrupted
        # heads first, then tails: rows equal to the positive (possible only where the positive
        # itself is allowed) may sit on either side of the boundary, so some boundary must fit
        lo = int(np.flatnonzero(h2 != h).max()) + 1 if np.any(h2 != h) else 0
        hi = int(np.flatnonzero(t2 != t).min()) if np.any(t2 != t) else neg
        assert lo <= hi, (b, h2, t2)
        fits = None
        for n_head in range(lo, hi + 1):
            heads, tails = h2[:n_head].tolist(), t2[n_head:].tolist()
            ok = not (set(heads) & bad_h) and not (set(tails) & bad_t)      # filter respected
            for side, bad in ((heads, bad_h), (tails, bad_t)):
                allowed = n_local - len(bad)
                ok = ok and len(set(side)) == min(len(side), allowed)       # distinct / all used once
            if ok:
                fits = (heads, tails)
                break
        assert fits is not None, (b, h, t, r, h2, t2)
        out.append(fits)
    return out


def _graph(rng, B, n_rel, l2g_kind, N=60):
    """N local nodes, 3,000 whole triples dense on them (and, under a map, on 40 globals outside
    the local list), B positives. The first positives are the key edges: both filter keys the
    smallest of their CSR, both the largest, and -- not a whole triple -- both absent."""
    if l2g_kind == "none":
        l2g, universe = None, np.arange(N, dtype=np.int64)
    else:
        if l2g_kind == "perm":
            universe = np.sort(rng.permutation(800)[:N + 40]).astype(np.int64)
        else:  # ids up to 3e9: keys g * n_rel + r above 2^32
            universe = np.unique(rng.integers(0, 3_000_000_000, N + 40)).astype(np.int64)
            assert len(universe) == N + 40
        inner = rng.permutation(universe[1:-1])[:N - 2]
        l2g = rng.permutation(np.concatenate([universe[[0, -1]], inner]))  # both extremes are local
    glob = (lambda x: np.asarray(x, np.int64)) if l2g is None else (lambda x: l2g[np.asarray(x, np.int64)])
    lmin, lmax = (0, N - 1) if l2g is None else (int(np.argmin(l2g)), int(np.argmax(l2g)))
    iso = [x for x in range(N) if x not in (lmin, lmax)][:2]  # two local nodes in no whole triple
    pool = np.setdiff1d(universe, glob(iso))
    wh, wr, wt = rng.choice(pool, 3000), rng.integers(0, n_rel, 3000), rng.choice(pool, 3000)
    eh, et, er = rng.integers(0, N, B), rng.integers(0, N, B), rng.integers(0, n_rel, B)
    for x in (eh, et):
        x[np.isin(x, iso)] = lmin
    edges = [(lmin, 0, lmin), (lmax, n_rel - 1, lmax), (iso[0], n_rel - 1, iso[1])]
    in_whole = np.ones(B, bool)
    for i, (h, r, t) in enumerate(edges if B >= 3 else edges[:1]):
        eh[i], er[i], et[i] = h, r, t
        in_whole[i] = i != 2
    wh = np.concatenate([wh, glob(eh[in_whole])])
    wr = np.concatenate([wr, er[in_whole]])
    wt = np.concatenate([wt, glob(et[in_whole])])
    return (wh, wr, wt), l2g, eh.astype(np.int64), et.astype(np.int64), er.astype(np.int64), in_whole


CASES = [  # B, neg, local_to_global, filter_flag, n_rel. Between them: B in {1, 63, 64, 65, 1000} (the
    # launch uses 64 threads per workgroup), neg in {0, 1, 10}, every map, filter on / off, n_rel in {1, 23}
    (1, 10, "none", True, 23),
    (63, 1, "perm", True, 1),
    (64, 10, "big", True, 23),
    (65, 0, "perm", False, 23),
    (1000, 10, "big", False, 1),
    (1000, 1, "none", True, 23),
]


@pytest.mark.parametrize("B,neg,l2g_kind,filt,n_rel", CASES)
def test_invariants(B, neg, l2g_kind, filt, n_rel):
    from mmre.sampler import RepoSampler
    rng = np.random.default_rng(B * 100 + neg)
    N = 60
    whole, l2g, eh, et, er, in_whole = _graph(rng, B, n_rel, l2g_kind, N)
    s = RepoSampler(list(whole), n_rel, DEV, filter_flag=filt, seed=3)
    g = (lambda x: int(x)) if l2g is None else (lambda x: int(l2g[x]))
    for keys, node in ((s.hf[0].cpu().numpy(), et), (s.tf[0].cpu().numpy(), eh)):  # the key edges
        assert keys[0] == g(node[0]) * n_rel + er[0]
        if B >= 3:
            assert keys[-1] == g(node[1]) * n_rel + er[1]
            assert g(node[2]) * n_rel + er[2] not in set(keys.tolist())
        if l2g_kind == "big" and n_rel > 1:
            assert keys[-1] > 2 ** 32
    ei, ety = _sample(s, eh, et, er, neg, N, l2g)
    _check(ei, ety, eh, et, er, neg, N, l2g, filt, whole, in_whole)


def test_one_allowed_among_many():
    """One allowed head and one allowed tail among 5,000 local nodes: 4,096 uniform draws miss it
    with probability (1 - 1/5000)^4096 = 0.44 per row, so without the bounded fallback scan a
    filtered node is emitted in some of the 64 rows with near certainty."""
    from mmre.sampler import RepoSampler
    N, R, B = 5000, 3, 64
    h, r, t, a, c = 10, 1, 20, 1234, 4321
    xs = np.array([x for x in range(N) if x != a])
    ys = np.array([y for y in range(N) if y != c])
    wh = np.concatenate([xs, np.full(len(ys), h)])
    wt = np.concatenate([np.full(len(xs), t), ys])
    wr = np.full(len(wh), r)
    s = RepoSampler([wh, wr, wt], R, DEV, seed=5)
    eh, et, er = np.full(B, h), np.full(B, t), np.full(B, r)
    ei, ety = _sample(s, eh, et, er, 1, N, None)
    _check(ei, ety, eh, et, er, 1, N, None, True, (wh, wr, wt))
    nh, nt = ei[0, B:], ei[1, B:]
    head_rows = nh != h
    assert np.all(nh[head_rows] == a) and np.all(nt[head_rows] == t)
    assert np.all(nt[~head_rows] == c) and np.all(nh[~head_rows] == h)
    assert 0 < head_rows.sum() < B  # both sides drawn


@pytest.mark.parametrize("filt", [True, False])
def test_fewer_allowed_than_asked(filt):
    """n_local = 6, neg = 10. Filtered: three allowed nodes per side, so a side asked for c negatives
    holds min(c, 3) distinct nodes and no filtered one. Unfiltered: all six are allowed on both
    sides (the positive's own h and t included), min(c, 6) distinct."""
    from mmre.sampler import RepoSampler
    N, R, B, neg = 6, 2, 64, 10
    h, r, t = 0, 0, 1
    wh = np.array([0, 2, 3, 0, 0, 0]); wt = np.array([1, 1, 1, 1, 2, 3]); wr = np.zeros(6, np.int64)
    allowed_h, allowed_t = ({1, 4, 5}, {0, 4, 5}) if filt else (set(range(6)), set(range(6)))
    s = RepoSampler([wh, wr, wt], R, DEV, filter_flag=filt, seed=9)
    eh, et, er = np.full(B, h), np.full(B, t), np.full(B, r)
    ei, ety = _sample(s, eh, et, er, neg, N, None)
    if filt:
        sides = _check(ei, ety, eh, et, er, neg, N, None, True, (wh, wr, wt))
        for heads, tails in sides:
            assert set(heads) <= allowed_h and set(tails) <= allowed_t
            assert len(set(heads)) == min(len(heads), 3) and len(set(tails)) == min(len(tails), 3)
        assert any(len(x) > 3 for pair in sides for x in pair)
    else:
        # unfiltered, a row may equal the positive, so the split is read from the rows that differ
        # and the boundary rows are tried on both sides (_check): some split must use all six
        # nodes of a side once before repeating -- also the positive's own t among the tails
        sides = _check(ei, ety, eh, et, er, neg, N, None, False, (wh, wr, wt))
        assert any(len(set(tails)) == 6 and t in tails for _, tails in sides)
        assert any(len(set(heads)) == 6 and h in heads for heads, _ in sides)


def test_determinism():
    from mmre.sampler import RepoSampler
    rng = np.random.default_rng(8)
    whole, l2g, eh, et, er, _ = _graph(rng, 200, 23, "perm")

    def draw(seed, n):
        s = RepoSampler(list(whole), 23, DEV, seed=seed)
        return [np.concatenate([x.ravel() for x in _sample(s, eh, et, er, 10, 60, l2g)]) for _ in range(n)]

    a, b, c = draw(1, 2), draw(1, 2), draw(2, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # same seed and call index
    assert not np.array_equal(a[0], a[1])                               # the next call differs
    assert not np.array_equal(a[0], c[0])                               # another seed differs


def test_distribution():
    """The reference's rule: each negative's side is a fair coin, its node uniform over the allowed
    local nodes. One seed, so the figures are deterministic. 4,096 copies of one positive x 8 =
    32,768 draws: head-side count within 6 sigma = 543 of 16,384 (binomial, sigma 90.5); per side
    Pearson chi^2 over the 40 allowed nodes below 117.02, the 1 - 1e-9 quantile at 39 degrees of
    freedom (distinctness within a positive only lowers the statistic)."""
    from mmre.sampler import RepoSampler
    N, R, B, neg = 50, 2, 4096, 8
    h, r, t = 0, 0, 1
    bad_h = [0] + list(range(2, 11))      # 10 known heads of (t, r), h among them
    bad_t = [1] + list(range(11, 20))     # 10 known tails of (h, r), t among them
    wh = np.array(bad_h + [h] * 10); wt = np.array([t] * 10 + bad_t); wr = np.zeros(20, np.int64)
    s = RepoSampler([wh, wr, wt], R, DEV, seed=11)
    eh, et, er = np.full(B, h), np.full(B, t), np.full(B, r)
    ei, ety = _sample(s, eh, et, er, neg, N, None)
    nh, nt = ei[0, B:], ei[1, B:]
    head = nh != h
    assert np.all((nh != h) ^ (nt != t))
    n_head = int(head.sum())
    print(f"repo sampler split: {n_head} head-side of {B * neg}")
    assert abs(n_head - 16384) <= 543
    for name, vals, bad in (("head", nh[head], bad_h), ("tail", nt[~head], bad_t)):
        cnt = np.bincount(vals, minlength=N)
        allowed = np.setdiff1d(np.arange(N), bad)
        assert len(allowed) == 40 and cnt[bad].sum() == 0
        exp = len(vals) / 40.0
        chi2 = float(((cnt[allowed] - exp) ** 2 / exp).sum())
        print(f"repo sampler {name} side: chi^2 = {chi2:.2f} over 40 nodes, min count {cnt[allowed].min()}")
        assert chi2 < 117.02
        assert np.all(cnt[allowed] > 0)
