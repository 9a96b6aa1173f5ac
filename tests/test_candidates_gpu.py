"""Edges of the candidate rankings (csrc/candidates.hip) through the C ABI.

k_candidate_rank_transe against the oracle's sequential C restatement: scores are the
canonical f32 chain, so bit-equal; ranks are #(s<p) + #(s==p)//2 + 1 recomputed in numpy from
the oracle's scores (IEEE compares, as torch's in main.py:247-249). k_cosine_rank against the
oracle's float64 numpy: three length-d sequential f32 sums (two norms, one dot product) on
unit-bounded quantities plus the S-term mean bound |score - f64| by (2d + S + 8) * 2^-24; ranks
are exact on lists built with no negative within 4x that bound of the true candidate.

Every call pre-fills `rank` with -7 and `scores` with a NaN of a known payload, so what the
kernel wrote is visible, and gives the id / candidate / score buffers one guard element past
off[-1]. An empty list ranks 0, reads no candidate and writes no score."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = np.uint32(0x7FC0DEAD)  # quiet NaN with a payload no arithmetic produces
RANK_FILL = -7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sentinel(n):
    return torch.from_numpy(np.full(n, SENT, np.uint32).view(np.float32).copy()).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_transe(ent, rel, qh, qr, off, ids, with_scores=True):
    """ids carries the guard already (len == off[-1] + 1). -> rank (Q,), score bits (len(ids),)"""
    from mmre._lib import call, ptr, stream_ptr
    t_ent, t_rel, t_qh, t_qr, t_off, t_ids = (_dev(x) for x in (ent, rel, qh, qr, off, ids))
    rank = torch.full((len(qh),), RANK_FILL, dtype=torch.int32, device=DEV)
    scores = _sentinel(len(ids)) if with_scores else None
    try:
        call("mmre_candidate_rank_transe", ptr(t_ent), ptr(t_rel), int(ent.shape[1]), ptr(t_qh), ptr(t_qr),
             len(qh), ptr(t_off), ptr(t_ids), ptr(scores), ptr(rank), stream_ptr(DEV))
    finally:
        torch.cuda.synchronize()
    assert np.array_equal(t_ids.cpu().numpy(), ids)
    return rank.cpu().numpy(), (scores.cpu().numpy() if with_scores else None)


def _rule(scores, off):
    """main.py:247-249 on given scores: #(s<p) + #(s==p)//2 + 1, 0 for an empty list."""
    out = np.zeros(len(off) - 1, np.int64)
    for q in range(len(off) - 1):
        a, b = int(off[q]), int(off[q + 1])
        if b > a:
            with np.errstate(invalid="ignore"):
                p, s = scores[a], scores[a + 1:b]
                out[q] = int((s < p).sum()) + int((s == p).sum()) // 2 + 1
    return out


def _owned(off, n):
    m = np.zeros(n, bool)
    m[int(off[0]):int(off[-1])] = True
    return m


def _check_transe(oracle_mod, ent, rel, qh, qr, off, ids, nan_ok=False):
    """Run the kernel, compare with the oracle; returns (rank, oracle scores)."""
    o_s, o_r = oracle_mod.candidate_rank_transe(ent, rel, qh, qr, off, ids)
    want = _rule(o_s, off)
    assert np.array_equal(o_r, want)  # the oracle's own ranks follow the rule
    rank, sc = _run_transe(ent, rel, qh, qr, off, ids)
    own = _owned(off, len(ids))
    got, ref = sc.copy(), o_s.copy()
    if nan_ok:  # a computed NaN's sign / payload is the platform's; everything else is bit-equal
        both = np.isnan(got) & np.isnan(ref) & own
        assert not np.any(_bits(got)[both] == SENT)
        got[both], ref[both] = 0.0, 0.0
    assert np.array_equal(_bits(got)[own], _bits(ref)[own])
    assert np.all(_bits(sc)[~own] == SENT)  # the guard and every slot no list owns: untouched
    assert np.array_equal(rank, want)
    rank2, _ = _run_transe(ent, rel, qh, qr, off, ids, with_scores=False)  # d_scores = NULL
    assert np.array_equal(rank2, want)
    return rank, o_s


def _tables(rng, E, R, d):
    return (rng.uniform(-0.3, 0.3, (E, d)).astype(np.float32), rng.uniform(-0.3, 0.3, (R, d)).astype(np.float32))


def _random_lists(rng, E, lens, lead=0):
    """lens: entries per list (true tail included; 0 = empty). -> off, ids (+ one guard id)."""
    off = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, E, int(off[-1]) + 1).astype(np.int64)
    return off, ids


@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 200, 256, 257, 1024])
def test_transe_width(oracle_mod, d):
    rng = np.random.default_rng(100 + d)
    E, R = 300, 7
    ent, rel = _tables(rng, E, R, d)
    lens = [1, 6, 301, 70, 2]
    off, ids = _random_lists(rng, E, lens)
    qh, qr = rng.integers(0, E, len(lens)), rng.integers(0, R, len(lens))
    _check_transe(oracle_mod, ent, rel, qh, qr, off, ids)


def test_transe_width_above_cap_is_rejected():
    from mmre._lib import MMREError
    rng = np.random.default_rng(7)
    ent, rel = _tables(rng, 20, 3, 1025)
    off, ids = _random_lists(rng, 20, [4, 3])
    from mmre._lib import call, ptr, stream_ptr
    t = [_dev(x) for x in (ent, rel, np.array([1, 2]), np.array([0, 1]), off, ids)]
    rank = torch.full((2,), RANK_FILL, dtype=torch.int32, device=DEV)
    scores = _sentinel(len(ids))
    with pytest.raises(MMREError, match=r"unsupported shape \(code 3\)"):
        call("mmre_candidate_rank_transe", ptr(t[0]), ptr(t[1]), 1025, ptr(t[2]), ptr(t[3]), 2, ptr(t[4]), ptr(t[5]),
             ptr(scores), ptr(rank), stream_ptr(DEV))
    torch.cuda.synchronize()
    assert np.all(rank.cpu().numpy() == RANK_FILL) and np.all(_bits(scores.cpu().numpy()) == SENT)


NEGS = [0, 1, 255, 256, 257, 512, 513, 999]


def test_transe_list_lengths(oracle_mod):
    rng = np.random.default_rng(11)
    E, R, d = 400, 5, 20
    ent, rel = _tables(rng, E, R, d)
    lens = [n + 1 for n in NEGS]
    off, ids = _random_lists(rng, E, lens)
    qh, qr = rng.integers(0, E, len(lens)), rng.integers(0, R, len(lens))
    rank, _ = _check_transe(oracle_mod, ent, rel, qh, qr, off, ids)
    for i in range(len(lens)):  # each list as a single-query call
        a, b = int(off[i]), int(off[i + 1])
        one_ids = np.concatenate([ids[a:b], [0]]).astype(np.int64)
        r1, _ = _check_transe(oracle_mod, ent, rel, qh[i:i + 1], qr[i:i + 1], np.array([0, b - a], np.int64), one_ids)
        assert r1[0] == rank[i]


def test_transe_above_grid_cap(oracle_mod):
    rng = np.random.default_rng(12)
    Q, E, R, d = 8200, 64, 9, 8
    ent, rel = _tables(rng, E, R, d)
    lens = rng.integers(1, 5, Q)
    off, ids = _random_lists(rng, E, lens)
    qh, qr = rng.integers(0, E, Q), rng.integers(0, R, Q)
    qh[8192:] = (qh[:Q - 8192] + 1) % E  # the workgroup's second query has another (h, r) ...
    qr[8192:] = (qr[:Q - 8192] + 1) % R
    rank, _ = _check_transe(oracle_mod, ent, rel, qh, qr, off, ids)
    assert len(set(rank.tolist())) > 1


TIE_POS = [1, 63, 64, 255, 256, 300]


@pytest.mark.parametrize("way", ["same_id", "same_row"])
def test_transe_exact_ties(oracle_mod, way):
    rng = np.random.default_rng(13)
    E, R, d, L = 500, 4, 33, 320
    ent, rel = _tables(rng, E, R, d)
    true_ids = np.arange(6)           # query m's true tail
    twins = 10 + np.arange(6 * 5).reshape(6, 5)  # ids whose rows equal the true tail's
    for m in range(6):
        ent[twins[m]] = ent[true_ids[m]]
    rows, lens = [], []
    for m in range(6):
        lst = rng.integers(100, E, L).astype(np.int64)  # none of them a true tail or a twin
        lst[0] = true_ids[m]
        pos = (TIE_POS[m:] + TIE_POS[:m])[:m]
        for j, p in enumerate(pos):
            lst[p] = true_ids[m] if way == "same_id" else twins[m][j]
        rows.append(lst)
        lens.append(L)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(rows + [np.array([0])]).astype(np.int64)
    qh, qr = rng.integers(100, E, 6), rng.integers(0, R, 6)
    rank, o_s = _check_transe(oracle_mod, ent, rel, qh, qr, off, ids)
    for m in range(6):
        a, b = int(off[m]), int(off[m + 1])
        assert int((o_s[a + 1:b] == o_s[a]).sum()) == m
        assert rank[m] == int((o_s[a + 1:b] < o_s[a]).sum()) + m // 2 + 1
    used = sorted({p for m in range(6) for p in (TIE_POS[m:] + TIE_POS[:m])[:m]})
    assert used == TIE_POS


def test_transe_non_finite(oracle_mod):
    rng = np.random.default_rng(14)
    E, R, d = 200, 4, 16
    ent, rel = _tables(rng, E, R, d)
    NAN, PINF, NINF, MIX = 0, 1, 2, 3
    ent[NAN, 5] = np.nan
    ent[PINF, 2] = np.inf
    ent[NINF, 9] = -np.inf
    ent[MIX, 0], ent[MIX, 1] = np.inf, np.nan
    L = 300
    lists = []
    for true in (NAN, PINF, NINF, 50, MIX):
        lst = rng.integers(10, E, L).astype(np.int64)
        lst[0] = true
        lst[[1, 63, 64, 255, 256, 299]] = [PINF, NAN, NINF, PINF, MIX, NAN]
        lists.append(lst)
    off = (np.arange(6) * L).astype(np.int64)
    ids = np.concatenate(lists + [np.array([0])]).astype(np.int64)
    qh, qr = rng.integers(10, E, 5), rng.integers(0, R, 5)
    rank, o_s = _check_transe(oracle_mod, ent, rel, qh, qr, off, ids, nan_ok=True)
    assert np.isnan(o_s[off[0]]) and rank[0] == 1 and rank[4] == 1  # p is NaN: nothing is less or equal
    for q in (1, 2):  # p = +inf: every finite score is less, every +inf score equal (3 of them), NaN neither
        s = o_s[off[q] + 1:off[q + 1]]
        assert np.isposinf(o_s[off[q]]) and int(np.isposinf(s).sum()) == 3 and int(np.isnan(s).sum()) == 3
        assert rank[q] == int(np.isfinite(s).sum()) + 3 // 2 + 1
    s = o_s[off[3] + 1:off[4]]
    assert np.isfinite(o_s[off[3]]) and rank[3] == int((s[np.isfinite(s)] < o_s[off[3]]).sum()) + 1


def test_transe_empty_lists(oracle_mod):
    rng = np.random.default_rng(15)
    E, R, d = 300, 5, 24
    ent, rel = _tables(rng, E, R, d)
    lens = [0, 5, 0, 7, 0, 0, 300, 1, 0]  # first, middle, two adjacent, last
    off, ids = _random_lists(rng, E, lens, lead=3)  # three leading slots and the guard belong to no list
    qh, qr = rng.integers(0, E, len(lens)), rng.integers(0, R, len(lens))
    rank, _ = _check_transe(oracle_mod, ent, rel, qh, qr, off, ids)
    assert [int(r) for r in rank[[0, 2, 4, 5, 8]]] == [0] * 5 and np.all(rank[[1, 3, 6, 7]] >= 1)
    # nothing but empty lists, and a single empty query
    off0 = np.full(4, 2, np.int64)
    r0, _ = _check_transe(oracle_mod, ent, rel, qh[:3], qr[:3], off0, ids[:3].copy())
    assert r0.tolist() == [0, 0, 0]
    r1, _ = _check_transe(oracle_mod, ent, rel, qh[:1], qr[:1], off0[:2], ids[:3].copy())
    assert r1.tolist() == [0]


def test_transe_wrapper_dtypes_and_views(oracle_mod):
    from mmre.candidates import candidate_rank_transe
    rng = np.random.default_rng(16)
    E, R, d = 120, 5, 40
    ent, rel = _tables(rng, E, R, d)
    lens = [4, 0, 260, 1]
    off, ids = _random_lists(rng, E, lens)
    ids = ids[:-1]
    qh, qr = rng.integers(0, E, len(lens)), rng.integers(0, R, len(lens))
    o_s, _ = oracle_mod.candidate_rank_transe(ent, rel, qh, qr, off, ids)
    want = _rule(o_s, off)
    wide = np.zeros((E, 2 * d), np.float32)
    wide[:, ::2] = ent
    wide[:, 1::2] = 9.0
    variants = {
        "int64": (_dev(ent), _dev(rel), [_dev(x.astype(np.int64)) for x in (qh, qr, off, ids)]),
        "int32": (_dev(ent), _dev(rel), [_dev(x.astype(np.int32)) for x in (qh, qr, off, ids)]),
        "view": (_dev(wide)[:, ::2], _dev(rel), [_dev(x.astype(np.int32)) for x in (qh, qr, off, ids)]),
        "float64": (_dev(ent.astype(np.float64)), _dev(rel.astype(np.float64)),
                    [_dev(x.astype(np.int64)) for x in (qh, qr, off, ids)]),
    }
    assert not variants["view"][0].is_contiguous()
    for name, (e, r, (a, b, c, dd)) in variants.items():
        rank, sc = candidate_rank_transe(e, r, a, b, c, dd, return_scores=True)
        torch.cuda.synchronize()
        assert np.array_equal(rank.cpu().numpy(), want), name  # the empty list's rank is 0, not stale memory
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(o_s)), name
        assert np.array_equal(candidate_rank_transe(e, r, a, b, c, dd).cpu().numpy(), want), name


# ------------------------------------------------------------------------------ cosine rank --
def _tol(d, S):
    return (2 * d + S + 8) * 2.0 ** -24


def _run_cosine(cand, off, relv, roq, with_scores=True):
    """cand carries one guard row past off[-1]. -> rank (Q,), scores (len(cand),)"""
    from mmre._lib import call, ptr, stream_ptr
    t_cand, t_off, t_rel, t_roq = _dev(cand), _dev(off), _dev(relv), _dev(roq)
    rank = torch.full((len(roq),), RANK_FILL, dtype=torch.int32, device=DEV)
    scores = _sentinel(len(cand)) if with_scores else None
    try:
        call("mmre_cosine_rank", ptr(t_cand), int(cand.shape[1]), ptr(t_off), len(roq), ptr(t_rel),
             int(relv.shape[1]), ptr(t_roq), ptr(scores), ptr(rank), stream_ptr(DEV))
    finally:
        torch.cuda.synchronize()
    return rank.cpu().numpy(), (scores.cpu().numpy() if with_scores else None)


def _cosine_case(oracle_mod, d, S, lens, roq, seed, n_sets=5, before_screen=None):
    """Relation samples dirn + 0.5 noise; candidates 0.3 g dirn + noise. Negatives within 4 tol of
    their list's true candidate (float64) are dropped before the lists are cut to `lens` entries;
    under 5 % may be. -> cand (+ guard row), off, relv, roq"""
    rng = np.random.default_rng(seed)
    tol = _tol(d, S)
    dirn = rng.standard_normal((n_sets, d))
    relv = (dirn[:, None, :] + 0.5 * rng.standard_normal((n_sets, S, d))).astype(np.float32)
    roq = np.asarray(roq, np.int64)
    gen = [0 if n == 0 else n + max(8, n // 8) for n in lens]
    pool = np.concatenate([0.3 * rng.standard_normal((n, 1)) * dirn[s] + rng.standard_normal((n, d))
                           for n, s in zip(gen, roq)] + [np.ones((1, d))]).astype(np.float32)
    poff = np.concatenate([[0], np.cumsum(gen)]).astype(np.int64)
    if before_screen is not None:
        before_screen(pool, poff, relv)
    s64, _ = oracle_mod.cosine_rank(pool[:-1], poff, relv, roq)
    rows, dropped, negs = [], 0, 0
    for q, n in enumerate(lens):
        a, b = int(poff[q]), int(poff[q + 1])
        if n == 0:
            continue
        far = np.abs(s64[a + 1:b] - s64[a]) > 4 * tol
        dropped += int((~far).sum())
        negs += b - a - 1
        keep = a + 1 + np.flatnonzero(far)[:n - 1]
        assert len(keep) == n - 1
        rows += [pool[a:a + 1], pool[keep]]
    assert dropped * 20 < max(negs, 1), (dropped, negs)
    cand = np.concatenate(rows + [np.ones((1, d), np.float32)]) if rows else np.ones((1, d), np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.ascontiguousarray(cand, np.float32), off, relv, roq


def _check_cosine(oracle_mod, cand, off, relv, roq, ranks=True, label=""):
    d, S = cand.shape[1], relv.shape[1]
    o_s, o_r = oracle_mod.cosine_rank(cand[:-1], off, relv, roq)
    rank, sc = _run_cosine(cand, off, relv, roq)
    n = int(off[-1])
    err = float(np.abs(sc[:n].astype(np.float64) - o_s[:n]).max()) if n else 0.0
    print(f"cosine_rank {label} d={d} S={S} Q={len(roq)}: max |score - f64| = {err:.3e}, bound {_tol(d, S):.3e}")
    assert np.all(np.isfinite(sc[:n])) and err <= _tol(d, S)
    assert np.all(_bits(sc)[n:] == SENT)  # the guard slot
    empty = off[1:] == off[:-1]
    assert np.all(rank[empty] == 0) and np.all(o_r[empty] == 0)
    if ranks:
        assert np.array_equal(rank, o_r)
        rank2, _ = _run_cosine(cand, off, relv, roq, with_scores=False)
        assert np.array_equal(rank2, o_r)
    return rank, sc, o_s


LENS = [0, 1, 2, 0, 257, 1000, 3, 0]  # empty first, middle and last
ROQ = [3, 1, 4, 1, 0, 2, 3, 0]        # non-monotone, repeating


@pytest.mark.parametrize("d,S", [(2, 1), (7, 20), (48, 20), (65, 64), (200, 20), (300, 64), (1024, 24)])
def test_cosine_shapes(oracle_mod, d, S):
    """(300, 64) asks for 76,800 B of dynamic LDS, (1024, 24) for 98,304 B: the host cap. Both
    launch on gfx950 (160 KiB of LDS per CU) without raising the kernel's dynamic-LDS limit."""
    cand, off, relv, roq = _cosine_case(oracle_mod, d, S, LENS, ROQ, seed=1000 + d)
    rank, _, _ = _check_cosine(oracle_mod, cand, off, relv, roq, label="shapes")
    assert rank[5] > 1 or rank[4] > 1  # the long lists are not all won by the true candidate


def test_cosine_dim_one_scores(oracle_mod):
    cand, off, relv, roq = _cosine_case(oracle_mod, 2, 3, LENS, ROQ, seed=5)
    cand, relv = np.ascontiguousarray(cand[:, :1]), np.ascontiguousarray(relv[:, :, :1])
    _check_cosine(oracle_mod, cand, off, relv, roq, ranks=False, label="dim1")  # every score a mean of +-1: ties


@pytest.mark.parametrize("d,S", [(8, 65), (1024, 25)])
def test_cosine_rejected_shapes(d, S):
    from mmre._lib import MMREError
    rng = np.random.default_rng(3)
    cand = rng.standard_normal((6, d)).astype(np.float32)
    relv = rng.standard_normal((2, S, d)).astype(np.float32)
    from mmre._lib import call, ptr, stream_ptr
    rank = torch.full((2,), RANK_FILL, dtype=torch.int32, device=DEV)
    scores = _sentinel(6)
    t = [_dev(cand), _dev(np.array([0, 2, 5], np.int64)), _dev(relv), _dev(np.array([1, 0], np.int64))]
    with pytest.raises(MMREError, match=r"unsupported shape \(code 3\)"):
        call("mmre_cosine_rank", ptr(t[0]), d, ptr(t[1]), 2, ptr(t[2]), S, ptr(t[3]), ptr(scores), ptr(rank),
             stream_ptr(DEV))
    torch.cuda.synchronize()
    assert np.all(rank.cpu().numpy() == RANK_FILL) and np.all(_bits(scores.cpu().numpy()) == SENT)


def test_cosine_above_grid_cap(oracle_mod):
    rng = np.random.default_rng(21)
    Q = 8200
    lens = rng.integers(1, 4, Q).tolist()
    roq = rng.integers(0, 5, Q)
    roq[8192:] = (roq[:Q - 8192] + 1 + rng.integers(0, 4, Q - 8192)) % 5  # q and q + 8192: different sets
    assert np.all(roq[8192:] != roq[:Q - 8192])
    cand, off, relv, roq = _cosine_case(oracle_mod, 8, 2, lens, roq, seed=22)
    rank, _, _ = _check_cosine(oracle_mod, cand, off, relv, roq, label="grid cap")
    assert set(rank.tolist()) == {1, 2, 3}


def test_cosine_zero_norms(oracle_mod):
    d, S = 48, 20

    def zero(pool, poff, relv):
        pool[poff[1] + 3] = 0.0   # an all-zero negative
        pool[poff[2]] = 0.0       # an all-zero true candidate
        relv[1, 4] = 0.0          # an all-zero relation sample in a used set

    lens, roq = [1, 40, 40, 30, 300], [1, 1, 0, 2, 1]
    cand, off, relv, roq = _cosine_case(oracle_mod, d, S, lens, roq, seed=31, before_screen=zero)
    relv[2] = 0.0                 # a whole set of zero samples (list 3 alone uses it): every score 0
    o_s, o_r = oracle_mod.cosine_rank(cand[:-1], off, relv, np.asarray(roq))
    rank, sc = _run_cosine(cand, off, relv, np.asarray(roq))
    n = int(off[-1])
    assert np.abs(sc[:n] - o_s).max() <= _tol(d, S)
    zero_rows = np.flatnonzero(~cand[:n].any(1))
    assert len(zero_rows) == 2 and np.all(_bits(sc[zero_rows]) == 0)  # exactly +0
    assert np.all(_bits(sc[off[3]:off[4]]) == 0)  # zero samples contribute 0
    keep = [0, 1, 2, 4]  # list 3 is all ties: outside the rank contract
    assert np.array_equal(rank[keep], o_r[keep]) and rank[3] == 1


def test_cosine_copies_of_the_true_row_do_not_count(oracle_mod):
    d, S = 65, 7
    cand, off, relv, roq = _cosine_case(oracle_mod, d, S, [320, 320], [2, 0], seed=41)
    for p in (1, 63, 64, 255, 256, 300):
        cand[off[1] + p] = cand[off[1]]
    rank, sc, o_s = _check_cosine(oracle_mod, cand, off, relv, roq, label="copies")
    a = int(off[1])
    assert np.all(_bits(sc[a + np.array([1, 63, 64, 255, 256, 300])]) == _bits(sc[a:a + 1]))
    assert rank[1] == 1 + int((o_s[a + 1:off[2]] > o_s[a]).sum())


def test_cosine_wrapper_dtypes_and_views(oracle_mod):
    from mmre.candidates import cosine_rank
    cand, off, relv, roq = _cosine_case(oracle_mod, 20, 6, [5, 0, 270, 1], [1, 0, 1, 2], seed=51, n_sets=3)
    cand = cand[:-1]
    _, o_r = oracle_mod.cosine_rank(cand, off, relv, roq)
    wide = np.zeros((len(cand), 40), np.float32)
    wide[:, ::2] = cand
    wide[:, 1::2] = 9.0
    base, sc0 = cosine_rank(_dev(cand), _dev(off), _dev(relv), _dev(roq), return_scores=True)
    assert np.array_equal(base.cpu().numpy(), o_r)
    for name, (c, o, v, r) in {
        "int32": (_dev(cand), _dev(off.astype(np.int32)), _dev(relv), _dev(roq.astype(np.int32))),
        "view": (_dev(wide)[:, ::2], _dev(off.astype(np.int32)), _dev(relv), _dev(roq)),
        "float64": (_dev(cand.astype(np.float64)), _dev(off), _dev(relv.astype(np.float64)), _dev(roq)),
    }.items():
        rank, sc = cosine_rank(c, o, v, r, return_scores=True)
        torch.cuda.synchronize()
        assert np.array_equal(rank.cpu().numpy(), o_r), name
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(sc0.cpu().numpy())), name
