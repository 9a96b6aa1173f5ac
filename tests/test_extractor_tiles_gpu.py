"""The ZSL encode kernel's persistent tile loop (csrc/extractor.hip, k_extractor_encode) and
k_extractor_targets, against float64.

A ZSL evaluation scores millions of rows, so every workgroup of the encode kernel walks many
64-row tiles and carries the state of its two-buffer weight ring (and the prefetched chunk in
registers) from one tile into the next. Small inputs never do that: the grid is
min(tiles, resident workgroups) and the resident count is at least 256. These tests make
workgroups take several tiles -- with the `max_blocks` cap of mmre.extractor.encode at every
built width, and with an uncapped launch of more than twice the resident count of tiles -- and
hold the results to float64 at the bars of test_extractor_gpu.py (1e-4 on g, 1e-5 on cosine
scores) and bit for bit to the one-tile-per-workgroup launch: a row's arithmetic depends on
neither the tile, wave or lane group it lands in nor the trip it is computed in.

The float64 reference is written here in plain torch:
  x = left[li] + right[ri];  g = LayerNorm(W2 relu(W1 x + b1) + b2 + x)  (biased variance, eps
  inside the sqrt);  score = g . t / |g|  (g . t when not normalising).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_NODES, N_TARGETS = 37, 3
DIMS = (64, 100, 128, 200, 256)


@functools.lru_cache(maxsize=None)
def _setup(d):
    """One randomly initialised SupportEncoder(d, 2d) per width, packed the way
    mmre.extractor.support_encode packs it, with node tables and targets; shared, never changed."""
    from mmre._lib import call, lib, ptr, stream_ptr
    from module.submodule import SupportEncoder
    torch.manual_seed(1000 + d)
    se = SupportEncoder(d, 2 * d)
    with torch.no_grad():  # the perturbation of test_support_encoder_matches_torch
        se.proj1.bias.normal_(0, 0.1)
        se.proj2.bias.normal_(0, 0.1)
        se.layer_norm.weight.normal_(1, 0.1)
        se.layer_norm.bias.normal_(0, 0.1)
    left, right = torch.randn(N_NODES, d), torch.randn(N_NODES, d)
    targets = torch.randn(N_TARGETS, d)
    h = d // 2
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
    c = lambda t: t.detach().contiguous().float().to(DEV)
    ws = [z(h, d), z(h), z(h, d), z(h), z(h, d), z(h), z(d, 2 * d), z(d), c(se.proj1.weight), c(se.proj1.bias),
          c(se.proj2.weight), c(se.proj2.bias), c(se.layer_norm.weight), c(se.layer_norm.bias)]
    pack = torch.empty(int(lib().mmre_extractor_pack_size(d)), dtype=torch.float32, device=DEV)
    call("mmre_extractor_pack", d, *[ptr(w) for w in ws], ptr(pack), stream_ptr(DEV))
    torch.cuda.synchronize()
    dbl = lambda t: t.detach().double()
    return dict(d=d, eps=float(se.layer_norm.eps), pack=pack, left=left.to(DEV), right=right.to(DEV),
                targets=targets.to(DEV), left64=dbl(left), right64=dbl(right), targets64=dbl(targets),
                w1=dbl(se.proj1.weight), b1=dbl(se.proj1.bias), w2=dbl(se.proj2.weight), b2=dbl(se.proj2.bias),
                lw=dbl(se.layer_norm.weight), lb=dbl(se.layer_norm.bias))


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, N_NODES, (n,), generator=g), torch.randint(0, N_NODES, (n,), generator=g),
            torch.randint(0, N_TARGETS, (n,), generator=g))


def _ref(S, li, ri, row_target, normalize):
    """float64 (g, score) of the rows (li, ri, row_target), host tensors."""
    x = S["left64"][li] + S["right64"][ri]
    y = torch.relu(x @ S["w1"].t() + S["b1"]) @ S["w2"].t() + S["b2"] + x
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    g = (y - mu) / torch.sqrt(var + S["eps"]) * S["lw"] + S["lb"]
    t = S["targets64"][row_target] if row_target is not None else S["targets64"][0].expand_as(g)
    dot = (g * t).sum(1)
    return g, (dot / g.norm(dim=1) if normalize else dot)


def _encode(S, li, ri, row_target, normalize, max_blocks, want_g=True):
    from mmre.extractor import encode
    g, s = encode(S["pack"], S["d"], S["eps"], S["left"], li.to(DEV), S["right"], ri.to(DEV), targets=S["targets"],
                  row_target=None if row_target is None else row_target.to(DEV), normalize=normalize,
                  want_g=want_g, want_score=True, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return (None if g is None else g.cpu()), s.cpu()


def _check_scores(got, ref, normalize):
    err = (got.double() - ref).abs().max().item()
    bar = 1e-5 if normalize else 1e-4 * max(1.0, ref.abs().max().item())
    assert err <= bar, (err, bar)


def _trips(tiles, grid):
    """tiles each workgroup of a `grid`-wide launch takes (tile = blockIdx.x + j * gridDim.x)."""
    return [len(range(b, tiles, grid)) for b in range(grid)]


CAPS = (1, 2, 3, 8, None)


@pytest.mark.parametrize("d", DIMS)
def test_capped_launches_match_float64_and_each_other(d):
    """461 rows = 7 full tiles + 13 rows, under caps 1, 2, 3, 8 and none: one workgroup taking
    all eight tiles, uneven trip counts (3, 3, 2), and one tile per workgroup. g and both kinds
    of score within the float64 bars for every cap, and bit-identical across the caps. Would
    catch a wrong ring parity, a stale prefetched chunk or a stale accumulator on a later trip
    (wrong values from the second tile on), and a ragged last tile handled differently when it
    is a workgroup's second or third tile."""
    from mmre.extractor import encode_blocks
    S = _setup(d)
    n, tiles = 461, 8
    assert (n + 63) // 64 == tiles and n % 64 == 13
    assert encode_blocks(d, n) == tiles          # the default launch: one tile per workgroup
    assert _trips(tiles, 1) == [8] and _trips(tiles, 2) == [4, 4] and _trips(tiles, 3) == [3, 3, 2]
    assert _trips(tiles, min(tiles, 8)) == [1] * 8
    li, ri, rt = _rows(n, 7 * d)
    for normalize, row_target in ((True, rt), (False, rt), (True, None)):
        ref_g, ref_s = _ref(S, li, ri, row_target, normalize)
        first = None
        for cap in CAPS:
            g, s = _encode(S, li, ri, row_target, normalize, cap)
            assert g.shape == (n, d) and s.shape == (n,)
            err_g = (g.double() - ref_g).abs().max().item()
            assert err_g <= 1e-4, (cap, normalize, err_g)
            _check_scores(s, ref_s, normalize)
            if first is None:
                first = (g, s)
            else:
                assert torch.equal(g, first[0]), (cap, normalize)
                assert torch.equal(s, first[1]), (cap, normalize)


@pytest.mark.parametrize("d", DIMS)
def test_one_full_tile(d):
    """64 rows exactly: one full tile, no ragged rows, capped to one workgroup and uncapped."""
    from mmre.extractor import encode_blocks
    S = _setup(d)
    assert encode_blocks(d, 64) == 1
    li, ri, rt = _rows(64, 11 * d)
    ref_g, ref_s = _ref(S, li, ri, rt, True)
    g1, s1 = _encode(S, li, ri, rt, True, 1)
    g0, s0 = _encode(S, li, ri, rt, True, None)
    assert (g1.double() - ref_g).abs().max().item() <= 1e-4
    _check_scores(s1, ref_s, True)
    assert torch.equal(g1, g0) and torch.equal(s1, s0)


@pytest.mark.parametrize("d", [200, 100])
def test_uncapped_launch_past_the_resident_count(d):
    """The benchmark's shape in small: 64 (2R + 3) + 5 rows for R resident workgroups, scores
    only, no cap -- the launch is R workgroups wide and every one of them takes two or three
    tiles. Float64 on the first tile, the first second-trip tile, the last full tile, the ragged
    rows and 2,000 random rows; every row bit-identical to the same rows run in launches of at
    most R tiles (one tile per workgroup). Would catch what the capped test catches, in the
    launch bench.py's zsl config times. Both widths are kept: at R = 512 this is 65,733 rows."""
    from mmre.extractor import encode_blocks
    S = _setup(d)
    R = encode_blocks(d, 1 << 40)
    tiles = 2 * R + 3
    n = 64 * tiles + 5
    tiles += 1                                                # the ragged one
    print(f"d = {d}: resident workgroups R = {R}, {n} rows, {tiles} tiles")
    assert R >= 1 and n <= 300_000, (R, n)
    assert encode_blocks(d, n) == R and R < tiles
    assert min(_trips(tiles, R)) >= 2 and max(_trips(tiles, R)) >= 3
    li, ri, rt = _rows(n, 13 * d)
    _, s = _encode(S, li, ri, rt, True, None, want_g=False)
    g = torch.Generator().manual_seed(d)
    ar = torch.arange
    sub = torch.cat([ar(0, 64), ar(64 * R, 64 * R + 64), ar(64 * (2 * R + 2), 64 * (2 * R + 3)), ar(n - 5, n),
                     torch.randint(0, n, (2000,), generator=g)])
    _, ref_s = _ref(S, li[sub], ri[sub], rt[sub], True)
    _check_scores(s[sub], ref_s, True)
    chunk = 64 * R
    parts = []
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        assert encode_blocks(d, b - a) == (b - a + 63) // 64  # one tile per workgroup
        parts.append(_encode(S, li[a:b], ri[a:b], rt[a:b], True, R, want_g=False)[1])
    assert torch.equal(s, torch.cat(parts))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("dim", [64, 100, 200])
@pytest.mark.parametrize("n_samples", [1, 20, 64])
def test_targets_match_float64(n_samples, dim, normalize):
    """k_extractor_targets: the mean over S samples of the (L2-normalised) rows, one all-zero
    sample among them (weight 0, as in sklearn's cosine), S from one to the limit of 64. Would
    catch a sample dropped past the first pass of the four waves, a wrong divisor and a NaN
    from the zero row."""
    from mmre.extractor import targets
    g = torch.Generator().manual_seed(n_samples * 1000 + dim)
    v = torch.randn(2, n_samples, dim, generator=g)
    v[1, n_samples // 2] = 0.0
    v64 = v.double()
    if normalize:
        nrm = v64.norm(dim=2, keepdim=True)
        v64 = v64 * torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
    ref = v64.mean(1)
    got = targets(v.to(DEV), normalize=normalize)
    torch.cuda.synchronize()
    assert got.shape == (2, dim)
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 1e-6 * max(1.0, ref.abs().max().item()), err


def test_targets_sample_limit():
    from mmre._lib import MMREError
    from mmre.extractor import targets
    with pytest.raises(MMREError, match="unsupported shape"):
        targets(torch.randn(1, 65, 64).to(DEV))
