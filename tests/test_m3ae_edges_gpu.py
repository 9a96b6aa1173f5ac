"""The paths of the M3AE text encoder (csrc/m3ae.hip) that tests/test_m3ae_gpu.py never launches:
the 64 x 128 linear tile, K pipelines of 1-5 stages, the plan's scan past one 1,024-row chunk,
every LDS geometry of attention up to 336 rows, LayerNorm on constant and large-mean rows, and
the whole encoder at d 768 / 1024 / 1280 and over a plan of more than 1,024 unique sequences.
References: float64 torch, the oracle oracle/m3ae_text.py, the numpy plan of tests/m3ae_restate.py."""
import numpy as np
import pytest
import torch

import m3ae_restate
from test_m3ae_gpu import _close, _encoder, _rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24  # unit roundoff of float32
NAN = float("nan")


# ---------------------------------------------------------------- linear, both tiles

def _linear_case(m, k, n, epi):
    """Inputs as in test_linear_matches_float64, the float64 result and the per-element bound
    (K + 8) u (|a| |w|^T + |bias|): a length-K fp32 chain in any order stays below K u sum|a w|
    to first order, 8 u covers the bias add, the epilogue's own roundings and the higher-order terms.
    Residual: + u |resid| (its add). GELU: slope at most 1.13, + 8 u max(1, |ref|) for erff and
    the two multiplies."""
    g = torch.Generator().manual_seed(m + k + n)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = 0.1 * torch.randn(n, generator=g)
    r = torch.randn(m, n, generator=g)
    ad, wd, bd = a.double(), w.double(), b.double()
    ref = ad @ wd.T + bd
    bound = (k + 8) * U * (ad.abs() @ wd.abs().T + bd.abs())
    if epi == 1:
        ref = torch.nn.functional.gelu(ref)
        bound = 1.13 * bound + 8 * U * ref.abs().clamp(min=1.0)
    if epi == 2:
        ref = r.double() + ref
        bound = bound + U * r.double().abs()
    return a, w, b, r, ref, bound


def _run_linear(monkeypatch, tile, epi, ad, wd, bd, rd, separate):
    """One launch with MMRE_M3AE_TILE = tile (None: unset) into a NaN-filled output (the aliased
    residual form starts from the residual instead); checks the launcher's own tile choice."""
    from mmre._lib import call, lib, ptr, stream_ptr
    if tile is None:
        monkeypatch.delenv("MMRE_M3AE_TILE", raising=False)
    else:
        monkeypatch.setenv("MMRE_M3AE_TILE", str(tile))
    (m, k), n = ad.shape, wd.shape[0]
    chosen = lib().mmre_m3ae_linear_tile(m, n)
    if tile is not None:
        assert chosen == (128 if tile == 128 and n % 128 == 0 else 64)
    aliased = epi == 2 and not separate
    out = rd.clone() if aliased else torch.full((m, n), NAN, device=DEV)
    resid = None if epi != 2 else out if aliased else rd
    call("mmre_m3ae_linear", epi, ptr(ad), m, k, ptr(wd), n, ptr(bd), ptr(resid), ptr(out), stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu(), chosen


def _ratio(out, ref, bound):
    assert not torch.isnan(out).any(), "output elements left unwritten"
    return ((out.double() - ref).abs() / bound).max().item()


LINEAR_CASES = (
    [(65, k, 128, 0, False) for k in (32, 64, 96, 128, 160)]            # nkt = 1 .. 5
    + [(m, 96, 256, 0, False) for m in (1, 63, 64, 65, 129)]           # M edges of the 64-row tile
    + [(70, 64, 192, 0, False)]                                        # n % 128 != 0: narrow even when 128 is forced
    + [(200, 384, 1536, e, False) for e in (0, 1, 2)]
    + [(77, 1536, 384, e, False) for e in (0, 1, 2)]
    + [(77, 1536, 384, 2, True)]                                       # residual in a buffer of its own
)


@pytest.mark.parametrize("m,k,n,epi,separate", LINEAR_CASES,
                         ids=[f"{m}x{k}x{n}-epi{e}{'-sep' if s else ''}" for m, k, n, e, s in LINEAR_CASES])
def test_linear_both_tiles(monkeypatch, record_property, m, k, n, epi, separate):
    """k_m3ae_linear<epi, 64> and <epi, 128> on the same inputs: bit-equal to each other (an
    output element's chain is the same in both: K ascending, one mfma_f32_32x32x2 per k pair, bias,
    epilogue) and each inside the per-element bound of float64 (_linear_case)."""
    a, w, b, r, ref, bound = _linear_case(m, k, n, epi)
    ad, wd, bd, rd = a.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    narrow, _ = _run_linear(monkeypatch, 64, epi, ad, wd, bd, rd, separate)
    wide, _ = _run_linear(monkeypatch, 128, epi, ad, wd, bd, rd, separate)
    if separate:
        assert torch.equal(rd.cpu(), r)  # the residual buffer is only read
    r64, r128 = _ratio(narrow, ref, bound), _ratio(wide, ref, bound)
    record_property("err_over_bound_64", r64)
    record_property("err_over_bound_128", r128)
    same = torch.equal(narrow, wide)
    print(f"\nlinear {m}x{k}x{n} epi {epi}{' sep' if separate else ''}: err/bound tile 64 {r64:.4f}, "
          f"tile 128 {r128:.4f}, bit-equal {same}")
    assert r64 <= 1.0 and r128 <= 1.0, (r64, r128)
    assert same


def test_linear_reaches_the_wide_tile_unforced(monkeypatch, record_property):
    """10,881 x 32 x 1536 with GELU and the environment unset: ceil(10881 / 64) * 12 = 2,052 tiles
    of 64 x 128 (no multiple of 8: the XCD tile order's ragged end), one K stage, a ragged last
    M tile. One row fewer stays narrow."""
    from mmre._lib import lib
    m, k, n, epi = 10881, 32, 1536, 1
    a, w, b, r, ref, bound = _linear_case(m, k, n, epi)
    ad, wd, bd, rd = a.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    wide, chosen = _run_linear(monkeypatch, None, epi, ad, wd, bd, rd, False)
    assert chosen == 128 and lib().mmre_m3ae_linear_tile(m - 1, n) == 64
    narrow, _ = _run_linear(monkeypatch, 64, epi, ad, wd, bd, rd, False)
    r64, r128, same = _ratio(narrow, ref, bound), _ratio(wide, ref, bound), torch.equal(narrow, wide)
    record_property("err_over_bound_64", r64)
    record_property("err_over_bound_128", r128)
    print(f"\nlinear {m}x{k}x{n} epi {epi} unforced: err/bound tile 64 {r64:.4f}, tile 128 {r128:.4f}, "
          f"bit-equal {same}")
    assert r64 <= 1.0 and r128 <= 1.0, (r64, r128)
    assert same


# ---------------------------------------------------------------- plan

VOCAB = 50


def _gpu_plan(tok, msk, dedupe, vocab=VOCAB):
    """mmre_m3ae_plan on numpy rows (null pointers when L = 0); the plan buffer as numpy."""
    from mmre._lib import call, lib, ptr, stream_ptr
    B, L = tok.shape
    td = torch.from_numpy(np.ascontiguousarray(tok, dtype=np.int32)).to(DEV) if L else None
    md = torch.from_numpy(np.ascontiguousarray(msk, dtype=np.float32)).to(DEV) if L else None
    plan = torch.full((int(lib().mmre_m3ae_plan_size(B)),), -7, dtype=torch.int32, device=DEV)
    call("mmre_m3ae_plan", ptr(td), ptr(md), B, L, dedupe, vocab, ptr(plan), stream_ptr(DEV))
    torch.cuda.synchronize()
    return plan.cpu().numpy()


def _run_rows(n_seq, L, seed):
    """n_seq rows in runs of 1-5 equal rows (short runs likelier: mean 2.1, so 2,600 rows hold more
    than 1,024 runs); lengths 0 .. L, ids up to vocab + 2 (some out of range), and ids on padded
    positions redrawn per row, which must not split a run."""
    rng = np.random.default_rng(seed)
    n_run = n_seq
    runs = rng.choice([1, 2, 3, 4, 5], size=n_run, p=[0.4, 0.3, 0.15, 0.1, 0.05])
    idx = np.repeat(np.arange(n_run), runs)[:n_seq]
    base_tok = rng.integers(0, VOCAB + 3, (n_run, L)).astype(np.int32)
    base_len = rng.integers(0, L + 1, n_run)
    tok = base_tok[idx]
    msk = (np.arange(L)[None, :] >= base_len[idx][:, None]).astype(np.float32)
    tok = np.where(msk > 0, rng.integers(-5, VOCAB + 50, tok.shape).astype(np.int32), tok)
    return tok, msk


def _full(v, L=8):
    return np.full(L, v, dtype=np.int32), np.zeros(L, dtype=np.float32)


@pytest.mark.parametrize("dedupe", [1, 0])
@pytest.mark.parametrize("n_seq", [1, 1023, 1024, 1025, 2049, 2600])
def test_plan_row_counts(n_seq, dedupe):
    """k_m3ae_plan_scan's two loops over 1,024-row chunks: carry (unique index), run (packed
    offset), the maximum and the bad-id total all cross chunk edges."""
    tok, msk = _run_rows(n_seq, 8, seed=n_seq)
    ref = m3ae_restate.plan(tok, msk, dedupe, VOCAB)
    if n_seq == 2600:
        assert ref["info"][0] > 1024  # the offset scan reaches its second chunk in both modes
        assert ref["info"][3] > 0
    m3ae_restate.assert_plan_equal(_gpu_plan(tok, msk, dedupe), n_seq, ref)


@pytest.mark.parametrize("layout", ["run_across_1024", "new_at_1024"])
def test_plan_chunk_edge_layouts(layout):
    """A run of equal rows that starts at row 1023 and continues into the second chunk, and a
    new sequence that starts exactly at row 1024."""
    n_seq = 2049
    tok, msk = _run_rows(n_seq, 8, seed=7)
    if layout == "run_across_1024":
        tok[1022], msk[1022] = _full(3)
        for i in (1023, 1024, 1025):
            tok[i], msk[i] = _full(4)
        tok[1026], msk[1026] = _full(5)
    else:
        for i in (1022, 1023):
            tok[i], msk[i] = _full(3)
        tok[1024], msk[1024] = _full(4)
    ref = m3ae_restate.plan(tok, msk, 1, VOCAB)
    if layout == "run_across_1024":
        assert list(ref["head"][1022:1027]) == [1, 1, 0, 0, 1]
    else:
        assert list(ref["head"][1022:1025]) == [1, 0, 1]
    m3ae_restate.assert_plan_equal(_gpu_plan(tok, msk, 1), n_seq, ref)


def _content_rows(L):
    """Adjacent rows that differ only at position p = L - 1 (the last one the lanes visit), with
    the head flags they must get when dedupe is on."""
    rng = np.random.default_rng(L)
    base = rng.integers(0, VOCAB, L).astype(np.int32)
    last, other = base.copy(), base.copy()
    last[L - 1] = (base[L - 1] + 1) % VOCAB
    other[L - 1] = (base[L - 1] + 8) % VOCAB
    rows = [(base, 0.0, 1),
            (last, 0.0, 1),            # another token at p, nothing else
            (last, 0.0, 0),
            (last, 1.0, 1),            # tokens equal, p padded: the padding pattern differs
            (other, 1.0, 0),           # differs on the padded position only: an equal row
            (other, 2.5, 0),           # any positive mask value is the same padding
            (last, 0.0, 1),
            (last, -1.0, 0),           # mask > 0 is false for -1, -0.0 and NaN: p stays unpadded
            (last, -0.0, 0),
            (last, NAN, 0),
            (last, 1e-40, 1),          # a positive denormal is padding
            (other, float("inf"), 0),  # so is +inf (and the token there is ignored)
            (other, 0.0, 1),
            (last, -1.0, 1)]           # unpadded again on both rows: the token at p counts
    tok = np.stack([t for t, _, _ in rows])
    msk = np.zeros((len(rows), L), dtype=np.float32)
    msk[:, L - 1] = [v for _, v, _ in rows]
    return tok, msk, [h for _, _, h in rows]


@pytest.mark.parametrize("L", [1, 63, 65, 335])
def test_plan_row_contents(L):
    """What makes two adjacent rows equal, at row lengths below, at and past one 64-lane sweep:
    a difference at position L - 1 alone, in the padding pattern alone (tokens equal), on padded
    positions alone (equal rows), and the mask rule `mask > 0` on -1, -0.0, NaN, 1e-40, +inf."""
    tok, msk, heads = _content_rows(L)
    ref = m3ae_restate.plan(tok, msk, 1, VOCAB)
    assert list(ref["head"]) == heads
    assert list(ref["cnt"]) == [1 + L - (v > 0) for v in msk[:, L - 1]]
    m3ae_restate.assert_plan_equal(_gpu_plan(tok, msk, 1), len(heads), ref)
    m3ae_restate.assert_plan_equal(_gpu_plan(tok, msk, 0), len(heads), m3ae_restate.plan(tok, msk, 0, VOCAB))


@pytest.mark.parametrize("n_seq", [3, 1030])
def test_plan_empty_rows(n_seq):
    """L = 0 with null token and mask pointers: one packed row (the CLS row) per sequence, and
    with dedupe a single unique sequence."""
    tok, msk = np.zeros((n_seq, 0), np.int32), np.zeros((n_seq, 0), np.float32)
    p = m3ae_restate.split(_gpu_plan(tok, msk, 1), n_seq)
    assert list(p["info"]) == [1, 1, 1, 0] and not p["uniq"].any()
    assert list(p["src"]) == [0] and list(p["off"]) == [0, 1]
    p = m3ae_restate.split(_gpu_plan(tok, msk, 0), n_seq)
    assert list(p["info"]) == [n_seq, n_seq, 1, 0]
    assert np.array_equal(p["uniq"], np.arange(n_seq)) and np.array_equal(p["src"], np.arange(n_seq))
    assert np.array_equal(p["off"], np.arange(n_seq + 1))
    m3ae_restate.assert_plan_equal(_gpu_plan(tok, msk, 1), n_seq, m3ae_restate.plan(tok, msk, 1, VOCAB))


# ---------------------------------------------------------------- attention

def _attn_lens(max_rows):
    """A handful of sequences: the longest first, one row, and lengths around the 16-row query
    blocks and around the end of the longest."""
    cand = [max_rows, 1, max_rows - 1, 15, 16, 17, 31, 33, max_rows - 16, max_rows - 15]
    return list(dict.fromkeys(n for n in cand if 1 <= n <= max_rows))


def _attn_check(heads, hd, lens, max_rows, q_scale=1.0):
    """mmre_m3ae_attention, full and cls_only, against the float64 softmax((q k^T) hd^-0.5) v of
    test_attention_matches_float64, at its 1e-5 bound; outputs start as NaN."""
    from mmre._lib import call, ptr, stream_ptr
    assert max(lens) <= max_rows  # the logit rows in LDS are sized by max_rows
    D = heads * hd
    off = np.r_[0, np.cumsum(lens)].astype(np.int32)
    g = torch.Generator().manual_seed(hd + max_rows)
    qkv = torch.randn(int(off[-1]), 3 * D, generator=g)
    qkv[:, :D] *= q_scale
    scale = hd ** -0.5
    ref = torch.empty(int(off[-1]), D, dtype=torch.float64)
    for s, n in enumerate(lens):
        blk = qkv[off[s]:off[s + 1]].double().view(n, 3, heads, hd).permute(1, 2, 0, 3)
        q, k, v = blk[0], blk[1], blk[2]
        p = torch.softmax((q @ k.transpose(-2, -1)) * scale, -1)
        ref[off[s]:off[s + 1]] = (p @ v).permute(1, 0, 2).reshape(n, D)
    qd, od = qkv.to(DEV), torch.from_numpy(off).to(DEV)
    out = torch.full((int(off[-1]), D), NAN, device=DEV)
    cls = torch.full((len(lens), D), NAN, device=DEV)
    for cls_only, dst in ((0, out), (1, cls)):
        call("mmre_m3ae_attention", ptr(qd), ptr(od), len(lens), max_rows, heads, hd, float(np.float32(scale)),
             cls_only, ptr(dst), stream_ptr(DEV))
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(cls).any()
    _close(out, ref, 1e-5)
    _close(cls, ref[torch.from_numpy(off[:-1]).long()], 1e-5)


@pytest.mark.parametrize("max_rows", [1, 2, 15, 16, 17, 32, 33, 48, 49, 63, 64, 336])
@pytest.mark.parametrize("heads,hd", [(6, 64), (16, 80)])
def test_attention_lds_geometries(heads, hd, max_rows):
    """Every key-chunk size launch_attn picks (16, 32, 48, 64 keys), row pitches from 5 to 337
    floats, one to 21 query blocks, up to the last legal size of 336 rows."""
    _attn_check(heads, hd, _attn_lens(max_rows), max_rows)


@pytest.mark.parametrize("max_rows", [48, 336])
@pytest.mark.parametrize("heads,hd", [(6, 64), (16, 80)])
def test_attention_max_rows_above_every_sequence(heads, hd, max_rows):
    """max_rows only has to be at least the longest sequence: a larger one changes the LDS
    layout and launches query blocks that find no rows."""
    _attn_check(heads, hd, [20, 1, 17, 5], max_rows)


@pytest.mark.parametrize("heads,hd", [(6, 64), (16, 80)])
def test_attention_wide_logits(heads, hd):
    """336 rows with q scaled by 4: logits spanning about +-22 instead of randn's +-5, so the
    row maximum and the exp of far-below-maximum logits matter. (torch float32 on the CPU is
    6.0e-6 / 6.6e-6 from float64 on a 336-row sequence at this scale for the two head shapes, and
    1.3e-5 / 1.6e-5 at scale 8, where float32 itself is too close to the 1e-5 rule to use.)"""
    _attn_check(heads, hd, [336, 1, 170], 336, q_scale=4.0)


# ---------------------------------------------------------------- LayerNorm

def _layernorm(x, w, b):
    from mmre._lib import call, ptr, stream_ptr
    n, d = x.shape
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.full((n, d), NAN, device=DEV)
    call("mmre_m3ae_layernorm", ptr(xd), n, d, ptr(wd), ptr(bd), 1e-5, ptr(y), stream_ptr(DEV))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("d", [384, 768, 1024, 1280])
def test_layernorm_constant_rows_give_the_bias(d, n):
    """A constant row has x - mean = 0 exactly, so y = bias bit for bit. The constants have at
    most 2 significant bits, so every partial sum of up to 1,280 of them is exact in fp32
    in any order and the mean is the constant itself. n = 1, 4, 5: a partial, a full and a
    second workgroup of 4 rows."""
    g = torch.Generator().manual_seed(d + n)
    consts = torch.tensor([1.5, 0.0, -3072.0, 2.0 ** -10, 6.0])[:n]
    x = consts[:, None].repeat(1, d)
    w, b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    y = _layernorm(x, w, b)
    assert torch.equal(y, b[None, :].repeat(n, 1))


LN_C_CPU = 1.62  # largest error of torch float32 on the CPU over the 12 cases below, in units of u |mean| rstd max|w|


@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("d", [384, 768, 1024, 1280])
def test_layernorm_large_mean_rows(d, n):
    """Rows of mean 1e3 and standard deviation 1: the rounding of the mean (relative u per add)
    is scaled by |mean| rstd |w| in the output. Bound per row: 1e-5 + c u |mean| / sqrt(var + eps)
    max|w| with c = 4 * LN_C_CPU = 6.48. LN_C_CPU is what torch float32 on the CPU reaches on
    these same inputs: 0.11 .. 1.61 over the 12 cases, the largest at d = 768, n = 5 (absolute
    errors up to 1.2e-4); a wave-tree sum and torch's sum round differently, hence the factor 4.
    The constant is the largest over the cases, not each case's own value: the error is mostly the
    one rounding of the mean, anywhere in [0, 2) units by chance (d = 1024, n = 1: CPU 0.11).
    The GPU kernel measured 0.47 .. 1.44 in the same units (the largest at d = 1280, n = 5,
    absolute 1.1e-4), against the allowed 6.48 + 1e-5."""
    g = torch.Generator().manual_seed(d + n)
    x = 1e3 + torch.randn(n, d, generator=g)
    w, b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (d,), w.double(), b.double(), eps=1e-5)
    xd = x.double()
    unit = U * xd.mean(1).abs() / torch.sqrt(xd.var(1, unbiased=False) + 1e-5) * w.abs().max().item()
    cpu = (torch.nn.functional.layer_norm(x, (d,), w, b, eps=1e-5).double() - ref).abs().max(1).values
    y = _layernorm(x, w, b)
    assert not torch.isnan(y).any()
    err = (y.double() - ref).abs().max(1).values
    print(f"\nlayernorm d {d} n {n}: CPU float32 {(cpu / unit).max().item():.3f}, GPU {(err / unit).max().item():.3f} "
          f"(units of u |mean| rstd max|w|); GPU abs err {err.max().item():.3e}")
    assert (err <= 1e-5 + 4 * LN_C_CPU * unit).all(), (err / unit).tolist()


# ---------------------------------------------------------------- whole encoder

@pytest.mark.parametrize("d,heads", [(768, 12), (1024, 16), (1280, 16)])
def test_encoder_other_sizes_match_oracle(d, heads):
    """The encode path and param_list at the sizes of MODEL_SIZES beyond d = 384 (head dim 64 and
    80): empty, one-token, 17-token and full rows, interior holes on the last."""
    import m3ae_text as om
    vocab, L = 200, 40
    enc = _encoder(vocab, depth=2, d=d, heads=heads)
    tok, msk = _rows([0, 1, 17, 40], L, vocab, seed=d, holes=True)
    ref, _ = om.forward_representation_text(enc.state_dict(), tok, msk, heads)
    enc = enc.to(DEV)
    cls = enc.encode(tok.to(DEV), msk.to(DEV))
    torch.cuda.synchronize()
    assert cls.shape == (4, d)
    _close(cls, ref[:, 0])


def test_encoder_long_plan():
    """1,100 distinct rows of 1-3 tokens: the plan's second chunk feeds embed, attention and the
    final gather. Rows are independent of their packing, so the whole batch is bit-identical to
    its two halves; rows on both sides of the chunk edge match the oracle."""
    import m3ae_text as om
    vocab, L, n = 200, 4, 1100
    enc = _encoder(vocab, depth=1)
    g = torch.Generator().manual_seed(11)
    tok = torch.randint(0, vocab, (n, L), generator=g).to(torch.int32)
    tok[:, 0] = torch.arange(n, dtype=torch.int32) % vocab  # adjacent rows differ on an unpadded token
    lens = torch.randint(1, 4, (n,), generator=g)
    msk = (torch.arange(L)[None, :] >= lens[:, None]).float()
    pick = [0, 1023, 1024, 1099]
    ref, _ = om.forward_representation_text(enc.state_dict(), tok[pick], msk[pick], 6)
    enc = enc.to(DEV)
    tok_d, msk_d = tok.to(DEV), msk.to(DEV)
    plan = m3ae_restate.split(_gpu_plan(tok.numpy(), msk.numpy(), 1, vocab), n)
    assert plan["info"][0] == n  # every row is a unique sequence of its own
    whole = enc.encode(tok_d, msk_d)
    halves = torch.cat([enc.encode(tok_d[:n // 2], msk_d[:n // 2]), enc.encode(tok_d[n // 2:], msk_d[n // 2:])])
    torch.cuda.synchronize()
    assert torch.equal(whole, halves)
    _close(whole[pick], ref[:, 0])
