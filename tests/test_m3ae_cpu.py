"""CPU checks of the M3AE text-encoder path: the host pieces (position
table, reference parameter names, state-dict loading), the oracle's padding
invariances -- the property the padding-free HIP path relies on -- and the C ABI exports and
argument checks (nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

BLOCK_KEYS = ("layer_norm1.weight", "layer_norm1.bias", "attention.qkv_linear.weight", "attention.qkv_linear.bias",
              "attention.fc.weight", "attention.fc.bias", "layer_norm2.weight", "layer_norm2.bias",
              "transformer_mlp.fc1.weight", "transformer_mlp.fc1.bias", "transformer_mlp.fc2.weight",
              "transformer_mlp.fc2.bias")


def _encoder(vocab=50, depth=2, seed=0):
    from mmre.m3ae import M3AETextEncoder
    torch.manual_seed(seed)
    enc = M3AETextEncoder(vocab, 384, depth, 6)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return enc


def test_pos_table_matches_reference_formula():
    import m3ae_text as om
    from mmre.m3ae import sincos_pos_embed_1d
    t = sincos_pos_embed_1d(384, 320)
    assert torch.equal(t, om.sincos_pos_embed_1d(384, 320)[0])
    pos = np.arange(320)[:, None].astype(np.float64)
    omega = 1.0 / 10000 ** (np.arange(192) / 192.0)
    ref = np.concatenate([np.sin(pos * omega), np.cos(pos * omega)], 1)
    assert np.abs(t.numpy() - ref).max() < 1e-4  # fp32 evaluation of model.py:113-133


def test_state_dict_names_follow_reference():
    enc = _encoder(depth=2)
    keys = set(enc.state_dict())
    expected = {"text_embedding.weight", "encoder_text_type_embedding", "cls_token", "encoder.layer_norm.weight",
                "encoder.layer_norm.bias"}
    expected |= {f"encoder.blocks.{i}.{k}" for i in range(2) for k in BLOCK_KEYS}
    assert keys == expected
    sd = enc.state_dict()
    assert sd["encoder.blocks.0.attention.qkv_linear.weight"].shape == (1152, 384)
    assert sd["encoder.blocks.1.transformer_mlp.fc1.weight"].shape == (1536, 384)
    assert sd["cls_token"].shape == (1, 1, 384)
    assert not any(p.requires_grad for p in enc.parameters())


def test_model_type_sizes():
    from mmre.m3ae import M3AETextEncoder
    e = M3AETextEncoder(10, model_type="tiny")
    assert (e.emb_dim, e.depth, e.num_heads) == (384, 2, 6)


def test_load_reference_state_dict_ignores_decoder():
    enc, other = _encoder(seed=0), _encoder(seed=1)
    full = dict(enc.state_dict())
    full["decoder.blocks.0.layer_norm1.weight"] = torch.ones(512)
    full["image_embedding.weight"] = torch.zeros(384, 768)
    other.load_reference_state_dict(full)
    for k, v in other.state_dict().items():
        assert torch.equal(v, full[k])
    del full["cls_token"]
    with pytest.raises(KeyError):
        other.load_reference_state_dict(full)


def test_oracle_padding_is_inert():
    """What the padding-free HIP path relies on: the CLS output does not depend on the token ids
    at padded positions (bit-identical: their softmax weights are exactly 0), and a right-padded
    row equals its truncation up to summation order."""
    import m3ae_text as om
    enc = _encoder(vocab=60, depth=2)
    sd = enc.state_dict()
    g = torch.Generator().manual_seed(3)
    L = 24
    tok = torch.randint(0, 60, (3, L), generator=g)
    msk = torch.zeros(3, L)
    msk[0, 10:] = 1
    msk[1, 3:7] = 1
    msk[1, 15:] = 1
    cls, _ = om.forward_representation_text(sd, tok, msk, 6)
    tok2 = torch.where(msk > 0, torch.randint(0, 60, (3, L), generator=g), tok)
    cls2, _ = om.forward_representation_text(sd, tok2, msk, 6)
    assert torch.equal(cls, cls2)
    short, _ = om.forward_representation_text(sd, tok[:1, :10], msk[:1, :10], 6)
    assert torch.allclose(short, cls[:1], atol=1e-5, rtol=0)


def test_m3ae_c_abi_exports_and_argument_checks():
    from mmre import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("mmre_m3ae_max_len", "mmre_m3ae_plan_size", "mmre_m3ae_plan", "mmre_m3ae_workspace", "mmre_m3ae_encode",
              "mmre_m3ae_layernorm", "mmre_m3ae_linear", "mmre_m3ae_attention", "mmre_m3ae_linear_tile"):
        assert hasattr(L, n)
    lib = _lib.lib()
    assert lib.mmre_m3ae_max_len() >= 320
    assert lib.mmre_m3ae_workspace(100, 4, 384) == 100 * 384 * 10 + 4 * 384 * 7
    dummy = ctypes.c_void_p(16)
    # shape / argument errors come back as status codes before any launch
    assert lib.mmre_m3ae_linear(0, dummy, 10, 100, dummy, 384, dummy, None, dummy, None) == 3  # k % 32
    assert lib.mmre_m3ae_linear(0, dummy, 10, 384, dummy, 200, dummy, None, dummy, None) == 3  # n % 64
    assert lib.mmre_m3ae_linear(2, dummy, 10, 384, dummy, 384, dummy, None, dummy, None) == 1  # no residual
    assert lib.mmre_m3ae_layernorm(dummy, 4, 200, dummy, dummy, 1e-5, dummy, None) == 3
    assert lib.mmre_m3ae_attention(dummy, dummy, 2, 400, 6, 64, 0.125, 0, dummy, None) == 3  # rows > max
    assert lib.mmre_m3ae_attention(dummy, dummy, 2, 10, 6, 32, 0.125, 0, dummy, None) == 3  # head dim
    assert lib.mmre_m3ae_plan_size(10) == 65
    assert lib.mmre_m3ae_plan(dummy, dummy, 2, 400, 1, 10, dummy, None) == 1  # len > max_len
    params = (ctypes.c_void_p * 30)(*([16] * 30))
    assert lib.mmre_m3ae_encode(ctypes.cast(params, ctypes.c_void_p), 2, 200, 4, 1e-5, dummy, dummy, 1, 8, 10,
                                dummy, 1, 9, 9, dummy, 10 ** 6, dummy, None) == 3  # d = 200 unsupported
    assert lib.mmre_m3ae_encode(ctypes.cast(params, ctypes.c_void_p), 2, 384, 6, 1e-5, dummy, dummy, 2, 8, 10,
                                dummy, 3, 9, 9, dummy, 10 ** 6, dummy, None) == 1  # n_unique > n_seq


def test_linear_tile_threshold_and_override(monkeypatch):
    """mmre_m3ae_linear_tile, the launcher's own choice: 128 exactly when n % 128 == 0 and
    ceil(m / 64) * (n / 128) >= 2048; MMRE_M3AE_TILE is read at every call and cannot force 128
    on an n that is no multiple of 128; -1 for the shapes mmre_m3ae_linear refuses."""
    from mmre import _lib
    tile = _lib.lib().mmre_m3ae_linear_tile
    monkeypatch.delenv("MMRE_M3AE_TILE", raising=False)
    assert tile(10880, 1536) == 64 and tile(10881, 1536) == 128
    assert tile(10 ** 6, 192) == 64
    for n in (64, 128, 192, 256, 384, 1152, 1536, 5120):
        for mt in (1, 2047, 2048, -(-2048 * 128 // n) - 1, -(-2048 * 128 // n), 4096):
            for m in (64 * mt - 63, 64 * mt, 64 * mt + 1):
                rule = n % 128 == 0 and -(-m // 64) * (n // 128) >= 2048
                assert tile(m, n) == (128 if rule else 64), (m, n)
    assert tile(0, 128) == 64  # an empty output is accepted (nothing is launched)
    for m, n in ((-1, 128), (10, 0), (10, -64), (10, 200), (10, 96), (2 ** 40, 64)):
        assert tile(m, n) == -1, (m, n)
    monkeypatch.setenv("MMRE_M3AE_TILE", "128")
    assert tile(1, 128) == 128 and tile(10880, 1536) == 128
    assert tile(70, 192) == 64 and tile(10 ** 6, 192) == 64
    assert tile(10, 200) == -1
    monkeypatch.setenv("MMRE_M3AE_TILE", "64")
    assert tile(10881, 1536) == 64 and tile(1, 128) == 64
    monkeypatch.setenv("MMRE_M3AE_TILE", "")
    assert tile(10880, 1536) == 64 and tile(10881, 1536) == 128
    monkeypatch.delenv("MMRE_M3AE_TILE")
    assert tile(10880, 1536) == 64 and tile(10881, 1536) == 128


def test_encode_refuses_too_many_unique_sequences_before_any_launch():
    """Attention's grid holds 65,535 sequences; an otherwise valid encode of 65,536 is refused in
    the argument checks (nothing is launched: this passes without a device)."""
    from mmre import _lib
    lib = _lib.lib()
    dummy = ctypes.c_void_p(16)
    params = (ctypes.c_void_p * 30)(*([16] * 30))
    n = 65536
    work = lib.mmre_m3ae_workspace(2 * n, n, 384)
    assert lib.mmre_m3ae_encode(ctypes.cast(params, ctypes.c_void_p), 2, 384, 6, 1e-5, dummy, dummy, n, 8, 10,
                                dummy, n, 2 * n, 9, dummy, work, dummy, None) == 3
    assert lib.mmre_m3ae_encode(ctypes.cast(params, ctypes.c_void_p), 2, 384, 6, 1e-5, dummy, dummy, n + 5, 8, 10,
                                dummy, n, 2 * n, 9, dummy, work, dummy, None) == 3
    # the other checks still win where they applied before
    assert lib.mmre_m3ae_encode(ctypes.cast(params, ctypes.c_void_p), 2, 384, 6, 1e-5, dummy, dummy, n, 8, 10,
                                dummy, n + 1, 2 * n, 9, dummy, work, dummy, None) == 1  # n_unique > n_seq


def test_plan_restatement_on_handwritten_rows():
    """tests/m3ae_restate.py on the six rows of test_plan_dedupes_adjacent_repeats_and_counts_bad_ids
    (tests/test_m3ae_gpu.py), whose expected plan is written out by hand."""
    import m3ae_restate
    L = 8
    rows = [([1, 2, 3, 0, 0, 0, 0, 0], 3), ([1, 2, 3, 9, 9, 9, 9, 9], 3), ([1, 2, 3, 0, 0, 0, 0, 0], 4),
            ([1, 2, 3, 0, 0, 0, 0, 0], 4), ([5, 5, 5, 5, 5, 5, 5, 5], 8), ([1, 2, 3, 0, 0, 0, 0, 0], 3)]
    tok = np.array([r for r, _ in rows], dtype=np.int32)
    msk = np.array([[0.0] * n + [1.0] * (L - n) for _, n in rows], dtype=np.float32)
    p = m3ae_restate.plan(tok, msk, 1, 10)
    assert list(p["cnt"]) == [4, 4, 5, 5, 9, 4] and list(p["head"]) == [1, 0, 1, 0, 1, 1]
    assert list(p["uniq"]) == [0, 0, 1, 1, 2, 3]
    assert list(p["src"]) == [0, 2, 4, 5]
    assert list(p["off"]) == [0, 4, 9, 18, 22]
    assert list(p["info"]) == [4, 22, 9, 0]
    p = m3ae_restate.plan(tok, msk, 0, 5)
    assert list(p["uniq"]) == list(range(6)) and list(p["src"]) == list(range(6))
    assert list(p["off"]) == [0, 4, 8, 13, 18, 27, 31]
    assert list(p["info"]) == [6, 31, 9, 8]
    # the mask rule is `mask > 0`: -1, -0.0 and NaN are unpadded, a denormal and +inf are padding
    m = np.array([[-1.0, -0.0, np.nan, 1e-40, np.inf]], dtype=np.float32)
    assert list(m3ae_restate.plan(np.zeros((1, 5), np.int32), m, 1, 10)["cnt"]) == [4]
    # no rows / empty rows
    assert list(m3ae_restate.plan(np.zeros((0, 3), np.int32), np.zeros((0, 3)), 1, 10)["info"]) == [0, 0, 1, 0]
    p = m3ae_restate.plan(np.zeros((3, 0), np.int32), np.zeros((3, 0)), 1, 10)
    assert list(p["uniq"]) == [0, 0, 0] and list(p["off"]) == [0, 1] and list(p["info"]) == [1, 1, 1, 0]
    # split() reads the same fields back out of a plan buffer
    buf = np.full(6 * 6 + 5, -7, dtype=np.int32)
    p = m3ae_restate.plan(tok, msk, 1, 10)
    buf[:6], buf[6:10], buf[12:17], buf[19:23] = p["uniq"], p["src"], p["off"], p["info"]
    m3ae_restate.assert_plan_equal(buf, 6, p)
    buf[14] += 1
    with pytest.raises(AssertionError):
        m3ae_restate.assert_plan_equal(buf, 6, p)


def test_encoder_needs_device_tensors():
    from mmre._lib import MMREError
    enc = _encoder()
    with pytest.raises(MMREError):
        enc.encode(torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4)))
