"""GPU checks of the small split-K GEMM (csrc/gemm.hip) behind the GAN Discriminator's products
and their autograd (mmre/gemm.py): values against float64, strided (transposed) operands, the
K-split path, and first and second derivatives against torch's float64 autograd -- the
gradient penalty differentiates the Discriminator's gradient (module/utils.py:692-707)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _close(got, ref, tol=1e-5):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("m,k,n", [(512, 200, 200), (200, 512, 200), (206, 512, 200), (512, 200, 1), (1, 7, 3),
                                   (33, 1000, 65), (5, 0, 4)])
def test_mm_values_and_strides(m, k, n):
    from mmre import _lib
    from mmre.gemm import mm_hip
    g = torch.Generator().manual_seed(m * 7 + k + n)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(k, n, generator=g)
    ref = a.double() @ b.double()
    _close(mm_hip(a.to(DEV), b.to(DEV)), ref)
    # transposed views: a stored (k, m), b stored (n, k)
    at = a.t().contiguous().to(DEV).t()
    bt = b.t().contiguous().to(DEV).t()
    _close(mm_hip(at, bt), ref)
    torch.cuda.synchronize()
    assert _lib.lib().mmre_gemm_splits(m, n, k) >= 1


def test_mm_double_backward_matches_float64():
    """grad of a gradient-penalty-like objective through mm (create_graph=True)."""
    from mmre.gemm import mm
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(64, 48, generator=g)
    w0 = torch.randn(40, 48, generator=g) / 7
    c0 = torch.randn(30, 40, generator=g)

    def objective(x, w, c, matmul):
        h = torch.tanh(matmul(x, w.t()))
        s = matmul(h, c.t())
        gx = torch.autograd.grad(s.sum(), x, create_graph=True)[0]
        return ((gx.norm(2, dim=1) - 1) ** 2).mean()

    xs, ws, cs = (t.double().requires_grad_() for t in (x0, w0, c0))
    ref = objective(xs, ws, cs, torch.matmul)
    ref.backward()
    xd, wd, cd = (t.to(DEV).requires_grad_() for t in (x0, w0, c0))
    out = objective(xd, wd, cd, mm)
    out.backward()
    torch.cuda.synchronize()
    _close(out, ref, 1e-4)
    for a, b in ((xd, xs), (wd, ws), (cd, cs)):
        _close(a.grad, b.grad, 1e-4)


def test_mm_bias_and_splits():
    from mmre.gemm import gemm_splits, mm
    g = torch.Generator().manual_seed(5)
    a, b, bias = torch.randn(512, 200, generator=g), torch.randn(200, 384, generator=g), torch.randn(384, generator=g)
    ref = a.double() @ b.double() + bias.double()
    _close(mm(a.to(DEV), b.to(DEV), bias.to(DEV)), ref)
    assert 1 <= gemm_splits(512, 200, 200) <= 8 and gemm_splits(32, 32, 4096) == 8 and gemm_splits(7, 7, 31) == 1


# (m, k, n) -> (slices, kslice) the launch is claimed to take: S = min(8, k // 32, ceil(1024 / tiles))
# (at least 1), kslice = ceil(k / S). One output tile: S = min(8, k // 32), so k = 65 gives two
# slices of 33 and 32 -- the second wave starts on an odd k, and the (k, k + 1) pairing of
# v_mfma_f32_32x32x2_f32 straddles the slice boundary; k = 257 gives eight slices of 33 with a
# last slice of 26; k < 32 and 32 <= k < 64 are the single-slice path, one or several load rounds.
_EXACT = {(32, k, 32): (max(1, min(8, k // 32)), None)
          for k in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 255, 256, 257, 1000)}
_EXACT.update({
    (32, 65, 32): (2, 33), (32, 95, 32): (2, 48), (32, 255, 32): (7, 37), (32, 257, 32): (8, 33),
    (32, 1000, 32): (8, 125), (32, 63, 32): (1, 63),
    (31, 65, 33): (2, 33),      # two tiles, ragged rows and one ragged column
    (33, 65, 31): (2, 33),      # two tiles the other way
    (1, 257, 1): (8, 33),       # one row, one column, odd slices
    (200, 257, 384): (8, 33),   # 84 tiles: ceil(1024 / 84) = 13, still the K limit of 8
    (97, 1024, 65): (8, 128),   # 12 tiles, the longest exact K
    (512, 257, 384): (6, 43),   # 192 tiles: ceil(1024 / 192) = 6 slices, set by the tile count
})


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


@pytest.mark.parametrize("m,k,n", sorted(_EXACT))
def test_mm_exact_at_slice_boundaries(m, k, n):
    """Operands drawn from the integers in [-4, 4], K <= 1024: every product and partial sum is
    an integer below 2^14, exact in float32 in any order, so mm_hip must EQUAL the float64
    product -- a dropped, doubled or misplaced k fails whatever its size (randn inputs under a
    1e-5 bar can hide one small term). Shapes sit on the K-slicing boundaries (table above);
    the slice count and slice length are asserted. Each shape also runs with both operands as
    transposed views, a as a column-strided slice, b as a stride-0 expand of one row, and a
    bias."""
    from mmre.gemm import gemm_splits, mm_hip
    S, kslice = _EXACT[(m, k, n)]
    tiles = ((m + 31) // 32) * ((n + 31) // 32)
    assert S == max(1, min(8, k // 32, -(-1024 // tiles)))
    assert gemm_splits(m, n, k) == S
    assert kslice is None or -(-k // S) == kslice
    g = torch.Generator().manual_seed(m * 131 + k * 7 + n)
    a, b, bias = _ints(g, m, k), _ints(g, k, n), _ints(g, n)
    ref = (a.double() @ b.double()).float()
    ad, bd = a.to(DEV), b.to(DEV)
    assert torch.equal(mm_hip(ad, bd).cpu(), ref)
    # transposed views: a stored (k, m), b stored (n, k)
    assert torch.equal(mm_hip(a.t().contiguous().to(DEV).t(), b.t().contiguous().to(DEV).t()).cpu(), ref)
    # a as every second column of a (m, 2k) matrix (the other columns must not be read as a's)
    big = _ints(g, m, 2 * k)
    big[:, ::2] = a
    a_sl = big.to(DEV)[:, ::2]
    assert a_sl.stride() == (2 * k, 2)
    assert torch.equal(mm_hip(a_sl, bd).cpu(), ref)
    # b as one row repeated down k with stride 0
    row = _ints(g, 1, n)
    b_ex = row.to(DEV).expand(k, n)
    assert k == 1 or b_ex.stride() == (0, 1)
    assert torch.equal(mm_hip(ad, b_ex).cpu(), (a.double() @ row.double().expand(k, n)).float())
    # bias in the epilogue
    assert torch.equal(mm_hip(ad, bd, bias.to(DEV)).cpu(), (a.double() @ b.double() + bias.double()).float())


def test_mm_repeats_bit_for_bit():
    """(200, 257, 384), 84 tiles of 8 odd slices: the slice-order sum is fixed, two runs agree
    bit for bit (randn operands, so a changed order would show)."""
    from mmre.gemm import mm_hip
    g = torch.Generator().manual_seed(17)
    a, b = torch.randn(200, 257, generator=g).to(DEV), torch.randn(257, 384, generator=g).to(DEV)
    first = mm_hip(a, b).cpu()
    assert torch.equal(mm_hip(a, b).cpu(), first)
    _close(first, a.cpu().double() @ b.cpu().double())


def test_mm_zero_sizes():
    """m == 0 and n == 0 (k > 0) give empty outputs -- PretrainStep.loss reaches m == 0 when a
    relation has no query triples left -- and backpropagate to zero gradients of the right
    shapes; k == 0 with a bias returns the bias rows. Would catch the NULL pointers of empty
    tensors being refused as bad arguments."""
    from mmre.gemm import mm, mm_hip
    g = torch.Generator().manual_seed(19)
    a0, b = torch.zeros(0, 5, device=DEV), torch.randn(5, 7, generator=g).to(DEV)
    a, b0 = torch.randn(4, 5, generator=g).to(DEV), torch.zeros(5, 0, device=DEV)
    bias = torch.randn(7, generator=g).to(DEV)
    for out, shape in ((mm_hip(a0, b), (0, 7)), (mm_hip(a0, b, bias), (0, 7)), (mm_hip(a, b0), (4, 0)),
                       (mm_hip(a0, b0), (0, 0))):
        assert out.shape == shape and out.dtype == torch.float32 and out.is_cuda
    for x, y, bz in ((a0, b, bias), (a, b0, torch.zeros(0, device=DEV))):
        x, y, bz = (t.clone().requires_grad_() for t in (x, y, bz))
        out = mm(x, y, bz)
        assert out.shape == (x.shape[0], y.shape[1])
        out.sum().backward()
        torch.cuda.synchronize()
        for t in (x, y, bz):
            assert t.grad.shape == t.shape and not t.grad.any()
    k0 = mm_hip(torch.zeros(5, 0, device=DEV), torch.zeros(0, 7, device=DEV), bias)
    assert torch.equal(k0, bias.expand(5, 7))
    assert torch.equal(mm_hip(torch.zeros(5, 0, device=DEV), torch.zeros(0, 7, device=DEV)),
                       torch.zeros(5, 7, device=DEV))


def _power_iterations(w, u, v, n=3, eps=1e-12):
    """n float64 power iterations of spectral_norm.py:74-85 on the host -> (u, v, sigma)."""
    import torch.nn.functional as F
    for _ in range(n):
        v = F.normalize(torch.mv(w.t(), u), dim=0, eps=eps)
        u = F.normalize(torch.mv(w, v), dim=0, eps=eps)
    return u, v, torch.dot(u, torch.mv(w, v))


# column sums over four row quarters (empty when out < 4), 256 columns per pass (255 / 256 / 257),
# one wave per row for the dot products, and the limit of 1024 on either side
_SN_SHAPES = [(200, 200), (1, 200), (384, 399),
              (1, 1), (3, 5), (4, 256), (5, 257), (65, 64), (7, 1024), (1024, 7), (1024, 1024)]


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("out,inn", _SN_SHAPES)
def test_sn_weight_matches_spectral_norm(train, out, inn):
    """mmre.gemm.sn_weight == torch.nn.utils.spectral_norm's weight (spectral_norm.py:39-89):
    W / sigma, the in-place u, v update of the power iteration, and dL/dW_orig. Training mode is
    well conditioned (after one power iteration sigma = |W v|). Eval mode uses u, v as they
    stand, and from random u, v the sum u . W v can cancel to almost nothing, where float64
    itself no longer pins W / sigma: so eval mode starts from three float64 power iterations,
    and the reference's |sigma| is asserted to be at least half the spectral norm."""
    from mmre.gemm import sn_weight
    torch.manual_seed(out + inn)
    ref = torch.nn.utils.spectral_norm(torch.nn.Linear(inn, out)).double()
    mod = torch.nn.utils.spectral_norm(torch.nn.Linear(inn, out)).to(DEV)
    if not train:
        with torch.no_grad():
            w64 = ref.weight_orig.detach()
            u, v, sigma = _power_iterations(w64, ref.weight_u.clone(), ref.weight_v.clone())
            ref.weight_u.copy_(u)
            ref.weight_v.copy_(v)
            assert sigma.abs().item() >= 0.5 * torch.linalg.matrix_norm(w64, 2).item()
    with torch.no_grad():
        mod.weight_orig.copy_(ref.weight_orig.float())
        mod.weight_u.copy_(ref.weight_u.float())
        mod.weight_v.copy_(ref.weight_v.float())
    ref.train(train)
    mod.train(train)
    up = torch.randn(out, inn)
    ref(torch.zeros(1, inn, dtype=torch.float64))  # runs the hook: ref.weight = W / sigma
    (ref.weight * up.double()).sum().backward()
    w = sn_weight(mod)
    (w * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _close(w, ref.weight, 1e-5)
    _close(mod.weight_u, ref.weight_u, 1e-5)
    _close(mod.weight_v, ref.weight_v, 1e-5)
    _close(mod.weight_orig.grad, ref.weight_orig.grad, 1e-4)


def test_layer_norm_first_and_second_order():
    """mmre.gemm.layer_norm == LayerNormalization (module/submodule.py:58-77): values, the
    first-order backward (HIP) and a create_graph double backward (torch ops)."""
    from mmre.gemm import layer_norm
    from module.submodule import LayerNormalization
    torch.manual_seed(11)
    ln = LayerNormalization(200)
    with torch.no_grad():
        ln.a_2.normal_(1.0, 0.2)
        ln.b_2.normal_(0.0, 0.2)
    z0, up = torch.randn(300, 200) * 3 + 1, torch.randn(300, 200)
    import torch.nn as nn
    import zsl_gan

    class _RefLN(nn.Module):  # the reference formula in float64 torch ops (oracle/zsl_gan.py)
        def __init__(self):
            super().__init__()
            self.a_2 = nn.Parameter(ln.a_2.detach().double().clone())
            self.b_2 = nn.Parameter(ln.b_2.detach().double().clone())

        def forward(self, z):
            return zsl_gan.layer_norm_ref(z, self.a_2, self.b_2, ln.eps)

    lref = _RefLN()
    zr = z0.double().requires_grad_()
    out_r = lref(zr)
    (out_r * up.double()).sum().backward()
    lhip = ln.to(DEV)
    zd = z0.to(DEV).requires_grad_()
    out_d = layer_norm(lhip, zd)
    (out_d * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _close(out_d, out_r, 1e-5)
    for got, want in ((zd.grad, zr.grad), (lhip.a_2.grad, lref.a_2.grad), (lhip.b_2.grad, lref.b_2.grad)):
        _close(got, want, 1e-4)

    def penalty(z, f):
        o = f(z)
        gz = torch.autograd.grad((o * o).sum(), z, create_graph=True)[0]
        return (gz.norm(2, dim=1) - 1).pow(2).mean()

    lref.zero_grad()
    lhip.zero_grad()
    zr = z0.double().requires_grad_()
    pr = penalty(zr, lref)
    pr.backward()
    zd = z0.to(DEV).requires_grad_()
    pd = penalty(zd, lambda z: layer_norm(lhip, z))
    pd.backward()
    torch.cuda.synchronize()
    _close(pd, pr, 1e-4)
    for got, want in ((zd.grad, zr.grad), (lhip.a_2.grad, lref.a_2.grad), (lhip.b_2.grad, lref.b_2.grad)):
        _close(got, want, 1e-4)


@pytest.mark.parametrize("out,inn", [(1025, 8), (8, 1025)])
def test_sn_weight_size_limit(out, inn):
    """One 1024-thread workgroup with 1024-float scratch per side: a larger side is refused."""
    from mmre._lib import MMREError
    from mmre.gemm import sn_weight
    mod = torch.nn.utils.spectral_norm(torch.nn.Linear(inn, out)).to(DEV)
    with pytest.raises(MMREError, match="unsupported shape"):
        sn_weight(mod)


def _ln_pair(D, seed):
    """(HIP-side LayerNormalization on the device, float64 a_2 / b_2 leaves of the reference)."""
    from module.submodule import LayerNormalization
    torch.manual_seed(seed)
    ln = LayerNormalization(D)
    with torch.no_grad():
        ln.a_2.normal_(1.0, 0.2)
        ln.b_2.normal_(0.0, 0.2)
    a64 = ln.a_2.detach().double().clone().requires_grad_()
    b64 = ln.b_2.detach().double().clone().requires_grad_()
    return ln.to(DEV), a64, b64


# one wave per row, four rows per workgroup, 16 row slices per column sum (empty when n < 16):
# D below, at and above one pass of the 64 lanes and far above; n below 4, off a multiple of 4,
# and above 16
@pytest.mark.parametrize("n", [1, 5, 17])
@pytest.mark.parametrize("D", [2, 3, 63, 64, 65, 200, 1000])
def test_layer_norm_sizes(D, n):
    """mmre.gemm.layer_norm at other sizes than (300, 200): values, the HIP first-order backward
    (z, a_2, b_2 gradients) and the create_graph torch-op backward against
    zsl_gan.layer_norm_ref in float64 (1e-5 on values, 1e-4 on gradients), and the two backwards
    against each other within 1e-5 -- every bar relative to max(1, max|ref|), as in the rest of
    this file. Would catch a lane loop that drops the columns past a
    multiple of 64, a row slice of the column sums that is skipped or taken twice when n is
    small, and the last workgroup's missing rows."""
    import zsl_gan
    from mmre.gemm import layer_norm
    ln, a64, b64 = _ln_pair(D, 100 * D + n)
    z0, up = torch.randn(n, D) * 3 + 1, torch.randn(n, D)
    zr = z0.double().requires_grad_()
    out_r = zsl_gan.layer_norm_ref(zr, a64, b64, ln.eps)
    gr = torch.autograd.grad((out_r * up.double()).sum(), (zr, a64, b64))
    zd = z0.to(DEV).requires_grad_()
    out_d = layer_norm(ln, zd)
    loss = (out_d * up.to(DEV)).sum()
    g_hip = torch.autograd.grad(loss, (zd, ln.a_2, ln.b_2), retain_graph=True)                 # HIP backward
    g_ops = torch.autograd.grad(loss, (zd, ln.a_2, ln.b_2), create_graph=True)                 # torch-op form
    torch.cuda.synchronize()
    _close(out_d, out_r, 1e-5)
    for hip, ops, want in zip(g_hip, g_ops, gr):
        assert hip.shape == want.shape and ops.shape == want.shape
        _close(hip, want, 1e-4)
        _close(ops, want, 1e-4)
        _close(hip, ops.detach(), 1e-5)


@pytest.mark.parametrize("D", [2, 3, 63, 64, 65, 200, 1000])
def test_layer_norm_offset_rows(D):
    """Rows far from zero (z = randn + 64): a two-pass float32 LayerNormalization, which the
    kernel is, stays at or below 1.7e-5 of float64 here; a one-pass variance
    (sum z^2 - n mean^2) loses the variance's leading digits to the offset and is at or above
    1.1e-3. The bar of 1e-4 sits between the two."""
    import zsl_gan
    from mmre.gemm import layer_norm
    ln, a64, b64 = _ln_pair(D, 7 * D)
    z0 = torch.randn(5, D) + 64
    ref = zsl_gan.layer_norm_ref(z0.double(), a64, b64, ln.eps).detach()
    with torch.no_grad():
        out = layer_norm(ln, z0.to(DEV))
    torch.cuda.synchronize()
    _close(out, ref, 1e-4)


def test_layer_norm_degenerate_sizes():
    """D == 1 is the identity with the gradient passed through (submodule.py:69-70); n == 0
    gives an empty output, an empty z gradient and zero a_2 / b_2 gradients, from the HIP
    backward and from the create_graph form."""
    from mmre.gemm import layer_norm
    ln, _, _ = _ln_pair(1, 3)
    z = torch.randn(6, 1).to(DEV).requires_grad_()
    up = torch.randn(6, 1).to(DEV)
    out = layer_norm(ln, z)
    assert torch.equal(out, z)
    (out * up).sum().backward()
    assert torch.equal(z.grad, up)
    ln, _, _ = _ln_pair(200, 4)
    for create_graph in (False, True):
        z = torch.zeros(0, 200, device=DEV).requires_grad_()
        out = layer_norm(ln, z)
        assert out.shape == (0, 200)
        gz, ga, gb = torch.autograd.grad(out.sum(), (z, ln.a_2, ln.b_2), create_graph=create_graph)
        torch.cuda.synchronize()
        assert gz.shape == (0, 200)
        for p in (ga, gb):
            assert p.shape == (200,) and not p.any()
