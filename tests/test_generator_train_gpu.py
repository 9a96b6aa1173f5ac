"""GPU parity of the generator's training form: forward with the spectral-norm power
iteration and the HIP backward (mmre_generator_backward) against the float64 torch-autograd
restatement of spectral_norm.py:39-89 / model.py:679-686 (oracle/zsl_gan.py). Tolerance
1e-4 relative to each gradient's largest magnitude."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _power_iterations(w, u, v, n=3, eps=1e-12):
    """n float64 power iterations of spectral_norm.py:74-85 on the host -> (u, v, sigma)."""
    import torch.nn.functional as F
    for _ in range(n):
        v = F.normalize(torch.mv(w.t(), u), dim=0, eps=eps)
        u = F.normalize(torch.mv(w, v), dim=0, eps=eps)
    return u, v, torch.dot(u, torch.mv(w, v))


# (reduced_dim, noise_dim, D, n, train). The first four are the reference's widths; the others
# move every size: one row (column sums over empty row slices, one output tile row), D = 2 and
# a single noise column (row quarters of the power iteration empty for out < 4), sizes off the
# multiples of 4, 32 and 64, more rows than one GEMM tile with n off a multiple of 4, and the
# limit of 1024 on the first layer's input (1009 + 15) with D = 1024.
_CASES = [pytest.param(384, 15, 200, 512, True, id="512-200-True"),
          pytest.param(384, 15, 200, 20, False, id="20-200-False"),
          pytest.param(384, 15, 256, 37, True, id="37-256-True"),
          pytest.param(384, 15, 1, 9, True, id="9-1-True")]
_CASES += [(*c, t) for c in ((384, 15, 200, 1), (64, 1, 2, 3), (16, 3, 33, 70), (250, 7, 65, 5), (1009, 15, 1024, 6))
           for t in (True, False)]


@pytest.mark.parametrize("rd,nd,D,n,train", _CASES)
def test_generator_backward_matches_autograd(rd, nd, D, n, train):
    """Eval mode takes u, v as they stand; from random u, v the sum u . W v can cancel to almost
    nothing, where float64 itself no longer pins W / sigma. So eval mode starts from three
    float64 power iterations per layer, and |sigma| >= half the spectral norm is asserted on
    the reference."""
    import zsl_gan as og
    from mmre.generator import RelationGenerator
    torch.manual_seed(n + D)
    gen = RelationGenerator(rd, nd, D)
    with torch.no_grad():
        gen.ln_a.normal_(1.0, 0.1)
        gen.ln_b.normal_(0.0, 0.1)
        if not train:
            for L in (gen.generate_fc_layer, gen.des_rel_map_layer1, gen.des_rel_map_layer2):
                w64 = L.weight_orig.double()
                u, v, sigma = _power_iterations(w64, L.weight_u.double(), L.weight_v.double())
                assert sigma.abs().item() >= 0.5 * torch.linalg.matrix_norm(w64, 2).item()
                L.weight_u.copy_(u.float())
                L.weight_v.copy_(v.float())
    layers = [(L.weight_orig.detach().double().clone().requires_grad_(), L.bias.detach().double().clone()
               .requires_grad_(), L.weight_u.double().clone(), L.weight_v.double().clone())
              for L in (gen.generate_fc_layer, gen.des_rel_map_layer1, gen.des_rel_map_layer2)]
    a = gen.ln_a.detach().double().clone().requires_grad_()
    b = gen.ln_b.detach().double().clone().requires_grad_()
    cls, noise = torch.randn(n, rd), 0.1 * torch.randn(n, nd)
    up = torch.randn(n, D)
    ref, uv = og.generator(noise.double(), cls.double(), layers, a, b, train)
    (ref * up.double()).sum().backward()
    gen = gen.to(DEV).train(train)
    out = gen(cls.to(DEV), noise.to(DEV))
    (out * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    got = [gen.generate_fc_layer.weight_orig, gen.generate_fc_layer.bias, gen.des_rel_map_layer1.weight_orig,
           gen.des_rel_map_layer1.bias, gen.des_rel_map_layer2.weight_orig, gen.des_rel_map_layer2.bias,
           gen.ln_a, gen.ln_b]
    want = [layers[0][0], layers[0][1], layers[1][0], layers[1][1], layers[2][0], layers[2][1], a, b]
    for i, (g, w) in enumerate(zip(got, want)):
        gg = g.grad.detach().cpu().double()
        ww = w.grad if w.grad is not None else torch.zeros_like(gg)  # D = 1: LN is the identity
        scale = ww.abs().max().item()
        # + 1e-6 absolute: a 1x1 SN weight (D = 1) is scale-invariant, its exact gradient is 0
        assert (gg - ww).abs().max().item() <= 1e-4 * scale + 1e-6, (i, (gg - ww).abs().max().item(), scale)
    for L, (u2, v2) in zip((gen.generate_fc_layer, gen.des_rel_map_layer1, gen.des_rel_map_layer2), uv):
        assert np.allclose(L.weight_u.cpu().numpy(), u2.numpy(), atol=1e-5)
        assert np.allclose(L.weight_v.cpu().numpy(), v2.numpy(), atol=1e-5)


def test_generator_input_limit():
    """reduced_dim + noise_dim = 1025 is past the power iteration's 1024-float scratch."""
    from mmre._lib import MMREError
    from mmre.generator import RelationGenerator
    gen = RelationGenerator(1010, 15, 8).to(DEV)
    with pytest.raises(MMREError, match="unsupported shape"):
        gen(torch.randn(2, 1010).to(DEV), torch.randn(2, 15).to(DEV))


@pytest.mark.parametrize("grad", [True, False])
@pytest.mark.parametrize("cls_shape,noise_shape", [((4, 63), (4, 5)), ((4, 65), (4, 5)), ((4, 64), (4, 4)),
                                                   ((4, 64), (4, 6)), ((4, 64), (3, 5)), ((3, 64), (4, 5)),
                                                   ((64,), (5,))])
def test_generator_refuses_misshapen_inputs(cls_shape, noise_shape, grad):
    """cls must be (n, reduced_dim) and noise (n, noise_dim) with the same n: the kernels index
    both by those sizes, so a narrower or shorter tensor would be read out of bounds. Refused on
    the host, on the autograd path and the plain one."""
    from mmre._lib import MMREError
    from mmre.generator import RelationGenerator
    gen = RelationGenerator(64, 5, 8).to(DEV)
    with torch.set_grad_enabled(grad), pytest.raises((MMREError, ValueError)):
        gen(torch.randn(*cls_shape).to(DEV), torch.randn(*noise_shape).to(DEV))
