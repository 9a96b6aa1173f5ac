"""mmre.optim.Adagrad: the HIP step (mmre_adagrad_step) and the step fused into the negative-
sampling backward's row owner against torch.optim.Adagrad, bit for bit -- parameters,
state["sum"] and state["step"]."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in ((7, 3), (1001,), (13, 5))]  # 21, 1001, 65: no multiple of 4


def _steps(opt_cls, **kw):
    ps = [p.to(DEV).clone().requires_grad_(True) for p in _params()]
    opt = opt_cls(ps, lr=0.5, **kw)
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        ps[0].grad = (torch.randn(ps[0].shape, generator=g) * (3.0 if step != 1 else 1e-3)).to(DEV)
        ps[1].grad = torch.randn(ps[1].shape, generator=g).to(DEV)
        ps[1].grad[::5] = 0.0
        # ps[2]: no gradient
        opt.step()
    torch.cuda.synchronize()
    return ps, opt


def test_adagrad_step_equals_torch():
    from mmre.optim import Adagrad
    before = Adagrad.fallback_steps
    mine, mo = _steps(Adagrad)
    assert Adagrad.fallback_steps == before
    ref, ro = _steps(torch.optim.Adagrad)
    start = _params()
    for a, b, s in zip(mine, ref, start):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(mo.state[a]["sum"], ro.state[b]["sum"])
        assert torch.equal(mo.state[a]["step"].cpu(), ro.state[b]["step"].cpu())
    assert not torch.equal(mine[0].detach().cpu(), start[0]) and torch.equal(mine[2].detach().cpu(), start[2])
    assert float(mo.state[mine[0]]["step"]) == 3.0 and float(mo.state[mine[2]]["step"]) == 0.0
    sd = mo.state_dict()  # torch's own layout: loads into torch's optimizer
    ro.load_state_dict(sd)


def test_adagrad_other_configurations_fall_back_and_are_counted():
    from mmre.optim import Adagrad
    before = Adagrad.fallback_steps
    mine, mo = _steps(Adagrad, weight_decay=0.1)
    assert Adagrad.fallback_steps == before + 3 and "weight_decay" in Adagrad.fallback_reason
    ref, ro = _steps(torch.optim.Adagrad, weight_decay=0.1)
    for a, b in zip(mine, ref):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(mo.state[a]["sum"], ro.state[b]["sum"])


def _ns_setup(model):
    from mmre.link import rotate_phase_denom
    from mmre.ns import NSSpec
    E, R, B, K = 500, 11, 37, 25
    d = {"distmult": 200, "complex": 72, "rotate": 130}[model]
    g = torch.Generator().manual_seed(3)
    u = lambda n, c, s: (torch.rand((n, c), generator=g) * 2 - 1) * s
    if model == "distmult":
        tabs = {"ent": u(E, d, 0.5), "rel": u(R, d, 0.5)}
    elif model == "complex":
        tabs = {"ent": u(E, d, 0.5), "rel": u(R, d, 0.5), "ent_im": u(E, d, 0.5), "rel_im": u(R, d, 0.5)}
    else:
        tabs = {"ent": u(E, 2 * d, 8.0 / (2 * d)), "rel": u(R, d, 8.0 / d)}
    spec = NSSpec(model, d, model_margin=6.0 if model == "rotate" else None,
                  phase_denom=rotate_phase_denom(6.0, 2.0, d) if model == "rotate" else 0.0)
    batches = []
    for _ in range(3):
        h, t, r = (torch.randint(0, n, (B,), generator=g) for n in (E, E, R))
        H, T = [h], [t]
        for j in range(K):
            c = torch.randint(0, E, (B,), generator=g)
            H.append(c if j % 2 == 0 else h)
            T.append(t if j % 2 == 0 else c)
        batches.append((torch.cat(H).to(DEV), torch.cat(T).to(DEV), r.repeat(K + 1).to(DEV)))
    return tabs, spec, batches, B, K


@pytest.mark.parametrize("model", ["distmult", "complex", "rotate"])
def test_fused_adagrad_step_equals_backward_then_torch_step(model):
    from mmre.ns import fused_ns_loss
    from mmre.optim import Adagrad
    tabs, spec, batches, B, K = _ns_setup(model)
    out = []
    before = Adagrad.fallback_steps
    for fuse in (False, True):
        T = {n: v.to(DEV).clone().requires_grad_(True) for n, v in tabs.items()}
        opt = (Adagrad if fuse else torch.optim.Adagrad)(list(T.values()), lr=0.5)
        for h, t, r in batches:
            opt.zero_grad(set_to_none=True)
            loss, _ = fused_ns_loss(spec, T["ent"], T["rel"], h, t, r, B, K, 0.0, None, 1.0, ent_im=T.get("ent_im"),
                                    rel_im=T.get("rel_im"), loss="softplus", optimizer=opt if fuse else None)
            loss.backward()
            if fuse:
                assert len(opt._fused_done) == len(T)
            opt.step()
        torch.cuda.synchronize()
        out.append({n: (v.detach().clone(), v.grad.clone(), opt.state[v]["sum"].clone(), float(opt.state[v]["step"]))
                    for n, v in T.items()})
    assert Adagrad.fallback_steps == before
    for n in tabs:
        assert torch.equal(out[0][n][0], out[1][n][0]), n  # parameters
        assert torch.equal(out[0][n][1], out[1][n][1]), n  # gradients
        assert torch.equal(out[0][n][2], out[1][n][2]), n  # sum
        assert out[0][n][3] == out[1][n][3] == 3.0
        assert not torch.equal(out[0][n][0], tabs[n].to(DEV))


def test_second_backward_before_step_raises():
    from mmre.ns import fused_ns_loss
    from mmre.optim import Adagrad
    tabs, spec, batches, B, K = _ns_setup("distmult")
    T = {n: v.to(DEV).clone().requires_grad_(True) for n, v in tabs.items()}
    opt = Adagrad(list(T.values()), lr=0.5)
    opt.zero_grad(set_to_none=True)
    h, t, r = batches[0]
    loss, _ = fused_ns_loss(spec, T["ent"], T["rel"], h, t, r, B, K, 0.0, None, 1.0, loss="softplus", optimizer=opt)
    loss.backward()
    loss2, _ = fused_ns_loss(spec, T["ent"], T["rel"], h, t, r, B, K, 0.0, None, 1.0, loss="softplus", optimizer=opt)
    loss2.backward()
    with pytest.raises(RuntimeError):
        opt.step()


def test_single_tensor_implementation_falls_back():
    """foreach=False is torch's single-tensor step, which scales the quotient instead of the gradient
    (other roundings wherever lr is not a power of two): torch's own step runs, counted."""
    from mmre.optim import Adagrad
    before = Adagrad.fallback_steps
    outs = []
    for cls in (Adagrad, torch.optim.Adagrad):
        p = _params()[1].to(DEV).clone().requires_grad_(True)
        opt = cls([p], lr=0.0123, foreach=False)
        p.grad = _params(seed=2)[1].to(DEV)
        opt.step()
        outs.append((p.detach().clone(), opt.state[p]["sum"].clone()))
    assert Adagrad.fallback_steps == before + 1 and "foreach" in Adagrad.fallback_reason
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
