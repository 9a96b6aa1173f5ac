"""Which rounding does torch.optim.Adagrad's plain step (lr_decay 0, weight_decay 0, no
maximize) use on this ROCm build? Three steps of torch's optimizer are compared bit for bit with
host float32 / float64 models of
    sum <- sum + g*g       as one fma, or as a rounded product then an add
    std  = sqrt(sum) + eps (correctly rounded sqrt -- taken in float64 and rounded once more,
                            which is exact for a square root: the host's float32 sqrt is
                            vectorised and not correctly rounded -- then a float add)
    p   <- p + (g * -lr) / std   as rounded product, correctly rounded quotient, add
                                 or as the product times a rounded reciprocal, then add
and with the same sequence through torch's own elementwise device kernels, for the default
(foreach), foreach=False and fused=True implementations, and state["step"]'s type is printed.
The host's float32 +, * and / are IEEE (one rounding each); the fma model forms the exact product
in float64 (48 significant bits) and rounds the sum once more."""
import torch

torch.manual_seed(0)
dev = torch.device("cuda:0")
n = 1 << 20


def models(p, s, g, lr32, eps32):
    """host candidates from host float32 tensors: dict name -> (p', sum')"""
    s_fma = (s.double() + g.double() * g.double()).float()
    s_mul = s + g * g
    out = {}
    for sn, s1 in (("fma", s_fma), ("mul+add", s_mul)):
        std = torch.sqrt(s1.double()).float() + eps32
        num = g * (-lr32)
        out[f"sum {sn}, p + num/std"] = (p + num / std, s1)
        out[f"sum {sn}, p + num*(1/std)"] = (p + num * (1.0 / std), s1)
        out[f"sum {sn}, fma(num, 1/std, p)"] = ((p.double() + num.double() * (1.0 / std).double()).float(), s1)
    # the same sequence through torch's own elementwise kernels on the device: its sqrt and quotient
    # as the optimizer's kernels compute them (the build's divide / sqrt, IEEE or not)
    pd, sd, gd = p.to(dev), s.to(dev), g.to(dev)
    s1 = sd + gd * gd
    out["device ops: sum mul+add, p + num/std"] = ((pd + (gd * (-lr32.item())) / (torch.sqrt(s1) + eps32.item())).cpu(),
                                                   s1.cpu())
    return out


for lr, eps in ((0.5, 1e-10), (0.0123, 1e-10), (1.0, 1e-3)):
    lr32 = torch.tensor(lr, dtype=torch.float32)
    eps32 = torch.tensor(eps, dtype=torch.float32)
    for kw in ({}, {"foreach": False}, {"fused": True}):
        p0 = torch.randn(n, device=dev)
        try:
            p = p0.clone().requires_grad_(True)
            opt = torch.optim.Adagrad([p], lr=lr, eps=eps, **kw)
        except Exception as e:  # an implementation this build does not offer
            print(f"lr {lr} eps {eps} {kw}: not available ({type(e).__name__})")
            continue
        alive = None
        try:
            p.grad = torch.zeros_like(p)
            opt.step()  # fused=True is refused at the first step on a device this build does not fuse
            opt.state[p]["step"].zero_()
        except RuntimeError as e:
            print(f"lr {lr} eps {eps} {kw}: not available ({str(e)[:60]}...)")
            continue
        for step in range(3):
            g = torch.randn(n, device=dev) * (3.7 if step != 1 else 1e-3)
            g[::7] = 0.0  # torch leaves p and sum of a zero gradient unchanged?
            before_p, before_s = p.detach().clone().cpu(), opt.state[p]["sum"].clone().cpu()
            p.grad = g.clone()
            opt.step()
            got_p, got_s = p.detach().cpu(), opt.state[p]["sum"].cpu()
            cand = models(before_p, before_s, g.cpu(), lr32, eps32)
            zero_same = bool(torch.equal(got_p[::7], before_p[::7]) and torch.equal(got_s[::7], before_s[::7]))
            names = [k for k, (cp, cs) in cand.items() if torch.equal(cp, got_p) and torch.equal(cs, got_s)]
            alive = set(names) if alive is None else alive & set(names)
            diffs = {k: ((cp != got_p).sum().item(), (cs != got_s).sum().item()) for k, (cp, cs) in cand.items()}
            print(f"lr {lr} eps {eps} {kw or 'default'} step {step + 1}: g == 0 leaves p, sum unchanged {zero_same}; "
                  f"(p, sum) elements differing per model {diffs}")
        st = opt.state[p]["step"]
        print(f"lr {lr} eps {eps} {kw or 'default'}: bit-equal over 3 steps: {sorted(alive)}; state['step'] = "
              f"{st!r} ({st.dtype}, {st.device})")
sq = torch.rand(n, device=dev) * 100
exact = torch.sqrt(sq.cpu().double()).float()  # correctly rounded
print("device sqrt == correctly rounded sqrt:", torch.equal(torch.sqrt(sq).cpu(), exact), "differing",
      (torch.sqrt(sq).cpu() != exact).sum().item(), "; host float32 sqrt differing from it",
      (torch.sqrt(sq.cpu()) != exact).sum().item())
num = torch.randn(n, device=dev)
print("device quotient == host quotient:", torch.equal((num / sq).cpu(), num.cpu() / sq.cpu()),
      "differing", ((num / sq).cpu() != num.cpu() / sq.cpu()).sum().item())
