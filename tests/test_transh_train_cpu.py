"""CPU side of the TransH training path (csrc/transh_train.hip, mmre.transh_ns): the entry points'
error codes and their precedence (model, then null pointers, then shape) on never-dereferenced
addresses -- every call below carries a fault that is refused before the first launch -- the
supported() rule, the workspace's monotonicity, the seed search of every GPU case
(tests/transh_train_cases.py), the float64 restatement against the reference's own numbers
(tests/golden/transh_train.npz) and a CPU model's training through autograd."""
import itertools

import numpy as np
import pytest
import torch

import transh_train_cases as C

ARG, MODEL, SHAPE = 1, 2, 3
TRANSH_L1, TRANSH_L2 = 5, 6
_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, never dereferenced

HEAD = ("model", "norm_flag", "model_margin", "use_model_margin", "ent", "rel", "norm", "n_ent", "n_rel", "dim", "h",
        "t", "r", "batch", "neg", "loss_margin", "adv_t", "regul_rate")
PARAMS = {
    "mmre_transh_ns_forward": HEAD + ("score", "loss", "work", "stream"),
    "mmre_transh_ns_grad": HEAD + ("score", "grad_loss", "grad_ent", "grad_rel", "grad_norm", "work", "lr", "stream"),
}
POINTERS = ("ent", "rel", "norm", "h", "t", "r", "score", "loss", "work", "grad_loss", "grad_ent", "grad_rel",
            "grad_norm")


def run(name, **over):
    from mmre import _lib
    a = {p: fake() for p in PARAMS[name] if p in POINTERS}
    a.update(model=TRANSH_L1, norm_flag=1, model_margin=0.0, use_model_margin=0, n_ent=10, n_rel=3, dim=8, batch=4,
             neg=2, loss_margin=1.0, adv_t=0.0, regul_rate=0.0, lr=0.0, stream=None)
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    return getattr(_lib.lib(), name)(*[a[p] for p in PARAMS[name]])


def test_signatures_and_header():
    import os
    import re
    from mmre import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmre.h")).read()
    for name, params in PARAMS.items():
        assert len(_lib.SIGNATURES[name][1]) == len(params), name
    for name in list(PARAMS) + ["mmre_transh_ns_supported", "mmre_transh_ns_workspace"]:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name), name


@pytest.mark.parametrize("name", list(PARAMS))
def test_error_codes_and_precedence(name):
    for m in (-1, 0, 1, 2, 3, 4, 7):   # the TransH ids only
        assert run(name, model=m) == MODEL, m
        assert run(name, model=m, ent=None, dim=4096) == MODEL, m   # ... before pointers and shape
    for p in PARAMS[name]:
        if p in POINTERS:
            assert run(name, **{p: None}) == ARG, p
            assert run(name, **{p: None}, dim=513) == ARG, p        # pointers before the shape
            assert run(name, **{p: None}, model=TRANSH_L2, neg=0) == ARG, p
    for bad in (dict(dim=0), dict(dim=513), dict(dim=-4), dict(neg=0), dict(neg=513), dict(batch=0), dict(n_ent=0),
                dict(n_rel=0), dict(n_ent=1 << 31), dict(n_rel=1 << 31), dict(batch=1 << 27, neg=1)):
        for m in (TRANSH_L1, TRANSH_L2):
            assert run(name, model=m, **bad) == SHAPE, bad


def test_the_generic_ns_entry_points_still_refuse_transh():
    from mmre import _lib
    import test_ns_abi_cpu as ns
    for name in ("mmre_ns_forward", "mmre_ns_fused_forward", "mmre_ns_fused_grad", "mmre_ns_fused_grad_sgd"):
        for m in (TRANSH_L1, TRANSH_L2):
            assert ns.run(name, False, model=m) == MODEL, (name, m)
    assert not _lib.lib().mmre_ns_fused_supported(TRANSH_L1, 64, 4, 0)


def test_supported_rule():
    from mmre import _lib, transh_ns
    fn = _lib.lib().mmre_transh_ns_supported
    for dim in (-1, 0, 1, 7, 64, 65, 512, 513, 2048):
        for neg in (-1, 0, 1, 25, 512, 513):
            want = 1 <= dim <= 512 and 1 <= neg <= 512
            assert transh_ns.supported(dim, neg) is want, (dim, neg)
            for m in range(-1, 9):
                assert bool(fn(m, dim, neg)) is (want and m in (TRANSH_L1, TRANSH_L2)), (m, dim, neg)


def test_workspace_is_monotone():
    from mmre import _lib
    ws = _lib.lib().mmre_transh_ns_workspace
    base = dict(batch=5, neg=3, n_ent=301, n_rel=6, dim=64)
    order = ("batch", "neg", "n_ent", "n_rel", "dim")
    w0 = ws(*[base[k] for k in order])
    assert w0 >= 4 * 5 * 4 * 64   # a record for each (row, table) pair at least
    for k, steps in dict(batch=(6, 256, 257, 2721), neg=(4, 25, 512), n_ent=(302, 14541), n_rel=(7, 237),
                         dim=(65, 200, 512)).items():
        prev = w0
        for v in steps:
            w = ws(*[dict(base, **{k: v})[q] for q in order])
            assert w >= prev > 0, (k, v)
            prev = w
    assert ws(5, 3, 301, 6, 513) < 0 and ws(5, 0, 301, 6, 64) < 0 and ws(0, 3, 301, 6, 64) < 0
    # the training shape stays within a 32-bit count of floats times four: addressable, and under 1 GiB
    assert 0 < ws(2721, 25, 14541, 237, 200) * 4 < (1 << 30)


def test_every_gpu_case_has_a_clear_seed():
    keys = C.all_case_keys()
    assert len(keys) > 100
    for args, kw in keys:
        c = C.case(*args, **kw)
        assert C.clear(c["ref"], c["B"], c["K"], kw.get("both_sides", True)), (args, kw)
        assert np.isfinite(c["ref"][0]) and all(np.isfinite(g).all() for g in c["ref"][2].values()), (args, kw)


def test_restatement_equals_the_reference_fixture(golden):
    """The repo's float64 TransH ops + MarginLoss + regularization (the yardstick of the GPU
    tests) on the fixture's inputs against what the reference's own classes computed."""
    g = golden("transh_train")
    names = [str(n) for n in g["names"]]
    assert len(names) == 8
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    for name in names:
        z = lambda k: g[f"{name}.{k}"]
        w = lambda k: torch.from_numpy(g[f"d{int(z('d'))}.{k}"])   # a width's four cases share tables and batch
        tabs = {k: w(k) for k in ("ent", "rel", "norm")}
        assert all(v.dtype == torch.float32 for v in tabs.values())
        h, t, r = (w(k) for k in ("h", "t", "r"))
        ref = C.reference(tabs, h, t, r, int(z("B")), int(z("p_norm")), bool(z("norm_flag")), float(z("loss_margin")),
                          None, float(z("regul")))
        assert C.clear(ref, int(z("B")), int(z("K"))), name
        assert rel(ref[0], z("loss")) <= 1e-12 and rel(ref[1], z("score")) <= 1e-12, name
        for k in ("ent", "rel", "norm"):
            assert rel(ref[2][k], z("grad_" + k)) <= 1e-12, (name, k)


def test_cpu_model_trains_through_autograd():
    from mmre import transh_ns
    from openke.module.loss import MarginLoss
    from openke.module.model import TransH
    from openke.module.strategy import NegativeSampling
    torch.manual_seed(0)
    m = TransH(C.E, C.R, dim=16, p_norm=1, norm_flag=True)
    assert m.ns_spec() is None and m.fused_ns(3) is None   # CPU tables: no offer
    st = NegativeSampling(model=m, loss=MarginLoss(margin=4.0), batch_size=4, regul_rate=0.1)
    h, t, r = C.batch(4, 3, 7)
    opt = torch.optim.SGD(st.parameters(), lr=0.5)
    n0, losses = transh_ns.calls, []
    for _ in range(3):
        opt.zero_grad()
        loss = st({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert transh_ns.calls == n0 and losses[2] < losses[0]
    for w in (m.ent_embeddings.weight, m.rel_embeddings.weight, m.norm_vector.weight):
        assert w.grad is not None and float(w.grad.abs().sum()) > 0
