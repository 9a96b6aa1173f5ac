"""CPU side of the TransR training path (csrc/transh_train.hip's TransR part, mmre.transr_ns): the
entry points' error codes and their precedence (model, then null pointers, then shape) on
never-dereferenced addresses -- every call below carries a fault that is refused before the first
launch -- the supported() rule, the workspace's monotonicity and what it reserves, the seed search
of every GPU case (tests/transr_train_cases.py), the float64 restatement against the reference's
own numbers (tests/golden/transr_train.npz) and a CPU model's training through autograd."""
import itertools

import numpy as np
import pytest
import torch

import transr_train_cases as C
from mmre import transr_ns  # noqa: F401  (the path under test: without it nothing here has a subject)

ARG, MODEL, SHAPE = 1, 2, 3
TRANSR_L1, TRANSR_L2 = 9, 10
_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, never dereferenced

HEAD = ("model", "norm_flag", "model_margin", "use_model_margin", "ent", "rel", "transfer_matrix", "n_ent", "n_rel",
        "dim_e", "dim_r", "h", "t", "r", "batch", "neg", "loss_margin", "adv_t", "regul_rate")
PARAMS = {
    "mmre_transr_ns_forward": HEAD + ("score", "loss", "work", "stream"),
    "mmre_transr_ns_grad": HEAD + ("score", "grad_loss", "grad_ent", "grad_rel", "grad_transfer_matrix", "work", "lr",
                                   "stream"),
}
POINTERS = ("ent", "rel", "transfer_matrix", "h", "t", "r", "score", "loss", "work", "grad_loss", "grad_ent", "grad_rel",
            "grad_transfer_matrix")


def run(name, **over):
    from mmre import _lib
    a = {p: fake() for p in PARAMS[name] if p in POINTERS}
    a.update(model=TRANSR_L1, norm_flag=1, model_margin=0.0, use_model_margin=0, n_ent=10, n_rel=3, dim_e=12, dim_r=8,
             batch=4, neg=2, loss_margin=1.0, adv_t=0.0, regul_rate=0.0, lr=0.0, stream=None)
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
    assert len(_lib.SIGNATURES["mmre_transr_ns_supported"][1]) == 4
    assert len(_lib.SIGNATURES["mmre_transr_ns_workspace"][1]) == 6
    for name in list(PARAMS) + ["mmre_transr_ns_supported", "mmre_transr_ns_workspace"]:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name), name


@pytest.mark.parametrize("name", list(PARAMS))
def test_error_codes_and_precedence(name):
    for m in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11):   # the TransR ids only
        assert run(name, model=m) == MODEL, m
        assert run(name, model=m, ent=None, dim_e=4096) == MODEL, m   # ... before pointers and shape
    for p in PARAMS[name]:
        if p in POINTERS:
            assert run(name, **{p: None}) == ARG, p
            assert run(name, **{p: None}, dim_e=513) == ARG, p        # pointers before the shape
            assert run(name, **{p: None}, model=TRANSR_L2, neg=0) == ARG, p
    for bad in (dict(dim_e=0), dict(dim_e=513), dict(dim_e=-4), dict(dim_r=0), dict(dim_r=513), dict(dim_r=-1),
                dict(dim_e=513, dim_r=513), dict(neg=0), dict(neg=513), dict(batch=0), dict(n_ent=0), dict(n_rel=0),
                dict(n_ent=1 << 31), dict(n_rel=1 << 31), dict(batch=1 << 27, neg=1)):
        for m in (TRANSR_L1, TRANSR_L2):
            assert run(name, model=m, **bad) == SHAPE, bad


def test_older_training_entry_points_still_refuse_transr():
    from mmre import _lib
    import test_ns_abi_cpu as ns
    import test_transd_train_cpu as tdt
    import test_transh_train_cpu as tht
    for m in (TRANSR_L1, TRANSR_L2):
        for name in ("mmre_ns_forward", "mmre_ns_fused_forward", "mmre_ns_fused_grad", "mmre_ns_fused_grad_sgd"):
            assert ns.run(name, False, model=m) == MODEL, (name, m)
        assert not _lib.lib().mmre_ns_fused_supported(m, 64, 4, 0)
        for name in tht.PARAMS:
            assert tht.run(name, model=m) == MODEL, (name, m)
        for name in tdt.PARAMS:
            assert tdt.run(name, model=m) == MODEL, (name, m)
        assert not _lib.lib().mmre_transh_ns_supported(m, 64, 4)
        assert not _lib.lib().mmre_transd_ns_supported(m, 64, 64, 4)


def test_supported_rule():
    from mmre import _lib, transr_ns
    fn = _lib.lib().mmre_transr_ns_supported
    for de in (-1, 0, 1, 7, 64, 65, 512, 513, 2048):
        for dr in (-1, 0, 1, 7, 64, 65, 512, 513):
            for neg in (-1, 0, 1, 25, 512, 513):
                want = 1 <= dr <= 512 and 1 <= de <= 512 and 1 <= neg <= 512   # either order of the dims
                assert transr_ns.supported(de, dr, neg) is want, (de, dr, neg)
                for m in range(-1, 12):
                    assert bool(fn(m, de, dr, neg)) is (want and m in (TRANSR_L1, TRANSR_L2)), (m, de, dr, neg)


def test_workspace_is_monotone():
    from mmre import _lib
    ws = _lib.lib().mmre_transr_ns_workspace
    base = dict(batch=5, neg=3, n_ent=301, n_rel=6, dim_e=64, dim_r=8)
    order = ("batch", "neg", "n_ent", "n_rel", "dim_e", "dim_r")
    w0 = ws(*[base[k] for k in order])
    # per row: two slots of (projection, its gradient, entity record) and a relation record; one partial matrix
    assert w0 >= 5 * 4 * (2 * (2 * 8 + 64) + 8) + 64 * 8
    for k, steps in dict(batch=(6, 256, 257, 2721), neg=(4, 25, 512), n_ent=(302, 14541), n_rel=(7, 237, 1345),
                         dim_e=(65, 200, 512), dim_r=(9, 63, 64, 200, 512)).items():
        prev = w0
        for v in steps:
            w = ws(*[dict(base, **{k: v})[q] for q in order])
            assert w >= prev > 0, (k, v)
            prev = w
    for bad in ((5, 3, 301, 6, 513, 64), (5, 3, 301, 6, 64, 513), (5, 3, 301, 6, 64, 0), (5, 3, 301, 6, 0, 64),
                (5, 0, 301, 6, 64, 64), (5, 513, 301, 6, 64, 64), (0, 3, 301, 6, 64, 64)):
        assert ws(*bad) == -1, bad
    assert ws(5, 3, 301, 6, 8, 64) > 0 and ws(1, 1, 1, 1, 1, 1) > 0 and ws(1, 512, 2, 1, 512, 512) > 0
    # the training shape stays addressable, and under 1 GiB
    assert 0 < ws(2721, 25, 14541, 237, 200, 200) * 4 < (1 << 30)
    assert 0 < ws(2721, 25, 14208, 235, 200, 200) * 4 < (1 << 30)


def test_every_gpu_case_has_a_clear_seed():
    keys = C.all_case_keys()
    assert len(keys) > 100
    for args, kw in keys:
        c = C.case(*args, **kw)
        assert 50 <= c["seed"] < 90
        assert C.clear(c["ref"], c["B"], c["K"], kw.get("both_sides", True)), (args, kw)
        assert np.isfinite(c["ref"][0]) and all(np.isfinite(g).all() for g in c["ref"][2].values()), (args, kw)
        if c["B"] * c["K"] >= 20 and kw.get("both_sides", True):
            assert 0.0 < c["ref"][3][2] < 1.0, (args, kw)
        if kw.get("zero_rows"):   # the clamped gradients are large, and representable in float32
            assert max(np.abs(g).max() for g in c["ref"][2].values()) < 1e30, (args, kw)
        if not kw.get("identity") and not kw.get("zero_rows"):   # general matrices: an identity hides transpositions
            M = c["tabs"]["transfer_matrix"].view(c["n_rel"], c["de"], c["dr"])
            assert float(M[:, 0, 1:].abs().min()) > 0 and float(M[:, 1:, 0].abs().min()) > 0   # off the diagonal


def test_live_slot_counts_straddle_the_kernels_constants():
    """The one-relation cases lie on both sides of the row tile, the rank segment and the dmat
    segment; live_slots restates the sharing rule of the kernels' index."""
    h = torch.tensor([1, 2, 1, 5, 1, 2])
    t = torch.tensor([3, 4, 3, 4, 9, 4])
    r = torch.tensor([0, 1, 0, 1, 1, 1])
    # B = 2: row 2 repeats positive 0 (no slot); row 3 shares its tail with positive 1; row 4 has
    # another relation than positive 0 (two slots); row 5 repeats positive 1
    assert C.live_slots(h, t, r, 2) == 4 + 0 + 1 + 2 + 0
    slots = [C.case(1, True, 9, 7, B, K, n_rel=1)["slots"] for B, K in C.HUB_EDGE]
    assert slots[0] <= C.TR_TM < slots[1] and slots[2] <= C.TR_DSEG == C.TR_ISEG < slots[3], slots
    big = [C.case(1, True, 9, 7, B, K, n_rel=1)["slots"] for B, K in C.HUB_SEG[:3]]
    assert min(big) > C.TR_DSEG and max(big) > 2 * C.TR_DSEG, big


def test_restatement_equals_the_reference_fixture(golden):
    """The repo's float64 TransR ops + MarginLoss + regularization (the yardstick of the GPU
    tests) on the fixture's inputs against what the reference's own classes computed."""
    g = golden("transr_train")
    names = [str(n) for n in g["names"]]
    assert len(names) == 8
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    for name in names:
        z = lambda k: g[f"{name}.{k}"]
        de, dr = int(z("dim_e")), int(z("dim_r"))
        w = lambda k: torch.from_numpy(g[f"d{de}_{dr}.{k}"])   # shared per width pair
        tabs = {k: w(k) for k in C.KEYS}
        assert all(v.dtype == torch.float32 for v in tabs.values())
        assert tabs["ent"].shape[1] == de and tabs["rel"].shape[1] == dr and tabs["transfer_matrix"].shape[1] == de * dr
        h, t, r = (w(k) for k in ("h", "t", "r"))
        ref = C.reference(tabs, de, dr, h, t, r, int(z("B")), int(z("p_norm")), bool(z("norm_flag")),
                          float(z("loss_margin")), None, float(z("regul")))
        assert C.clear(ref, int(z("B")), int(z("K"))), name
        assert rel(ref[0], z("loss")) <= 1e-12 and rel(ref[1], z("score")) <= 1e-12, name
        for k in C.KEYS:
            assert rel(ref[2][k], z("grad_" + k)) <= 1e-12, (name, k)


def test_cpu_model_trains_through_autograd():
    from mmre import transr_ns
    from openke.module.loss import MarginLoss
    from openke.module.model import TransR
    from openke.module.strategy import NegativeSampling
    torch.manual_seed(0)
    m = TransR(C.E, C.R, dim_e=20, dim_r=16, p_norm=1, norm_flag=True, rand_init=True)
    assert m.ns_spec() is None and m.fused_ns_transr(3) is None   # CPU tables: no offer
    st = NegativeSampling(model=m, loss=MarginLoss(margin=4.0), batch_size=4, regul_rate=0.1)
    h, t, r = C.batch(4, 3, 7)
    opt = torch.optim.SGD(st.parameters(), lr=0.5)
    n0, losses = transr_ns.calls, []
    for _ in range(3):
        opt.zero_grad()
        loss = st({"batch_h": h, "batch_t": t, "batch_r": r, "mode": "normal"})
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert transr_ns.calls == n0 and losses[2] < losses[0]
    for w in C.weights(m).values():
        assert w.grad is not None and float(w.grad.abs().sum()) > 0
