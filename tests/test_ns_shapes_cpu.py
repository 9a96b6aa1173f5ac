"""mmre_ns_fused_supported / mmre_ns_rows_supported (host-only queries: the library loads without a
device) against the rule as DESIGN.md section 10d states it in prose -- TransE: the margin loss
only, dim <= 512, K <= 32; DistMult / ComplEx / RotatE: any loss, dim <= 512, K <= 512; the rows
path: dim <= 2048, K <= 512 -- and OpenKETrainStep refusing a shape without fused kernels when it is
built, not at its first call."""
import itertools

import pytest
import torch

MODELS = {"transe": 0, "transe_l2": 1, "distmult": 2, "complex": 3, "rotate": 4}
DIMS = (1, 64, 65, 512, 513, 2048, 2049)
KS = (0, 1, 32, 33, 512, 513)
KINDS = {"margin": 0, "softplus": 1, "sigmoid": 2}


def _rule(model, dim, K, kind):
    """The prose rule, written without the library's helpers."""
    if model in ("transe", "transe_l2"):
        return kind == "margin" and dim <= 512 and K <= 32
    return dim <= 512 and K <= 512


def test_fused_supported_truth_table():
    from mmre import _lib
    from mmre.ns import MODEL_IDS
    assert MODEL_IDS == MODELS and _lib.LOSS_KINDS == KINDS
    lib = _lib.lib()
    assert "mmre_ns_fused_supported" in _lib.SIGNATURES and "mmre_ns_rows_supported" in _lib.SIGNATURES
    for (model, mid), dim, K, (kind, kid) in itertools.product(MODELS.items(), DIMS, KS, KINDS.items()):
        got = lib.mmre_ns_fused_supported(mid, dim, K, kid)
        assert got == int(_rule(model, dim, K, kind)), (model, dim, K, kind, got)


def test_python_query_is_the_library_query():
    from mmre.ns import NSSpec, fused_supported, rows_supported
    for model, dim, K, (kind, kid) in itertools.product(MODELS, DIMS, KS, KINDS.items()):
        assert fused_supported(NSSpec(model, dim), K, kid) is _rule(model, dim, K, kind), (model, dim, K, kind)
    for dim, K in itertools.product(DIMS, KS):
        assert rows_supported(NSSpec("transe", dim), K) is (dim <= 2048 and K <= 512), (dim, K)


def test_queries_reject_what_is_no_shape():
    from mmre import _lib
    lib = _lib.lib()
    for mid, dim, K, kid in ((-1, 64, 5, 0), (5, 64, 5, 0), (2, 0, 5, 0), (2, -3, 5, 0), (0, 64, -1, 0), (2, 64, 5, 3),
                             (2, 64, 5, -1)):
        assert lib.mmre_ns_fused_supported(mid, dim, K, kid) == 0, (mid, dim, K, kid)
    for dim, K in ((0, 5), (-1, 5), (64, -1)):
        assert lib.mmre_ns_rows_supported(dim, K) == 0, (dim, K)


def test_every_fused_shape_is_a_rows_shape():
    """The rows path is the fall-back of every shape the fused kernels lack: it has to cover theirs."""
    from mmre import _lib
    lib = _lib.lib()
    for mid, dim, K, kid in itertools.product(MODELS.values(), DIMS, KS, KINDS.values()):
        if lib.mmre_ns_fused_supported(mid, dim, K, kid):
            assert lib.mmre_ns_rows_supported(dim, K) == 1, (mid, dim, K, kid)


@pytest.mark.parametrize("model,dim,K,loss", [("transe", 64, 33, "margin"), ("transe", 513, 5, "margin"),
                                              ("transe_l2", 1024, 64, "margin"), ("distmult", 513, 5, "softplus"),
                                              ("rotate", 520, 64, "sigmoid"), ("complex", 64, 513, "margin"),
                                              ("distmult", 64, 0, "margin")])
def test_train_step_refuses_an_unsupported_shape_when_built(model, dim, K, loss):
    """ValueError from the constructor, before any tensor is looked at (host tensors, no sampler)."""
    from mmre.ns import NSSpec, OpenKETrainStep
    spec = NSSpec(model, dim, model_margin=6.0 if model == "rotate" else None, phase_denom=1.0 if model == "rotate" else 0.0)
    ent, rel = torch.zeros(4, 2 * dim if model == "rotate" else dim), torch.zeros(2, dim)
    im = dict(ent_im=torch.zeros(4, dim), rel_im=torch.zeros(2, dim)) if model == "complex" else {}
    with pytest.raises(ValueError, match="no fused kernels"):
        OpenKETrainStep(None, spec, ent, rel, 3, K, 1.0, 0.5, loss=loss, **im)
