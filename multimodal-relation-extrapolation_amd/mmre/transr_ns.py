"""Fused TransR negative-sampling loss (csrc/transh_train.hip, the TransR part) as a
torch.autograd.Function: mmre.transd_ns.fused_ns_loss for a model with one dim_e x dim_r matrix per
relation.

forward  = TransR.forward in 'normal' mode for the B (1 + K) rows of [pos | neg_1 | ... | neg_K]
           -> MarginLoss (optionally self-adversarial) + regul_rate * TransR.regularization (the
           squared one) (OpenKE TransR.py:37-95, NegativeSampling.py:23-32, MarginLoss.py:24-28):
           the relation-major index of the batch's projection slots, the projection as a grouped
           GEMM on f32 MFMA, row kernels and a fixed-order reduction (mmre_transr_ns_forward).
backward = d(loss)/d(ent, rel, transfer_matrix) into dense gradient tables, every row written, no
           float atomics, bit-reproducible: two more grouped MFMA GEMMs and the row owners
           (mmre_transr_ns_grad). With `optimizer` (an mmre.optim.SGD doing plain SGD on the three
           tables) the same pass applies its step, p <- fma(-lr, g, p), and optimizer.step() then
           skips the tables.
"""
from __future__ import annotations

import torch

from ._lib import MMREError, call, lib, mark_written, ptr, require_cuda, stream_ptr
from .transr import MODEL_IDS

# calls of fused_ns_loss since import: which path a strategy took (tests, scripts/bench_transr_train.py)
calls = 0


class TRSpec:
    """Static description of TransR.forward: p_norm, dim_e, dim_r, norm_flag and the model's margin."""

    def __init__(self, p_norm: int, dim_e: int, dim_r: int, norm_flag: bool = True, model_margin: float | None = None):
        if p_norm not in (1, 2):
            raise ValueError("TRSpec: p_norm must be 1 or 2")
        self.model = "transr" if p_norm == 1 else "transr_l2"
        self.model_id = MODEL_IDS[self.model]
        self.dim_e, self.dim_r = int(dim_e), int(dim_r)
        self.norm_flag = bool(norm_flag)
        self.use_model_margin = model_margin is not None
        self.model_margin = float(model_margin or 0.0)


def supported(dim_e: int, dim_r: int, neg: int) -> bool:
    """Whether the kernels exist for the shape: 1 <= dim_e, dim_r <= 512 in either order and
    1 <= neg <= 512 (mmre_transr_ns_supported, the library's own rule)."""
    fn = getattr(lib(), "mmre_transr_ns_supported", None)
    if fn is None:
        raise MMREError("libmmre_hip.so does not export mmre_transr_ns_supported: rebuild it")
    return bool(fn(MODEL_IDS["transr"], int(dim_e), int(dim_r), int(neg)))


def _head(spec, ent, rel, tmat, h, t, r, batch, neg, loss_margin, adv_t, regul_rate):
    return (spec.model_id, int(spec.norm_flag), spec.model_margin, int(spec.use_model_margin), ptr(ent), ptr(rel),
            ptr(tmat), int(ent.shape[0]), int(rel.shape[0]), spec.dim_e, spec.dim_r, ptr(h), ptr(t), ptr(r), batch, neg,
            float(loss_margin), float(adv_t), float(regul_rate))


class _FusedTransRNS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ent, rel, tmat, h, t, r, spec, batch, neg, loss_margin, adv_t, regul_rate, sgd):
        dev = ent.device
        n = batch * (1 + neg)
        score = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(score)
        ctx.set_materialize_grads(False)
        need = int(lib().mmre_transr_ns_workspace(batch, neg, int(ent.shape[0]), int(rel.shape[0]), spec.dim_e,
                                                  spec.dim_r))
        if need < 0:
            raise MMREError("transr_ns.fused_ns_loss: unsupported sizes (code 3): the batch, the negatives and the "
                            "tables' rows together exceed the kernels' index range")
        work = torch.empty(need, dtype=torch.float32, device=dev)
        head = _head(spec, ent, rel, tmat, h, t, r, batch, neg, loss_margin, adv_t, regul_rate)
        call("mmre_transr_ns_forward", *head, ptr(score), ptr(loss), ptr(work), stream_ptr(dev))
        ctx.cfg = (spec, batch, neg, loss_margin, adv_t, regul_rate)
        ctx.work, ctx.sgd = work, sgd   # the index, the projections and the regulariser's value stay in `work`
        ctx.save_for_backward(ent, rel, tmat, h, t, r, score)
        return loss[0], score

    @staticmethod
    def backward(ctx, g_loss, g_score):
        if g_loss is None:
            return (None,) * 13
        ent, rel, tmat, h, t, r, score = ctx.saved_tensors
        spec, batch, neg, loss_margin, adv_t, regul_rate = ctx.cfg
        dev = ent.device
        gl = g_loss.reshape(1).to(torch.float32).contiguous()
        grads = tuple(torch.empty_like(x) for x in (ent, rel, tmat))  # every row written: no fills
        lr, sgd = 0.0, ctx.sgd
        if sgd is not None:
            lr = float(sgd[1])
        head = _head(spec, ent, rel, tmat, h, t, r, batch, neg, loss_margin, adv_t, regul_rate)
        call("mmre_transr_ns_grad", *head, ptr(score), ptr(gl), *(ptr(g) for g in grads), ptr(ctx.work), lr,
             stream_ptr(dev))
        if sgd is not None and lr != 0.0:  # the optimizer's plain step rode in the owner pass: step() skips these
            opt, _, tables = sgd
            mark_written(*tables)
            opt._fused_applied(tables)
        ctx.work = ctx.sgd = None
        return grads + (None,) * 10


def fused_ns_loss(spec: TRSpec, ent, rel, transfer_matrix, h, t, r, batch: int, neg: int, loss_margin: float,
                  adv_temperature: float | None = None, regul_rate: float = 0.0, optimizer=None):
    """Returns (loss scalar tensor, scores (B (1 + K),)); differentiable w.r.t. the three tables
    (float32 device tensors). h / t / r: the batch's ids, laid out [pos | neg_1 | ... ].
    optimizer: taken only when it is an mmre.optim.SGD whose fusable_lr(the three tables) is not
    None (plain SGD, the tables in one group, no gradient on them yet): the backward then applies
    its step as well and optimizer.step() skips the tables -- parameters bit-identical to
    backward() + step(), p.grad still written. Any other optimizer (Adagrad, momentum, ...) is
    ignored here and step() does the update. A shape without kernels (supported()) raises
    MMREError before anything is launched."""
    global calls
    require_cuda(ent, rel, transfer_matrix, h, t, r)
    tables = [ent, rel, transfer_matrix]
    if any(x.dtype != torch.float32 for x in tables):
        raise TypeError("transr_ns.fused_ns_loss: float32 tables")
    if (int(ent.shape[1]) != spec.dim_e or int(rel.shape[1]) != spec.dim_r
            or tuple(transfer_matrix.shape) != (int(rel.shape[0]), spec.dim_e * spec.dim_r)):
        raise ValueError("transr_ns.fused_ns_loss: ent (E, dim_e), rel (R, dim_r), transfer_matrix (R, dim_e * dim_r)")
    batch, neg = int(batch), int(neg)
    if not supported(spec.dim_e, spec.dim_r, neg):
        raise MMREError(f"transr_ns.fused_ns_loss: unsupported shape (code 3): dim_e {spec.dim_e}, dim_r {spec.dim_r} "
                        f"(1 .. 512 each), neg {neg} (1 .. 512)")
    h, t, r = (x.to(torch.int64).contiguous().reshape(-1) for x in (h, t, r))
    if any(int(x.shape[0]) != batch * (1 + neg) for x in (h, t, r)):
        raise ValueError("transr_ns.fused_ns_loss: h, t and r hold batch * (1 + neg) ids each")
    if not all(x.is_contiguous() for x in tables):
        raise ValueError("transr_ns.fused_ns_loss: contiguous tables")
    sgd = None
    if optimizer is not None and hasattr(optimizer, "fusable_lr") and not hasattr(optimizer, "fused_state"):
        lr = optimizer.fusable_lr(tables)
        if lr is not None:
            sgd = (optimizer, lr, tables)
    calls += 1
    return _FusedTransRNS.apply(ent, rel, transfer_matrix, h, t, r, spec, batch, neg, float(loss_margin),
                                float(adv_temperature or 0.0), float(regul_rate), sgd)
