"""Fused TransD negative-sampling loss (csrc/transh_train.hip, the TransD part) as a
torch.autograd.Function: mmre.transh_ns.fused_ns_loss for a model with two rows per entity and two
per relation.

forward  = TransD.forward in 'normal' mode for the B (1 + K) rows of [pos | neg_1 | ... | neg_K]
           -> MarginLoss (optionally self-adversarial) + regul_rate * TransD.regularization
           (OpenKE TransD.py:94-147, NegativeSampling.py:23-32, MarginLoss.py:24-28): one launch
           and a fixed-order reduction (mmre_transd_ns_forward).
backward = d(loss)/d(ent, ent_transfer, rel, rel_transfer) into dense gradient tables, every row
           written, no float atomics, bit-reproducible (mmre_transd_ns_grad). With `optimizer` (an
           mmre.optim.SGD doing plain SGD on the four tables) the same pass applies its step,
           p <- fma(-lr, g, p), and optimizer.step() then skips the tables.
"""
from __future__ import annotations

import torch

from ._lib import MMREError, call, lib, mark_written, ptr, require_cuda, stream_ptr
from .transd import MODEL_IDS

# calls of fused_ns_loss since import: which path a strategy took (tests, scripts/bench_transd_train.py)
calls = 0


class TDSpec:
    """Static description of TransD.forward: p_norm, dim_e, dim_r, norm_flag and the model's margin."""

    def __init__(self, p_norm: int, dim_e: int, dim_r: int, norm_flag: bool = True, model_margin: float | None = None):
        if p_norm not in (1, 2):
            raise ValueError("TDSpec: p_norm must be 1 or 2")
        self.model = "transd" if p_norm == 1 else "transd_l2"
        self.model_id = MODEL_IDS[self.model]
        self.dim_e, self.dim_r = int(dim_e), int(dim_r)
        self.norm_flag = bool(norm_flag)
        self.use_model_margin = model_margin is not None
        self.model_margin = float(model_margin or 0.0)


def supported(dim_e: int, dim_r: int, neg: int) -> bool:
    """Whether the kernels exist for the shape: 1 <= dim_r <= dim_e <= 512 and 1 <= neg <= 512
    (mmre_transd_ns_supported, the library's own rule)."""
    fn = getattr(lib(), "mmre_transd_ns_supported", None)
    if fn is None:
        raise MMREError("libmmre_hip.so does not export mmre_transd_ns_supported: rebuild it")
    return bool(fn(MODEL_IDS["transd"], int(dim_e), int(dim_r), int(neg)))


def _head(spec, ent, ept, rel, rpt, h, t, r, batch, neg, loss_margin, adv_t, regul_rate):
    return (spec.model_id, int(spec.norm_flag), spec.model_margin, int(spec.use_model_margin), ptr(ent), ptr(ept),
            ptr(rel), ptr(rpt), int(ent.shape[0]), int(rel.shape[0]), spec.dim_e, spec.dim_r, ptr(h), ptr(t), ptr(r),
            batch, neg, float(loss_margin), float(adv_t), float(regul_rate))


class _FusedTransDNS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ent, ept, rel, rpt, h, t, r, spec, batch, neg, loss_margin, adv_t, regul_rate, sgd):
        dev = ent.device
        n = batch * (1 + neg)
        score = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(score)
        ctx.set_materialize_grads(False)
        need = int(lib().mmre_transd_ns_workspace(batch, neg, int(ent.shape[0]), int(rel.shape[0]), spec.dim_e,
                                                  spec.dim_r))
        work = torch.empty(need, dtype=torch.float32, device=dev)
        head = _head(spec, ent, ept, rel, rpt, h, t, r, batch, neg, loss_margin, adv_t, regul_rate)
        call("mmre_transd_ns_forward", *head, ptr(score), ptr(loss), ptr(work), stream_ptr(dev))
        ctx.cfg = (spec, batch, neg, loss_margin, adv_t, regul_rate)
        ctx.work, ctx.sgd = work, sgd
        ctx.save_for_backward(ent, ept, rel, rpt, h, t, r, score)
        return loss[0], score

    @staticmethod
    def backward(ctx, g_loss, g_score):
        if g_loss is None:
            return (None,) * 14
        ent, ept, rel, rpt, h, t, r, score = ctx.saved_tensors
        spec, batch, neg, loss_margin, adv_t, regul_rate = ctx.cfg
        dev = ent.device
        gl = g_loss.reshape(1).to(torch.float32).contiguous()
        grads = tuple(torch.empty_like(x) for x in (ent, ept, rel, rpt))  # every row written: no fills
        lr, sgd = 0.0, ctx.sgd
        if sgd is not None:
            lr = float(sgd[1])
        head = _head(spec, ent, ept, rel, rpt, h, t, r, batch, neg, loss_margin, adv_t, regul_rate)
        call("mmre_transd_ns_grad", *head, ptr(score), ptr(gl), *(ptr(g) for g in grads), ptr(ctx.work), lr,
             stream_ptr(dev))
        if sgd is not None and lr != 0.0:  # the optimizer's plain step rode in the owner pass: step() skips these
            opt, _, tables = sgd
            mark_written(*tables)
            opt._fused_applied(tables)
        ctx.work = ctx.sgd = None
        return grads + (None,) * 10


def fused_ns_loss(spec: TDSpec, ent, ent_transfer, rel, rel_transfer, h, t, r, batch: int, neg: int,
                  loss_margin: float, adv_temperature: float | None = None, regul_rate: float = 0.0, optimizer=None):
    """Returns (loss scalar tensor, scores (B (1 + K),)); differentiable w.r.t. the four tables
    (float32 device tensors). h / t / r: the batch's ids, laid out [pos | neg_1 | ... ].
    optimizer: taken only when it is an mmre.optim.SGD whose fusable_lr(the four tables) is not
    None (plain SGD, the tables in one group, no gradient on them yet): the backward then applies
    its step as well and optimizer.step() skips the tables -- parameters bit-identical to
    backward() + step(), p.grad still written. Any other optimizer (Adagrad, momentum, ...) is
    ignored here and step() does the update. A shape without kernels (supported()) raises
    MMREError before anything is launched."""
    global calls
    require_cuda(ent, ent_transfer, rel, rel_transfer, h, t, r)
    tables = [ent, ent_transfer, rel, rel_transfer]
    if any(x.dtype != torch.float32 for x in tables):
        raise TypeError("transd_ns.fused_ns_loss: float32 tables")
    if (tuple(ent.shape) != tuple(ent_transfer.shape) or tuple(rel.shape) != tuple(rel_transfer.shape)
            or int(ent.shape[1]) != spec.dim_e or int(rel.shape[1]) != spec.dim_r):
        raise ValueError("transd_ns.fused_ns_loss: ent and ent_transfer (E, dim_e), rel and rel_transfer (R, dim_r)")
    batch, neg = int(batch), int(neg)
    if not supported(spec.dim_e, spec.dim_r, neg):
        raise MMREError(f"transd_ns.fused_ns_loss: unsupported shape (code 3): dim_e {spec.dim_e}, dim_r {spec.dim_r} "
                        f"(1 <= dim_r <= dim_e <= 512), neg {neg} (1 .. 512)")
    h, t, r = (x.to(torch.int64).contiguous().reshape(-1) for x in (h, t, r))
    if any(int(x.shape[0]) != batch * (1 + neg) for x in (h, t, r)):
        raise ValueError("transd_ns.fused_ns_loss: h, t and r hold batch * (1 + neg) ids each")
    if not all(x.is_contiguous() for x in tables):
        raise ValueError("transd_ns.fused_ns_loss: contiguous tables")
    sgd = None
    if optimizer is not None and hasattr(optimizer, "fusable_lr") and not hasattr(optimizer, "fused_state"):
        lr = optimizer.fusable_lr(tables)
        if lr is not None:
            sgd = (optimizer, lr, tables)
    calls += 1
    return _FusedTransDNS.apply(ent, ent_transfer, rel, rel_transfer, h, t, r, spec, batch, neg, float(loss_margin),
                                float(adv_temperature or 0.0), float(regul_rate), sgd)
