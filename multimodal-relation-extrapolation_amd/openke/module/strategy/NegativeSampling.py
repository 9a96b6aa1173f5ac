"""NegativeSampling strategy (OpenKE/openke/module/strategy/NegativeSampling.py:3-32).

With a MarginLoss, SoftplusLoss or SigmoidLoss and 'normal'-mode batches the forward is ONE
fused HIP launch sequence (mmre.ns.fused_ns_loss): row scores -> positive/negative split ->
(self-adversarial) hinge / softplus / log-sigmoid -> mean -> + regul_rate * regularization, with
a fused backward into the embedding tables. Other losses / cross-sampling modes score through
model(data) (HIP) and apply the loss module on the score tensors. `fuse_optimizer(opt)` (the
Trainer calls it for its mmre.optim.SGD or Adagrad) lets that backward also apply the
optimizer's plain step to the tables in the same pass (bit-identical parameters; step() then
skips them). TransH has its own kernels (mmre.transh_ns.fused_ns_loss, through the model's
fused_ns() hook): MarginLoss in 'normal' mode on float32 device tables at a supported shape;
everything else about a TransH model takes the generic branch. TransD likewise
(mmre.transd_ns.fused_ns_loss, through the model's fused_ns_transd() hook), and TransR
(mmre.transr_ns.fused_ns_loss, through fused_ns_transr())."""
import torch

from mmre.ns import fused_ns_loss
from mmre.transd_ns import fused_ns_loss as transd_fused_ns_loss
from mmre.transh_ns import fused_ns_loss as transh_fused_ns_loss
from mmre.transr_ns import fused_ns_loss as transr_fused_ns_loss

from ..loss.MarginLoss import MarginLoss
from ..loss.SigmoidLoss import SigmoidLoss
from ..loss.SoftplusLoss import SoftplusLoss
from .Strategy import Strategy


class NegativeSampling(Strategy):
    def __init__(self, model=None, loss=None, batch_size=256, regul_rate=0.0, l3_regul_rate=0.0):
        super().__init__()
        self.model = model
        self.loss = loss
        self.batch_size = batch_size
        self.regul_rate = regul_rate
        self.l3_regul_rate = l3_regul_rate
        self.fused_optimizer = None

    def fuse_optimizer(self, optimizer):
        self.fused_optimizer = optimizer

    def _get_positive_score(self, score):
        return score[:self.batch_size].view(-1, self.batch_size).permute(1, 0)

    def _get_negative_score(self, score):
        return score[self.batch_size:].view(-1, self.batch_size).permute(1, 0)

    def _transh_fused(self, data, mode):
        """((spec, ent, rel, norm_vector), neg) when this batch takes the fused TransH path: a
        MarginLoss, 'normal' mode, a model with the fused_ns hook that offers the shape; else None."""
        return self._offer("fused_ns", data, mode)

    def _transd_fused(self, data, mode):
        """((spec, ent, ent_transfer, rel, rel_transfer), neg) when this batch takes the fused
        TransD path: TransH's conditions with the model's fused_ns_transd hook; else None."""
        return self._offer("fused_ns_transd", data, mode)

    def _transr_fused(self, data, mode):
        """((spec, ent, rel, transfer_matrix), neg) when this batch takes the fused TransR path:
        TransH's conditions with the model's fused_ns_transr hook; else None."""
        return self._offer("fused_ns_transr", data, mode)

    def _offer(self, hook_name, data, mode):
        hook = getattr(self.model, hook_name, None)
        if hook is None or not isinstance(self.loss, MarginLoss) or mode != "normal":
            return None
        n = int(data["batch_h"].shape[0])
        if n % self.batch_size:
            return None
        neg = n // self.batch_size - 1
        offer = hook(neg)
        return None if offer is None else (offer, neg)

    def forward(self, data):
        mode = data.get("mode", "normal")
        # (a model without a fused step -- ns_spec() None: TransH -- scores through model(data))
        fused = isinstance(self.loss, (MarginLoss, SoftplusLoss, SigmoidLoss)) and mode == "normal"
        spec = self.model.ns_spec() if fused else None
        th = self._transh_fused(data, mode) if spec is None else None
        td = self._transd_fused(data, mode) if spec is None and th is None else None
        tr = self._transr_fused(data, mode) if spec is None and th is None and td is None else None
        if spec is not None:
            ent, rel, ent_im, rel_im = self.model._tables()
            dev = ent.device
            h = data["batch_h"].to(dev)
            t = data["batch_t"].to(dev)
            r = data["batch_r"].to(dev)
            n = int(h.shape[0])
            neg = n // self.batch_size - 1
            margin, adv = self.loss.fused_args()
            kind = "margin"
            if not isinstance(self.loss, MarginLoss):  # (kind, adv): these losses have no margin
                kind, margin = margin, 0.0
            loss_res, _ = fused_ns_loss(spec, ent, rel, h, t, r, self.batch_size, neg, margin,
                                        adv, self.regul_rate, ent_im=ent_im, rel_im=rel_im,
                                        optimizer=self.fused_optimizer if self.l3_regul_rate == 0 else None,
                                        loss=kind)
        elif th is not None:
            (spec, ent, rel, nv), neg = th
            h, t, r = (torch.as_tensor(data[k]).to(ent.device) for k in ("batch_h", "batch_t", "batch_r"))
            margin, adv = self.loss.fused_args()
            loss_res, _ = transh_fused_ns_loss(spec, ent, rel, nv, h, t, r, self.batch_size, neg, margin, adv,
                                               self.regul_rate,
                                               optimizer=self.fused_optimizer if self.l3_regul_rate == 0 else None)
        elif td is not None:
            (spec, *tables), neg = td
            h, t, r = (torch.as_tensor(data[k]).to(tables[0].device) for k in ("batch_h", "batch_t", "batch_r"))
            margin, adv = self.loss.fused_args()
            loss_res, _ = transd_fused_ns_loss(spec, *tables, h, t, r, self.batch_size, neg, margin, adv,
                                               self.regul_rate,
                                               optimizer=self.fused_optimizer if self.l3_regul_rate == 0 else None)
        elif tr is not None:
            (spec, *tables), neg = tr
            h, t, r = (torch.as_tensor(data[k]).to(tables[0].device) for k in ("batch_h", "batch_t", "batch_r"))
            margin, adv = self.loss.fused_args()
            loss_res, _ = transr_fused_ns_loss(spec, *tables, h, t, r, self.batch_size, neg, margin, adv,
                                               self.regul_rate,
                                               optimizer=self.fused_optimizer if self.l3_regul_rate == 0 else None)
        else:
            score = self.model(data)
            loss_res = self.loss(self._get_positive_score(score), self._get_negative_score(score))
            if self.regul_rate != 0:
                loss_res = loss_res + self.regul_rate * self.model.regularization(data)
        if self.l3_regul_rate != 0:
            loss_res = loss_res + self.l3_regul_rate * self.model.l3_regularization()
        return loss_res
