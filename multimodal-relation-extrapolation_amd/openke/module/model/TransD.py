"""TransD (OpenKE/openke/module/model/TransD.py:6-155): same constructor, init branches,
parameter names and state-dict keys.

forward(data) and regularization(data) are the reference's torch ops (differentiable);
predict(data) and the Tester's evaluations run on libmmre_hip.so (mmre.transd: TransH's fused sweep
behind TransD's prologue, and the row kernel). Training under NegativeSampling + MarginLoss runs on
libmmre_hip.so as well: fused_ns_transd() hands the strategy the four tables and the static spec
of mmre.transd_ns.fused_ns_loss (the fused loss, row-owner gradients, the in-pass SGD step).
ns_spec() stays None -- the generic mmre.ns kernels and the one-call sampler-fused step have no
TransD instance -- and every other loss or mode trains on autograd over forward()."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmre import transd as _transd
from mmre import transd_ns as _transd_ns
from mmre.link import ScoreSpec

from .Model import Model


class TransD(Model):
    def __init__(self, ent_tot, rel_tot, dim_e=100, dim_r=100, p_norm=1, norm_flag=True, margin=None, epsilon=None):
        super().__init__(ent_tot, rel_tot)
        if p_norm not in (1, 2):
            raise ValueError("TransD: p_norm must be 1 or 2")
        if dim_e < dim_r:
            raise ValueError(f"TransD: dim_e ({dim_e}) < dim_r ({dim_r}) is not served: an entity row is cut to "
                             "dim_r values, never padded (the reference itself fails there with a TypeError: "
                             "F.pad has no `paddings` argument, TransD.py:76)")
        self.dim_e = dim_e
        self.dim_r = dim_r
        self.margin = margin
        self.epsilon = epsilon
        self.norm_flag = norm_flag
        self.p_norm = p_norm
        self.ent_embeddings = nn.Embedding(self.ent_tot, self.dim_e)
        self.rel_embeddings = nn.Embedding(self.rel_tot, self.dim_r)
        self.ent_transfer = nn.Embedding(self.ent_tot, self.dim_e)
        self.rel_transfer = nn.Embedding(self.rel_tot, self.dim_r)
        tables = (self.ent_embeddings, self.rel_embeddings, self.ent_transfer, self.rel_transfer)
        if margin is None or epsilon is None:
            for emb in tables:
                nn.init.xavier_uniform_(emb.weight.data)
        else:
            self.ent_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_e]),
                                                    requires_grad=False)
            self.rel_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_r]),
                                                    requires_grad=False)
            for emb, rng in zip(tables, (self.ent_embedding_range, self.rel_embedding_range) * 2):
                nn.init.uniform_(emb.weight.data, -rng.item(), rng.item())
        if margin is not None:
            self.margin = nn.Parameter(torch.Tensor([margin]), requires_grad=False)
            self.margin_flag = True
        else:
            self.margin_flag = False

    def _m(self):
        return float(self.margin.item()) if self.margin_flag else None

    def _tables(self):
        return self.ent_embeddings.weight, self.rel_embeddings.weight, None, None

    def ns_spec(self):
        """No instance of the generic mmre.ns kernels for TransD (a triple has six rows): the
        strategy asks fused_ns_transd() instead."""
        return None

    def fused_ns_transd(self, neg):
        """(spec, ent, ent_transfer, rel, rel_transfer) for mmre.transd_ns.fused_ns_loss when the
        fused TransD training kernels serve this model with `neg` negatives per positive --
        float32 contiguous device tables, dim_r <= dim_e <= 512, 1 <= neg <= 512 -- else None (the
        strategy then scores through forward() and autograd)."""
        tables = (self.ent_embeddings.weight, self.ent_transfer.weight, self.rel_embeddings.weight,
                  self.rel_transfer.weight)
        if any(not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() for x in tables):
            return None
        if neg < 1 or not _transd_ns.supported(self.dim_e, self.dim_r, neg):
            return None
        return (_transd_ns.TDSpec(self.p_norm, self.dim_e, self.dim_r, self.norm_flag, self._m()),) + tables

    def score_spec(self):
        # predict() = margin - forward = m - (m - s) when margin_flag, else s   (TransD.py:149-155)
        return ScoreSpec(model="transd" if self.p_norm == 1 else "transd_l2", ent=self.ent_embeddings.weight,
                         rel=self.rel_embeddings.weight, dim=self.dim_r, norm_flag=self.norm_flag,
                         pred_kind=1 if self.margin_flag else 0, margin=self._m() or 0.0,
                         ent_transfer=self.ent_transfer.weight, rel_transfer=self.rel_transfer.weight,
                         dim_e=self.dim_e)

    # ---- the reference's torch ops (TransD.py:62-129) ----
    def _resize(self, tensor, axis, size):
        osize = tensor.size()[axis]
        if osize == size:
            return tensor
        if osize > size:
            return torch.narrow(tensor, axis, 0, size)
        raise ValueError("TransD: dim_e < dim_r")  # (the constructor refuses it)

    def _calc(self, h, t, r, mode):
        if self.norm_flag:
            h = F.normalize(h, 2, -1)
            r = F.normalize(r, 2, -1)
            t = F.normalize(t, 2, -1)
        if mode != "normal":
            h = h.view(-1, r.shape[0], h.shape[-1])
            t = t.view(-1, r.shape[0], t.shape[-1])
            r = r.view(-1, r.shape[0], r.shape[-1])
        if mode == "head_batch":
            score = h + (r - t)
        else:
            score = (h + r) - t
        return torch.norm(score, self.p_norm, -1).flatten()

    def _transfer(self, e, e_transfer, r_transfer):
        if e.shape[0] != r_transfer.shape[0]:
            e = e.view(-1, r_transfer.shape[0], e.shape[-1])
            e_transfer = e_transfer.view(-1, r_transfer.shape[0], e_transfer.shape[-1])
            r_transfer = r_transfer.view(-1, r_transfer.shape[0], r_transfer.shape[-1])
            e = F.normalize(self._resize(e, -1, r_transfer.size()[-1]) + torch.sum(e * e_transfer, -1, True) * r_transfer,
                            p=2, dim=-1)
            return e.view(-1, e.shape[-1])
        return F.normalize(self._resize(e, -1, r_transfer.size()[-1]) + torch.sum(e * e_transfer, -1, True) * r_transfer,
                           p=2, dim=-1)

    def _index(self, data):
        dev = self.ent_embeddings.weight.device
        return tuple(torch.as_tensor(data[k]).to(dev).long() for k in ("batch_h", "batch_t", "batch_r"))

    def forward(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        mode = data.get("mode", "normal")
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        h_transfer = self.ent_transfer(batch_h)
        t_transfer = self.ent_transfer(batch_t)
        r_transfer = self.rel_transfer(batch_r)
        h = self._transfer(h, h_transfer, r_transfer)
        t = self._transfer(t, t_transfer, r_transfer)
        score = self._calc(h, t, r, mode)
        return self.margin - score if self.margin_flag else score

    def predict(self, data):
        h, t, r = self._expand(data)
        with torch.no_grad():
            score = _transd.score_rows(self.score_spec(), h, r, t, mode=data.get("mode", "normal"))
        return score.cpu().numpy()

    def regularization(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        h_transfer = self.ent_transfer(batch_h)
        t_transfer = self.ent_transfer(batch_t)
        r_transfer = self.rel_transfer(batch_r)
        return (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2) + torch.mean(h_transfer ** 2) +
                torch.mean(t_transfer ** 2) + torch.mean(r_transfer ** 2)) / 6
