"""TransR (OpenKE/openke/module/model/TransR.py:6-103): same constructor, identity / rand_init
initialisation, parameter names and state-dict keys (ent_embeddings, rel_embeddings,
transfer_matrix, margin).

forward(data) and regularization(data) are the reference's torch ops (differentiable);
predict(data) and the Tester's evaluations run on libmmre_hip.so (mmre.transr: the relation
projection on f32 MFMA, the fused sweep over its planes, and the row kernel). Training runs on
libmmre_hip.so as well: fused_ns_transr() hands the strategy the three tables and the static spec
of mmre.transr_ns.fused_ns_loss (the fused loss, grouped f32-MFMA GEMMs for the projection and its
two gradients, row-owner sums, the in-pass SGD step)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmre import transr as _transr
from mmre import transr_ns as _transr_ns
from mmre.link import ScoreSpec

from .Model import Model


class TransR(Model):
    def __init__(self, ent_tot, rel_tot, dim_e=100, dim_r=100, p_norm=1, norm_flag=True, rand_init=False, margin=None):
        super().__init__(ent_tot, rel_tot)
        if p_norm not in (1, 2):
            raise ValueError("TransR: p_norm must be 1 or 2")
        self.dim_e = dim_e
        self.dim_r = dim_r
        self.margin = margin
        self.norm_flag = norm_flag
        self.p_norm = p_norm
        self.rand_init = rand_init
        self.ent_embeddings = nn.Embedding(self.ent_tot, self.dim_e)
        self.rel_embeddings = nn.Embedding(self.rel_tot, self.dim_r)
        nn.init.xavier_uniform_(self.ent_embeddings.weight.data)
        nn.init.xavier_uniform_(self.rel_embeddings.weight.data)
        self.transfer_matrix = nn.Embedding(self.rel_tot, self.dim_e * self.dim_r)
        if not self.rand_init:
            identity = torch.zeros(self.dim_e, self.dim_r)
            for i in range(min(self.dim_e, self.dim_r)):
                identity[i][i] = 1
            self.transfer_matrix.weight.data[:] = identity.view(self.dim_r * self.dim_e)
        else:
            nn.init.xavier_uniform_(self.transfer_matrix.weight.data)
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
        """No instance of the generic mmre.ns kernels for TransR (a row carries a matrix): the
        strategy asks fused_ns_transr() instead."""
        return None

    def fused_ns_transr(self, neg):
        """(spec, ent, rel, transfer_matrix) for mmre.transr_ns.fused_ns_loss when the fused TransR
        training kernels serve this model with `neg` negatives per positive -- float32 contiguous
        device tables, 1 <= dim_e, dim_r <= 512, 1 <= neg <= 512 -- else None (the strategy then
        scores through forward() and autograd)."""
        tables = (self.ent_embeddings.weight, self.rel_embeddings.weight, self.transfer_matrix.weight)
        if any(not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() for x in tables):
            return None
        if neg < 1 or not _transr_ns.supported(self.dim_e, self.dim_r, neg):
            return None
        return (_transr_ns.TRSpec(self.p_norm, self.dim_e, self.dim_r, self.norm_flag, self._m()),) + tables

    def score_spec(self):
        # predict() = margin - forward = m - (m - s) when margin_flag, else s   (TransR.py:97-103)
        return ScoreSpec(model="transr" if self.p_norm == 1 else "transr_l2", ent=self.ent_embeddings.weight,
                         rel=self.rel_embeddings.weight, dim=self.dim_r, norm_flag=self.norm_flag,
                         pred_kind=1 if self.margin_flag else 0, margin=self._m() or 0.0, dim_e=self.dim_e,
                         transfer_matrix=self.transfer_matrix.weight)

    # ---- the reference's torch ops (TransR.py:40-95) ----
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

    def _transfer(self, e, r_transfer):
        r_transfer = r_transfer.view(-1, self.dim_e, self.dim_r)
        if e.shape[0] != r_transfer.shape[0]:
            e = e.view(-1, r_transfer.shape[0], self.dim_e).permute(1, 0, 2)
            e = torch.matmul(e, r_transfer).permute(1, 0, 2)
        else:
            e = e.view(-1, 1, self.dim_e)
            e = torch.matmul(e, r_transfer)
        return e.reshape(-1, self.dim_r)

    def _index(self, data):
        dev = self.ent_embeddings.weight.device
        return tuple(torch.as_tensor(data[k]).to(dev).long() for k in ("batch_h", "batch_t", "batch_r"))

    def forward(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        mode = data.get("mode", "normal")
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        r_transfer = self.transfer_matrix(batch_r)
        h = self._transfer(h, r_transfer)
        t = self._transfer(t, r_transfer)
        score = self._calc(h, t, r, mode)
        return self.margin - score if self.margin_flag else score

    def predict(self, data):
        h, t, r = self._expand(data)
        with torch.no_grad():
            score = _transr.score_rows(self.score_spec(), h, r, t, mode=data.get("mode", "normal"))
        return score.cpu().numpy()

    def regularization(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        r_transfer = self.transfer_matrix(batch_r)
        regul = (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2) + torch.mean(r_transfer ** 2)) / 4
        return regul * regul
