"""TransH (OpenKE/openke/module/model/TransH.py:6-115): same constructor, init branches,
parameter names and state-dict keys.

forward(data) is the reference's torch ops (differentiable); predict(data) and the Tester's
evaluations run on libmmre_hip.so (mmre.transh: the fused hyperplane-projected sweep and its row
kernel). Training under NegativeSampling + MarginLoss runs on libmmre_hip.so as well: fused_ns()
hands the strategy the three tables and the static spec of mmre.transh_ns.fused_ns_loss (the
fused loss, row-owner gradients, the in-pass SGD step). ns_spec() stays None -- the generic
mmre.ns kernels and the one-call sampler-fused step have no TransH instance."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mmre import transh as _transh
from mmre import transh_ns as _transh_ns
from mmre.link import ScoreSpec

from .Model import Model


class TransH(Model):
    def __init__(self, ent_tot, rel_tot, dim=100, p_norm=1, norm_flag=True, margin=None, epsilon=None):
        super().__init__(ent_tot, rel_tot)
        if p_norm not in (1, 2):
            raise ValueError("TransH: p_norm must be 1 or 2")
        self.dim = dim
        self.margin = margin
        self.epsilon = epsilon
        self.norm_flag = norm_flag
        self.p_norm = p_norm
        self.ent_embeddings = nn.Embedding(self.ent_tot, self.dim)
        self.rel_embeddings = nn.Embedding(self.rel_tot, self.dim)
        self.norm_vector = nn.Embedding(self.rel_tot, self.dim)
        if margin is None or epsilon is None:
            nn.init.xavier_uniform_(self.ent_embeddings.weight.data)
            nn.init.xavier_uniform_(self.rel_embeddings.weight.data)
            nn.init.xavier_uniform_(self.norm_vector.weight.data)
        else:
            self.embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim]),
                                                requires_grad=False)
            for emb in (self.ent_embeddings, self.rel_embeddings, self.norm_vector):
                nn.init.uniform_(emb.weight.data, -self.embedding_range.item(), self.embedding_range.item())
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
        """No instance of the generic mmre.ns kernels for TransH (a triple has a fourth row, the
        normal): the strategy asks fused_ns() instead."""
        return None

    def fused_ns(self, neg):
        """(spec, ent, rel, norm_vector) for mmre.transh_ns.fused_ns_loss when the fused TransH
        training kernels serve this model with `neg` negatives per positive -- float32 device
        tables, dim <= 512, 1 <= neg <= 512 -- else None (the strategy then scores through
        forward() and autograd)."""
        tables = (self.ent_embeddings.weight, self.rel_embeddings.weight, self.norm_vector.weight)
        if any(not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() for x in tables):
            return None
        if neg < 1 or not _transh_ns.supported(self.dim, neg):
            return None
        return (_transh_ns.THSpec(self.p_norm, self.dim, self.norm_flag, self._m()),) + tables

    def score_spec(self):
        # predict() = margin - forward = m - (m - s) when margin_flag, else s   (TransH.py:109-115)
        return ScoreSpec(model="transh" if self.p_norm == 1 else "transh_l2", ent=self.ent_embeddings.weight,
                         rel=self.rel_embeddings.weight, dim=self.dim, norm_flag=self.norm_flag,
                         pred_kind=1 if self.margin_flag else 0, margin=self._m() or 0.0,
                         norm_vec=self.norm_vector.weight)

    # ---- the reference's torch ops (TransH.py:52-93) ----
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

    def _transfer(self, e, norm):
        norm = F.normalize(norm, p=2, dim=-1)
        if e.shape[0] != norm.shape[0]:
            e = e.view(-1, norm.shape[0], e.shape[-1])
            norm = norm.view(-1, norm.shape[0], norm.shape[-1])
            e = e - torch.sum(e * norm, -1, True) * norm
            return e.view(-1, e.shape[-1])
        return e - torch.sum(e * norm, -1, True) * norm

    def _index(self, data):
        dev = self.ent_embeddings.weight.device
        return tuple(torch.as_tensor(data[k]).to(dev).long() for k in ("batch_h", "batch_t", "batch_r"))

    def forward(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        mode = data.get("mode", "normal")
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        r_norm = self.norm_vector(batch_r)
        h = self._transfer(h, r_norm)
        t = self._transfer(t, r_norm)
        score = self._calc(h, t, r, mode)
        return self.margin - score if self.margin_flag else score

    def predict(self, data):
        h, t, r = self._expand(data)
        with torch.no_grad():
            score = _transh.score_rows(self.score_spec(), h, r, t, mode=data.get("mode", "normal"))
        return score.cpu().numpy()

    def regularization(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_embeddings(batch_r)
        r_norm = self.norm_vector(batch_r)
        return (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2) + torch.mean(r_norm ** 2)) / 4
