"""RESCAL (OpenKE/openke/module/model/RESCAL.py:5-46): same constructor, initialisation order,
parameter names and state-dict keys (ent_embeddings, rel_matrices).

forward(data) and regularization(data) are the reference's torch ops (differentiable): training
runs on autograd over forward() -- ns_spec() is None and there is no fused hook, so
NegativeSampling takes the generic branch. predict(data) and the Tester's evaluations run on
libmmre_hip.so (mmre.rescal: the relation planes on f32 MFMA, the sweep with a per-tile entity
operand, and the row kernel).

predict returns -forward = +sum_i h_i (M_r t)_i, and the Tester ranks ascending on it: the
reference's behaviour (RESCAL.py:44-46), reproduced as it is."""
import torch
import torch.nn as nn

from mmre import rescal as _rescal
from mmre.link import ScoreSpec

from .Model import Model


class RESCAL(Model):
    def __init__(self, ent_tot, rel_tot, dim=100):
        super().__init__(ent_tot, rel_tot)
        self.dim = dim
        self.ent_embeddings = nn.Embedding(self.ent_tot, self.dim)
        self.rel_matrices = nn.Embedding(self.rel_tot, self.dim * self.dim)
        nn.init.xavier_uniform_(self.ent_embeddings.weight.data)
        nn.init.xavier_uniform_(self.rel_matrices.weight.data)

    def _tables(self):
        return self.ent_embeddings.weight, self.rel_matrices.weight, None, None

    def ns_spec(self):
        """No fused training step for RESCAL yet (a row carries a matrix): the strategy scores
        through forward() and autograd."""
        return None

    def score_spec(self):
        # predict() = -forward = -(-s) = s, bit for bit   (RESCAL.py:22, :44-46)
        return ScoreSpec(model="rescal", ent=self.ent_embeddings.weight, rel=None, dim=self.dim, pred_kind=0,
                         rel_matrices=self.rel_matrices.weight)

    # ---- the reference's torch ops (RESCAL.py:17-42) ----
    def _calc(self, h, t, r):
        t = t.view(-1, self.dim, 1)
        r = r.view(-1, self.dim, self.dim)
        tr = torch.matmul(r, t)
        tr = tr.view(-1, self.dim)
        return -torch.sum(h * tr, -1)

    def _index(self, data):
        dev = self.ent_embeddings.weight.device
        return tuple(torch.as_tensor(data[k]).to(dev).long() for k in ("batch_h", "batch_t", "batch_r"))

    def forward(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_matrices(batch_r)
        return self._calc(h, t, r)

    def predict(self, data):
        h, t, r = self._expand(data)
        with torch.no_grad():
            score = _rescal.score_rows(self.score_spec(), h, r, t, mode=data.get("mode", "normal"))
        return score.cpu().numpy()

    def regularization(self, data):
        batch_h, batch_t, batch_r = self._index(data)
        h = self.ent_embeddings(batch_h)
        t = self.ent_embeddings(batch_t)
        r = self.rel_matrices(batch_r)
        return (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2)) / 3
