"""The reference's DistMult / ComplEx recipes (OpenKE examples/train_distmult_WN18RR.py,
train_complex_WN18RR.py: SoftplusLoss, regul_rate 1.0, Adagrad) and RotatE + SigmoidLoss(adv) +
SGD in normal mode through Trainer.run() on the small dataset: the one-call step is taken and
equals the per-batch path bit for bit; TransE + SoftplusLoss + Adagrad trains on the fused rows
path without the loss module's torch ops."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "small") + "/"


@pytest.mark.parametrize("recipe", ["distmult", "complex", "rotate"])
def test_reference_recipes_take_the_one_call_step(recipe):
    from mmre.optim import Adagrad
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SigmoidLoss, SoftplusLoss
    from openke.module.model import ComplEx, DistMult, RotatE
    from openke.module.strategy import NegativeSampling
    before = Adagrad.fallback_steps
    runs = []
    for one_call in (True, False):
        torch.manual_seed(0)
        tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1,
                              filter_flag=1, neg_ent=25, neg_rel=0)
        E, R = tdl.get_ent_tot(), tdl.get_rel_tot()
        if recipe == "rotate":
            kg = RotatE(ent_tot=E, rel_tot=R, dim=32, margin=6.0, epsilon=2.0)
            model = NegativeSampling(model=kg, loss=SigmoidLoss(adv_temperature=2), batch_size=tdl.get_batch_size(),
                                     regul_rate=0.0)
            trainer = Trainer(model=model, data_loader=tdl, train_times=3, alpha=0.5, use_gpu=True, opt_method="sgd")
        else:
            kg = (DistMult if recipe == "distmult" else ComplEx)(ent_tot=E, rel_tot=R, dim=32)
            model = NegativeSampling(model=kg, loss=SoftplusLoss(), batch_size=tdl.get_batch_size(), regul_rate=1.0)
            trainer = Trainer(model=model, data_loader=tdl, train_times=3, alpha=0.5, use_gpu=True,
                              opt_method="adagrad")
        trainer.one_call_step = one_call
        trainer.run()
        assert trainer.used_one_call_step is one_call
        tables = [t for t in kg._tables() if t is not None]
        sums = []
        if recipe != "rotate":
            assert isinstance(trainer.optimizer, Adagrad)
            sums = [trainer.optimizer.state[t]["sum"].clone() for t in tables]
            assert all(float(trainer.optimizer.state[t]["step"]) == 30.0 for t in tables)
            assert all(bool((s > 0).any()) for s in sums)
        runs.append((list(trainer.log), [t.detach().clone() for t in tables], sums, tdl.sampler.seeds.copy()))
    (la, ta, ua, sa), (lb, tb, ub, sb) = runs
    assert la == lb
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert all(torch.equal(x, y) for x, y in zip(ua, ub))
    assert np.array_equal(sa, sb)
    assert all(np.isfinite(la))
    assert Adagrad.fallback_steps == before


def test_transe_softplus_adagrad_trains_on_the_rows_path(monkeypatch):
    from mmre.optim import Adagrad
    from openke.config import Trainer
    from openke.data import TrainDataLoader
    from openke.module.loss import SoftplusLoss
    from openke.module.model import TransE
    from openke.module.strategy import NegativeSampling

    def no_torch_loss(self, p_score, n_score):
        raise AssertionError("SoftplusLoss.forward ran: the loss module's torch ops are on the path")

    monkeypatch.setattr(SoftplusLoss, "forward", no_torch_loss)
    before = Adagrad.fallback_steps
    torch.manual_seed(0)
    tdl = TrainDataLoader(in_path=SMALL, nbatches=10, threads=8, sampling_mode="normal", bern_flag=1, filter_flag=1,
                          neg_ent=25, neg_rel=0)
    transe = TransE(ent_tot=tdl.get_ent_tot(), rel_tot=tdl.get_rel_tot(), dim=32, p_norm=1, norm_flag=True)
    model = NegativeSampling(model=transe, loss=SoftplusLoss(), batch_size=tdl.get_batch_size(), regul_rate=0.0)
    trainer = Trainer(model=model, data_loader=tdl, train_times=30, alpha=0.1, use_gpu=True, opt_method="adagrad")
    trainer.run()
    assert trainer.used_one_call_step is False
    assert isinstance(trainer.optimizer, Adagrad) and Adagrad.fallback_steps == before
    assert np.isfinite(trainer.log).all() and trainer.log[-1] < trainer.log[0]
