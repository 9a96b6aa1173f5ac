"""Tester (OpenKE/openke/config/Tester.py:17-91).

run_link_prediction replaces the per-query Python loop (getHeadBatch -> predict -> D2H ->
testHead, per test triple) with ONE fused evaluation on the GPU (mmre.link): every head- and
tail-batch sweep of the test set against every entity, filtered and type-constrained ranks
counted in the sweep's epilogue, then the Test.h metric reduction (test_link_prediction,
Test.h:232-327) with the reference's float order. Returns (mrr, mr, hit10, hit3, hit1) like
the reference. run_relation_prediction does the same for the reference's relation-prediction
loop (getRelBatch -> predict -> testRel, Test.h:55-62, :194-228, :329-354), and
run_triple_classification for getTestBatch -> predict on both batches -> get_best_threshlod
(Test.h:393-422, Tester.py:93-151): negatives, both score arrays and the sort-free threshold search
in one fused call (mmre.tripleclass)."""
import numpy as np
import torch

from mmre.link import evaluate_link_prediction, evaluate_relation_prediction
from mmre.tripleclass import best_threshold, evaluate_triple_classification


class Tester(object):
    def __init__(self, model=None, data_loader=None, use_gpu=True):
        self.model = model
        self.data_loader = data_loader
        self.use_gpu = use_gpu
        self.last = None
        if self.use_gpu and self.model is not None:
            self.model.cuda()

    def set_model(self, model):
        self.model = model

    def set_data_loader(self, data_loader):
        self.data_loader = data_loader

    def set_use_gpu(self, use_gpu):
        self.use_gpu = use_gpu
        if self.use_gpu and self.model is not None:
            self.model.cuda()

    def to_var(self, x, use_gpu):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        return t.cuda() if use_gpu else t

    def test_one_step(self, data):
        return self.model.predict({"batch_h": self.to_var(data["batch_h"], self.use_gpu),
                                   "batch_t": self.to_var(data["batch_t"], self.use_gpu),
                                   "batch_r": self.to_var(data["batch_r"], self.use_gpu),
                                   "mode": data["mode"]})

    def run_link_prediction(self, type_constrain=False):
        dl = self.data_loader
        dl.set_sampling_mode("link")
        metrics, counts = evaluate_link_prediction(self.model.score_spec(), dl.test_h, dl.test_r, dl.test_t,
                                                   index=dl.filter_index(), type_constrain=bool(type_constrain))
        self.last = {"metrics": metrics, "counts": counts}
        self._print(metrics, type_constrain)
        grp = metrics["filter_tc" if type_constrain else "filter"]
        print(grp["hit10"])
        return grp["mrr"], grp["mr"], grp["hit10"], grp["hit3"], grp["hit1"]

    @staticmethod
    def _print(m, tc):
        def line(name, g):
            return f"{name}\t {g['mrr']:f} \t {g['mr']:f} \t {g['hit10']:f} \t {g['hit3']:f} \t {g['hit1']:f} "
        print("no type constraint results:")
        print("metric:\t\t\t MRR \t\t MR \t\t hit@10 \t hit@3  \t hit@1 ")
        print(line("averaged(raw):\t\t", m["raw"]))
        print(line("averaged(filter):\t", m["filter"]))
        if tc:
            print("type constraint results:")
            print(line("averaged(raw):\t\t", m["raw_tc"]))
            print(line("averaged(filter):\t", m["filter_tc"]))

    def run_relation_prediction(self):
        """Which relation holds between h and t: the reference's loop getRelBatch -> predict ->
        testRel per test triple and test_relation_prediction (Test.h:55-62, :194-228, :329-354) as
        ONE fused evaluation (mmre.link.evaluate_relation_prediction). Prints the lines
        Test.h:346-353 prints; returns the filtered (mrr, mr, hit10, hit3, hit1)."""
        dl = self.data_loader
        metrics, counts = evaluate_relation_prediction(self.model.score_spec(), dl.test_h, dl.test_r, dl.test_t,
                                                       index=dl.filter_index())
        self.last = {"metrics": metrics, "counts": counts}
        print("no type constraint results:")
        print("metric:\t\t\t MRR \t\t MR \t\t hit@10 \t hit@3  \t hit@1 ")
        for name, g in (("averaged(raw):\t\t", metrics["raw"]), ("\naveraged(filter):\t", metrics["filter"])):
            print(f"{name} {g['mrr']:f} \t {g['mr']:f} \t {g['hit10']:f} \t {g['hit3']:f} \t {g['hit1']:f} ")
        grp = metrics["filter"]
        return grp["mrr"], grp["mr"], grp["hit10"], grp["hit3"], grp["hit1"]

    def get_best_threshlod(self, score, ans):
        """Tester.py:93-112 (the reference's spelling): the threshold of the best accuracy of the rule
        `score <= threshlod`, and that accuracy. score, ans: arrays of equal length, ans == 1 marking the
        positives. The search runs on the GPU (mmre_tc_threshold); with tied scores the accuracy is
        the one the rule attains (include/mmre.h). (None, 0.0), as the reference's walk from res_mx = 0.0
        gives, when no threshold classifies anything correctly."""
        score = np.asarray(score, np.float32).reshape(-1)
        ans = np.asarray(ans).reshape(-1)
        res = best_threshold(score[ans == 1], score[ans != 1])
        if res["threshold"] != res["threshold"] or not res["accuracy"] > 0.0:
            return None, 0.0
        return res["threshold"], res["accuracy"]

    def run_triple_classification(self, threshlod=None):
        """Tester.py:114-151 as ONE fused evaluation (mmre.tripleclass.evaluate_triple_classification):
        the loader's test list, its negatives from the loader's thread-0 state (which advances as a
        'classification' pass of the loader does), predict on both, and the best threshold -- or the
        accuracy at the given one. Returns (acc, threshlod); self.last keeps the negatives, both score
        arrays and the counts."""
        dl = self.data_loader
        dl.set_sampling_mode("classification")
        res = evaluate_triple_classification(self.model.score_spec(), dl.test_h, dl.test_r, dl.test_t,
                                             dl.train_index(), dl.get_seed_state(), threshold=threshlod)
        dl.set_seed_state(res["seed_state_after"])
        self.last = res
        return res["accuracy"], res["threshold"]
