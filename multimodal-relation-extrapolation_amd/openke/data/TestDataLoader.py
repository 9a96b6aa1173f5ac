"""TestDataLoader -- the openke.data contract (OpenKE Tester.py:70-82; absent from the reference
tree). Iterating in 'link' mode yields [data_head, data_tail] per test triple exactly like the
Base.so-backed loader (getHeadBatch/getTailBatch, Test.h:36-53), in testList order (sorted by
(r, h, t), Reader.h:227). In 'classification' mode it yields once [pos_ins, neg_ins], the whole
test list and one corrupted copy of every triple (getTestBatch, Test.h:411-422), the negatives
drawn on the GPU bit-exactly from work thread 0's state (mmre.tripleclass). The MI355X Tester
does not iterate: it hands the whole test list to the fused evaluations (mmre.link,
mmre.tripleclass)."""
import os

import numpy as np

from mmre.data import OpenKEDataset, TrainIndex
from mmre.link import FilterIndex


class TestDataLoader(object):
    def __init__(self, in_path="./", sampling_mode="link", type_constrain=True):
        self.in_path = in_path
        self.sampling_mode = sampling_mode
        self.type_constrain = type_constrain
        self.ds = OpenKEDataset(in_path)
        self.entTotal, self.relTotal = self.ds.n_ent, self.ds.n_rel
        self.test_h, self.test_r, self.test_t = self.ds.test_list()
        self.testTotal = len(self.test_h)
        self._index = None
        self._train_index = None
        self._seed_state = None

    def train_index(self):
        """The train index the negatives are filtered against (importTrainFiles, Reader.h:53-160)."""
        if self._train_index is None:
            tr = self.ds.train
            self._train_index = TrainIndex(tr[:, 0], tr[:, 1], tr[:, 2], self.entTotal, self.relTotal)
        return self._train_index

    def get_seed_state(self):
        """Work thread 0's LCG state before the next classification batch: by default the first
        value of the process's glibc rand() stream, which is what a fresh randReset gives."""
        if self._seed_state is None:
            from mmre.sampler import glibc_seeds
            self._seed_state = int(glibc_seeds(1)[0])
        return self._seed_state

    def set_seed_state(self, state):
        self._seed_state = int(state) & (2 ** 64 - 1)

    def filter_index(self):
        """train + valid + test known triples (Reader.h:201-226) and type constraints."""
        if self._index is None:
            h, r, t = self.ds.all_triples()
            th, tt = (self.ds.type_heads, self.ds.type_tails) if self.type_constrain else (None, None)
            self._index = FilterIndex(h, r, t, self.entTotal, self.relTotal, th, tt)
        return self._index

    def set_sampling_mode(self, sampling_mode):
        self.sampling_mode = sampling_mode

    def get_ent_tot(self):
        return self.entTotal

    def get_rel_tot(self):
        return self.relTotal

    def get_triple_tot(self):
        return self.testTotal

    def sampling_lp(self, i):
        E = self.entTotal
        h, r, t = int(self.test_h[i]), int(self.test_r[i]), int(self.test_t[i])
        head = {"batch_h": np.arange(E, dtype=np.int64), "batch_t": np.array([t], np.int64),
                "batch_r": np.array([r], np.int64), "mode": "head_batch"}
        tail = {"batch_h": np.array([h], np.int64), "batch_t": np.arange(E, dtype=np.int64),
                "batch_r": np.array([r], np.int64), "mode": "tail_batch"}
        return [head, tail]

    def sampling_tc(self):
        """[pos_ins, neg_ins] (getTestBatch): the test list and its negatives as int64 arrays. Each
        call advances thread 0's state by 2 x testTotal draws, so a second pass gives Base.so's
        second batch."""
        from mmre.tripleclass import advance_state, classification_negatives
        state = self.get_seed_state()
        nh, nt = classification_negatives(self.train_index(), self.test_h, self.test_r, self.test_t, state)
        self._seed_state = advance_state(state, self.testTotal)
        pos = {"batch_h": np.array(self.test_h, np.int64), "batch_t": np.array(self.test_t, np.int64),
               "batch_r": np.array(self.test_r, np.int64), "mode": "normal"}
        neg = {"batch_h": nh.cpu().numpy(), "batch_t": nt.cpu().numpy(), "batch_r": np.array(self.test_r, np.int64),
               "mode": "normal"}
        return [pos, neg]

    def __iter__(self):
        if self.sampling_mode == "link":
            for i in range(self.testTotal):
                yield self.sampling_lp(i)
        elif self.sampling_mode == "classification":
            yield self.sampling_tc()
        else:
            raise ValueError("unknown sampling mode %r (link, classification)" % (self.sampling_mode,))

    def __len__(self):
        return self.testTotal
