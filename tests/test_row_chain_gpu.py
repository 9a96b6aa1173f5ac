"""The row-wise score chain (csrc/row_chain.h) across its users, at the dims where the kernels
change instance (NC 1 / 2 / 4 / 8: d = 64, 128, 256 and their neighbours, 1 and 512).

One batch of B positives with K negatives each, in the training layout (positive b at row b, its
negative j at row b + (j + 1) B): head, tail and relation corrupted, and one negative that shares
no row with its positive; one positive's first negative is a copy of it. That is every case of the
generic training forward (neg_code 0, 1, 2, 4 and 3), more than one workgroup of four waves and a
ragged last one. The reference is mmre.ns.score_rows on all N rows, computed once per case; every
leg is compared with it bit for bit on every row:

  - the scores fused_ns_loss returns under the margin loss, with gradients wanted (the fused
    training forward) and without (the rows forward);
  - relation_sweep(return_scores=True) at each row's own relation, after predict's transform;
  - classification_scores on the positives paired with each column of negatives, likewise.

Left out: the TransE configurations of the fused training forward (gradients wanted, dim <= 512,
neg <= 32). Its kernel, the fused TransE step, reduces a row in an order of its own
and agrees with score_rows to the last bits only: before the chain was shared it differed from
score_rows in 24 of these 27 cases (every d >= 63), and it still does. tests/test_ns_shapes_gpu.py
holds it to its own reference."""
import numpy as np
import pytest
import torch

from test_relpred_gpu import CONFIGS, E, _random_tables, _same_bits, _specs, _to

pytestmark = pytest.mark.gpu

DIMS = (1, 63, 64, 65, 128, 129, 256, 257, 512)
R, B, K = 13, 5, 4


def _batch(rng):
    """(h, t, r) of the N = B (1 + K) rows."""
    ph, pt, pr = rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, R, B)
    other = lambda x, n: (x + rng.integers(1, n, B)) % n  # a different id, row by row
    negs = ((other(ph, E), pt, pr), (ph, other(pt, E), pr), (ph, pt, other(pr, R)),
            (other(ph, E), other(pt, E), other(pr, R)))
    h, t, r = (np.concatenate([p] + [n[i] for n in negs]).astype(np.int64) for i, p in enumerate((ph, pt, pr)))
    h[B] = ph[0]  # positive 0's first negative: the positive itself
    return h, t, r


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("config", CONFIGS)
def test_every_user_of_the_chain_equals_score_rows(config, d):
    from mmre.link import relation_sweep
    from mmre.ns import fused_ns_loss, score_rows
    from mmre.tripleclass import classification_scores
    sp, ns, tr = _specs(config, *_random_tables(config, R, d, seed=7000 + d))
    h, t, r = _batch(np.random.default_rng(d))
    dh, dt, dr = _to(h), _to(t), _to(r)
    im = dict(ent_im=sp.ent_im, rel_im=sp.rel_im)
    with torch.no_grad():
        fwd = score_rows(ns, sp.ent, sp.rel, dh, dt, dr, **im)
        rows = fused_ns_loss(ns, sp.ent, sp.rel, dh, dt, dr, B, K, 1.0, **im)[1].cpu().numpy()
    pred = tr(fwd).cpu().numpy()
    fwd = fwd.cpu().numpy()
    assert _same_bits(rows, fwd), "fused_ns_loss, rows forward"
    sweep = relation_sweep(sp, dh, dr, dt, return_scores=True)["scores"].cpu().numpy()
    assert _same_bits(sweep[np.arange(len(r)), r], pred), "relation_sweep"
    for j in range(1, K + 1):
        n = slice(j * B, (j + 1) * B)
        pos, neg = classification_scores(sp, h[:B], r[:B], t[:B], h[n], t[n], neg_r=r[n])
        assert _same_bits(pos.cpu().numpy(), pred[:B]), "classification_scores, positives"
        assert _same_bits(neg.cpu().numpy(), pred[n]), "classification_scores, negatives %d" % j
    if config.startswith("transe"):  # the fused TransE step: see the docstring
        return
    g = lambda x: None if x is None else x.clone().requires_grad_(True)
    fused = fused_ns_loss(ns, g(sp.ent), g(sp.rel), dh, dt, dr, B, K, 1.0, ent_im=g(sp.ent_im),
                          rel_im=g(sp.rel_im))[1].cpu().numpy()
    assert _same_bits(fused, fwd), "fused_ns_loss, fused forward"
