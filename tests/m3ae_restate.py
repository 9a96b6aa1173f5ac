"""numpy restatement of the M3AE encoder's plan (mmre_m3ae_plan, include/mmre.h), shared by
test_m3ae_cpu.py and test_m3ae_edges_gpu.py (not a test module).

Per input row b of tokens (n_seq, L) / mask (n_seq, L): a position is unpadded unless
mask > 0 (so -1, -0.0 and NaN are unpadded; any positive value, a denormal included, is padding);
cnt[b] = 1 + unpadded positions (the CLS row first); head[b] = 0 when dedupe is on and row b
equals row b - 1 on the padding pattern and on every unpadded token (ids on padded positions may
differ); the unique sequences are the head rows in order.
"""
import numpy as np


def plan(tokens, mask, dedupe, vocab):
    """cnt, head, uniq (n_seq each), src (n_unique), off (n_unique + 1) and
    info = [n_unique, n_rows, max_rows, unpadded ids outside [0, vocab)], all int64."""
    tokens = np.asarray(tokens).astype(np.int64)
    mask = np.asarray(mask, dtype=np.float32)
    n_seq = tokens.shape[0]
    with np.errstate(invalid="ignore"):
        valid = ~(mask > 0)
    cnt = 1 + valid.sum(1)
    head = np.ones(n_seq, dtype=np.int64)
    if dedupe and n_seq > 1:
        same = (valid[1:] == valid[:-1]).all(1) & (~valid[1:] | (tokens[1:] == tokens[:-1])).all(1)
        head[1:] = ~same
    uniq = np.cumsum(head) - 1
    src = np.flatnonzero(head)
    off = np.concatenate([[0], np.cumsum(cnt[src])])
    bad = int((valid & ((tokens < 0) | (tokens >= vocab))).sum())
    info = np.array([len(src), off[-1], max(1, cnt.max(initial=1)), bad], dtype=np.int64)
    return {"cnt": cnt, "head": head, "uniq": uniq, "src": src, "off": off, "info": info}


def split(buf, n_seq):
    """The same fields as views of a plan buffer (6 n_seq + 5 int32) that the library filled."""
    buf = np.asarray(buf)
    info = buf[3 * n_seq + 1:3 * n_seq + 5]
    nu = int(info[0])
    return {"uniq": buf[:n_seq], "src": buf[n_seq:n_seq + nu], "off": buf[2 * n_seq:2 * n_seq + nu + 1], "info": info}


def assert_plan_equal(buf, n_seq, ref):
    got = split(buf, n_seq)
    assert list(got["info"]) == list(ref["info"]), (list(got["info"]), list(ref["info"]))
    for k in ("uniq", "src", "off"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert bad.size == 0, (k, int(bad[0]), int(got[k][bad[0]]), int(ref[k][bad[0]]))
