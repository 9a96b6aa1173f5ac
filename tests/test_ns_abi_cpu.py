"""The error codes of the NS entry points (csrc/ns.hip) for arguments they refuse before anything is
launched: every fault class on its own, and the pairs of faults whose precedence is part of the ABI
(the options first, the model before the pointers, TransE under a non-margin loss before the null
checks, an unsupported shape after them, ...). The addresses are never dereferenced: every call
below carries at least one fault that is rejected before the first launch or memset, so nothing
reaches a device (the library loads without one)."""
import ctypes
import itertools

import pytest
import torch  # noqa: F401  (the library binds to torch's HIP runtime)

ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
TRANSE, TRANSE_L2, DISTMULT, COMPLEX, ROTATE = range(5)
BIG = 1 << 62  # a workspace size no shape below exceeds

_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, never dereferenced

MODEL_HEAD = ("model", "norm_flag", "model_margin", "use_model_margin", "ent", "ent_im", "rel", "rel_im")
SIZES = ("n_ent", "n_rel")
ROWS = ("dim", "phase_denom", "h", "t", "r")
LOSS = ("batch", "neg", "loss_margin", "adv_t", "regul_rate")
GRADS = ("grad_ent", "grad_ent_im", "grad_rel", "grad_rel_im")
SAMPLER = ("train_list", "train_total", "head_hrt", "tail_hrt", "rel_hrt", "lef_head", "rig_head", "lef_tail",
           "rig_tail", "lef_rel", "rig_rel", "left_mean", "right_mean", "seeds", "work_threads", "mode", "blocks",
           "n_blocks", "batch_h", "batch_t", "batch_r", "batch_y", "ticket")
NEXT = ("next_h", "next_t", "next_r", "next_y")
STEP = SAMPLER + ("model", "norm_flag", "ent", "rel") + SIZES + ("dim",) + LOSS + (
    "score", "loss", "grad_ent", "grad_rel", "work", "lr", "stream")

# argument names in the order of include/mmre.h; the _ex twins take `opts` last
PARAMS = {
    "mmre_ns_forward": MODEL_HEAD + ROWS + LOSS + ("score", "loss", "work", "stream"),
    "mmre_ns_backward": MODEL_HEAD + ROWS + LOSS + ("score", "grad_loss") + GRADS + SIZES + (
        "work", "work_floats", "stream"),
    "mmre_score_rows_backward": MODEL_HEAD + ROWS + ("batch", "grad_score") + GRADS + SIZES + (
        "work", "work_floats", "stream"),
    "mmre_ns_fused_forward": MODEL_HEAD + SIZES + ROWS + LOSS + ("score", "loss", "work", "stream"),
    "mmre_ns_fused_grad": MODEL_HEAD + SIZES + ROWS + LOSS + ("score", "grad_loss") + GRADS + ("work", "stream"),
    "mmre_ns_fused_grad_sgd": MODEL_HEAD + SIZES + ROWS + LOSS + ("score", "grad_loss") + GRADS + (
        "work", "lr", "stream"),
    "mmre_ns_forward_backward": MODEL_HEAD + SIZES + ROWS + LOSS + ("score", "loss") + GRADS + ("work", "stream"),
    "mmre_ns_step_openke": STEP,
    "mmre_ns_step_openke_pipe": STEP + ("prepared", "parity") + NEXT,
    "mmre_ns_step_openke_gen_pipe": SAMPLER + ("model", "model_margin", "use_model_margin", "ent", "ent_im", "rel",
                                               "rel_im") + SIZES + ("dim", "phase_denom") + LOSS + (
        "score", "loss") + GRADS + ("work", "lr", "stream", "prepared") + NEXT,
}
HAS_EX = ("mmre_ns_forward", "mmre_ns_backward", "mmre_ns_fused_forward", "mmre_ns_fused_grad",
          "mmre_ns_fused_grad_sgd", "mmre_ns_step_openke_gen_pipe")
ONE_CALL = ("mmre_ns_step_openke", "mmre_ns_step_openke_pipe", "mmre_ns_step_openke_gen_pipe")
POINTERS = {"ent", "ent_im", "rel", "rel_im", "h", "t", "r", "score", "loss", "work", "grad_loss", "grad_score",
            *GRADS, *NEXT, *(s for s in SAMPLER if s not in ("train_total", "work_threads", "mode", "n_blocks"))}


def valid(name):
    """Arguments `name` accepts (DistMult, or TransE for the TransE-only steps; dim 8, 4 positives, 2
    negatives), by name."""
    a = {p: fake() for p in PARAMS[name] if p in POINTERS}
    a.update(model=TRANSE if name in ONE_CALL[:2] else DISTMULT, norm_flag=0, model_margin=0.0, use_model_margin=0,
             ent_im=None, rel_im=None, grad_ent_im=None, grad_rel_im=None, n_ent=10, n_rel=3, dim=8, phase_denom=0.0,
             batch=4, neg=2, loss_margin=1.0, adv_t=0.0, regul_rate=0.0, stream=None, work_floats=BIG, lr=0.5,
             train_total=20, work_threads=4, mode=0, blocks=None, n_blocks=0, prepared=0, parity=0)
    return a


def opts(loss_kind=0, optimizer=0, sums=0):
    from mmre import _lib
    o = _lib.NSOpts(loss_kind=loss_kind, optimizer=optimizer, eps=1e-10)
    if sums >= 2:
        o.d_sum_ent, o.d_sum_rel = fake(), fake()
    if sums >= 4:
        o.d_sum_ent_im, o.d_sum_rel_im = fake(), fake()
    return o


def run(name, ex, **over):
    """Return code of `name` (ex: its _ex twin, with over['opts']) at valid(name) changed by `over`."""
    from mmre import _lib
    o = over.pop("opts", None)
    a = valid(name)
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    args = [a[p] for p in PARAMS[name]]
    if ex:
        return getattr(_lib.lib(), name + "_ex")(*args, ctypes.byref(o) if o is not None else None)
    assert o is None
    return getattr(_lib.lib(), name)(*args)


COMPLEX_OK = dict(model=COMPLEX, ent_im=1 << 16, rel_im=2 << 16, grad_ent_im=3 << 16, grad_rel_im=4 << 16)
ROTATE_OK = dict(model=ROTATE, phase_denom=1.0)
BAD_OPTS = (dict(loss_kind=7), dict(loss_kind=-1), dict(optimizer=5), dict(optimizer=-1))
ROW_ENTRIES = ("mmre_ns_forward", "mmre_ns_backward", "mmre_score_rows_backward", "mmre_ns_fused_forward",
               "mmre_ns_fused_grad", "mmre_ns_fused_grad_sgd", "mmre_ns_forward_backward")
FUSED = ("mmre_ns_fused_forward", "mmre_ns_fused_grad", "mmre_ns_fused_grad_sgd")


def both(name):
    """(name, ex) for the entry point and, where it has one, its _ex twin."""
    return [(name, False)] + ([(name, True)] if name in HAS_EX else [])


def only(keys, name):
    return {k: v for k, v in keys.items() if k in PARAMS[name]}


def test_signatures_cover_the_tables_above():
    from mmre import _lib
    for name, params in PARAMS.items():
        assert len(_lib.SIGNATURES[name][1]) == len(params), name
        if name in HAS_EX:
            assert len(_lib.SIGNATURES[name + "_ex"][1]) == len(params) + 1, name


@pytest.mark.parametrize("name", HAS_EX)
def test_bad_options_come_first(name):
    for bad in BAD_OPTS:
        assert run(name, True, opts=opts(**bad)) == ARG, bad
        # ... before the model, the pointers and the shape
        assert run(name, True, opts=opts(**bad), model=9) == ARG, bad
        assert run(name, True, opts=opts(**bad), ent=None, dim=4096) == ARG, bad


@pytest.mark.parametrize("name", ROW_ENTRIES)
def test_model_then_the_common_arguments(name):
    for n, ex in both(name):
        for m in (-1, 5):
            assert run(n, ex, model=m) == MODEL, (ex, m)
            assert run(n, ex, model=m, ent=None, batch=0) == MODEL, (ex, m)  # the model before the pointers
        for p in ("ent", "rel", "h", "t", "r"):
            assert run(n, ex, **{p: None}) == ARG, (ex, p)
        assert run(n, ex, batch=0) == ARG and run(n, ex, batch=-4) == ARG, ex
        assert run(n, ex, dim=0) == ARG and run(n, ex, dim=-8) == ARG, ex
        if "neg" in PARAMS[n]:
            assert run(n, ex, neg=-1) == ARG, ex
        # ComplEx without its im tables, RotatE without a phase
        cx = only(COMPLEX_OK, n)
        assert run(n, ex, **{**cx, "ent_im": None}) == ARG and run(n, ex, **{**cx, "rel_im": None}) == ARG, ex
        assert run(n, ex, model=ROTATE, phase_denom=0.0) == ARG, ex


def test_forward():
    for n, ex in both("mmre_ns_forward"):
        assert run(n, ex, score=None) == ARG and run(n, ex, work=None) == ARG
        assert run(n, ex, neg=513) == SHAPE
        assert run(n, ex, score=None, neg=513) == ARG  # the pointers before the shape
        assert run(n, ex, model=COMPLEX, neg=513) == ARG  # (ComplEx without im tables)
    assert run("mmre_ns_forward", True, opts=opts(loss_kind=2), neg=513) == SHAPE


def test_backward():
    for n, ex in both("mmre_ns_backward"):
        for p in ("score", "grad_ent", "grad_rel", "work"):
            assert run(n, ex, **{p: None}) == ARG, p
        assert run(n, ex, n_ent=0) == ARG and run(n, ex, n_rel=-1) == ARG
        assert run(n, ex, **{**COMPLEX_OK, "grad_ent_im": None}) == ARG
        assert run(n, ex, **{**COMPLEX_OK, "grad_rel_im": None}) == ARG
        assert run(n, ex, dim=2049) == SHAPE and run(n, ex, neg=513) == SHAPE
        assert run(n, ex, work_floats=0) == WORKSPACE and run(n, ex, work_floats=1000) == WORKSPACE
        assert run(n, ex, dim=2049, work_floats=0) == SHAPE  # the shape before the workspace
        assert run(n, ex, grad_ent=None, dim=2049) == ARG  # the pointers before the shape
        assert run(n, ex, **{**COMPLEX_OK, "grad_ent_im": None, "work_floats": 0}) == ARG
    assert run("mmre_ns_backward", True, opts=opts(loss_kind=1), model=TRANSE, dim=2049, work_floats=0) == SHAPE


def test_score_rows_backward():
    n = "mmre_score_rows_backward"
    for p in ("grad_score", "grad_ent", "grad_rel", "work"):
        assert run(n, False, **{p: None}) == ARG, p
    assert run(n, False, n_ent=0) == ARG and run(n, False, n_rel=0) == ARG
    cx = only(COMPLEX_OK, n)
    assert run(n, False, **{**cx, "grad_ent_im": None}) == ARG and run(n, False, **{**cx, "grad_rel_im": None}) == ARG
    assert run(n, False, work_floats=0) == WORKSPACE
    assert run(n, False, dim=2049) == SHAPE
    assert run(n, False, n_ent=1 << 32) == SHAPE  # table rows past the slot keys' 32 bits
    assert run(n, False, batch=1 << 30) == SHAPE  # slots past 31 bits
    assert run(n, False, dim=2049, work_floats=0) == WORKSPACE  # here the workspace comes first
    assert run(n, False, grad_ent=None, work_floats=0) == ARG


@pytest.mark.parametrize("name", FUSED + ("mmre_ns_forward_backward",))
def test_fused_entry_points(name):
    grad = name in FUSED[1:]
    for n, ex in both(name):
        assert run(n, ex, score=None) == ARG and run(n, ex, work=None) == ARG, ex
        assert run(n, ex, n_ent=0) == ARG and run(n, ex, n_rel=0) == ARG, ex
        if not grad:
            assert run(n, ex, loss=None) == ARG, ex
        if grad:
            assert run(n, ex, grad_ent=None) == ARG and run(n, ex, grad_rel=None) == ARG, ex
            assert run(n, ex, **{**COMPLEX_OK, "grad_ent_im": None}) == ARG, ex
            assert run(n, ex, **{**COMPLEX_OK, "grad_rel_im": None}) == ARG, ex
        # shapes without fused kernels: the generic models past dim 512 / K 512, TransE past K 32
        assert run(n, ex, dim=513) == SHAPE and run(n, ex, neg=513) == SHAPE, ex
        assert run(n, ex, model=TRANSE, neg=33) == SHAPE and run(n, ex, model=TRANSE_L2, dim=513) == SHAPE, ex
        assert run(n, ex, **only(COMPLEX_OK, n), dim=1024) == SHAPE and run(n, ex, **ROTATE_OK, neg=600) == SHAPE, ex
        assert run(n, ex, score=None, dim=513) == ARG, ex  # the null checks before the shape
        assert run(n, ex, n_rel=0, model=TRANSE, neg=33) == ARG, ex
    if name == "mmre_ns_forward_backward":  # the forward's refusal, before its launch: the gradient's faults unseen
        assert run(name, False, grad_ent=None, dim=513) == SHAPE
        assert run(name, False, grad_ent=None, score=None) == ARG
        return
    # TransE has the margin loss only: refused as a model, before the null checks and the shape
    for kind in (1, 2):
        for m in (TRANSE, TRANSE_L2):
            assert run(name, True, opts=opts(loss_kind=kind), model=m) == MODEL
            assert run(name, True, opts=opts(loss_kind=kind), model=m, score=None, work=None) == MODEL
            assert run(name, True, opts=opts(loss_kind=kind), model=m, neg=33) == MODEL
            assert run(name, True, opts=opts(loss_kind=kind), model=m, ent=None) == ARG  # ns_args' checks before it
        assert run(name, True, opts=opts(loss_kind=kind), dim=513) == SHAPE  # DistMult: every loss, same shapes
        assert run(name, True, opts=opts(loss_kind=kind), score=None) == ARG


def test_fused_grad_sgd():
    for n, ex in both("mmre_ns_fused_grad_sgd"):
        assert run(n, ex, lr=0.0) == ARG
        assert run(n, ex, lr=0.0, model=9) == ARG  # lr first: before the model
        assert run(n, ex, lr=0.0, dim=513) == ARG
    n = "mmre_ns_fused_grad_sgd"
    assert run(n, True, opts=opts(loss_kind=1), lr=0.0, model=TRANSE) == ARG
    # Adagrad: the generic models only, with its sum tables (ComplEx: all four) -- after the model and
    # TransE's loss, before the null checks and the shape
    ada = lambda sums=0, **kw: opts(optimizer=1, sums=sums, **kw)
    assert run(n, True, opts=ada()) == ARG
    assert run(n, True, opts=ada(2), **COMPLEX_OK) == ARG
    assert run(n, True, opts=ada(4), model=TRANSE) == ARG
    o = ada(2)
    o.d_sum_rel = None
    assert run(n, True, opts=o) == ARG
    assert run(n, True, opts=ada(), model=9) == MODEL
    assert run(n, True, opts=ada(), ent=None) == ARG
    assert run(n, True, opts=ada(4, loss_kind=1), model=TRANSE) == MODEL  # TransE's loss before Adagrad's refusal
    assert run(n, True, opts=ada(), dim=513) == ARG  # Adagrad's state before the shape
    assert run(n, True, opts=ada(4), model=TRANSE, neg=33) == ARG
    assert run(n, True, opts=ada(2), dim=513) == SHAPE  # with its state: the remaining fault
    assert run(n, True, opts=ada(2), score=None) == ARG
    assert run(n, True, opts=ada(4), **COMPLEX_OK, neg=513) == SHAPE
    # mmre_ns_fused_grad_ex applies no step (lr 0): Adagrad's state is not looked at
    assert run("mmre_ns_fused_grad", True, opts=ada(), dim=513) == SHAPE
    assert run("mmre_ns_fused_grad", True, opts=ada(), model=TRANSE, neg=33) == SHAPE


def _one_call_names():
    return [(n, ex) for name in ONE_CALL for n, ex in both(name)]


@pytest.mark.parametrize("name,ex", _one_call_names())
def test_one_call_steps(name, ex):
    gen = name == "mmre_ns_step_openke_gen_pipe"
    pipe = name != "mmre_ns_step_openke"
    for p in ("train_list", "head_hrt", "tail_hrt", "lef_head", "rig_head", "lef_tail", "rig_tail", "seeds", "batch_h",
              "batch_t", "batch_r", "batch_y", "ticket"):
        assert run(name, ex, **{p: None}) == ARG, p
    assert run(name, ex, left_mean=None) == ARG and run(name, ex, right_mean=None) == ARG  # both or neither
    for k, v in (("train_total", 0), ("n_ent", 1), ("work_threads", 0), ("batch", 0), ("neg", 0), ("mode", -2),
                 ("mode", 2), ("n_blocks", -1), ("n_blocks", 3), ("n_rel", 0), ("lr", 0.0)):
        assert run(name, ex, **{k: v}) == ARG, (k, v)
    for p in ("score", "loss", "grad_ent", "grad_rel", "work"):
        assert run(name, ex, **{p: None}) == ARG, p
    if pipe:
        assert run(name, ex, prepared=-1) == ARG and run(name, ex, prepared=4) == ARG
        for p in NEXT[1:]:
            assert run(name, ex, **{p: None}) == ARG, p  # with d_next_h, all of the next batch's buffers
        b = fake()
        assert run(name, ex, batch_h=b, next_h=b) == ARG  # the next batch's buffer is the current one
        assert run(name, ex, prepared=4, model=9) == ARG and run(name, ex, next_t=None, model=9) == ARG
    if name == "mmre_ns_step_openke_pipe":
        assert run(name, ex, parity=-1) == ARG and run(name, ex, parity=2) == ARG
        assert run(name, ex, parity=2, neg=33) == ARG
    # the model, the tables and the shape come after all of the above
    assert run(name, ex, model=-1) == MODEL and run(name, ex, model=5) == MODEL
    assert run(name, ex, model=5, lr=0.0) == ARG and run(name, ex, model=5, seeds=None) == ARG
    assert run(name, ex, model=5, ent=None) == MODEL
    assert run(name, ex, ent=None) == ARG and run(name, ex, rel=None) == ARG and run(name, ex, dim=0) == ARG
    assert run(name, ex, dim=513) == SHAPE and run(name, ex, dim=513, score=None) == ARG
    if gen:  # DistMult / ComplEx / RotatE only
        assert run(name, ex, model=TRANSE) == SHAPE and run(name, ex, model=TRANSE_L2) == SHAPE
        assert run(name, ex, neg=513) == SHAPE
        assert run(name, ex, **{**COMPLEX_OK, "ent_im": None}) == ARG
        assert run(name, ex, **{**COMPLEX_OK, "grad_rel_im": None}) == ARG
        assert run(name, ex, **{**COMPLEX_OK, "grad_rel_im": None, "dim": 513}) == ARG
        assert run(name, ex, model=ROTATE, phase_denom=0.0) == ARG
        assert run(name, ex, model=ROTATE, phase_denom=0.0, dim=513) == ARG
        assert run(name, ex, **COMPLEX_OK, dim=513) == SHAPE and run(name, ex, **ROTATE_OK, neg=513) == SHAPE
    else:  # TransE only
        assert run(name, ex, model=DISTMULT) == SHAPE
        # (these two have no im tables and no phase here: refused as arguments, before the shape)
        assert run(name, ex, model=COMPLEX) == ARG and run(name, ex, model=ROTATE) == ARG
        assert run(name, ex, neg=33) == SHAPE and run(name, ex, model=TRANSE_L2, neg=33, dim=600) == SHAPE


def test_generic_step_options():
    n = "mmre_ns_step_openke_gen_pipe"
    ada = lambda sums=0, **kw: opts(optimizer=1, sums=sums, **kw)
    assert run(n, True, opts=opts(loss_kind=3), model=9, seeds=None) == ARG
    assert run(n, True, opts=ada()) == ARG
    assert run(n, True, opts=ada(2), **COMPLEX_OK) == ARG
    assert run(n, True, opts=ada(), model=9) == MODEL  # the model before Adagrad's state
    assert run(n, True, opts=ada(), dim=513) == ARG  # Adagrad's state before the shape
    assert run(n, True, opts=ada(), model=TRANSE) == ARG
    assert run(n, True, opts=ada(2), dim=513) == SHAPE
    assert run(n, True, opts=ada(2, loss_kind=2), model=TRANSE) == SHAPE
    assert run(n, True, opts=ada(4, loss_kind=1), **COMPLEX_OK, neg=513) == SHAPE
    assert run(n, True, opts=ada(2), lr=0.0) == ARG
