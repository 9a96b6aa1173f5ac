"""The error codes of the link-prediction entry points (csrc/link.hip) for arguments they refuse
before anything is launched: every fault class on its own, the pairs of faults whose precedence is
part of the ABI, and the byte counts of the three workspace functions. The addresses are never
dereferenced: every call below carries at least one fault that is rejected before the first launch,
so nothing reaches a device (the library loads without one)."""
import itertools

import pytest
import torch  # noqa: F401  (the library binds to torch's HIP runtime)

ARG, MODEL, SHAPE, WORKSPACE = 1, 2, 3, 4
TRANSE, TRANSE_L2, DISTMULT, COMPLEX, ROTATE = range(5)
BIG = 1 << 62  # a workspace size no shape below exceeds
INT32_MAX = (1 << 31) - 1

_addr = itertools.count(1 << 20, 4096)
fake = lambda: next(_addr)  # distinct, 16-byte aligned, never dereferenced

TYPES = ("type_head", "type_tail")
SLICE = ("e_begin", "e_end")
QUERY = ("q_true", "qr", "qmode", "n_query", "q_pad", "dim")
GROUPS = ("grp_qoff", "grp_q", "n_groups", "filt_off", "filt_ids", "entry_q", "n_entries")
WORK = ("work", "work_bytes", "stream")

# argument names in the order of include/mmre.h
PARAMS = {
    "prepare_entities": ("model", "norm_flag", "ent", "ent_im", "n_ent", "dim", "ent_km", "e_pad", "ent_rows",
                         "stream"),
    "prepare_queries": ("model", "norm_flag", "ent_rows", "rel", "rel_im", "n_ent", "n_rel", "dim", "phase_denom",
                        "qh", "qr", "qt", "qmode", "n_query", "q_km", "q_pad", "q_true", "rel_work", "q_rows",
                        "stream"),
    "truth": ("model", "pred_kind", "margin", "ent_km", "n_ent", "e_pad", "ent_rows", "q_km") + QUERY + (
        "filt_off", "filt_ids") + TYPES + ("counts", "truth", "stream"),
    "truth_grouped": ("model", "pred_kind", "margin", "ent_rows", "n_ent", "q_rows", "q_true", "qr", "qmode",
                      "n_query", "dim") + GROUPS + TYPES + ("list_scores", "counts", "truth", "stream"),
    "sweep": ("model", "pred_kind", "margin", "ent_km", "n_ent", "e_pad", "q_km") + QUERY + TYPES + (
        "counts", "truth", "scores", "stream"),
    "sweep_range": ("model", "pred_kind", "margin", "ent_km", "n_ent", "e_pad") + SLICE + ("q_km",) + QUERY + TYPES + (
        "counts", "truth", "stream"),
    "sweep_l1q": ("pred_kind", "margin", "ent_km", "ent_rows", "n_ent", "e_pad") + SLICE + ("q_km", "q_rows") + QUERY
    + TYPES + ("counts", "truth") + WORK,
    "sweep_bf3": ("model", "pred_kind", "margin", "ent_km", "ent_rows", "n_ent", "e_pad") + SLICE + (
        "q_km", "q_rows") + QUERY + ("counts", "truth") + WORK,
    "sweep_bf3_rows": ("model", "pred_kind", "margin", "ent_rows", "n_ent", "e_pad") + SLICE + (
        "ent_km", "q_km", "q_rows") + QUERY + ("counts", "truth") + WORK,
    "evaluate_l1q": ("norm_flag", "ent", "n_ent", "rel", "n_rel", "dim", "qh", "qr", "qt", "qmode", "n_query")
    + GROUPS + SLICE + ("ent_km", "e_pad", "ent_rows", "q_km", "q_pad", "q_rows", "q_true", "list_scores", "counts",
                        "truth", "undecided_q") + WORK,
    "l1q_stats": ("work", "work_bytes", "out", "stream"),
    "bf3_stats": ("work", "work_bytes", "out", "stream"),
}
POINTERS = {"ent", "ent_im", "rel", "rel_im", "ent_km", "ent_rows", "q_km", "q_rows", "q_true", "qh", "qr", "qt",
            "qmode", "rel_work", "filt_off", "filt_ids", "grp_qoff", "grp_q", "entry_q", "list_scores", "counts",
            "truth", "scores", "undecided_q", "work", "out", *TYPES}
OPTIONAL = {"ent_im", "rel_im", "scores", "undecided_q", *TYPES}  # NULL in valid()
MFMA_ONLY = ("sweep_bf3", "sweep_bf3_rows")
# the entry points that start with check_link_args (sweep_bf3 after its model check)
CHECKED = ("truth", "sweep", "sweep_range", "sweep_l1q", "sweep_bf3", "sweep_bf3_rows")
RANGED = ("sweep_range", "sweep_l1q", "sweep_bf3", "sweep_bf3_rows", "evaluate_l1q")
WORKED = ("sweep_l1q", "sweep_bf3", "sweep_bf3_rows", "evaluate_l1q")


def valid(name):
    """Arguments `name` would accept (TransE L1, or DistMult for the split-bf16 sweeps; 300 entities,
    130 queries in 40 groups, dim 16), by name."""
    a = {p: (None if p in OPTIONAL else fake()) for p in PARAMS[name] if p in POINTERS}
    a.update(model=DISTMULT if name in MFMA_ONLY else TRANSE, norm_flag=0, pred_kind=0, margin=0.0, n_ent=300,
             e_pad=384, n_rel=5, dim=16, phase_denom=0.0, n_query=130, q_pad=256, n_groups=40, n_entries=7,
             e_begin=0, e_end=300, work_bytes=BIG, stream=None)
    return a


def run(name, **over):
    """Return code of mmre_link_`name` at valid(name) changed by `over`."""
    from mmre import _lib
    a = valid(name)
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    return getattr(_lib.lib(), "mmre_link_" + name)(*[a[p] for p in PARAMS[name] if p in a])


def has(name, *keys):
    return all(k in PARAMS[name] for k in keys)


def test_signatures_cover_the_tables_above():
    from mmre import _lib
    for name, params in PARAMS.items():
        assert len(_lib.SIGNATURES["mmre_link_" + name][1]) == len(params), name


# ------------------------------------------------------------ every fault class on its own ---
@pytest.mark.parametrize("name", [n for n in PARAMS if has(n, "model")])
def test_bad_model(name):
    for m in (-1, 5):  # (the raw-row sweep refuses anything but DistMult as a SHAPE first)
        assert run(name, model=m) == (SHAPE if name == "sweep_bf3_rows" else MODEL), m


def test_bf3_sweeps_take_mfma_models_only():
    for m in (TRANSE, TRANSE_L2, ROTATE):
        assert run("sweep_bf3", model=m) == MODEL, m
    # the raw-row twin: the row-major table must be the plane layout itself
    assert run("sweep_bf3_rows", model=COMPLEX) == SHAPE
    for m in (TRANSE, ROTATE):
        assert run("sweep_bf3_rows", model=m) == SHAPE, m
    for dim in (1, 8, 24, 200):
        assert run("sweep_bf3_rows", dim=dim) == SHAPE, dim
    assert run("sweep_bf3_rows", ent_rows=fake() + 4) == ARG
    assert run("sweep_bf3_rows", ent_rows=fake() + 8) == ARG
    assert run("sweep_bf3_rows", ent_rows=None) == ARG
    assert run("sweep_bf3_rows", ent_km=None) == ARG


@pytest.mark.parametrize("name", [n for n in PARAMS if has(n, "pred_kind")])
def test_pred_kind_outside_0_to_4(name):
    for pk in (-1, 5):
        assert run(name, pred_kind=pk) == ARG, pk


REQUIRED = {
    "prepare_entities": ("ent", "ent_km", "ent_rows"),
    "prepare_queries": ("ent_rows", "rel", "qh", "qr", "qt", "qmode", "q_km", "q_true"),
    "truth": ("ent_km", "q_km", "q_true", "counts", "truth", "qmode", "qr", "ent_rows"),
    "truth_grouped": ("ent_rows", "q_rows", "q_true", "qr", "qmode", "counts", "truth", "grp_qoff", "grp_q",
                      "filt_off"),
    "sweep": ("ent_km", "q_km", "q_true", "counts", "truth", "qmode", "qr"),
    "sweep_range": ("ent_km", "q_km", "q_true", "counts", "truth", "qmode", "qr"),
    "sweep_l1q": ("ent_km", "q_km", "q_true", "counts", "truth", "qmode", "qr"),
    "sweep_bf3": ("ent_km", "q_km", "q_true", "counts", "truth", "qmode", "qr"),
    "sweep_bf3_rows": ("ent_km", "ent_rows", "q_km", "q_true", "counts", "truth", "qmode", "qr"),
    "evaluate_l1q": ("ent", "rel", "qh", "qr", "qt", "qmode", "ent_km", "ent_rows", "q_km", "q_rows", "q_true",
                     "counts", "truth", "grp_qoff", "grp_q", "filt_off"),
    "l1q_stats": ("work", "out"),
    "bf3_stats": ("work", "out"),
}


@pytest.mark.parametrize("name", list(REQUIRED))
def test_each_required_pointer_null(name):
    for p in REQUIRED[name]:
        assert run(name, **{p: None}) == ARG, p


def test_workspace_pointers_and_sizes():
    from mmre import _lib
    L = _lib.lib()
    need = {"sweep_l1q": L.mmre_link_l1q_workspace(16, 384, 256),
            "sweep_bf3": L.mmre_link_bf3_workspace(DISTMULT, 16, 384, 256),
            "sweep_bf3_rows": L.mmre_link_bf3_workspace(DISTMULT, 16, 384, 256),
            "evaluate_l1q": L.mmre_link_evaluate_l1q_workspace(16, 384, 256)}
    for name in WORKED:
        assert run(name, work=None) == WORKSPACE, name
        assert run(name, work_bytes=0) == WORKSPACE, name
        assert run(name, work_bytes=need[name] - 1) == WORKSPACE, name
        if name != "evaluate_l1q":
            # the exact size is accepted (the next check, a bad range, answers)
            assert run(name, work_bytes=need[name], e_begin=-128) == ARG, name
            assert run(name, q_rows=None) == WORKSPACE, name  # the row-major copies the rescoring reads
    # (evaluate_l1q: only the LDS bound follows its workspace check)
    assert run("evaluate_l1q", dim=681, work_bytes=L.mmre_link_evaluate_l1q_workspace(681, 384, 256)) == SHAPE
    assert run("evaluate_l1q", dim=681, work_bytes=L.mmre_link_evaluate_l1q_workspace(681, 384, 256) - 1) == WORKSPACE
    assert run("sweep_l1q", ent_rows=None) == WORKSPACE
    assert run("sweep_bf3", ent_rows=None) == WORKSPACE
    for name in ("l1q_stats", "bf3_stats"):
        assert run(name, work_bytes=0) == ARG
        assert run(name, work_bytes=8191) == ARG  # both headers are at least 8 KB


SIZE_FAULTS = (dict(n_query=0), dict(n_query=-1), dict(n_ent=0), dict(n_ent=-5), dict(e_pad=256), dict(e_pad=300),
               dict(e_pad=448), dict(q_pad=128), dict(q_pad=130), dict(q_pad=320), dict(dim=0), dict(dim=-3),
               dict(n_rel=0), dict(n_groups=0), dict(n_groups=131), dict(n_entries=-1))
# dim is not read before the launch by the sweeps (a plane count, no check) nor by mmre_link_truth
NO_DIM_CHECK = CHECKED


@pytest.mark.parametrize("name", [n for n in PARAMS if has(n, "n_ent")])
def test_each_size_fault(name):
    for f in SIZE_FAULTS:
        (k, v), = f.items()
        if not has(name, k) or (k == "dim" and name in NO_DIM_CHECK):
            continue
        assert run(name, **f) == ARG, f


@pytest.mark.parametrize("name", [n for n in PARAMS if has(n, *TYPES)])
def test_one_type_mask_without_the_other(name):
    assert run(name, type_head=fake()) == ARG
    assert run(name, type_tail=fake()) == ARG


def test_truth_filter_list_halves():
    assert run("truth", filt_off=None) == ARG
    assert run("truth", filt_ids=None) == ARG


@pytest.mark.parametrize("name", CHECKED + ("evaluate_l1q",))
def test_entity_ids_stay_int32(name):
    big = INT32_MAX - 255
    e_pad = (big + 127) // 128 * 128
    assert run(name, n_ent=big, e_pad=e_pad) == SHAPE
    assert run(name, n_ent=big + 1, e_pad=1 << 31) == SHAPE


def test_truth_grouped_sizes_stay_int32():
    assert run("truth_grouped", n_ent=INT32_MAX) == SHAPE
    assert run("truth_grouped", n_query=INT32_MAX, n_groups=40) == SHAPE
    q = INT32_MAX
    assert run("evaluate_l1q", n_query=q, q_pad=(q + 127) // 128 * 128) == SHAPE


RANGE_FAULTS = (dict(e_begin=-128), dict(e_begin=64), dict(e_begin=1), dict(e_begin=128, e_end=128),
                dict(e_begin=256, e_end=128), dict(e_end=0), dict(e_end=301), dict(e_end=384))


@pytest.mark.parametrize("name", RANGED)
def test_each_entity_range_fault(name):
    for f in RANGE_FAULTS:
        assert run(name, **f) == ARG, f


def test_sweep_needs_entities_first():
    assert run("sweep", n_ent=0) == ARG
    assert run("sweep", n_ent=0, model=9) == ARG  # before the shared checks


def test_score_rows_are_whole_table():
    """mmre_link_sweep alone stores score rows, and always sweeps the whole table: the refusal of a
    partial range with score rows is unreachable through the ABI (mmre_link_sweep_range passes no
    score pointer). What the ABI shows: score rows come with every prior check still applied."""
    assert run("sweep", scores=fake(), type_head=fake()) == ARG
    assert run("sweep", scores=fake(), q_pad=130) == ARG


def test_model_operands():
    for name in ("prepare_entities", "prepare_queries"):
        im = "ent_im" if name == "prepare_entities" else "rel_im"
        assert run(name, model=COMPLEX) == ARG  # no imaginary table
        assert run(name, model=COMPLEX, **{im: fake()}, n_ent=0) == ARG
    assert run("prepare_queries", model=ROTATE, phase_denom=0.0) == ARG
    for m in (TRANSE, TRANSE_L2):
        assert run("prepare_queries", model=m, norm_flag=1, rel_work=None) == WORKSPACE


@pytest.mark.parametrize("name", ("truth_grouped", "evaluate_l1q"))
def test_filter_lists(name):
    assert run(name, n_groups=131) == ARG  # more groups than queries
    for p in ("filt_ids", "entry_q", "list_scores"):
        assert run(name, **{p: None}) == WORKSPACE, p
        assert run(name, **{p: None}, n_entries=0, n_ent=0) == ARG, p  # not needed without entries


# The smallest dim whose staged rows exceed 64 KB of LDS (each one below it passes this check):
#   prepare_entities / prepare_queries  one row of K + 1 floats: K = 16,384
#   truth                               the query's planes: K > 16,384 (RotatE: two planes, > 8,192)
#   evaluate_l1q                        K1 stages max(rb, 3 rb / 2) rows of K + 1 floats, rb 16 while 16
#                                       rows fit: 24 rows of 689 floats
LDS_DIMS = (("prepare_entities", TRANSE, 16377), ("prepare_entities", DISTMULT, 16369),
            ("prepare_entities", ROTATE, 8185), ("prepare_queries", TRANSE, 16377),
            ("prepare_queries", COMPLEX, 8185), ("truth", TRANSE, 16385), ("truth", ROTATE, 8193),
            ("truth", DISTMULT, 16385), ("evaluate_l1q", TRANSE, 681))


@pytest.mark.parametrize("name,model,dim", LDS_DIMS)
def test_rows_too_wide_for_lds(name, model, dim):
    over = dict(dim=dim)
    if has(name, "model"):
        over["model"] = model
        if model == COMPLEX:
            over["ent_im" if name == "prepare_entities" else "rel_im"] = fake()
    assert run(name, **over) == SHAPE


# --------------------------------------------------------------------------- precedences ---
# check_link_args: model, pred_kind, null pointers, sizes, the type pair, SHAPE; then the callers'
# own checks. Each step as a pair: the earlier fault answers.
LADDER = (("model", dict(model=7), MODEL), ("pred_kind", dict(pred_kind=5), ARG), ("null", dict(q_km=None), ARG),
          ("size", dict(q_pad=130), ARG), ("types", dict(type_head=1 << 16), ARG))


@pytest.mark.parametrize("name", CHECKED)
def test_check_link_args_order(name):
    big = INT32_MAX - 255
    shape = dict(n_ent=big, e_pad=(big + 127) // 128 * 128)
    if name == "sweep_bf3_rows":  # its own SHAPE / ARG checks precede everything: below
        return
    # a model fault beats every later one
    for _, later, _ in LADDER[1:]:
        if has(name, *later) and has(name, "model"):
            assert run(name, model=7, **later) == MODEL, later
    # SHAPE distinguishes itself from the ARG classes before it: each of them with an oversized table
    for label, f, rc in LADDER:
        if has(name, *f):
            assert run(name, **f, **shape) == rc, label
    # ... and from what follows it
    if name in RANGED:
        assert run(name, **shape, e_begin=64) == SHAPE
    if name in WORKED:
        assert run(name, **shape, work=None) == SHAPE
        assert run(name, work=None, e_begin=64) == WORKSPACE  # check_link_args, WORKSPACE, the range
        for _, f, rc in LADDER:
            if has(name, *f):
                assert run(name, work=None, **f) == rc, f
    if name == "truth":
        assert run(name, **shape, ent_rows=None) == SHAPE
        assert run(name, **shape, filt_off=None) == SHAPE
    # the ARG classes among themselves return the same code; the ladder's MODEL / WORKSPACE / SHAPE
    # ends are what a caller can tell apart


def test_sweep_bf3_model_first():
    for f in (dict(pred_kind=9), dict(ent_km=None), dict(n_query=0), dict(work=None), dict(e_begin=64),
              dict(n_ent=INT32_MAX - 255, e_pad=1 << 31)):
        assert run("sweep_bf3", model=TRANSE, **f) == MODEL, f
        assert run("sweep_bf3", model=11, **f) == MODEL, f


def test_sweep_bf3_rows_order():
    # SHAPE (not the raw-row layout) before ARG (its pointers) before the shared checks
    assert run("sweep_bf3_rows", model=COMPLEX, ent_rows=None) == SHAPE
    assert run("sweep_bf3_rows", dim=24, ent_rows=fake() + 4) == SHAPE
    assert run("sweep_bf3_rows", model=7, ent_km=None) == SHAPE
    assert run("sweep_bf3_rows", model=TRANSE, pred_kind=9) == SHAPE
    assert run("sweep_bf3_rows", ent_rows=fake() + 4, work=None) == ARG
    assert run("sweep_bf3_rows", ent_km=None, n_ent=INT32_MAX - 255, e_pad=1 << 31) == ARG
    big = INT32_MAX - 255
    shape = dict(n_ent=big, e_pad=(big + 127) // 128 * 128)
    assert run("sweep_bf3_rows", **shape, work=None) == SHAPE
    assert run("sweep_bf3_rows", **shape, e_begin=64) == SHAPE
    assert run("sweep_bf3_rows", work=None, e_begin=64) == WORKSPACE


def test_prepare_queries_order():
    # MODEL, ARG (pointers, sizes, model operands), WORKSPACE (TransE norm scratch), SHAPE (LDS)
    assert run("prepare_queries", model=9, rel=None) == MODEL
    assert run("prepare_queries", norm_flag=1, rel_work=None, q_pad=130) == ARG
    assert run("prepare_queries", norm_flag=1, rel_work=None, qh=None) == ARG
    assert run("prepare_queries", norm_flag=1, rel_work=None, dim=16377) == WORKSPACE
    assert run("prepare_queries", dim=16377, n_rel=0) == ARG
    assert run("prepare_entities", model=9, ent=None) == MODEL
    assert run("prepare_entities", dim=16377, e_pad=300) == ARG
    assert run("prepare_entities", model=COMPLEX, dim=8185) == ARG


def test_truth_order():
    assert run("truth", ent_rows=None, filt_off=None) == ARG
    assert run("truth", dim=16385, ent_rows=None) == ARG  # the LDS bound comes last
    assert run("truth", dim=16385, filt_ids=None) == ARG


def test_truth_grouped_order():
    # MODEL, pred_kind, pointers, sizes, WORKSPACE (the lists), the type pair, SHAPE
    assert run("truth_grouped", model=9, pred_kind=9) == MODEL
    assert run("truth_grouped", filt_ids=None, pred_kind=9) == ARG
    assert run("truth_grouped", filt_ids=None, grp_q=None) == ARG
    assert run("truth_grouped", filt_ids=None, n_groups=0) == ARG
    assert run("truth_grouped", filt_ids=None, type_head=fake()) == WORKSPACE
    assert run("truth_grouped", filt_ids=None, n_ent=INT32_MAX) == WORKSPACE
    assert run("truth_grouped", type_tail=fake(), n_ent=INT32_MAX) == ARG


def test_evaluate_l1q_order():
    """Its seven checks in order: pointers, sizes, the paddings, the entity range (all ARG), the
    filter lists (WORKSPACE), int32 sizes (SHAPE), the workspace (WORKSPACE), the LDS bound (SHAPE)."""
    big = INT32_MAX - 255
    shape = dict(n_ent=big, e_pad=(big + 127) // 128 * 128, e_end=big)
    lists = dict(filt_ids=None)
    assert run("evaluate_l1q", **lists, ent=None) == ARG           # 1 before 5
    assert run("evaluate_l1q", **lists, n_groups=0) == ARG         # 2 before 5
    assert run("evaluate_l1q", **lists, q_pad=130) == ARG          # 3 before 5
    assert run("evaluate_l1q", **lists, e_begin=64) == ARG         # 4 before 5
    assert run("evaluate_l1q", **shape, e_begin=64) == ARG         # 4 before 6
    assert run("evaluate_l1q", **shape, q_pad=130) == ARG          # 3 before 6
    assert run("evaluate_l1q", **lists, **shape) == WORKSPACE      # 5 before 6
    assert run("evaluate_l1q", **shape, work=None) == SHAPE        # 6 before 7
    assert run("evaluate_l1q", work=None, dim=681) == WORKSPACE    # 7 before the LDS bound
    assert run("evaluate_l1q", work=None, e_end=301) == ARG        # 4 before 7
    assert run("evaluate_l1q", dim=681, n_rel=0) == ARG


# ------------------------------------------------------------------ workspace byte counts ---
# Literals from the build this refactor started from (MMRE_BF3_CAP unset): (dim, e_pad, q_pad) ->
# l1q, evaluate_l1q, bf3 DistMult, bf3 ComplEx.
WORKSPACES = {
    (1, 128, 128): (25088, 27392, 551312, 551312),
    (7, 256, 128): (33280, 35584, 560032, 560032),
    (200, 14336, 256): (9348096, 9359104, 12735616, 23942272),
    (200, 14336, 14336): (18415616, 18609920, 27306112, 49326208),
    (2048, 1048576, 14336): (6564610048, 6566937344, 8946762112, 17654137216),
    (200, 1048576, 1048576): (1346379776, 1360568576, 2298618240, 3909230976),
    (7, 128, 1048576): (71319552, 84984320, 81806224, 81806224),
    (2048, 256, 256): (3171328, 3176448, 4731296, 8925600),
}


@pytest.mark.parametrize("shape", list(WORKSPACES))
def test_workspace_bytes(monkeypatch, shape):
    from mmre import _lib
    monkeypatch.delenv("MMRE_BF3_CAP", raising=False)
    L = _lib.lib()
    dim, e_pad, q_pad = shape
    got = (L.mmre_link_l1q_workspace(dim, e_pad, q_pad), L.mmre_link_evaluate_l1q_workspace(dim, e_pad, q_pad),
           L.mmre_link_bf3_workspace(DISTMULT, dim, e_pad, q_pad), L.mmre_link_bf3_workspace(COMPLEX, dim, e_pad, q_pad))
    assert got == WORKSPACES[shape]


def test_workspace_zero_for_bad_arguments(monkeypatch):
    from mmre import _lib
    monkeypatch.delenv("MMRE_BF3_CAP", raising=False)
    L = _lib.lib()
    for dim, e_pad, q_pad in ((0, 128, 128), (-1, 128, 128), (8, 0, 128), (8, 128, 0), (8, -128, 128), (8, 128, -128)):
        assert L.mmre_link_l1q_workspace(dim, e_pad, q_pad) == 0
        assert L.mmre_link_evaluate_l1q_workspace(dim, e_pad, q_pad) == 0
        assert L.mmre_link_bf3_workspace(DISTMULT, dim, e_pad, q_pad) == 0
    for model in (TRANSE, TRANSE_L2, ROTATE, -1, 5):
        assert L.mmre_link_bf3_workspace(model, 8, 128, 128) == 0
