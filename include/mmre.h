/*
 * mmre.h -- C ABI of libmmre_hip.so, the MI355X-native hot path of
 * luisrui/Multimodal-Relation-Extrapolation (KG scoring sweep, negative-sampling
 * margin loss, zero-shot relation-embedding generator).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - Pointers named d_* are DEVICE pointers (hipMalloc / torch CUDA tensors);
 *     pointers named h_* are HOST pointers. Every device entry point takes an
 *     explicit hipStream_t (passed as void*; NULL = default stream) and only
 *     enqueues work: no allocation, no synchronisation, graph-capturable.
 *   - Return value: 0 on success, MMRE_ERR_* (> 0) on a bad argument, or
 *     MMRE_ERR_HIP_BASE + hipError_t for a HIP failure. Nothing aborts.
 *   - The library is stateless: all state lives in caller-owned buffers.
 *   - Model ids: MMRE_TRANSE_L1 / _L2 / DISTMULT / COMPLEX / ROTATE.
 *
 * Each entry point names the reference interface it replaces (file:line under
 * the reference tree). INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 */
#ifndef MMRE_H
#define MMRE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MMRE_TRANSE_L1 = 0,
  MMRE_TRANSE_L2 = 1,
  MMRE_DISTMULT = 2,
  MMRE_COMPLEX = 3,
  MMRE_ROTATE = 4,
  /* TransH (mmre_transh_* only; the entry points above answer MMRE_ERR_MODEL for them) */
  MMRE_TRANSH_L1 = 5,
  MMRE_TRANSH_L2 = 6,
  /* TransD (mmre_transd_* only; every other entry point answers MMRE_ERR_MODEL for them) */
  MMRE_TRANSD_L1 = 7,
  MMRE_TRANSD_L2 = 8,
  /* TransR (mmre_transr_* only; every other entry point answers MMRE_ERR_MODEL for them) */
  MMRE_TRANSR_L1 = 9,
  MMRE_TRANSR_L2 = 10,
  /* RESCAL (mmre_rescal_* only; every other entry point answers MMRE_ERR_MODEL for it) */
  MMRE_RESCAL = 11
};
enum { MMRE_HEAD_BATCH = 0, MMRE_TAIL_BATCH = 1 };
/* Loss of the negative-sampling entry points (mmre_ns_opts_t) and the optimizer whose step the
 * row owner applies. */
enum { MMRE_LOSS_MARGIN = 0, MMRE_LOSS_SOFTPLUS = 1, MMRE_LOSS_SIGMOID = 2 };
enum { MMRE_OPT_SGD = 0, MMRE_OPT_ADAGRAD = 1 };
enum {
  MMRE_OK = 0,
  MMRE_ERR_ARG = 1,
  MMRE_ERR_MODEL = 2,
  MMRE_ERR_SHAPE = 3,
  MMRE_ERR_WORKSPACE = 4,
  MMRE_ERR_HIP_BASE = 1000
};

/* Library / ABI version (major*10000 + minor*100 + patch). */
int mmre_version(void);

/* ====================================================================== *
 *  Link prediction: the all-entity score sweep with fused rank epilogue.  *
 *  Replaces, per evaluation, the Tester loop (OpenKE/openke/config/       *
 *  Tester.py:70-91) = getHeadBatch/getTailBatch (Test.h:36-53) +          *
 *  model.predict (TransE.py:104-110, DistMult.py:70-72, ComplEx.py:60-62, *
 *  RotatE.py:89-91) + testHead/testTail (Test.h:65-192, _find            *
 *  Corrupt.h:166-177).                                                    *
 * ====================================================================== */

/* Width K of the k-major planes for a model (d, or 2d for ComplEx/RotatE),
 * rounded up to the sweep's K step. */
int64_t mmre_link_k(int model, int dim);
/* Padded entity / query counts used by the k-major planes. */
int64_t mmre_link_pad(int64_t n);

/* Entity table -> k-major planes d_ent_km[K][e_pad] for the sweep and the same
 * values row-major in d_ent_rows[n_ent][K] for per-entity gathers (F.normalize
 * first when norm_flag, TransE.py:63-66). Tables: TransE/DistMult (E, d);
 * ComplEx re/im (E, d) each; RotatE (E, 2d) = [re | im] (RotatE.py:48-49). */
int mmre_link_prepare_entities(int model, int norm_flag, const float* d_ent, const float* d_ent_im,
                               int64_t n_ent, int dim, float* d_ent_km, int64_t e_pad, float* d_ent_rows,
                               void* stream);

/* Query vectors for each (h, r, t, mode) -> d_q_km[K][q_pad] (element-wise from the
 * prepared d_ent_rows); d_q_true[i] = the entity the sweep must rank (h for
 * head_batch, t for tail_batch). d_rel_work: (n_rel, d) floats, required for
 * TransE with norm_flag (normalised relation rows). phase_denom: RotatE's
 * rel_range/pi as torch evaluates it (RotatE.py:51). d_q_rows (nullable): the
 * same vectors row-major [n_query][K], for mmre_link_truth_grouped. */
int mmre_link_prepare_queries(int model, int norm_flag, const float* d_ent_rows, const float* d_rel,
                              const float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim, float phase_denom,
                              const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                              const int8_t* d_qmode, int64_t n_query, float* d_q_km, int64_t q_pad,
                              int32_t* d_q_true, float* d_rel_work, float* d_q_rows, void* stream);

/* Per-query threshold and filter bookkeeping, enqueued before the sweep:
 * writes d_truth[i] = pred(true(i)) with exactly the sweep's arithmetic and
 * initialises d_counts[.][i] = {0, -c, 0, -c_tc}, c = the known entities j of query i
 * (j != true) with pred(j) < pred(true) -- Test.h:85 `not _find(...)` -- so the
 * sweep's raw additions leave the filtered columns filtered.
 * filter CSR: d_filt_off[n_query+1] (int64), d_filt_ids (int32): the known heads
 *   (head_batch) / tails (tail_batch) of the query in train+valid+test
 *   (Reader.h:201-226); NULL/NULL = no filtering.
 * type masks: uint32 [n_rel][ceil(E/32)] bitsets of the relation's allowed heads
 *   / tails (type_constrain.txt, Reader.h:266-317); NULL/NULL disables.
 * d_counts: int32 [4][n_query] = raw, filt, raw_tc, filt_tc.
 * pred_kind: 0 s, 1 m-(m-s), 2 -s, 3 -(m-s), 4 m-s  (DESIGN.md §3). */
int mmre_link_truth(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                    int64_t e_pad, const float* d_ent_rows, const float* d_q_km, const int32_t* d_q_true, const int64_t* d_qr,
                    const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim,
                    const int64_t* d_filt_off, const int32_t* d_filt_ids, const uint32_t* d_type_head,
                    const uint32_t* d_type_tail, int32_t* d_counts, float* d_truth, void* stream);

/* mmre_link_truth for filter GROUPS: queries with the same (mode, r, anchor) -- the
 * key of Test.h:85's _find: (r, t) for head_batch, (h, r) for tail_batch -- share one
 * known-entity list, so each listed entity is scored once per group. Two launches:
 * every truth and every listed entity scored as one flat set of lanes (listed entity
 * p with the query vector of query d_entry_q[p], any member of its group), then one
 * wave per group counts, for each member, the listed entities that beat its truth.
 * d_q_rows: row-major query vectors [n_query][K] (mmre_link_prepare_queries).
 * d_grp_qoff[n_groups+1] (int64) / d_grp_q (int32): a partition of 0..n_query-1
 *   (every query in exactly one group; groups of <= 64 queries run best).
 * d_filt_off[n_groups+1] (int64) / d_filt_ids[n_entries] (int32): each group's list.
 * d_list_scores: float workspace [n_entries]. Writes d_truth and all of d_counts
 * exactly as mmre_link_truth does. */
int mmre_link_truth_grouped(int model, int pred_kind, float margin, const float* d_ent_rows, int64_t n_ent,
                            const float* d_q_rows, const int32_t* d_q_true, const int64_t* d_qr,
                            const int8_t* d_qmode, int64_t n_query, int dim, const int64_t* d_grp_qoff,
                            const int32_t* d_grp_q, int64_t n_groups, const int64_t* d_filt_off,
                            const int32_t* d_filt_ids, const int32_t* d_entry_q, int64_t n_entries,
                            const uint32_t* d_type_head, const uint32_t* d_type_tail, float* d_list_scores,
                            int32_t* d_counts, float* d_truth, void* stream);

/* The sweep (after mmre_link_truth[_grouped] on the same stream). For every query i and
 * every entity j != true(i):  raw += pred(j) < pred(true)   (Test.h:80-86, strict
 * <, ties favour the truth), added to the raw AND filtered columns (and the _tc
 * columns for allowed j when type masks are given, Test.h:88-98). The kernel adds to the
 * raw columns and a short pass after it adds them to the filtered ones, so every sweep
 * call completes the count table the truth pass initialised (one sweep call per truth pass).
 * d_scores (nullable): (n_query, E) predicted values, for parity tests only. */
int mmre_link_sweep(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                    int64_t e_pad, const float* d_q_km, const int32_t* d_q_true, const int64_t* d_qr,
                    const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim,
                    const uint32_t* d_type_head, const uint32_t* d_type_tail, int32_t* d_counts,
                    const float* d_truth, float* d_scores, void* stream);

/* The same sweep over the entity slice [e_begin, e_end) only (e_begin a multiple of 128), for
 * entity-sharded evaluation (the alternative for huge E): each rank sweeps every
 * query against its slice after a truth pass whose filter lists hold only the slice's entities
 * (mmre_link_truth[_grouped] with restricted lists), so summing d_counts over the ranks
 * (one all-reduce of int32) gives exactly the whole-table counts. Replaces the per-query
 * testHead/testTail scan of Test.h:65-192 for the slice. No score rows. */
int mmre_link_sweep_range(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                          int64_t e_pad, int64_t e_begin, int64_t e_end, const float* d_q_km,
                          const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode, int64_t n_query,
                          int64_t q_pad, int dim, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                          int32_t* d_counts, const float* d_truth, void* stream);

/* TransE L1 (model MMRE_TRANSE_L1) count-only sweep through an integer filter: same counts as
 * mmre_link_sweep / mmre_link_sweep_range (bit for bit; replaces the same Test.h:65-192 scan),
 * faster. The k-major planes are quantized over the largest |x| of both to 8-bit codes (four k
 * per dword, summed with one v_sad_u8 per four elements) or, when a fixed sample of pairs
 * scored with those codes leaves more than 0.6 % undecided, to 16-bit codes (v_sad_u16, two
 * elements per instruction); the choice is made on the device (short launches on the stream,
 * no host round trip). Every pair the quantization error bound leaves on both sides of its
 * query's threshold is rescored with the canonical f32 chain from the row-major copies
 * d_ent_rows (whole table, mmre_link_prepare_entities) and d_q_rows
 * (mmre_link_prepare_queries). e_begin / e_end as for mmre_link_sweep_range (0, n_ent: whole
 * table). d_work: mmre_link_l1q_workspace(dim, e_pad, q_pad) bytes of device scratch.
 * Environment MMRE_L1_BITS=8 / 16 forces a code width (tests, experiments). */
int64_t mmre_link_l1q_workspace(int dim, int64_t e_pad, int64_t q_pad);
/* The filter's own record of the last mmre_link_sweep_l1q on d_work (one tiny launch, no
 * synchronisation): d_out[0] = pairs the code bound left undecided (each rescored with the
 * canonical f32 chain), d_out[1] = the code width the sweep used: 0 = 8-bit codes, 2 = 16-bit
 * codes, 1 = the f32 fallback instead of the codes. The fallback is taken on the device when M
 * (the largest |x|) exceeds 128 x the mean |x| of the two planes -- one outlier value stretching
 * the code range, which would leave most pairs undecided -- or is not finite. Counts are the
 * same either way. d_out[2] = undecided-list entries the rescoring refused because their query
 * or entity id was out of range (a guard on the list's invariant: 0 unless the build is
 * defective), d_out[3] = the largest per-entity error offset of the 8-bit codes' tight bound (in
 * code steps; 0 with the uniform bound). d_out holds 4 uint64. */
int mmre_link_l1q_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream);
/* The per-query route of the last mmre_link_evaluate_l1q on this workspace: queries whose 8-bit
 * band holds a large share of the entities are counted by an exact f32 sweep of their own instead
 * of the code sweep and its rescoring (same counts). d_out[0] = queries flagged by the sampled
 * probe, d_out[1] = queries routed (the first `cap` flagged ones in query order), d_out[2] = sampled
 * entity columns, d_out[3] = the sampled-pair count that flags a query; all 0 when the route did
 * not act (small evaluations, 16-bit codes, a code width forced by MMRE_L1_BITS, the f32 fallback,
 * MMRE_L1_HEAVY=0; MMRE_L1_HEAVY=1 lets it act at any size and with forced 8-bit codes). d_out holds 4
 * uint64. mmre_link_l1q_route_cap: the routed list's cap for a shape, n_query / 16 (at least 1)
 * or what the workspace region it lives in holds; 0 on bad arguments. */
int mmre_link_l1q_route_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream);
int64_t mmre_link_l1q_route_cap(int dim, int64_t e_pad, int64_t q_pad, int64_t n_query);
int mmre_link_sweep_l1q(int pred_kind, float margin, const float* d_ent_km, const float* d_ent_rows, int64_t n_ent,
                        int64_t e_pad, int64_t e_begin, int64_t e_end, const float* d_q_km, const float* d_q_rows,
                        const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode, int64_t n_query,
                        int64_t q_pad, int dim, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                        int32_t* d_counts, const float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* The whole count-only TransE L1 link-prediction evaluation of a query set in ONE call (prediction
 * = the score, filter groups, no type constraints) -- what mmre_link_prepare_entities +
 * mmre_link_prepare_queries + mmre_link_truth_grouped + mmre_link_sweep_l1q compute, with the same
 * outputs bit for bit (the entity / query planes and rows, q_true, truth scores, counts), in
 * seven launches instead of thirteen: query blocks normalise their own anchor and truth rows
 * from the raw table (no wait on the entity prep), the truth scores ride on the query prep,
 * list scores share a launch with the quantization, filter counts with the code-width probe.
 * Replaces Tester.run_link_prediction's loop (Tester.py:70-91: getHeadBatch/getTailBatch
 * Test.h:36-53, TransE.predict TransE.py:104-110, testHead/testTail Test.h:65-192) for TransE.
 * d_ent / d_rel: the raw tables (n_ent x dim, n_rel x dim); norm_flag as TransE's. Filter
 * groups as for mmre_link_truth_grouped (FilterIndex.groups; restricted to [e_begin, e_end)
 * for an entity slice). d_work: mmre_link_evaluate_l1q_workspace(dim, e_pad, q_pad) bytes,
 * ZEROED before the first call (it holds grid tickets; every call leaves them zero).
 * d_undecided_q (NULL or n_query uint32): per query, the pairs the filter left undecided and
 * rescored with the canonical chain (the relation-sharded partition's cost calibration).
 * The group partition also shapes the sweep: the integer filter's code sweep runs once per
 * SWEEP ROW -- a group, cut into runs of at most 8 members -- and ranks every (row, entity) score
 * against each member's own threshold. Contract: d_grp_qoff (n_groups + 1 ascending offsets,
 * 0 .. n_query) and d_grp_q (a permutation of 0 .. n_query - 1) partition the queries, and the
 * members of a group share (mode, r, anchor), hence a bit-identical query vector. Results --
 * counts, the undecided record, d_undecided_q -- are the same for every such partition: any
 * group order, any group sizes (one query per group; one group holding every query of a key;
 * groups beyond 8 members). Speed is not: a 128-row tile costs its largest row's members, so
 * groups sorted by descending size and capped at 8 (FilterIndex.groups(order="size",
 * max_group=8)) sweep fastest. Where grouping would not pay -- the rows' upper bound
 * n_groups + n_query / 8 leaves resident workgroups without a unit, or exceeds 0.6 n_query
 * (little duplication, or one query per group) -- the call sweeps once per query, with the
 * launches of mmre_link_sweep_l1q. Queries whose
 * vectors differ must not share a group (their counts would be the first member's). */
int64_t mmre_link_evaluate_l1q_workspace(int dim, int64_t e_pad, int64_t q_pad);
int mmre_link_evaluate_l1q(int norm_flag, const float* d_ent, int64_t n_ent, const float* d_rel, int64_t n_rel,
                           int dim, const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                           const int8_t* d_qmode, int64_t n_query, const int64_t* d_grp_qoff, const int32_t* d_grp_q,
                           int64_t n_groups, const int64_t* d_filt_off, const int32_t* d_filt_ids,
                           const int32_t* d_entry_q, int64_t n_entries, int64_t e_begin, int64_t e_end,
                           float* d_ent_km, int64_t e_pad, float* d_ent_rows, float* d_q_km, int64_t q_pad,
                           float* d_q_rows, int32_t* d_q_true, float* d_list_scores, int32_t* d_counts,
                           float* d_truth, uint32_t* d_undecided_q, void* d_work, int64_t work_bytes,
                           void* stream);

/* DistMult / ComplEx (MMRE_DISTMULT, MMRE_COMPLEX) count-only sweep through a split-bf16 MFMA
 * filter: same counts as mmre_link_sweep / mmre_link_sweep_range without type constraints (bit
 * for bit; replaces the same Test.h:65-192 scan), faster. Each f32 plane value x is split into
 * hi = bf16(x) and lo = bf16(x - hi); the sweep computes Qhi.Ehi + Qhi.Elo + Qlo.Ehi on the bf16
 * MFMA (16 k per instruction against the f32 MFMA's 2) and decides a pair only when its
 * prediction is on one side of the query's threshold over the whole error bound
 * cb |q|_2 |e|_2; the rest (the truth, near ties, non-finite values) are listed and rescored
 * with the canonical f32 chain from the row-major copies d_ent_rows (whole table) and d_q_rows.
 * If the list overflows, the device resets the raw counts and runs the exact f32 sweep instead
 * (no host round trip). e_begin / e_end as for mmre_link_sweep_range (0, n_ent: whole table).
 * Where the split planes exceed 64 MB (and pred_kind = -score) the sweep runs its wide form
 * (256 x 256 units, per-query thresholds per 32-entity block, a looser bound than the per-pair
 * one, the same counts); env MMRE_BF3_WIDE=1 / 0 forces either, MMRE_BF3_QT=128 its query tile.
 * d_work: mmre_link_bf3_workspace(model, dim, e_pad, q_pad) bytes of device scratch (0 for a
 * model without the filter). */
int64_t mmre_link_bf3_workspace(int model, int dim, int64_t e_pad, int64_t q_pad);
/* The filter's record of the last mmre_link_sweep_bf3 on d_work (one tiny launch, no
 * synchronisation), four words: d_out[0] = pairs listed for exact rescoring, d_out[1] = 1 if the
 * list overflowed and the exact f32 sweep counted instead, d_out[2] = the appends a full segment
 * sent to the list's shared half (those past its end included: they set d_out[1]), d_out[3] = the
 * path record of that sweep as launched: bits 0-15 the wide sweep's query tile (256 / 128; 0: the
 * 128 x 128 sweep), bit 16 set if it ran the lock-step windows (env MMRE_BF3_BLOCKED=1 / 0 asks
 * for them or not, read per call; they need >= 8 entity tiles and a resident grid that is a
 * multiple of 8). */
int mmre_link_bf3_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream);
int mmre_link_sweep_bf3(int model, int pred_kind, float margin, const float* d_ent_km, const float* d_ent_rows,
                        int64_t n_ent, int64_t e_pad, int64_t e_begin, int64_t e_end, const float* d_q_km,
                        const float* d_q_rows, const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode,
                        int64_t n_query, int64_t q_pad, int dim, int32_t* d_counts, const float* d_truth,
                        void* d_work, int64_t work_bytes, void* stream);
/* mmre_link_sweep_bf3 for a table whose row-major layout IS the plane layout -- DistMult with d a
 * multiple of 16, whose evaluation needs no normalisation (DistMult.py:34-44, 70-72): d_ent_rows
 * is then the raw (n_ent, d) embedding table (16-B aligned), and no prepared copy of it is made
 * per evaluation (mmre_link_prepare_entities writes two, k-major and row-major). The split planes,
 * norms and block maxima come from one read of the rows; d_ent_km (k_pad x e_pad floats, any
 * contents) is written only when the list overflows, by the fallback itself, before the exact
 * f32 sweep reads it. Same counts as mmre_link_sweep_bf3, bit for bit. MMRE_ERR_SHAPE for any
 * other model / d. */
int mmre_link_sweep_bf3_rows(int model, int pred_kind, float margin, const float* d_ent_rows, int64_t n_ent,
                             int64_t e_pad, int64_t e_begin, int64_t e_end, float* d_ent_km, const float* d_q_km,
                             const float* d_q_rows, const int32_t* d_q_true, const int64_t* d_qr,
                             const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim, int32_t* d_counts,
                             const float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* Test.h:232-327 test_link_prediction + getTestLink* (Test.h:356-390), host side,
 * with the reference's float accumulation order (P14). Counts: int32, column c of
 * query i at counts[c*stride + i] (c = raw, filt, raw_tc, filt_tc).
 * h_out[20] = {mrr, mr, hit10, hit3, hit1} x {filter, raw, filter_tc, raw_tc}. */
int mmre_link_metrics(const int32_t* h_head_counts, const int32_t* h_tail_counts, int64_t n, int64_t stride,
                      float* h_out);

/* ====================================================================== *
 *  TransH (OpenKE/openke/module/model/TransH.py): link prediction with    *
 *  entities projected on the hyperplane of the query's relation, and      *
 *  predict for arbitrary rows. Models MMRE_TRANSH_L1 / MMRE_TRANSH_L2     *
 *  (p_norm 1 / 2). Tables: entities (E, d), relations (R, d), the         *
 *  hyperplane normals norm_vector (R, d).                                 *
 * ====================================================================== */

/* Bytes of d_work for mmre_transh_evaluate: the raw k-major and row-major entity copies, the
 * normalised relation vectors, the (a, n) table of 2 * n_used * e_pad floats (TransH.py:68-76:
 * a = e . w_hat, n = max(|e - a w_hat|, 1e-12) of TransH.py:54-56), the query planes of n_tiles
 * padded tiles and the n_entries listed scores. O(n_used * E + E * d), never O(n_used * E * d).
 * 0 for a non-positive size. */
int64_t mmre_transh_workspace(int64_t n_ent, int64_t n_rel, int dim, int64_t n_tiles, int64_t n_used,
                              int64_t n_entries);

/* One TransH link-prediction evaluation, enqueued on `stream`: replaces the Tester loop
 * (Tester.py:70-91: getHeadBatch / getTailBatch Test.h:36-53, TransH.predict TransH.py:109-115 =
 * forward TransH.py:78-93 with _transfer :68-76 and _calc :52-66, testHead / testTail
 * Test.h:65-192) for every query at once. Prologue (normalised vectors, the (a, n) table, query
 * vectors), truth and filter pass, the sweep, the finalize pass.
 * Queries (d_qh, d_qr, d_qt int64, d_qmode int8: MMRE_HEAD_BATCH / MMRE_TAIL_BATCH) in the
 * caller's order. The plan orders them by relation so that every 128-row sweep tile holds one
 * relation: d_perm[n_query] (int32) the stable order, d_tiles[n_tiles][3] (int32) = (relation,
 * first row of d_perm, rows <= 128), d_used[n_used] (int32) the relations that have queries and
 * d_rel_slot[n_rel] (int32) a relation's index in d_used or -1. A query no tile holds keeps
 * raw counts of 0.
 * Filter groups as mmre_link_truth_grouped takes them (d_grp_qoff NULL: no filtering). Type
 * masks as mmre_link_truth takes them (NULL / NULL disables; Test.h:88-98).
 * pred_kind 0: s; 1: m - (m - s), a model with a margin (TransH.py:109-115).
 * Writes d_truth[n_query] = pred(truth) and d_counts int32 [4][n_query] = raw, filt, raw_tc,
 * filt_tc: #{j != truth : pred(j) < pred(truth)}, strict, ties favour the truth (Test.h:83). */
int mmre_transh_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                         const float* d_rel, const float* d_norm, int64_t n_ent, int64_t n_rel, int dim,
                         const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt, const int8_t* d_qmode,
                         int64_t n_query, const int32_t* d_perm, const int32_t* d_tiles, int64_t n_tiles,
                         const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                         const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                         const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                         int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                         int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* TransH.predict / forward values of the rows (d_h[i], d_r[i], d_t[i]) (TransH.py:78-93,
 * :109-115), bit for bit what mmre_transh_evaluate scores for the same triple and mode (so a
 * rank recomputed from these values is the sweep's: Test.h:80-86). head_batch != 0: the
 * grouping h + (r - t) of TransH.py:61-62, else (h + r) - t. pred_kind as apply_pred's 0 .. 4
 * (4 = m - s, forward() of a model with a margin). A row with an id outside the tables gets NaN. */
int mmre_transh_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                           const float* d_rel, const float* d_norm, int64_t n_ent, int64_t n_rel, int dim,
                           const int64_t* d_h, const int64_t* d_r, const int64_t* d_t, int64_t n_rows,
                           int head_batch, float* d_out, void* stream);

/* ---- TransH negative-sampling training (csrc/transh_train.hip) ----
 * model(data) of TransH.py:52-107 in 'normal' mode for the B (1 + K) rows of a batch laid out
 * [pos | neg_1 | ... | neg_K] (row b + (j + 1) B is negative j of positive b,
 * NegativeSampling.py:23-32), MarginLoss(loss_margin, adv_temperature) of the split (adv_temperature
 * <= 0: none) + regul_rate (mean h^2 + mean t^2 + mean r^2 + mean w^2) / 4 (TransH.py:98-107).
 * model: MMRE_TRANSH_L1 / MMRE_TRANSH_L2 only (anything else: MMRE_ERR_MODEL; the mmre_ns_* entry
 * points keep answering MMRE_ERR_MODEL for these two). use_model_margin: forward = model_margin - s.
 * The arithmetic is the "TransH training chain" of DESIGN.md §3 (lane partials in increasing
 * element, wave sums): a score here agrees with mmre_transh_score_rows to rounding, not bit for bit.
 * Shapes: 1 <= dim <= 512 and 1 <= neg <= 512 (mmre_transh_ns_supported asks first); n_ent and
 * n_rel below 2^31 and batch (1 + neg) below 2^28; else MMRE_ERR_SHAPE. Checks run before the
 * first launch, in this order: model, null pointers (MMRE_ERR_ARG), shape. Every call only
 * enqueues on `stream`: no allocation, no synchronisation, no read-back; the counters a call
 * needs are zeroed by its own kernels. Ids are trusted to lie inside their tables. */

/* 1 when the kernels exist for (model, dim, neg), else 0. */
int mmre_transh_ns_supported(int model, int dim, int64_t neg);

/* Floats of d_work for both calls below (the same buffer serves a forward and its gradient);
 * -1 for a shape the calls answer MMRE_ERR_SHAPE to. Monotone in every argument. It reserves a
 * record of dim floats for each of the 4 B (1 + K) (row, table) pairs; a sampler-made batch
 * writes about (K + 4) B of them. */
int64_t mmre_transh_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim);

/* d_score[B (1 + K)] <- forward values, d_loss[0] <- the loss (per-positive partials summed in a
 * fixed order: the same bits every run). Two launches. */
int mmre_transh_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                           const float* d_ent, const float* d_rel, const float* d_norm, int64_t n_ent,
                           int64_t n_rel, int dim, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                           int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                           float regul_rate, float* d_score, float* d_loss, float* d_work, void* stream);

/* d_grad_ent[n_ent x dim], d_grad_rel, d_grad_norm[n_rel x dim] <- d(loss)/d(table) times
 * d_grad_loss[0], every row written (rows the batch does not touch: exactly 0), no float atomics,
 * the same bits every run: contribution rows are stored once and summed per table row in an order
 * fixed by the batch indices alone. d_score: what the forward wrote for the same arguments (the
 * tables unchanged since). lr != 0: the owner of a touched row also applies plain SGD,
 * p <- fma(-lr, g, p), in place -- parameters bit-identical to backward() + SGD.step(); the
 * gradient tables are written all the same. lr == 0: the tables are only read. */
int mmre_transh_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                        float* d_rel, float* d_norm, int64_t n_ent, int64_t n_rel, int dim, const int64_t* d_h,
                        const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin,
                        float adv_temperature, float regul_rate, const float* d_score, const float* d_grad_loss,
                        float* d_grad_ent, float* d_grad_rel, float* d_grad_norm, float* d_work, float lr,
                        void* stream);

/* ====================================================================== *
 *  TransD (OpenKE/openke/module/model/TransD.py): link prediction with    *
 *  entities moved by the transfer vectors of the entity and of the        *
 *  query's relation, and predict for arbitrary rows. Models               *
 *  MMRE_TRANSD_L1 / MMRE_TRANSD_L2 (p_norm 1 / 2). Tables: entities and   *
 *  ent_transfer (E, dim_e), relations and rel_transfer (R, dim_r),        *
 *  dim_e >= dim_r (a wider entity row is cut to its first dim_r values,   *
 *  TransD.py:62-68). csrc/transh.hip: TransH's sweep, another prologue.   *
 * ====================================================================== */

/* Bytes of d_work for mmre_transd_evaluate: mmre_transh_workspace at dim = dim_r (the k-major
 * and row-major copies of the narrowed entity table, the relation vectors, the (a, n) table of
 * 2 * n_used * e_pad floats, which holds (-s(e), N(r, e)): s = e . e_p over dim_e (TransD.py:100),
 * N the divisor of both normalisations (TransD.py:99-103, :79-82), the query planes and the listed
 * scores) plus s itself, e_pad floats. 0 for a non-positive size or dim_e < dim_r. */
int64_t mmre_transd_workspace(int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, int64_t n_tiles, int64_t n_used,
                              int64_t n_entries);

/* One TransD link-prediction evaluation, enqueued on `stream`: mmre_transh_evaluate's contract
 * (the Tester loop Tester.py:70-91 around TransD.predict TransD.py:149-155 = forward :112-129
 * with _transfer :94-110 and _calc :78-92) with TransD's tables. d_ent and d_ent_transfer
 * (E, dim_e), d_rel and d_rel_transfer (R, dim_r); d_ent_narrow (E, dim_r), contiguous: the first
 * dim_r columns of d_ent (it may be d_ent itself when dim_e == dim_r). Queries, the plan of
 * one-relation query tiles, filter groups, type masks, pred_kind (0 / 1), d_counts and d_truth as
 * mmre_transh_evaluate takes and writes them. norm_flag: _calc's normalisation of h, r and t;
 * _transfer's own is always applied.
 * Checked in this order: the model (MMRE_ERR_MODEL), null tables and arrays and the sizes
 * (MMRE_ERR_ARG), dim_r <= 0 or dim_e < dim_r (MMRE_ERR_SHAPE), work_bytes (MMRE_ERR_WORKSPACE). */
int mmre_transd_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                         const float* d_ent_transfer, const float* d_rel, const float* d_rel_transfer,
                         const float* d_ent_narrow, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r,
                         const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt, const int8_t* d_qmode,
                         int64_t n_query, const int32_t* d_perm, const int32_t* d_tiles, int64_t n_tiles,
                         const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                         const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                         const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                         int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                         int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* TransD.predict / forward values of the rows (d_h[i], d_r[i], d_t[i]) (TransD.py:112-129,
 * :149-155) from the raw tables, bit for bit what mmre_transd_evaluate scores for the same triple
 * and mode. head_batch != 0: the grouping h + (r - t) of TransD.py:87-88, else (h + r) - t.
 * pred_kind as apply_pred's 0 .. 4 (4 = m - s, forward() of a model with a margin). A row with an
 * id outside the tables gets NaN. */
int mmre_transd_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                           const float* d_ent_transfer, const float* d_rel, const float* d_rel_transfer,
                           int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h,
                           const int64_t* d_r, const int64_t* d_t, int64_t n_rows, int head_batch, float* d_out,
                           void* stream);

/* ---- TransD negative-sampling training (csrc/transh_train.hip) ----
 * The mmre_transh_ns_* contract for TransD.py:94-147: model(data) in 'normal' mode for the
 * B (1 + K) rows of [pos | neg_1 | ... | neg_K], MarginLoss(loss_margin, adv_temperature) +
 * regul_rate (mean h^2 + mean t^2 + mean r^2 + mean h_p^2 + mean t_p^2 + mean r_p^2) / 6, entity
 * means over N dim_e elements and relation means over N dim_r. Tables: d_ent and d_ent_transfer
 * (n_ent, dim_e), d_rel and d_rel_transfer (n_rel, dim_r). model: MMRE_TRANSD_L1 / MMRE_TRANSD_L2
 * only (anything else: MMRE_ERR_MODEL; mmre_ns_* and mmre_transh_ns_* keep refusing these two).
 * The arithmetic is the "TransD training chain" of DESIGN.md §3: a score agrees with
 * mmre_transd_score_rows to rounding, not bit for bit. Shapes: 1 <= dim_r <= dim_e <= 512 and
 * 1 <= neg <= 512 (mmre_transd_ns_supported asks first); n_ent, n_rel and batch as for TransH;
 * else MMRE_ERR_SHAPE. Checks run before the first launch: model, null pointers (MMRE_ERR_ARG),
 * shape. Every call only enqueues on `stream`. Ids are trusted to lie inside their tables. */

/* 1 when the kernels exist for (model, dim_e, dim_r, neg), else 0. */
int mmre_transd_ns_supported(int model, int dim_e, int dim_r, int64_t neg);

/* Floats of d_work for both calls below; -1 for a shape they answer MMRE_ERR_SHAPE to. Monotone in
 * every argument. It reserves 4 dim_e + 2 dim_r floats of records for each of the B (1 + K) rows. */
int64_t mmre_transd_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r);

/* d_score[B (1 + K)] <- forward values, d_loss[0] <- the loss, the same bits every run. Two launches. */
int mmre_transd_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                           const float* d_ent, const float* d_ent_transfer, const float* d_rel,
                           const float* d_rel_transfer, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r,
                           const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg,
                           float loss_margin, float adv_temperature, float regul_rate, float* d_score,
                           float* d_loss, float* d_work, void* stream);

/* The four gradient tables <- d(loss)/d(table) times d_grad_loss[0]: every row written (untouched
 * rows exactly 0), no float atomics, the same bits every run. d_score: what the forward wrote for
 * the same arguments. lr != 0: the owner of a touched row also applies p <- fma(-lr, g, p) in place
 * to all four tables, bit-identical to backward() + SGD.step(); lr == 0: the tables are only read. */
int mmre_transd_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                        float* d_ent_transfer, float* d_rel, float* d_rel_transfer, int64_t n_ent, int64_t n_rel,
                        int dim_e, int dim_r, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                        int64_t batch, int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                        const float* d_score, const float* d_grad_loss, float* d_grad_ent,
                        float* d_grad_ent_transfer, float* d_grad_rel, float* d_grad_rel_transfer, float* d_work,
                        float lr, void* stream);

/* ---- TransR negative-sampling training (csrc/transh_train.hip) ----
 * The mmre_transh_ns_* contract for TransR.py:37-85: model(data) in 'normal' mode for the
 * B (1 + K) rows of [pos | neg_1 | ... | neg_K], MarginLoss(loss_margin, adv_temperature) +
 * regul_rate ((mean h^2 + mean t^2 + mean r^2 + mean M_r^2) / 4)^2 -- squared, as
 * TransR.regularization is -- entity means over N dim_e elements, relation means over N dim_r,
 * matrix means over N dim_e dim_r. Tables: d_ent (n_ent, dim_e), d_rel (n_rel, dim_r) and
 * d_transfer_matrix (n_rel, dim_e * dim_r), row r the row-major dim_e x dim_r matrix M_r.
 * model: MMRE_TRANSR_L1 / MMRE_TRANSR_L2 only (anything else: MMRE_ERR_MODEL; mmre_ns_*,
 * mmre_transh_ns_* and mmre_transd_ns_* keep refusing these two). The arithmetic is the "TransR
 * training chain" of DESIGN.md §3 -- the projection, the entity gradient and the matrix gradient
 * are grouped GEMMs on v_mfma_f32_32x32x2_f32 -- so a score agrees with mmre_transr_score_rows to
 * rounding, not bit for bit. Shapes: 1 <= dim_e, dim_r <= 512 in either order and 1 <= neg <= 512
 * (mmre_transr_ns_supported asks first); n_ent, n_rel and batch as for TransH; else
 * MMRE_ERR_SHAPE. Checks run before the first launch: model, null pointers (MMRE_ERR_ARG), shape.
 * Every call only enqueues on `stream`: launch sizes are upper bounds from (batch, neg, n_rel), and
 * nothing is read back. Ids are trusted to lie inside their tables. */

/* 1 when the kernels exist for (model, dim_e, dim_r, neg), else 0. */
int mmre_transr_ns_supported(int model, int dim_e, int dim_r, int64_t neg);

/* Floats of d_work for both calls below; -1 for a shape they answer MMRE_ERR_SHAPE to. Monotone in
 * every argument. For each of the B (1 + K) rows it reserves two projection slots -- each dim_r
 * floats of projection, dim_r of its gradient and dim_e of entity record -- and dim_r floats of
 * relation record; beside them 4 B (1 + K) / 1024 + 1 partial matrices of dim_e dim_r floats.
 * The forward leaves its index, the projections and the regulariser's value there: the gradient
 * call takes the same d_work, untouched in between. */
int64_t mmre_transr_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r);

/* d_score[B (1 + K)] <- forward values, d_loss[0] <- the loss, the same bits every run. */
int mmre_transr_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                           const float* d_ent, const float* d_rel, const float* d_transfer_matrix, int64_t n_ent,
                           int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h, const int64_t* d_t,
                           const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin,
                           float adv_temperature, float regul_rate, float* d_score, float* d_loss, float* d_work,
                           void* stream);

/* The three gradient tables <- d(loss)/d(table) times d_grad_loss[0]: every row written (untouched
 * rows exactly 0), no float atomics, the same bits every run. d_score and d_work: what the forward
 * wrote for the same arguments. lr != 0: the owner of a touched row also applies p <- fma(-lr, g, p)
 * in place to all three tables, bit-identical to backward() + SGD.step(); lr == 0: the tables are
 * only read. */
int mmre_transr_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                        float* d_rel, float* d_transfer_matrix, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r,
                        const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg,
                        float loss_margin, float adv_temperature, float regul_rate, const float* d_score,
                        const float* d_grad_loss, float* d_grad_ent, float* d_grad_rel,
                        float* d_grad_transfer_matrix, float* d_work, float lr, void* stream);

/* ====================================================================== *
 *  TransR (OpenKE/openke/module/model/TransR.py): link prediction with    *
 *  entities projected by the matrix of the query's relation, and predict  *
 *  for arbitrary rows. Models MMRE_TRANSR_L1 / MMRE_TRANSR_L2 (p_norm     *
 *  1 / 2). Tables: entities (E, dim_e), relations (R, dim_r) and          *
 *  transfer_matrix (R, dim_e * dim_r), row r the row-major dim_e x dim_r  *
 *  matrix M_r (TransR.py:57). 1 <= dim_e, dim_r <= 512 in either order.   *
 *  csrc/transr.hip: the projection on f32 MFMA, a sweep over its planes.  *
 * ====================================================================== */

/* Bytes of d_work for mmre_transr_evaluate: one projected k-major plane of round_up(dim_r, 8) x
 * e_pad floats for EVERY used relation (no chunking: 29 relations x 14,208 entities at
 * dim_r = 200 are 330 MB, all 237 relations of FB15K237 2.8 GB), the relation vectors, the query
 * planes and the listed scores. 0 for a non-positive size or a dim outside 1 .. 512. */
int64_t mmre_transr_workspace(int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, int64_t n_tiles, int64_t n_used,
                              int64_t n_entries);

/* One TransR link-prediction evaluation, enqueued on `stream`: mmre_transh_evaluate's contract
 * (the Tester loop Tester.py:70-91 around TransR.predict TransR.py:97-103 = forward :65-85 with
 * _transfer :55-63 and _calc :37-53) with TransR's tables. Queries, the plan of one-relation query
 * tiles, filter groups, type masks, pred_kind (0 / 1), d_counts and d_truth as
 * mmre_transh_evaluate takes and writes them. norm_flag: _calc's normalisation of the projected
 * h and t and of r; without it the projection is used as it is.
 * Checked in this order, all before any GPU call: the model (MMRE_ERR_MODEL), null tables and
 * arrays and the sizes (MMRE_ERR_ARG), a dim outside 1 .. 512 (MMRE_ERR_SHAPE), work_bytes
 * (MMRE_ERR_WORKSPACE). */
int mmre_transr_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                         const float* d_rel, const float* d_transfer_matrix, int64_t n_ent, int64_t n_rel,
                         int dim_e, int dim_r, const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                         const int8_t* d_qmode, int64_t n_query, const int32_t* d_perm, const int32_t* d_tiles,
                         int64_t n_tiles, const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                         const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                         const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                         int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                         int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* TransR.predict / forward values of the rows (d_h[i], d_r[i], d_t[i]) (TransR.py:65-85, :97-103)
 * from the raw tables, bit for bit what mmre_transr_evaluate scores for the same triple and mode:
 * the projection is the MFMA's fmaf chain in ascending i, restated on the VALU. head_batch != 0:
 * the grouping h + (r - t) of TransR.py:46-47, else (h + r) - t. pred_kind as apply_pred's 0 .. 4
 * (4 = m - s, forward() of a model with a margin). A row with an id outside the tables gets NaN. */
int mmre_transr_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                           const float* d_rel, const float* d_transfer_matrix, int64_t n_ent, int64_t n_rel,
                           int dim_e, int dim_r, const int64_t* d_h, const int64_t* d_r, const int64_t* d_t,
                           int64_t n_rows, int head_batch, float* d_out, void* stream);

/* ====================================================================== *
 *  RESCAL (OpenKE/openke/module/model/RESCAL.py): link prediction with    *
 *  the bilinear score s = sum_i h_i (M_r t)_i, and predict for arbitrary  *
 *  rows. Model MMRE_RESCAL. Tables: entities (E, dim) and rel_matrices    *
 *  (R, dim * dim), row r the row-major matrix M_r[i][j] = row[i * dim +   *
 *  j] (RESCAL.py:18-19). 1 <= dim <= 512. No margin, norm_flag or p_norm. *
 *  csrc/rescal.hip: the planes P_r = E . M_r^T on f32 MFMA, an f32 MFMA   *
 *  sweep whose entity operand is picked per query tile.                   *
 * ====================================================================== */

/* Bytes of d_work for mmre_rescal_evaluate: one k-major plane of round_up(dim, 16) x e_pad floats
 * for EVERY used relation (no chunking), the k-major copy of the entity table (one more such
 * plane), the query planes and the listed scores. FB15K237 (E = 14,541, e_pad = 14,592; all 237
 * relations used) at dim = 50 (kp = 64): 238 x 64 x 14,592 x 4 = 889 MB of planes; 29 used
 * relations: 112 MB. 0 for a non-positive size or a dim outside 1 .. 512. */
int64_t mmre_rescal_workspace(int64_t n_ent, int64_t n_rel, int dim, int64_t n_tiles, int64_t n_used,
                              int64_t n_entries);

/* One RESCAL link-prediction evaluation, enqueued on `stream`: mmre_transr_evaluate's contract
 * (the Tester loop Tester.py:70-91 around RESCAL.predict RESCAL.py:44-46 = -forward :24-32)
 * without norm_flag, margin, the relation vectors and the second dim. The plan differs in one
 * thing: a query tile holds the queries of one KEY 2 * relation + side (side = the queries'
 * qmode: MMRE_HEAD_BATCH 0, MMRE_TAIL_BATCH 1), and d_tiles[3 t] is that key; d_used / d_rel_slot
 * stay per relation. pred_kind 0 (predict = s: the Tester ranks ascending on +s, as the reference
 * does) or 2 (-s). Filter groups, type masks, d_counts and d_truth as mmre_transh_evaluate takes
 * and writes them.
 * Checked in this order, all before any GPU call: the model (MMRE_ERR_MODEL), null tables and
 * arrays and the sizes (MMRE_ERR_ARG), a dim outside 1 .. 512 (MMRE_ERR_SHAPE), work_bytes
 * (MMRE_ERR_WORKSPACE). */
int mmre_rescal_evaluate(int model, int pred_kind, const float* d_ent, const float* d_rel_matrices, int64_t n_ent,
                         int64_t n_rel, int dim, const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                         const int8_t* d_qmode, int64_t n_query, const int32_t* d_perm, const int32_t* d_tiles,
                         int64_t n_tiles, const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                         const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                         const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                         int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                         int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes, void* stream);

/* RESCAL.predict / forward values of the rows (d_h[i], d_r[i], d_t[i]) from the raw tables, bit
 * for bit what mmre_rescal_evaluate scores for the same triple on either side: both chains are the
 * MFMA's fmaf chains, restated on the VALU. pred_kind as apply_pred's 0 .. 4 with margin 0
 * (0 = s, predict; 2 = -s, forward). A row with an id outside the tables gets NaN. */
int mmre_rescal_score_rows(int model, int pred_kind, const float* d_ent, const float* d_rel_matrices, int64_t n_ent,
                           int64_t n_rel, int dim, const int64_t* d_h, const int64_t* d_r, const int64_t* d_t,
                           int64_t n_rows, float* d_out, void* stream);

/* ====================================================================== *
 *  Relation prediction: every test pair (h, t) against every relation.   *
 *  Replaces, per evaluation, the loop getRelBatch (Test.h:55-62) +        *
 *  model.predict on R rows (h, j, t), mode 'normal' + testRel             *
 *  (Test.h:194-228, _find Corrupt.h:166-177) per test triple, and         *
 *  test_relation_prediction (Test.h:329-354).                             *
 * ====================================================================== */

/* Bytes of d_work for mmre_rel_evaluate: the per-relation values that do not depend on the
 * pair, written once per call by a prologue -- TransE: the F.normalize'd relation rows
 * (n_rel x dim floats, used with norm_flag); RotatE: sin and cos of every phase (2 x n_rel x
 * dim floats); DistMult / ComplEx: 0. Negative for an unknown model or a bad shape. */
int64_t mmre_rel_workspace(int model, int64_t n_rel, int dim);

/* For test triple i = (d_qh[i], d_qr[i], d_qt[i]): pred(j) = what model.predict returns for the
 * row (h, j, t) in 'normal' mode, j = 0..n_rel-1 (Test.h:55-62) -- bit for bit the score
 * chain of mmre_ns_forward for that row (the row-wise chain both are built from,
 * csrc/row_chain.h) followed by the pred_kind / margin
 * transform of mmre_link_truth (for TransE with a model margin and RotatE, mmre_ns_forward's
 * m - s IS that transform's inner step: pred_kind 1 / 3). Then, Test.h:200-213:
 *   d_counts[0][i] = #{ j != r : pred(j) < pred(r) }   strict: ties favour the truth, and a NaN
 *                                                      on either side never counts;
 *   d_counts[1][i] = the same without the relations listed for query i (the known relations
 *                    of (h, t) in train + valid + test; a list may hold r itself, relations that
 *                    do not beat the truth and ids outside [0, n_rel), which are ignored; no
 *                    relation twice);
 *   d_truth[i]     = pred(r);  d_scores[i * n_rel + j] = pred(j) when d_scores is given.
 * d_filt_off[n_query + 1] (int64) / d_filt_ids (int32): per-query CSR; NULL/NULL = no filter
 * (both columns equal). Tables as mmre_ns_forward takes them (RotatE entities (E, 2 dim)).
 * A query whose h, t or r is out of range reads nothing: counts 0, truth NaN, scores NaN.
 * Enqueues a prologue (TransE with norm_flag, RotatE) and one sweep launch; any n_rel >= 1.
 * Checked before any launch: MMRE_ERR_MODEL for an unknown model, MMRE_ERR_SHAPE for dim > 512,
 * MMRE_ERR_ARG for a null table / output, sizes < 1, n_query < 0, pred_kind outside 0..4, one
 * of the two filter arrays without the other, MMRE_ERR_WORKSPACE for a d_work smaller than
 * mmre_rel_workspace. n_query == 0 is a successful no-op. */
int mmre_rel_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                      const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                      int64_t n_rel, int dim, float phase_denom, const int64_t* d_qh, const int64_t* d_qr,
                      const int64_t* d_qt, int64_t n_query, const int64_t* d_filt_off, const int32_t* d_filt_ids,
                      int32_t* d_counts, float* d_truth, float* d_scores, void* d_work, int64_t work_bytes,
                      void* stream);

/* testRel's accumulation + test_relation_prediction (Test.h:215-225, :329-344), host side, in
 * query order with the reference's widths (float accumulators; `+= 1.0 / (count + 1)` a double
 * quotient added to a float; then / (float)n). Counts: int32, raw count of query i at
 * h_counts[i], filtered at h_counts[stride + i].
 * h_out[10] = {mrr, mr, hit10, hit3, hit1} x {filter, raw}. */
int mmre_rel_metrics(const int32_t* h_counts, int64_t n, int64_t stride, float* h_out);

/* ====================================================================== *
 *  Triple classification: one corrupted copy of every test triple         *
 *  (getNegTest / getTestBatch, Test.h:393-422), model.predict on both in   *
 *  'normal' mode, and the score threshold that separates them best         *
 *  (Tester.py:93-151 get_best_threshlod / run_triple_classification).      *
 *  Every entry: explicit stream, no allocation or synchronisation inside,  *
 *  every argument checked before any launch, n == 0 a successful no-op.    *
 * ====================================================================== */

/* getNegTest on the GPU, bit-exact with Base.so. For test triple i, in testList order, thread 0's
 * LCG (Random.h:18-29) is drawn exactly twice: the coin `randd(0) % 1000 < 500` (true: the TAIL is
 * replaced by corrupt_head(0, h, r); false: the HEAD by corrupt_tail(0, t, r)) and the corruption's
 * one rand_max, filtered against the TRAIN lists only. Triple i therefore starts from `state`
 * advanced by 2 i draws and all triples are sampled in parallel; the state after the call is
 * mmre_tc_advance(state, n). `state`: thread 0's state before the call. Index arrays: the
 * Reader.h:53-160 train index as mmre_sampler_openke takes it (int64 rows (h, r, t); head_hrt
 * sorted (h, r, t), tail_hrt (t, r, h); lef / rig per entity, rig = -1 for an entity absent from
 * that side). Outputs int64 d_neg_h[n], d_neg_t[n]; the negative's relation is the positive's.
 * Pinned where the reference is undefined: when the kept entity never occurs on that side of a train
 * triple, Corrupt.h computes ll = -1, rr = 0 and reads trainHead[-1]; here nothing is read, the
 * modulus is the one the reference computes (n_ent - 2) and the draw is returned unchanged. Every
 * other quirk of Corrupt.h is reproduced (a relation between, below or above the kept entity's
 * relations; that includes the one draw Corrupt.h shifts to n_ent itself, when the relation falls
 * into an empty block whose neighbouring rows' values descend -- mmre_tc_scores gives such a row
 * NaN). A test triple whose h or t is outside [0, n_ent) gives neg_h = neg_t = -1.
 * MMRE_ERR_ARG: a null index / triple / output array, train_total < 1, n_ent < 3, n < 0;
 * MMRE_ERR_SHAPE: n > INT32_MAX. */
int mmre_tc_negatives(const int64_t* d_head_hrt, const int64_t* d_tail_hrt, const int64_t* d_lef_head,
                      const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                      int64_t train_total, int64_t n_ent, const int64_t* d_test_h, const int64_t* d_test_r,
                      const int64_t* d_test_t, int64_t n, uint64_t state, int64_t* d_neg_h, int64_t* d_neg_t,
                      void* stream);
/* Host: thread 0's state after getNegTest over n test triples (2 n draws). */
uint64_t mmre_tc_advance(uint64_t state, int64_t n);

/* model.predict ('normal' mode) of n positive rows and their n negative rows: bit for bit the score
 * chain of mmre_ns_forward for each row followed by the pred_kind / margin transform of
 * mmre_link_truth -- the contract of mmre_rel_evaluate. One wave per pair of rows; a table row the
 * two share is loaded once. d_neg_r NULL: the negatives' relations are the positives'. Tables as
 * mmre_ns_forward takes them (RotatE entities (E, 2 dim)). A row with an id out of range reads
 * nothing and scores NaN. MMRE_ERR_MODEL: unknown model; MMRE_ERR_SHAPE: dim > 512, n > INT32_MAX;
 * MMRE_ERR_ARG: dim < 1, a null table / triple / output array, ComplEx without its imaginary tables,
 * RotatE with phase_denom 0 or NaN, n_ent < 1, n_rel < 1, n < 0, pred_kind outside 0..4. */
int mmre_tc_scores(int model, int norm_flag, int pred_kind, float margin, const float* d_ent, const float* d_ent_im,
                   const float* d_rel, const float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                   float phase_denom, const int64_t* d_pos_h, const int64_t* d_pos_r, const int64_t* d_pos_t,
                   const int64_t* d_neg_h, const int64_t* d_neg_r, const int64_t* d_neg_t, int64_t n,
                   float* d_pos_scores, float* d_neg_scores, void* stream);

/* Bytes of d_work for a threshold search over n_pos + n_neg scores (16 + 8 per score); negative for
 * sizes mmre_tc_threshold refuses. */
int64_t mmre_tc_threshold_workspace(int64_t n_pos, int64_t n_neg);
/* The threshold search of get_best_threshlod, without a sort. For a candidate c among the scores
 * P(c) = #{positives <= c}, A(c) = P(c) + #{negatives <= c}; the rule `score <= c` classifies
 * (2 P + F - A) of the T = n_pos + n_neg scores correctly (F = n_neg), so the winner maximises the
 * integer 2 P - A and, among equal maxima, is the smallest c (the reference's strict `>`).
 *   have_threshold == 0: d_out = {bits of the best threshold (float, low 32 bits), P, A, n_nan}
 *   have_threshold != 0: the same at `threshold`; no search runs, d_work may be NULL.
 * The accuracy is mmre_tc_accuracy(P, A, n_pos, n_neg) on the host. (n_pos + n_neg)^2 compares:
 * quadratic, meant for test sets up to some 10^5 scores. Integer atomics only: identical every run.
 * Pinned where the reference is undefined or unstable:
 *   ties   numpy's argsort is unstable, so inside a group of equal scores the reference's running
 *          value depends on the sort and its res_mx may exceed what any threshold attains; here a
 *          group counts at its end only. With pairwise-distinct scores both agree exactly. -0 and +0
 *          are one group, reported as +0.
 *   NaN    a NaN score is never <= anything: classified negative, never a candidate, counted in T and
 *          in F or the positives' total, and in n_nan. No non-NaN score at all: threshold NaN, P = A = 0.
 *   no score above the threshold (the reference's loop leaves `acc` unbound): A = all non-NaN scores.
 * The lengths may differ (get_best_threshlod is generic in `ans`); either may be 0.
 * MMRE_ERR_ARG: a negative length, a null array of positive length, a null d_out, a null d_work for a
 * search; MMRE_ERR_SHAPE: n_pos + n_neg > 2^30; MMRE_ERR_WORKSPACE: work_bytes too small.
 * n_pos + n_neg == 0: no-op, d_out untouched. */
int mmre_tc_threshold(const float* d_pos_scores, int64_t n_pos, const float* d_neg_scores, int64_t n_neg,
                      int have_threshold, float threshold, int64_t* d_out, void* d_work, int64_t work_bytes,
                      void* stream);
/* Host: (2 P + F - A) / T in double -- the reference's Python float, bit for bit. NaN for T == 0. */
double mmre_tc_accuracy(int64_t p, int64_t a, int64_t n_pos, int64_t n_neg);

/* The three stages enqueued in one call: mmre_tc_negatives on the test triples, mmre_tc_scores on
 * them and their negatives, mmre_tc_threshold over the two score arrays (n_pos = n_neg = n;
 * d_work >= mmre_tc_threshold_workspace(n, n) unless a threshold is given). Outputs: d_neg_h,
 * d_neg_t, d_pos_scores, d_neg_scores (n each) and d_out[4]. Checks, in order: mmre_tc_scores',
 * mmre_tc_negatives', mmre_tc_threshold's. */
int mmre_tc_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                     const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent, int64_t n_rel,
                     int dim, float phase_denom, const int64_t* d_head_hrt, const int64_t* d_tail_hrt,
                     const int64_t* d_lef_head, const int64_t* d_rig_head, const int64_t* d_lef_tail,
                     const int64_t* d_rig_tail, int64_t train_total, const int64_t* d_test_h,
                     const int64_t* d_test_r, const int64_t* d_test_t, int64_t n, uint64_t state,
                     int have_threshold, float threshold, int64_t* d_neg_h, int64_t* d_neg_t, float* d_pos_scores,
                     float* d_neg_scores, int64_t* d_out, void* d_work, int64_t work_bytes, void* stream);

/* ====================================================================== *
 *  OpenKE negative sampler (Base.cpp:78-197 sampling/getBatch,           *
 *  Corrupt.h:7-163 corrupt_head/tail/rel, Random.h:11-29).               *
 *  Bit-exact: each positive's LCG state is reached by affine jump-ahead  *
 *  from its thread's seed, so the whole batch samples in parallel.       *
 * ====================================================================== */
/* glibc rand() stream after srand(1) (randReset's seeds, Random.h:11-15). */
int mmre_glibc_rand(int64_t skip, int64_t n, int64_t* h_out);
/* LCG draws one positive consumes in getBatch (Base.cpp:103-146). */
int64_t mmre_sampler_draws_per_positive(int64_t neg_rate, int64_t neg_rel_rate, int64_t mode);
/* Advance host-side per-thread LCG states by one sampling() call. */
int mmre_sampler_advance(uint64_t* h_seeds, int64_t work_threads, int64_t batch_size, int64_t neg_rate,
                         int64_t neg_rel_rate, int64_t mode);
/* The same advance applied to device-resident states on a stream, so a training loop keeps
 * the seeds in HBM (no host copy per batch; the sequence can be captured in a hipGraph). */
int mmre_sampler_advance_device(uint64_t* d_seeds, int64_t work_threads, int64_t batch_size, int64_t neg_rate,
                                int64_t neg_rel_rate, int64_t mode, void* stream);
/* One sampling() call on the GPU. Index arrays are the Reader.h:53-160 train
 * index (int64 rows (h, r, t); head_hrt sorted (h,r,t), tail_hrt (t,r,h),
 * rel_hrt (h,t,r); lef/rig per entity). d_left_mean/d_right_mean NULL = bern off.
 * d_seeds: per-thread states BEFORE this call (device copy). Outputs int64/f32,
 * length batch_size * (1 + neg_rate + neg_rel_rate), negative k at [k*B, (k+1)*B). */
int mmre_sampler_openke(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                        const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                        const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                        const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                        const float* d_right_mean, int64_t n_ent, int64_t n_rel, const uint64_t* d_seeds,
                        int64_t work_threads, int64_t batch_size, int64_t neg_rate, int64_t neg_rel_rate,
                        int64_t mode, int64_t* d_batch_h, int64_t* d_batch_t, int64_t* d_batch_r,
                        float* d_batch_y, void* stream);

/* The (h, r) block of head_hrt and the (t, r) block of tail_hrt of every train row i, with
 * their first / last tail / head: int32 d_blocks[n_train][8] = (ll, rr, tail[ll], tail[rr],
 * ll', rr', head[ll'], head[rr']). What corrupt_head / corrupt_tail (Corrupt.h:7-81) look up
 * before their draw, built once per train index (n_train = rows of d_train_list). */
int mmre_sampler_blocks(const int64_t* d_train_list, int64_t n_train, const int64_t* d_head_hrt,
                        const int64_t* d_tail_hrt, const int64_t* d_lef_head, const int64_t* d_rig_head,
                        const int64_t* d_lef_tail, const int64_t* d_rig_tail, int32_t* d_blocks, void* stream);
/* mmre_sampler_openke reading the kept (entity, relation)'s block from d_blocks for train
 * rows i < n_blocks (bit-identical batches: the same blocks, found without the two binary
 * searches per negative); d_blocks NULL / n_blocks 0 is mmre_sampler_openke itself. */
int mmre_sampler_openke_blocked(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                                const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                                const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                                const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                                const float* d_right_mean, int64_t n_ent, int64_t n_rel, const uint64_t* d_seeds,
                                int64_t work_threads, int64_t batch_size, int64_t neg_rate, int64_t neg_rel_rate,
                                int64_t mode, const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h,
                                int64_t* d_batch_t, int64_t* d_batch_r, float* d_batch_y, void* stream);
/* mmre_sampler_openke_blocked that also leaves d_seeds advanced for the next call (what
 * mmre_sampler_advance_device does, without a launch of its own): the last workgroup to finish
 * -- an integer ticket in d_ticket, zero before the first call and reset by each call --
 * writes the advanced states once every workgroup has read the old ones. One launch per
 * batch, as Base.cpp's sampling is one call (Base.cpp:161-197). */
int mmre_sampler_openke_step(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                             const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                             const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                             const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                             const float* d_right_mean, int64_t n_ent, int64_t n_rel, uint64_t* d_seeds,
                             int64_t work_threads, int64_t batch_size, int64_t neg_rate, int64_t neg_rel_rate,
                             int64_t mode, const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h,
                             int64_t* d_batch_t, int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket,
                             void* stream);

/* importProb (Reader.h:26-49): kl_prob.txt at `path` (n_rel x (n_rel - 1) floats, fscanf
 * "%f") -> h_prob[n_rel][n_rel - 1] = exp(-kl / temperature) / row sum, in float. Host only. */
int mmre_import_prob(const char* path, int64_t n_rel, float temperature, float* h_prob);
/* mmre_sampler_openke_step with sampling(..., p = true): relation negatives drawn by
 * corrupt_rel's KL-weighted path (Corrupt.h:111-147) from d_rel_prob = mmre_import_prob's
 * table on the device; d_ticket may be NULL (seeds then left as they were, like
 * mmre_sampler_openke_blocked). Replaces Base.cpp:142's corrupt_rel(..., p). */
int mmre_sampler_openke_p(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                          const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                          const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                          const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                          const float* d_right_mean, int64_t n_ent, int64_t n_rel, uint64_t* d_seeds,
                          int64_t work_threads, int64_t batch_size, int64_t neg_rate, int64_t neg_rel_rate,
                          int64_t mode, const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h,
                          int64_t* d_batch_t, int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket,
                          const float* d_rel_prob, void* stream);

/* The repo's per-edge filtered sampler (module/NegativeSampling.py:114-140,
 * 321-375): per positive edge b (local ids d_eh/d_et, relation d_er), neg
 * negatives split head/tail by Bernoulli(0.5); candidates uniform over the local
 * node list [0, n_local) (NegativeSampling.py:210), rejected when their global id
 * (d_local_to_global, NULL = identity) is a known head of (t, r) (key t*n_rel+r in
 * the d_hf_* CSR over sorted keys) or a known tail of (h, r) (d_tf_*), distinct
 * within the positive. Counter-based (SplitMix64) draws from `seed` replace the
 * reference's unseeded Python `random` (P13). Output [pos | neg_1 | ... | neg_k],
 * head corruptions first, then tails.
 * Exhaustion: a negative whose 4,096 draws were all rejected is found by one scan of
 * [0, n_local) from its last draw. A filtered node is never emitted while an
 * allowed local node exists; the same-side negatives of a positive are distinct
 * whenever that side has at least as many allowed nodes as negatives, otherwise
 * every allowed node of the side is used once before any repeats (the reference
 * resamples until it has enough, :333-347). With no allowed node at all -- where
 * the reference never returns -- the last draw is emitted. */
int mmre_sampler_repo(const int64_t* d_eh, const int64_t* d_et, const int64_t* d_er, int64_t batch, int64_t neg,
                      int64_t n_local, const int64_t* d_local_to_global, int64_t n_rel, const int64_t* d_hf_keys,
                      const int64_t* d_hf_off, const int64_t* d_hf_vals, int64_t hf_n, const int64_t* d_tf_keys,
                      const int64_t* d_tf_off, const int64_t* d_tf_vals, int64_t tf_n, uint64_t seed,
                      int filter_flag, int64_t* d_out_h, int64_t* d_out_t, int64_t* d_out_r, void* stream);

/* Plain SGD step p <- p - lr * g (one fma per element) over `count` <= 8 float32 tensors in
 * one launch; params[t] / grads[t] 16-B aligned, numel[t] elements each. Replaces the
 * reference optimizer's step (optim.SGD without momentum / weight decay, OpenKE
 * Trainer.py:82-86) after the fused gradient. */
int mmre_sgd_step(float* const* params, const float* const* grads, const int64_t* numel, int count, float lr,
                  void* stream);

/* Adagrad step (torch.optim.Adagrad with lr_decay 0, weight_decay 0, maximize False -- the
 * optimizer of OpenKE/examples/train_distmult_WN18RR.py and train_complex_WN18RR.py through
 * Trainer.py:66-72) over `count` <= 8 float32 tensors in one launch, per element
 *   sum <- sum + g * g;  std = sqrt(sum) + eps;  p <- p + (g * -lr) / std
 * with every operation rounded once (the product before the add; IEEE sqrt and quotient): torch's foreach step on
 * this ROCm build bit for bit (scripts/probes/adagrad_rounding.py). sums[t] is torch's
 * state["sum"]. params[t] / grads[t] / sums[t] 16-B aligned, numel[t] elements each;
 * MMRE_ERR_ARG otherwise, or for count outside 1..8 (checked before anything is launched). */
int mmre_adagrad_step(float* const* params, const float* const* grads, float* const* sums, const int64_t* numel,
                      int count, float lr, float eps, void* stream);

/* ====================================================================== *
 *  Negative-sampling margin loss, fused (OpenKE strategy/NegativeSampling *
 *  .py:23-32 + loss/MarginLoss.py:24-28 + model forward/regularization;   *
 *  repo module/NegativeSampling.py:204-229,307-314 + module/loss.py:19-23)*
 *  Rows: N = B*(1+k), positive b at row b, its negative j at row b+(j+1)B.*
 *  Entity rows come from d_ent[idx], relation rows from d_rel[ridx].       *
 * ====================================================================== */
/* Forward. d_score[N]: model(data) (TransE.py:78-90 etc.); d_loss[0]: margin
 * loss (+ regul_rate * regularization when regul_rate != 0). adv_temperature
 * <= 0 disables the self-adversarial weights. d_work: >= mmre_ns_workspace(B, k) floats. */
int64_t mmre_ns_workspace(int64_t batch, int64_t neg);
int mmre_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                    const float* d_ent_im, const float* d_rel, const float* d_rel_im, int dim, float phase_denom,
                    const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg,
                    float loss_margin, float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                    float* d_work, void* stream);
/* Backward of the forward above: WRITES every row of the dense gradient tables with
 * d(loss)/d(table) * d_grad_loss[0] (d_grad_loss NULL means 1). Deterministic, no float
 * atomics: each scored row files its h / r / t gradient rows as slot records in its table
 * rows' buckets and one wave per table row sums them in batch order (bit-identical run to
 * run). d_work: >= mmre_rows_backward_workspace(model, batch * (1 + neg), n_ent, n_rel, dim)
 * floats. dim <= 2048 and neg <= 512 (mmre_ns_rows_supported), MMRE_ERR_SHAPE otherwise, before
 * anything is launched. */
int64_t mmre_rows_backward_workspace(int model, int64_t n_rows, int64_t n_ent, int64_t n_rel, int dim);
int mmre_ns_backward(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                     const float* d_ent_im, const float* d_rel, const float* d_rel_im, int dim,
                     float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch,
                     int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                     const float* d_score, const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_im,
                     float* d_grad_rel, float* d_grad_rel_im, int64_t n_ent, int64_t n_rel, float* d_work,
                     int64_t work_floats, void* stream);

/* Training: forward, loss and d(loss)/d(tables). mmre_ns_fused_forward computes the scores and
 * the loss and keeps what the gradient needs in d_work; mmre_ns_fused_grad then WRITES every
 * row of the dense gradient tables (no caller fill): d(loss)/d(table) * d_grad_loss[0] (NULL:
 * 1). mmre_ns_forward_backward is the two in sequence with an upstream gradient of 1. No float
 * atomics for any model -- every gradient contribution goes to a SLOT whose id is dropped into
 * its table row's bucket (integer atomics), and one wave per table row sums its bucket in
 * increasing slot id (batch order): bit-reproducible gradients.
 *   TransE (L1 / L2, dim <= 512, neg <= 32): a norm pre-pass, the fused kernel (each row read
 *   once, scores, loss partials and the contributions of a positive's group of rows), one
 *   workgroup for batches that are not OpenKE-shaped and the fixed-order loss reduction; the
 *   gradient is the row-owner pass.
 *   DistMult / ComplEx / RotatE (dim <= 512): the scoring pass + the loss reduction; the
 *   gradient is a slot pass (one wave per positive) + the row-owner pass.
 * Replaces strategy NegativeSampling.forward + loss.backward() (NegativeSampling.py:23-32,
 * Trainer.py:43-54) for one batch. d_work: >= mmre_ns_fused_workspace(model, norm_flag, B, k,
 * n_ent, n_rel, dim) floats, kept between the two calls.
 * The fused entry points (and the one-call steps below) serve exactly the shapes for which
 * mmre_ns_fused_supported returns 1, and return MMRE_ERR_SHAPE for any other before anything is
 * launched -- the forward too: no loss is returned whose gradient call would then fail. */
/* Host-only, no device needed. 1 when the fused entry points have kernels for (model, dim, neg,
 * loss_kind = MMRE_LOSS_*), else 0 (an unknown model or loss kind, dim <= 0 or neg < 0 included):
 *   TransE L1 / L2: the margin loss, dim <= 512, neg <= 32;
 *   DistMult / ComplEx / RotatE: any of the three losses, dim <= 512, neg <= 512.
 * Every other training shape is the rows path's (mmre_ns_forward[_ex] + mmre_ns_backward[_ex]):
 * mmre_ns_rows_supported is 1 for 0 < dim <= 2048 and 0 <= neg <= 512, any model, any loss. */
int mmre_ns_fused_supported(int model, int dim, int64_t neg, int loss_kind);
int mmre_ns_rows_supported(int dim, int64_t neg);
int64_t mmre_ns_fused_workspace(int model, int norm_flag, int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel,
                                int dim);
int mmre_ns_fused_forward(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                          const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                          int64_t n_rel, int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t,
                          const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                          float regul_rate, float* d_score, float* d_loss, float* d_work, void* stream);
int mmre_ns_fused_grad(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                       const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent, int64_t n_rel,
                       int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                       int64_t batch, int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                       const float* d_score, const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_im,
                       float* d_grad_rel, float* d_grad_rel_im, float* d_work, void* stream);
/* mmre_ns_fused_grad with the optimizer's plain SGD step fused in (OpenKE Trainer.py:82-86,
 * optim.SGD without momentum / weight decay; mmre.optim.SGD's fused mode): the gradient tables
 * are written as above AND every parameter row with a nonzero gradient becomes
 * fma(-lr, g, p) -- torch's SGD arithmetic, bit for bit -- in the same pass (rows outside the
 * batch keep p = p - lr 0). The tables are updated in place (d_ent ... are the parameters). */
int mmre_ns_fused_grad_sgd(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                           float* d_ent_im, float* d_rel, float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                           float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                           int64_t batch, int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                           const float* d_score, const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_im,
                           float* d_grad_rel, float* d_grad_rel_im, float* d_work, float lr, void* stream);
int mmre_ns_forward_backward(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                             const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                             int64_t n_rel, int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t,
                             const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                             float regul_rate, float* d_score, float* d_loss, float* d_grad_ent, float* d_grad_ent_im,
                             float* d_grad_rel, float* d_grad_rel_im, float* d_work, void* stream);

/* One OpenKE training step for TransE (Trainer.train_one_step, Trainer.py:43-54: Base.cpp:161-197's
 * sampling + strategy/NegativeSampling + MarginLoss forward/backward + optim.SGD): the sampler
 * arguments of mmre_sampler_openke_step (neg_rel_rate 0; d_ticket required; the batch lands in
 * d_batch_*), then the loss arguments of mmre_ns_fused_forward / mmre_ns_fused_grad_sgd (upstream
 * gradient 1; d_ent / d_rel updated in place by fma(-lr, g, p)). Values bit-identical to those
 * three calls in sequence; three launches instead of five (the sampler and the pre-pass share one
 * grid, the loss reduction rides in the gradient's). d_work: mmre_ns_fused_workspace. Only the
 * fused TransE shapes (dim <= 512, neg <= 32): MMRE_ERR_SHAPE otherwise. */
int mmre_ns_step_openke(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                        const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                        const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                        const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                        const float* d_right_mean, uint64_t* d_seeds, int64_t work_threads, int64_t mode,
                        const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h, int64_t* d_batch_t,
                        int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket, int model, int norm_flag,
                        float* d_ent, float* d_rel, int64_t n_ent, int64_t n_rel, int dim, int64_t batch, int64_t neg,
                        float loss_margin, float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                        float* d_grad_ent, float* d_grad_rel, float* d_work, float lr, void* stream);

/* The same step, pipelined across calls (a prefetching data loader; Trainer.py:43-54 over the
 * loader's batches): the row owner of this step also samples the NEXT batch into d_next_* (the
 * sampler's seeds advance by that batch) and writes the norms / normalised copies of the rows it
 * updates -- the pre-pass the next step needs (a row without gradient keeps its parameters, so
 * its entries stay current) -- and zeroes the other parity's slot counts. prepared: bit 0 =
 * d_batch_* already holds this step's batch (the previous call's d_next_*), bit 1 = the pre-pass
 * and the slot counts of `parity` are current (the previous call was this one's other parity,
 * d_ent / d_rel / d_work unchanged since). prepared = 3 skips the first launch; otherwise it
 * samples d_batch_* (bit 0 clear) and runs the pre-pass, as mmre_ns_step_openke (whose d_work
 * layout this shares). d_next_h == NULL: no next batch (the next call: prepared bit 0 clear).
 * Batches, losses, gradients, parameters and seeds are bit-identical to consecutive
 * mmre_ns_step_openke calls. */
int mmre_ns_step_openke_pipe(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                             const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                             const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                             const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                             const float* d_right_mean, uint64_t* d_seeds, int64_t work_threads, int64_t mode,
                             const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h, int64_t* d_batch_t,
                             int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket, int model, int norm_flag,
                             float* d_ent, float* d_rel, int64_t n_ent, int64_t n_rel, int dim, int64_t batch,
                             int64_t neg, float loss_margin, float adv_temperature, float regul_rate, float* d_score,
                             float* d_loss, float* d_grad_ent, float* d_grad_rel, float* d_work, float lr,
                             void* stream, int64_t prepared, int64_t parity, int64_t* d_next_h, int64_t* d_next_t,
                             int64_t* d_next_r, float* d_next_y);

/* The one-call training step for DistMult / ComplEx / RotatE (OpenKE Trainer.train_one_step over
 * the loader's sampling, NegativeSampling + MarginLoss, plain SGD; the models' own scoring as in
 * mmre_ns_fused_forward: d_ent_im / d_rel_im for ComplEx, model_margin / phase_denom for RotatE):
 * [sampler, unless prepared bit 0 says d_batch_* was drawn by the previous call] -> the forward
 * (scores + loss partials) -> the slot records -> the row owner (gradient + SGD), whose grid also
 * reduces the loss into d_loss and, with d_next_h, draws the next batch into d_next_*. Values
 * bit-identical to mmre_sampler_openke_step + mmre_ns_fused_forward + mmre_ns_fused_grad_sgd;
 * three launches a step instead of five. d_work: mmre_ns_fused_workspace. dim <= 512. */
int mmre_ns_step_openke_gen_pipe(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                                 const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                                 const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                                 const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                                 const float* d_right_mean, uint64_t* d_seeds, int64_t work_threads, int64_t mode,
                                 const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h, int64_t* d_batch_t,
                                 int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket, int model,
                                 float model_margin, int use_model_margin, float* d_ent, float* d_ent_im,
                                 float* d_rel, float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                                 float phase_denom, int64_t batch, int64_t neg, float loss_margin,
                                 float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                                 float* d_grad_ent, float* d_grad_ent_im, float* d_grad_rel, float* d_grad_rel_im,
                                 float* d_work, float lr, void* stream, int64_t prepared, int64_t* d_next_h,
                                 int64_t* d_next_t, int64_t* d_next_r, float* d_next_y);

/* ---- Other losses and optimizers: the `_ex` twin of each entry point above takes one more
 * argument, a const mmre_ns_opts_t* (NULL: the entry point without the suffix, which is a
 * one-line wrapper around its twin; values unchanged).
 *
 * loss_kind. MMRE_LOSS_MARGIN: as above. With p_b positive b's score, n_bj its k negatives,
 * B = batch, T = adv_temperature:
 *   MMRE_LOSS_SOFTPLUS (OpenKE SoftplusLoss.py:19-26, nn.Softplus(): sp(x) = x > 20 ? x :
 *     log1p(exp(x))):        L = ( (1/B) sum_b sp(-p_b) + sum_b sum_j c_bj sp(n_bj) ) / 2
 *   MMRE_LOSS_SIGMOID (SigmoidLoss.py:19-26, nn.LogSigmoid(): ls(x) = min(x, 0) -
 *     log1p(exp(-|x|))):     L = -( (1/B) sum_b ls(p_b) + sum_b sum_j c_bj ls(-n_bj) ) / 2
 *   c_bj = 1 / (B k), or with T > 0 softmax_j(+T n_bj) / B, detached (MarginLoss's weights
 *   use -T n). dL/dp_b = -sigma(-p_b) / (2 B), dL/dn_bj = c_bj sigma(n_bj) / 2 (softplus:
 *   sigma is exactly 1 past the threshold). + regul_rate * regularization exactly as for the
 *   margin loss; loss_margin is ignored (these losses have no such term). Evaluated without
 *   overflow for any finite score. An unknown kind: MMRE_ERR_ARG.
 *   Models: every model through mmre_ns_forward_ex / mmre_ns_backward_ex; DistMult, ComplEx and
 *   RotatE through the fused entry points and the one-call step as well. TransE's fused kernel
 *   is margin-only: the fused entry points return MMRE_ERR_MODEL for TransE with another loss
 *   (callers route it to mmre_ns_forward_ex / mmre_ns_backward_ex; mmre.ns does).
 *
 * optimizer (mmre_ns_fused_grad_sgd_ex, mmre_ns_step_openke_gen_pipe_ex; DistMult / ComplEx /
 * RotatE). MMRE_OPT_SGD: p <- fma(-lr, g, p) as above. MMRE_OPT_ADAGRAD: the row owner
 * applies mmre_adagrad_step's arithmetic to every table row with a slot -- sum <- sum + g * g,
 * p <- p + (g * -lr) / (sqrt(sum) + eps) -- reading and writing the row of the sum
 * table (torch's state["sum"], shaped like its parameter table): d_sum_ent [n_ent, dim] (RotatE
 * [n_ent, 2 dim]), d_sum_rel [n_rel, dim], d_sum_ent_im / d_sum_rel_im for ComplEx. Rows
 * without a slot have a zero gradient, for which the step leaves p and sum unchanged, so they
 * are skipped. Missing sum tables, or Adagrad on TransE: MMRE_ERR_ARG. The workspaces are those
 * of the entry points without the suffix. */
typedef struct mmre_ns_opts {
  int loss_kind; /* MMRE_LOSS_* */
  int optimizer; /* MMRE_OPT_* */
  float eps;     /* Adagrad's eps */
  float* d_sum_ent;
  float* d_sum_ent_im;
  float* d_sum_rel;
  float* d_sum_rel_im;
} mmre_ns_opts_t;

int mmre_ns_forward_ex(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                       const float* d_ent_im, const float* d_rel, const float* d_rel_im, int dim, float phase_denom,
                       const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg,
                       float loss_margin, float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                       float* d_work, void* stream, const mmre_ns_opts_t* opts);
int mmre_ns_backward_ex(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                        const float* d_ent_im, const float* d_rel, const float* d_rel_im, int dim,
                        float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch,
                        int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                        const float* d_score, const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_im,
                        float* d_grad_rel, float* d_grad_rel_im, int64_t n_ent, int64_t n_rel, float* d_work,
                        int64_t work_floats, void* stream, const mmre_ns_opts_t* opts);
int mmre_ns_fused_forward_ex(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                             const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                             int64_t n_rel, int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t,
                             const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                             float regul_rate, float* d_score, float* d_loss, float* d_work, void* stream,
                             const mmre_ns_opts_t* opts);
int mmre_ns_fused_grad_ex(int model, int norm_flag, float model_margin, int use_model_margin, const float* d_ent,
                          const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                          int64_t n_rel, int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t,
                          const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                          float regul_rate, const float* d_score, const float* d_grad_loss, float* d_grad_ent,
                          float* d_grad_ent_im, float* d_grad_rel, float* d_grad_rel_im, float* d_work, void* stream,
                          const mmre_ns_opts_t* opts);
int mmre_ns_fused_grad_sgd_ex(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                              float* d_ent_im, float* d_rel, float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                              float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                              int64_t batch, int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                              const float* d_score, const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_im,
                              float* d_grad_rel, float* d_grad_rel_im, float* d_work, float lr, void* stream,
                              const mmre_ns_opts_t* opts);
int mmre_ns_step_openke_gen_pipe_ex(const int64_t* d_train_list, int64_t train_total, const int64_t* d_head_hrt,
                                    const int64_t* d_tail_hrt, const int64_t* d_rel_hrt, const int64_t* d_lef_head,
                                    const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                                    const int64_t* d_lef_rel, const int64_t* d_rig_rel, const float* d_left_mean,
                                    const float* d_right_mean, uint64_t* d_seeds, int64_t work_threads, int64_t mode,
                                    const int32_t* d_blocks, int64_t n_blocks, int64_t* d_batch_h, int64_t* d_batch_t,
                                    int64_t* d_batch_r, float* d_batch_y, int32_t* d_ticket, int model,
                                    float model_margin, int use_model_margin, float* d_ent, float* d_ent_im,
                                    float* d_rel, float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                                    float phase_denom, int64_t batch, int64_t neg, float loss_margin,
                                    float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                                    float* d_grad_ent, float* d_grad_ent_im, float* d_grad_rel, float* d_grad_rel_im,
                                    float* d_work, float lr, void* stream, int64_t prepared, int64_t* d_next_h,
                                    int64_t* d_next_t, int64_t* d_next_r, float* d_next_y,
                                    const mmre_ns_opts_t* opts);

/* model(data) in 'normal' mode for n_rows arbitrary rows is mmre_ns_forward with
 * batch = n_rows, neg = 0, d_loss = NULL. Its backward (OpenKE Model.forward under any loss,
 * Model.py / SoftplusLoss.py:7-31 / SigmoidLoss.py:7-30; the repo's scoring_fn / _calc,
 * module/NegativeSampling.py:69-82): WRITES every row of the dense gradient tables (n_ent /
 * n_rel rows) with sum_i d_grad_score[i] * d(score_i)/d(tables), summed per table row in row
 * order i (no float atomics: bit-identical run to run). d_work: >=
 * mmre_rows_backward_workspace(model, n_rows, n_ent, n_rel, dim) floats. dim <= 512. */
int mmre_score_rows_backward(int model, int norm_flag, float model_margin, int use_model_margin,
                             const float* d_ent, const float* d_ent_im, const float* d_rel, const float* d_rel_im,
                             int dim, float phase_denom, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                             int64_t n_rows, const float* d_grad_score, float* d_grad_ent, float* d_grad_ent_im,
                             float* d_grad_rel, float* d_grad_rel_im, int64_t n_ent, int64_t n_rel, float* d_work,
                             int64_t work_floats, void* stream);

/* ====================================================================== *
 *  Zero-shot relation-embedding generator (module/model.py:674-686):     *
 *  cat(noise, cls) -> SN-Linear -> SN-Linear -> SN-Linear ->            *
 *  LayerNormalization (module/submodule.py:58-77). Spectral norm         *
 *  (module/spectral_norm.py:39-89): sigma = u . (W v); in training mode  *
 *  one power iteration first updates u, v in place.                      *
 * ====================================================================== */
int64_t mmre_generator_workspace(int64_t n_rows, int in0, int out0, int out1, int out2);
int mmre_generator_forward(const float* d_noise, int noise_dim, const float* d_cls, int cls_dim,
                           int64_t n_rows, const float* d_w0, const float* d_b0, float* d_u0, float* d_v0,
                           int out0, const float* d_w1, const float* d_b1, float* d_u1, float* d_v1, int out1,
                           const float* d_w2, const float* d_b2, float* d_u2, float* d_v2, int out2,
                           const float* d_ln_a, const float* d_ln_b, float ln_eps, int power_iteration,
                           float sn_eps, float* d_out, float* d_work, void* stream);
/* Floats of the activation buffer of mmre_generator_forward_save. */
int64_t mmre_generator_acts_size(int64_t n_rows, int in0, int out0, int out1, int out2);
/* Training forward: mmre_generator_forward that also keeps the layer outputs for the
 * backward in d_acts = [x0 (N, in0) | h1 (N, out0) | h2 (N, out1) | h3 (N, out2) |
 * W0/s0 (out0, in0) | W1/s1 (out1, out0) | W2/s2 (out2, out1)] (row-major, in0 =
 * noise_dim + cls_dim); sigma[3] is left at d_work + 3 * 2048. */
int mmre_generator_forward_save(const float* d_noise, int noise_dim, const float* d_cls, int cls_dim,
                                int64_t n_rows, const float* d_w0, const float* d_b0, float* d_u0, float* d_v0,
                                int out0, const float* d_w1, const float* d_b1, float* d_u1, float* d_v1, int out1,
                                const float* d_w2, const float* d_b2, float* d_u2, float* d_v2, int out2,
                                const float* d_ln_a, const float* d_ln_b, float ln_eps, int power_iteration,
                                float sn_eps, float* d_out, float* d_work, float* d_acts, void* stream);
/* Floats of the backward's workspace. */
int64_t mmre_generator_backward_workspace(int64_t n_rows, int in0, int out0, int out1, int out2);
/* Parameter gradients of the generator for loss_G.backward() (zsl_module.py:595; the
 * grad_list of :356-357: weight_orig, bias of the three SN layers, layer_norm a_2 / b_2),
 * written (not accumulated) from d_gout = dL/dout (N, out2). Spectral norm chain rule with
 * the forward's u, v, sigma (u, v constant, spectral_norm.py:85-89):
 *   dL/dW_orig = G / s - <G, W_orig> / s^2 * u v^T,  G = dL/d(W_orig / s). */
int mmre_generator_backward(const float* d_gout, int64_t n_rows, int in0, int out0, int out1, int out2,
                            const float* d_acts, const float* d_sigma, const float* d_w0, const float* d_u0,
                            const float* d_v0, const float* d_w1, const float* d_u1, const float* d_v1,
                            const float* d_w2, const float* d_u2, const float* d_v2, const float* d_ln_a,
                            float ln_eps, float* d_gw0, float* d_gb0, float* d_gw1, float* d_gb1, float* d_gw2,
                            float* d_gb2, float* d_gln_a, float* d_gln_b, float* d_work, void* stream);

/* ====================================================================== *
 *  Candidate-list rankings.                                               *
 * ====================================================================== */
/* main.evaluate (main.py:232-250): TransE L1, no normalisation
 * (module/NegativeSampling.py:294-302): score = |(h + r) - t|_1 for each
 * candidate of query i (CSR, true tail first); rank = #(s<p) + #(s==p)//2 + 1
 * with IEEE compares (a NaN score is neither less nor equal). dim <= 1024, else
 * MMRE_ERR_SHAPE and nothing is written. d_scores may be NULL.
 * Empty list (d_cand_off[i] == d_cand_off[i+1]): d_rank[i] = 0, no candidate is
 * read and no score is written (as mmre_rank_desc); this holds for
 * mmre_cosine_rank too. */
int mmre_candidate_rank_transe(const float* d_ent, const float* d_rel, int dim, const int64_t* d_qh,
                               const int64_t* d_qr, int64_t n_query, const int64_t* d_cand_off,
                               const int64_t* d_cand_ids, float* d_scores, int32_t* d_rank, void* stream);
/* ZSLmodule.eval (zsl_module.py:699-706): score = mean_s cos(cand, rel_vec[s]);
 * rank = 1 + #(score > score[true]) with the true candidate first. Tie-free
 * inputs are the contract (the reference's argsort leaves tie order unspecified);
 * a copy of the true row scores bit-equal to it and is not counted. A zero-norm
 * candidate scores 0 and a zero-norm relation sample contributes 0 (sklearn's
 * normalisation). n_samples <= 64 and n_samples * dim * 4 <= 98,304 bytes of
 * dynamic LDS, else MMRE_ERR_SHAPE and nothing is written. */
int mmre_cosine_rank(const float* d_cand, int dim, const int64_t* d_cand_off, int64_t n_query,
                     const float* d_rel_vecs, int n_samples, const int64_t* d_rel_of_query, float* d_scores,
                     int32_t* d_rank, void* stream);

/* ====================================================================== *
 *  ZSL Extractor (module/zsl_module.py:17-110) in eval mode, fused with   *
 *  ZSLmodule.eval's cosine ranking (zsl_module.py:666-706). Replaces, per *
 *  query, get_meta (:265-287) + Extractor(query, query, meta, meta)       *
 *  (:690-694) + sklearn cosine_similarity(...).mean(1) (:699-701) +       *
 *  argsort rank (:705-706). d = embed_dim in {64, 100, 128, 200, 256}.    *
 * ====================================================================== */

/* Floats of the packed-weight buffer for embed_dim `dim` (-1 if unsupported). */
int64_t mmre_extractor_pack_size(int dim);
/* Pack the Extractor's weights (nn.Linear layout (out, in) row-major, as in its
 * state_dict: gcn_w (d/2, d) + bias, fc1 / fc2 (d/2, d) + bias, reshape_layer
 * (d, 2d) + bias, support_encoder.proj1 (2d, d) + bias, proj2 (d, 2d) + bias,
 * support_encoder.layer_norm weight / bias (d)) into MFMA lane order. */
int mmre_extractor_pack(int dim, const float* d_gcn_w, const float* d_gcn_b, const float* d_fc1_w,
                        const float* d_fc1_b, const float* d_fc2_w, const float* d_fc2_b, const float* d_rs_w,
                        const float* d_rs_b, const float* d_p1_w, const float* d_p1_b, const float* d_p2_w,
                        const float* d_p2_b, const float* d_ln_w, const float* d_ln_b, float* d_pack, void* stream);
/* Per-node halves of reshape_layer's output (neighbor_encoder :47-59 and
 * entity_encoder :61-67 folded through the linear reshape_layer :92-96):
 *   d_left[n]  (as e1: left neighbours, fc1 part, + bias)   (n_nodes, d), or NULL
 *   d_right[n] (as e2: fc2 part, right neighbours)          (n_nodes, d), or NULL
 * for node n = symbol d_node_sym[n] with neighbour list d_conn[n][max_nb][2]
 * (column 1 = neighbour symbol id, PAD = the zero last row of d_sym_emb; the
 * layout of ZSLmodule.connections, :233-263) and degree d_deg[n] (float). */
int mmre_extractor_nodes(int dim, const float* d_pack, const float* d_sym_emb, const int64_t* d_node_sym,
                         const int64_t* d_conn, int max_nb, const float* d_deg, int64_t n_nodes, float* d_left,
                         float* d_right, void* stream);
/* Row r = (e1 = d_li[r], e2 = d_ri[r]): x = left[e1] + right[e2]; g = SupportEncoder(x)
 * (submodule.py:254-258, nn.LayerNorm eps ln_eps). Writes d_out_g (n_rows, d) if
 * non-NULL (the Extractor's query_g) and d_score[r] = g . t / (normalize ? |g| : 1)
 * with t = d_targets[d_row_target[r]] (row 0 if d_row_target is NULL). */
int mmre_extractor_encode(int dim, const float* d_pack, float ln_eps, const float* d_left, const int64_t* d_li,
                          const float* d_right, const int64_t* d_ri, int64_t n_rows, const float* d_targets,
                          const int64_t* d_row_target, int normalize, float* d_out_g, float* d_score, void* stream);
/* mmre_extractor_encode with a cap on the launch: the kernel is persistent, its
 * workgroups walk the 64-row tiles with stride gridDim.x, and the grid is
 * min(tiles, resident workgroups) -- or, with max_blocks > 0, min(that, max_blocks)
 * (max_blocks <= 0: exactly mmre_extractor_encode). The results do not depend on the
 * grid; the cap lets a small input give a workgroup many tiles. */
int mmre_extractor_encode_capped(int dim, const float* d_pack, float ln_eps, const float* d_left, const int64_t* d_li,
                                 const float* d_right, const int64_t* d_ri, int64_t n_rows, const float* d_targets,
                                 const int64_t* d_row_target, int normalize, float* d_out_g, float* d_score,
                                 int max_blocks, void* stream);
/* Workgroups mmre_extractor_encode launches for (dim, n_rows) on the current device
 * (the value the launch itself uses); -1 for an unsupported dim or n_rows <= 0. */
int64_t mmre_extractor_encode_blocks(int dim, int64_t n_rows);
/* d_targets[t] = mean_s v[t][s] / (normalize ? |v[t][s]| : 1) for d_vecs (n_sets, n_samples, dim),
 * n_samples <= 64: the sklearn-normalised mean relation vector of ZSL scoring, or
 * the support mean of Extractor.forward (:101). */
int mmre_extractor_targets(const float* d_vecs, int64_t n_sets, int n_samples, int dim, int normalize,
                           float* d_targets, void* stream);
/* Rank of the first entry of each list (CSR d_off) in descending order:
 * 1 + #(score > score[first]) (zsl_module.py:705-706, tie-free inputs). */
int mmre_rank_desc(const float* d_scores, const int64_t* d_off, int64_t n_query, int32_t* d_rank, void* stream);

/* ====================================================================== *
 *  ZSL Extractor in TRAINING mode (dropout active): pretrain_Extractor    *
 *  (module/zsl_module.py:289-348) and the GAN loop's Extractor calls      *
 *  while it is in training mode (:371-383, :430-440). The frozen          *
 *  symbol_emb side of the forward; the linears run on mmre_gemm_f32.      *
 * ====================================================================== */

/* Per row r of (d_pairs[r] = (e1, e2) symbol ids, neighbour lists d_conn_left/right[r]
 * (max_nb, 2), column 1 = neighbour symbol; the get_meta layout, :265-287):
 *   d_nsum_left[r]  = sum_s dropout(emb[conn_left[r][s][1]])     (neighbor_encoder :47-59
 *   d_nsum_right[r] = sum_s dropout(emb[conn_right[r][s][1]])     before gcn_w, whose linear
 *                                                                 part is applied to the sum)
 *   d_e1[r], d_e2[r] = dropout_e(emb[e1]), dropout_e(emb[e2])    (entity_encoder :61-67)
 * all (n_rows, dim). Dropout p (0 <= p < 1): kept values x * (1 / (1 - p)); the masks are a
 * counter hash of d_rng_state[0] (seed) and d_rng_state[1] (offset) on device, or -- when
 * d_mask_nb_left / d_mask_nb_right (n_rows, max_nb, dim) and d_mask_ent (n_rows, 2, dim) are
 * all given -- those 0/1 bytes. max_nb <= 64. */
int mmre_extractor_train_inputs(int dim, const float* d_sym_emb, const int64_t* d_pairs, const int64_t* d_conn_left,
                                const int64_t* d_conn_right, int max_nb, int64_t n_rows, float p,
                                const uint64_t* d_rng_state, const uint8_t* d_mask_nb_left,
                                const uint8_t* d_mask_nb_right, const uint8_t* d_mask_ent, float* d_nsum_left,
                                float* d_nsum_right, float* d_e1, float* d_e2, void* stream);
/* Elementwise dropout (nn.Dropout in training mode, e.g. SupportEncoder :257): d_y = keep ?
 * d_x * (1 / (1 - p)) : 0, the keep bytes to d_mask if non-NULL; draws from d_rng_state with
 * dropout stream `stream_id` (distinct streams of one step draw independent masks). */
int mmre_dropout(const float* d_x, float* d_y, uint8_t* d_mask, int64_t n, float p, const uint64_t* d_rng_state,
                 int stream_id, void* stream);

/* ====================================================================== *
 *  Frozen M3AE text encoder: the producer of the generator's CLS input.   *
 *  Replaces MaskedMultimodalAutoencoder.forward_representation(image=None,*
 *  text, text_padding_mask, deterministic=True) (module/model.py:323-356) *
 *  over Transformer/Block/Attention/TransformerMLP (module/submodule.py:  *
 *  128-238), as called by UnifiedModel.generate (model.py:674-679) and    *
 *  forward_relation_emb (model.py:599-604). Only the CLS row is returned. *
 *  Padded tokens (mask > 0) and, in the last block, non-CLS rows are not  *
 *  computed: they cannot reach the CLS output (masked logit -1e7 has      *
 *  softmax weight exactly 0); a row equal to the previous row on its      *
 *  unpadded tokens is encoded once. d in {384, 768, 1024, 1280}, head dim *
 *  64 or 80, len <= mmre_m3ae_max_len().                                  *
 * ====================================================================== */

/* Longest description row (tokens) the encoder accepts. */
int mmre_m3ae_max_len(void);
/* Int32 elements of the plan buffer for n_seq rows (6 n_seq + 5). */
int64_t mmre_m3ae_plan_size(int64_t n_seq);
/* Plan of an encode: per input row of d_tokens (n_seq, len) int32 / d_mask (n_seq, len) float32
 * (> 0 = padding, module/data.py:252-270): uniq[b] (the unique sequence it maps to; a row equal
 * to row b-1 on its padding pattern and unpadded tokens shares b-1's when dedupe != 0), the
 * unique sequences' source rows and packed row offsets (1 + unpadded tokens each, CLS row
 * first), and at d_plan[3 n_seq + 1 ..] info = {n_unique, n_rows, max_rows, unpadded token ids
 * outside [0, vocab)}. The host reads info (4 ints) to size the encode. */
int mmre_m3ae_plan(const int32_t* d_tokens, const float* d_mask, int64_t n_seq, int64_t len, int dedupe,
                   int64_t vocab, int32_t* d_plan, void* stream);
/* Floats of the workspace mmre_m3ae_encode needs for info's n_rows / n_unique. */
int64_t mmre_m3ae_workspace(int64_t n_rows, int64_t n_unique, int d);
/* CLS vectors d_cls (n_seq, d) of the description rows planned by mmre_m3ae_plan. h_params: HOST array
 * of 4 + 12 * depth + 2 DEVICE pointers, fp32 row-major as in the reference state dict:
 *   text_embedding.weight (vocab, d), the sin-cos position table (>= len, d)
 *   (get_1d_sincos_pos_embed, model.py:113-133), encoder_text_type_embedding (d), cls_token (d);
 *   per block i: layer_norm1.{weight,bias}, attention.qkv_linear.{weight (3d, d), bias},
 *   attention.fc.{weight, bias}, layer_norm2.{weight,bias}, transformer_mlp.fc1.{weight (4d, d),
 *   bias}, transformer_mlp.fc2.{weight (d, 4d), bias};
 *   encoder.layer_norm.{weight, bias}.
 * n_unique / n_rows / max_rows: the plan's info. At most 65,535 unique sequences per call (more:
 * MMRE_ERR_SHAPE, before anything is launched; encode such a batch in slices). */
int mmre_m3ae_encode(const float* const* h_params, int depth, int d, int heads, float ln_eps,
                     const int32_t* d_tokens, const float* d_mask, int64_t n_seq, int64_t len, int64_t vocab,
                     const int32_t* d_plan, int64_t n_unique, int64_t n_rows, int max_rows, float* d_work,
                     int64_t work_floats, float* d_cls, void* stream);
/* The encoder's building blocks (also exported for tests): nn.LayerNorm over rows;
 * out = a w^T + bias (epilogue 0), GELU(.) (1, F.gelu erf form), resid + (.) (2; resid may
 * alias out), n % 64 == 0, k % 32 == 0; packed multi-head attention over d_off sequences
 * (qkv rows [q | k | v]; cls_only: query row 0 of each sequence only, written to out row b). */
int mmre_m3ae_layernorm(const float* d_x, int64_t n_rows, int d, const float* d_w, const float* d_b, float eps,
                        float* d_y, void* stream);
int mmre_m3ae_linear(int epilogue, const float* d_a, int64_t m, int k, const float* d_w, int n, const float* d_bias,
                     const float* d_resid, float* d_out, void* stream);
int mmre_m3ae_attention(const float* d_qkv, const int32_t* d_off, int64_t n_seq, int max_rows, int heads,
                        int head_dim, float scale, int cls_only, float* d_out, void* stream);
/* Host only: the output tile width, 64 or 128, that mmre_m3ae_linear uses for an (m, n) output
 * (128 once ceil(m / 64) * (n / 128) >= 2048 and n % 128 == 0; MMRE_M3AE_TILE = "128" / "64",
 * read at every call, forces either where n allows it), -1 for a shape it refuses. */
int mmre_m3ae_linear_tile(int64_t m, int n);

/* ====================================================================== *
 *  Small fp32 GEMM of the GAN step's Discriminator (zsl_module.py:112-138: *
 *  its SN linears and class scores) and of their autograd, the gradient   *
 *  penalty's double backward included (module/utils.py:692-707).          *
 *  d_c (m, n) row-major = A B (+ d_bias[n] when given) with               *
 *  A(i, k) = d_a[i sam + k sak], B(k, j) = d_b[k sbk + j sbn] (transposes *
 *  are strides). One launch: 32 x 32 MFMA tiles, K split over             *
 *  mmre_gemm_splits(m, n, k) waves of a workgroup, summed in slice order. *
 *  m == 0 or n == 0 is a no-op (the NULL pointers of empty tensors are    *
 *  accepted); k == 0 writes the bias rows (or zeros).                     *
 * ====================================================================== */
int mmre_gemm_splits(int64_t m, int64_t n, int64_t k);
int mmre_gemm_f32(const float* d_a, int64_t sam, int64_t sak, const float* d_b, int64_t sbk, int64_t sbn, int64_t m,
                  int64_t n, int64_t k, const float* d_bias, float* d_c, void* stream);

/* Spectral normalisation of one weight (torch.nn.utils.spectral_norm's compute_weight, the
 * reference's SN layers: module/spectral_norm.py:39-89; Discriminator zsl_module.py:115-118).
 * power_iteration != 0 (training mode): one power iteration first updates d_u (out), d_v (in)
 * in place (v = normalize(W^T u), u = normalize(W v), eps). Then sigma = u . (W v),
 * d_w_hat = W / sigma, and d_u_snap / d_v_snap = the u, v used (for the backward).
 * d_work: 2048 floats. out, in <= 1024. */
int mmre_sn_weight(const float* d_w, int out, int in, float* d_u, float* d_v, int power_iteration, float eps,
                   float* d_sigma, float* d_u_snap, float* d_v_snap, float* d_w_hat, float* d_work, void* stream);
/* d_gw = G / s - <G, W> / s^2 u v^T for G = d_g = dL/dW_hat (u, v, s from mmre_sn_weight). */
int mmre_sn_weight_backward(const float* d_g, const float* d_w, int out, int in, const float* d_u, const float* d_v,
                            const float* d_sigma, float* d_gw, void* stream);
/* LayerNormalization (module/submodule.py:58-77): (z - mean) / (std_unbiased + eps) * a + b
 * per row of d_z (n_rows, d); d == 1 is the identity. n_rows == 0 is a no-op (d_z / d_out
 * may be NULL then). */
int mmre_layernorm_unbiased(const float* d_z, int64_t n_rows, int d, const float* d_a, const float* d_b, float eps,
                            float* d_out, void* stream);
/* Its backward for dL/dout = d_g: d_gz (n_rows, d), d_ga, d_gb (d). d_work: n_rows * d floats.
 * n_rows == 0 zeroes d_ga / d_gb (the row buffers may be NULL then). */
int mmre_layernorm_unbiased_backward(const float* d_g, const float* d_z, int64_t n_rows, int d, const float* d_a,
                                     float eps, float* d_gz, float* d_ga, float* d_gb, float* d_work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMRE_H */
