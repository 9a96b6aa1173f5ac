// rescal.hip -- RESCAL link prediction on MI355X: the relation planes on the matrix cores, the
// all-entity f32 MFMA sweep whose entity operand is picked per query tile, with the fused rank
// epilogue, and predict for arbitrary rows (OpenKE/openke/module/model/RESCAL.py:17-46 under the
// Tester loop, Tester.py:70-91, Test.h:65-192).
//
// RESCAL scores a triple with the relation's d x d matrix, s(h, r, t) = sum_i h_i (M_r t)_i
// (RESCAL.py:17-22; forward = -s, predict = -forward = s: the Tester ranks ascending on +s, as the
// reference does). With P_r[i][e] = (M_r e)_i a tail-side query (h, r, ?) is the dot product of the
// raw row h with every column of P_r, and a head-side query (?, r, t) the dot product of column t of
// P_r with every raw entity row: DistMult's sweep with an entity operand that depends on the query
// tile. For every relation that occurs in the queries the prologue writes P_r = E . M_r^T as a
// k-major plane P[slot][kp][e_pad] -- the sweep's own layout -- next to the k-major copy of the raw
// table; a query tile holds the queries of ONE (relation, side), key = 2 relation + side, and its
// units stage the relation's plane (tail side) or the raw copy (head side) as they are.
//
// Canonical arithmetic (RESCAL): f32, both chains FUSED because both run on
// v_mfma_f32_32x32x2_f32, which returns a k-ordered fmaf chain bit for bit:
//   tr(r, e)_i = fma(M_r[i][d-1], e_{d-1}, ... fma(M_r[i][0], e_0, +0.0f))       ascending j
//   s(h, r, t) = fma(h_{d-1}, tr(r, t)_{d-1}, ... fma(h_0, tr(r, t)_0, +0.0f))   ascending i
// fmaf is symmetric in its factors, so a head-side candidate's sum_i e_i P_r[i][t] and a tail-side
// candidate's sum_i h_i P_r[i][e] are the same chain over the plane: a triple has ONE bit pattern
// wherever it is computed (the sweep, the truth / filter pass, k_rescal_rows), the sweep's score of
// the true entity equals its threshold and `< thr` rejects it (ties favour the truth, Test.h:83).
// K rows padded with zeros in both operands leave either chain as it is up to the sign of a zero
// (transr.hip), which no comparison distinguishes.
//
// Kernels (one evaluation, one stream):
//   k_rs_ent_km        the k-major copy of the raw entity table
//   k_rs_planes        P[slot] for every used relation: f32 MFMA, accumulators stored to the plane
//   k_rs_queries       query vectors of the padded tile rows: raw h rows (tail side), column t of
//                      the tile relation's plane (head side)
//   k_rs_scores        truth of every query and every listed entity of every filter group
//   k_rs_filter_count  one wave per filter group: counts = {0, -c, 0, -cc}
//   k_sweep_rescal     128 x 128 units, four waves as 2 x 2, K in 16-row double-buffered LDS stages,
//                      ballot row counters (link.hip's k_sweep_mfma, KS = 16)
//   k_rescal_rows      predict of arbitrary (h, r, t) rows, one thread per row
// and, after the sweep, link.hip's finalize (launch_finalize: filtered columns += raw columns).
#include <algorithm>

#include "link_common.h"

namespace mmre {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RS_MAX_DIM = 512;
constexpr int RS_KS = KS_MFMA;  // K rows per LDS stage of the sweep, and the planes' row padding
__host__ __device__ inline int rs_kp(int dim) { return (int)round_up(dim, RS_KS); }

// ------------------------------------------------------------------ prologue ----
// ent_km[k][e] = ent[e][k]; rows at or past dim and columns at or past n_ent are zeros.
__global__ __launch_bounds__(256) void k_rs_ent_km(const float* __restrict__ ent, int64_t n_ent, int64_t e_pad, int dim,
                                                   int kp, float* __restrict__ ent_km) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < (int64_t)kp * e_pad;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t k = idx / e_pad, e = idx - k * e_pad;
    ent_km[idx] = (k < dim && e < n_ent) ? ent[e * dim + k] : 0.0f;
  }
}

// The planes. Workgroup (x, slot): PL_COLS entities of the relation used[slot] over ALL d plane
// rows, four waves. P_r[i][e] = sum_j M_r[i][j] e_j is E . M_r^T; the MFMA takes M_r's rows as its
// row operand and the entity rows as its column operand (the product is the same bits either way,
// fmaf being symmetric), so an accumulator's column is an entity and one store instruction writes
// 32 consecutive floats of a plane row. Both operands are read along K as they lie in memory (M_r
// row-major in j, the entity table row-major): no transposed copy of the matrix exists, the staging
// transposes into LDS. The plane rows go in chunks of PL_ROWS = two 32-high MFMA tiles; wave w owns
// row tile w & 1 and the column tiles 2 (w >> 1), 2 (w >> 1) + 1: two f32x16 accumulators that
// share the row operand. K runs in blocks of PL_KB through LDS -- sA[k][i], sB[k][e] -- the next
// block's values loaded into registers while the MFMAs of this one run. K ascends across blocks,
// across the instructions of a block and (the instruction's own order) inside an instruction; K
// rows at or past d are zeros in BOTH operands. There is no row norm, so nothing is kept in LDS
// beyond the stage: a finished chunk's accumulators go to the plane. Plane rows d .. kp and the
// columns of entities at or past n_ent are zeros.
constexpr int PL_COLS = 128, PL_ROWS = 64, PL_KB = 16, PL_SA = PL_ROWS + 4, PL_SB = PL_COLS + 4;
__global__ __launch_bounds__(256) void k_rs_planes(const float* __restrict__ ent, const float* __restrict__ mats,
                                                   int64_t n_ent, int64_t e_pad, int64_t n_rel, int dim, int kp,
                                                   const int32_t* __restrict__ used, int64_t n_used,
                                                   float* __restrict__ planes) {
  __shared__ float sA[PL_KB * PL_SA];
  __shared__ float sB[PL_KB * PL_SB];
  const int tid = threadIdx.x;
  const int64_t slot = blockIdx.y;
  const int64_t e0 = (int64_t)blockIdx.x * PL_COLS;
  if (slot >= n_used || e0 + PL_COLS > e_pad) return;  // uniform
  float* out = planes + slot * kp * e_pad;
  const int64_t r = used[slot];
  if (r < 0 || r >= n_rel) {  // uniform: a relation the tables do not hold gets a zero plane
    for (int idx = tid; idx < kp * PL_COLS; idx += 256) out[(int64_t)(idx >> 7) * e_pad + e0 + (idx & 127)] = 0.0f;
    return;
  }
  const float* M = mats + r * ((int64_t)dim * dim);

  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int rt = wave & 1, lc0 = (wave >> 1) * 64;  // row tile; first local column of the wave's two tiles
  // staging roles: A row a_row (a plane row i), k a_k .. a_k + 3; B row b_row (an entity), k b_k .. b_k + 7
  const int a_row = tid >> 2, a_k = (tid & 3) * 4;
  const int b_row = tid >> 1, b_k = (tid & 1) * 8;
  const int64_t b_e = e0 + b_row;
  const float* b_src = ent + b_e * dim;
  const bool b_in = b_e < n_ent;
  const int nkb = (dim + PL_KB - 1) / PL_KB;
  // uniform: a thread's four (A) or eight (B) k are aligned 16-B loads (k + 3 < dim follows from k < dim)
  const bool vec = (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(ent) | reinterpret_cast<uintptr_t>(mats)) & 15) == 0;

  for (int i0 = 0; i0 < kp; i0 += PL_ROWS) {
    const int a_i = i0 + a_row;
    const float* a_src = M + (int64_t)a_i * dim;
    const bool a_in = a_i < dim;
    const bool live = i0 + rt * 32 < dim;  // wave-uniform: the row tile has a row to compute
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
    float ra[4], rb[8];
    auto gload = [&](int kb) {
      const int k0 = kb * PL_KB;
      if (vec) {
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f}, w0 = v, w1 = v;
        if (a_in && k0 + a_k < dim) v = *reinterpret_cast<const float4*>(a_src + k0 + a_k);
        if (b_in && k0 + b_k < dim) w0 = *reinterpret_cast<const float4*>(b_src + k0 + b_k);
        if (b_in && k0 + b_k + 4 < dim) w1 = *reinterpret_cast<const float4*>(b_src + k0 + b_k + 4);
        ra[0] = v.x, ra[1] = v.y, ra[2] = v.z, ra[3] = v.w;
        rb[0] = w0.x, rb[1] = w0.y, rb[2] = w0.z, rb[3] = w0.w;
        rb[4] = w1.x, rb[5] = w1.y, rb[6] = w1.z, rb[7] = w1.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + a_k + u;
          ra[u] = (a_in && k < dim) ? a_src[k] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + b_k + u;
          rb[u] = (b_in && k < dim) ? b_src[k] : 0.0f;
        }
      }
    };
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
      __syncthreads();  // the block before is consumed
#pragma unroll
      for (int u = 0; u < 4; ++u) sA[(a_k + u) * PL_SA + a_row] = ra[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) sB[(b_k + u) * PL_SB + b_row] = rb[u];
      __syncthreads();
      if (kb + 1 < nkb) gload(kb + 1);
      if (live) {
#pragma unroll
        for (int s = 0; s < PL_KB / 2; ++s) {
          const float a = sA[(2 * s + lh) * PL_SA + rt * 32 + li];
          const float b0 = sB[(2 * s + lh) * PL_SB + lc0 + li];
          const float b1 = sB[(2 * s + lh) * PL_SB + lc0 + 32 + li];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
      }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int i = i0 + rt * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
      if (i < kp) {
        const int64_t c0 = e0 + lc0 + li, c1 = c0 + 32;
        out[(int64_t)i * e_pad + c0] = (i < dim && c0 < n_ent) ? acc0[g] : 0.0f;
        out[(int64_t)i * e_pad + c1] = (i < dim && c1 < n_ent) ? acc1[g] : 0.0f;
      }
    }
  }
}

// What the device kernels share about one evaluation.
struct RSEval {
  const float* ent;         // [n_ent][dim] the raw table
  const float* ent_km;      // [kp][e_pad] its k-major copy
  const float* planes;      // [n_used][kp][e_pad] P_r
  const int32_t* rel_slot;  // [n_rel] -> the relation's plane, -1 for a relation without queries
  int64_t n_ent, e_pad, n_rel, n_used, n_query;
  int dim, kp;
  const int64_t *qh, *qr, *qt;
  const int8_t* qmode;
};

// (side, relation, head, tail, truth, slot) of query q, or false for ids outside the tables
struct RSQuery {
  bool head;
  int64_t r, h, t, truth, slot;
};
__device__ __forceinline__ bool rs_query(const RSEval& P, int64_t q, RSQuery& Q) {
  if (q < 0 || q >= P.n_query) return false;
  Q.h = P.qh[q];
  Q.t = P.qt[q];
  Q.r = P.qr[q];
  Q.head = P.qmode[q] == MMRE_HEAD_BATCH;
  Q.truth = Q.head ? Q.h : Q.t;
  if (Q.h < 0 || Q.h >= P.n_ent || Q.t < 0 || Q.t >= P.n_ent || Q.r < 0 || Q.r >= P.n_rel) return false;
  Q.slot = P.rel_slot[Q.r];
  return Q.slot >= 0 && Q.slot < P.n_used;
}
// s(h, r, t) of the relation in `slot`: the second chain over the stored plane
__device__ __forceinline__ float rs_score(const RSEval& P, int64_t slot, int64_t h, int64_t t) {
  const float* pl = P.planes + slot * P.kp * P.e_pad + t;
  const float* hr = P.ent + h * P.dim;
  float s = 0.0f;
  for (int i = 0; i < P.dim; ++i) s = __builtin_fmaf(hr[i], pl[(int64_t)i * P.e_pad], s);
  return s;
}

// Query vectors of the padded tile rows, k-major q_km[kp][n_tiles * TQ], one thread per row; row_q:
// the row's query id in the caller's order (-1: padding, or a query / tile the tables do not hold).
// tiles[3 t] is the tile's key 2 relation + side (side = qmode).
__global__ __launch_bounds__(TQ) void k_rs_queries(RSEval P, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ tiles, int64_t n_tiles,
                                                   float* __restrict__ q_km, int32_t* __restrict__ row_q) {
  const int64_t tile = blockIdx.x;
  const int64_t key = tiles[3 * tile], first = tiles[3 * tile + 1], rows = tiles[3 * tile + 2];
  const int64_t q_pad = n_tiles * TQ, row = tile * TQ + threadIdx.x;
  RSQuery Q;
  int64_t q = -1;
  if (first >= 0 && rows >= 0 && rows <= TQ && first + rows <= P.n_query && (int64_t)threadIdx.x < rows) {
    q = perm[first + threadIdx.x];
    if (!rs_query(P, q, Q) || 2 * Q.r + (Q.head ? MMRE_HEAD_BATCH : MMRE_TAIL_BATCH) != key) q = -1;
  }
  row_q[row] = (int32_t)q;
  if (q < 0) {
    for (int k = 0; k < P.kp; ++k) q_km[(int64_t)k * q_pad + row] = 0.0f;
    return;
  }
  if (Q.head) {  // column t of the plane
    const float* pl = P.planes + Q.slot * P.kp * P.e_pad + Q.t;
    for (int k = 0; k < P.kp; ++k) q_km[(int64_t)k * q_pad + row] = k < P.dim ? pl[(int64_t)k * P.e_pad] : 0.0f;
  } else {  // the raw row h
    const float* hr = P.ent + Q.h * P.dim;
    for (int k = 0; k < P.kp; ++k) q_km[(int64_t)k * q_pad + row] = k < P.dim ? hr[k] : 0.0f;
  }
}

// ------------------------------------------------------- truth and filter pass ----
// One thread per chain: task t < n_query is the truth of query t -> thr[t]; task n_query + p is
// listed entity p of the filter CSR, scored for its group's representative query entry_q[p] ->
// list_v[p] (a group shares (mode, r, anchor): Test.h:85 `_find`). NaN marks what is never counted.
__global__ __launch_bounds__(256) void k_rs_scores(RSEval P, int pred_kind, const int32_t* __restrict__ entry_q,
                                                   const int32_t* __restrict__ ids, int64_t n_entries,
                                                   float* __restrict__ thr, float* __restrict__ list_v) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P.n_query + n_entries) return;
  RSQuery Q;
  if (t < P.n_query) {
    thr[t] = rs_query(P, t, Q) ? apply_pred(pred_kind, 0.0f, rs_score(P, Q.slot, Q.h, Q.t)) : __builtin_nanf("");
    return;
  }
  const int64_t p = t - P.n_query;
  const int64_t j = ids[p];
  if (j < 0 || j >= P.n_ent || !rs_query(P, entry_q[p], Q)) {
    list_v[p] = __builtin_nanf("");
    return;
  }
  list_v[p] = apply_pred(pred_kind, 0.0f, Q.head ? rs_score(P, Q.slot, j, Q.t) : rs_score(P, Q.slot, Q.h, j));
}

// One wave per filter group: the group's listed scores staged in LDS 64 at a time, every member
// (one per lane) counts those that beat its own truth (TransR's k_tr_filter_count over RSEval):
//   counts[.][q] = {0, -c, 0, -cc}, c = #{listed j != true(q) : pred(j) < thr[q]} (Test.h:85),
//   cc those the type constraint allows. grp_qoff == NULL: no filter, every query gets {0, 0, 0, 0}.
__global__ __launch_bounds__(64) void k_rs_filter_count(RSEval P, const int64_t* __restrict__ grp_qoff,
                                                        const int32_t* __restrict__ grp_q, int64_t n_groups,
                                                        const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ ids,
                                                        const float* __restrict__ list_v, int64_t n_entries,
                                                        const float* __restrict__ thr,
                                                        const uint32_t* __restrict__ type_head,
                                                        const uint32_t* __restrict__ type_tail, int64_t type_words,
                                                        int32_t* __restrict__ counts) {
  __shared__ int32_t s_id[64];
  __shared__ float s_v[64];
  __shared__ int32_t s_tb[64];
  const int tid = threadIdx.x;
  const int64_t nq = P.n_query;
  if (grp_qoff == nullptr) {
    for (int64_t q = (int64_t)blockIdx.x * 64 + tid; q < nq; q += (int64_t)gridDim.x * 64)
      counts[q] = counts[nq + q] = counts[2 * nq + q] = counts[3 * nq + q] = 0;
    return;
  }
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t qa = grp_qoff[g], qb = grp_qoff[g + 1];
    int64_t la = off[g], lb = off[g + 1];
    if (qa < 0 || qb > nq || qa >= qb) continue;  // uniform
    if (la < 0 || lb > n_entries || lb < la) la = lb = 0;
    const int64_t q0 = grp_q[qa];
    RSQuery G;
    const bool gv = rs_query(P, q0, G);
    const uint32_t* tm = (type_head && gv) ? (G.head ? type_head : type_tail) : nullptr;
    for (int64_t qc = qa; qc < qb; qc += 64) {
      const int64_t qi = qc + tid;
      int64_t q = qi < qb ? grp_q[qi] : -1;
      if (q >= nq) q = -1;
      const bool active = q >= 0;
      RSQuery Q;
      const bool qv = active && rs_query(P, q, Q);
      const int64_t tr = qv ? Q.truth : -1;
      const float th = active ? thr[q] : 0.0f;
      int c = 0, cc = 0;
      for (int64_t lc = la; lc < lb; lc += 64) {
        const int nl = (int)((lb - lc) < 64 ? (lb - lc) : 64);
        __syncthreads();  // s_* reuse
        int32_t id = -1, tb = 0;
        float v = 0.0f;
        if (tid < nl) {
          const int64_t j = ids[lc + tid];
          if (j >= 0 && j < P.n_ent) {
            id = (int32_t)j;
            v = list_v[lc + tid];
            tb = tm ? (int32_t)type_bit(tm, type_words, G.r, j) : 0;
          }
        }
        s_id[tid] = id;
        s_v[tid] = v;
        s_tb[tid] = tb;
        __syncthreads();
        if (qv) {
          for (int i = 0; i < nl; ++i) {
            const int b = (s_id[i] >= 0) & (s_id[i] != tr) & (s_v[i] < th);
            c += b;
            cc += b & s_tb[i];
          }
        }
      }
      if (active) {
        counts[q] = 0;
        counts[nq + q] = -c;
        counts[2 * nq + q] = 0;
        counts[3 * nq + q] = -cc;
      }
    }
  }
}

// ------------------------------------------------------------------- sweep ----
// link.hip's k_sweep_mfma in its 16-row-stage form -- (query tile of 128) x (entity tile of 128)
// units over link_common.h's UnitMap, four waves as 2 (q) x 2 (e), each 2 x 2 blocks of 32 x 32
// accumulators, K through double-buffered register-staged LDS stages, the row thresholds read from
// LDS once per unit, each row's 64 compares counted by two ballots into a counter held by the lane
// of that row, counts reaching HBM when the workgroup leaves the query tile -- with the one new
// thing that the entity operand's base depends on the query tile: tile key 2 r + side stages the
// plane of r on the tail side and the raw k-major table on the head side. The rows of a tile map to
// queries through row_q (the plan's order), and a tile's type words are ONE row of one mask (its
// relation's, on its side): a lane reads the two words of its two entity columns once per unit,
// at the unit's first stage, and the constrained count is a third and fourth ballot.
// The truth needs no exclusion test: its score is bit-identical to the threshold.
template <bool TC, int PK>
__global__ __launch_bounds__(NT, 4) void k_sweep_rescal(
    RSEval P, const float* __restrict__ q_km, int64_t q_pad, const int32_t* __restrict__ tiles, int n_qt, int n_et,
    int n_groups, const float* __restrict__ thr, const int32_t* __restrict__ row_q,
    const uint32_t* __restrict__ type_head, const uint32_t* __restrict__ type_tail, int64_t type_words,
    int32_t* __restrict__ counts) {
  constexpr int KS = RS_KS;
  __shared__ float sq[2][KS][TQ];
  __shared__ float se[2][KS][TE];
  __shared__ __attribute__((aligned(16))) float s_th[2][TQ];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const PredSel<PK> pred(PK, 0.0f);
  const int wq = wave >> 1, we = wave & 1;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  const UnitMap um(grp, n_groups, n_qt, n_et);
  const int u0 = (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = (int)((int64_t)(gmem + 1) * um.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  const int kp = P.kp, nkc = kp / KS;
  const int64_t e_pad = P.e_pad, n_ent = P.n_ent, n_query = P.n_query;

  // the tile's relation and side, clamped to the tables (k_rs_queries emptied the rows of a tile
  // they do not hold), and the entity operand it stages
  auto tile_key = [&](int qt, int64_t& rel, bool& head) {
    const int64_t key = tiles[3 * (int64_t)qt];
    rel = key >> 1;
    rel = rel < 0 ? 0 : (rel >= P.n_rel ? P.n_rel - 1 : rel);
    head = (key & 1) == MMRE_HEAD_BATCH;
  };
  auto tile_operand = [&](int qt) -> const float* {
    int64_t rel;
    bool head;
    tile_key(qt, rel, head);
    if (head) return P.ent_km;
    int64_t slot = P.rel_slot[rel];
    slot = slot < 0 ? 0 : (slot >= P.n_used ? P.n_used - 1 : slot);
    return P.planes + slot * kp * e_pad;
  };

  auto row_of = [&](int bi, int r) { return wq * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow; };
  int tpar = 0;  // s_th slot of the current query tile
  // per-row counters of the current query tile: lane L holds wave row L (tile row wq * 64 + L)
  int cntv = 0, cntv_tc = 0;
  const uint32_t* cur_tm = nullptr;  // type constraints: the current tile's row of its side's mask
  auto load_rows = [&](int qtile) {
    // thresholds into the other s_th slot: visible after the stage's closing barrier, and the
    // slot's previous tile was left at least one stage ago
    tpar ^= 1;
    if (tid < TQ) {
      const int32_t q = row_q[(int64_t)qtile * TQ + tid];
      s_th[tpar][tid] = (q >= 0 && q < n_query) ? thr[q] : -INFINITY;  // -inf: nothing beats a padded row
    }
    cntv = 0;
    cntv_tc = 0;
    if constexpr (TC) {
      int64_t rel;
      bool head;
      tile_key(qtile, rel, head);
      cur_tm = (head ? type_head : type_tail) + rel * type_words;
    }
  };
  auto flush_rows = [&](int qtile) {  // each lane its row's count (both column waves add)
    const int32_t q = row_q[(int64_t)qtile * TQ + wq * 64 + lane];
    if (q >= 0 && q < n_query) {
      if (cntv) atomicAdd(&counts[q], cntv);  // raw only (k_counts_finalize)
      if constexpr (TC) {
        if (cntv_tc) atomicAdd(&counts[2 * n_query + q], cntv_tc);
      }
    }
  };

  const int srow = tid >> 5, sc4 = tid & 31;  // rows srow, srow + 8 of the stage
  float4 rq0, rq1, re0, re1;
  int ld_unit = u0, ld_kc = 0, ld_qt, ld_et;
  um.at(u0, ld_qt, ld_et);
  const float* ld_ent = tile_operand(ld_qt);
  auto gload = [&]() {
    const int k = ld_kc * KS + srow;
    const float* qp = q_km + (int64_t)k * q_pad + (int64_t)ld_qt * TQ + sc4 * 4;
    const float* ep = ld_ent + (int64_t)k * e_pad + (int64_t)ld_et * TE + sc4 * 4;
    rq0 = *reinterpret_cast<const float4*>(qp);
    rq1 = *reinterpret_cast<const float4*>(qp + 8 * q_pad);
    re0 = *reinterpret_cast<const float4*>(ep);
    re1 = *reinterpret_cast<const float4*>(ep + 8 * e_pad);
    if (++ld_kc == nkc) {
      ld_kc = 0;
      if (++ld_unit < u1) {
        const int prev_qt = ld_qt;
        um.at(ld_unit, ld_qt, ld_et);
        if (ld_qt != prev_qt) ld_ent = tile_operand(ld_qt);
      }
    }
  };
  auto swrite = [&](int buf) {
    *reinterpret_cast<float4*>(&sq[buf][srow][sc4 * 4]) = rq0;
    *reinterpret_cast<float4*>(&sq[buf][srow + 8][sc4 * 4]) = rq1;
    *reinterpret_cast<float4*>(&se[buf][srow][sc4 * 4]) = re0;
    *reinterpret_cast<float4*>(&se[buf][srow + 8][sc4 * 4]) = re1;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  int cur_qt, cur_et;
  um.at(u0, cur_qt, cur_et);
  load_rows(cur_qt);
  gload();
  swrite(0);
  __syncthreads();

  uint32_t tw0 = 0u, tw1 = 0u;  // type constraints: the words of this lane's two entity columns
  int buf = 0;
  for (int unit = u0; unit < u1; ++unit) {
    for (int kc = 0; kc < nkc; ++kc) {
      const bool more = ld_unit < u1;
      if (more) gload();
      if constexpr (TC) {
        if (kc == 0) {  // the unit's type words, under its MFMAs
          const int64_t w = ((int64_t)cur_et * TE + we * 64) >> 5;
          tw0 = w < type_words ? cur_tm[w] : 0u;
          tw1 = w + 1 < type_words ? cur_tm[w + 1] : 0u;
        }
      }
      // the next stage's loads stay at the top of this one (k_sweep_mfma)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kp2 = 0; kp2 < KS; kp2 += 2) {
        const float a0 = sq[buf][kp2 + lrow][wq * 64 + lcol];
        const float a1 = sq[buf][kp2 + lrow][wq * 64 + 32 + lcol];
        const float b0 = se[buf][kp2 + lrow][we * 64 + lcol];
        const float b1 = se[buf][kp2 + lrow][we * 64 + 32 + lcol];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if (kc == nkc - 1) {  // unit finished: rank epilogue
        const int64_t ebase = (int64_t)cur_et * TE + we * 64;
        const int64_t e0 = ebase + lcol, e1 = ebase + 32 + lcol;
        const bool ev0 = e0 < n_ent, ev1 = e1 < n_ent;
        const bool tb0 = TC && ((tw0 >> lcol) & 1u), tb1 = TC && ((tw1 >> lcol) & 1u);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) {
          float tv[16];  // the lane's 16 row thresholds of block bi: 4 LDS reads issued together
#pragma unroll
          for (int r4 = 0; r4 < 16; r4 += 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(&s_th[tpar][row_of(bi, r4)]);
            tv[r4] = t4.x;
            tv[r4 + 1] = t4.y;
            tv[r4 + 2] = t4.z;
            tv[r4 + 3] = t4.w;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // row (bi, r) of lane half lrow is wave row L0 + 4 lrow; its 64 compares (2 column
            // blocks x 32 lanes) are counted by two ballots
            const float v0 = pred(acc[bi][0][r]), v1 = pred(acc[bi][1][r]);
            const bool b0 = ev0 && v0 < tv[r], b1 = ev1 && v1 < tv[r];
            const uint64_t m0 = __ballot(b0), m1 = __ballot(b1);
            const int L0 = bi * 32 + (r & 3) + 8 * (r >> 2);
            const int c_lo = __popcll(m0 & 0xffffffffull) + __popcll(m1 & 0xffffffffull);
            const int c_hi = __popcll(m0 >> 32) + __popcll(m1 >> 32);
            cntv += lane == L0 ? c_lo : (lane == L0 + 4 ? c_hi : 0);
            if constexpr (TC) {
              const uint64_t t0 = __ballot(b0 && tb0), t1 = __ballot(b1 && tb1);
              cntv_tc += lane == L0 ? __popcll(t0 & 0xffffffffull) + __popcll(t1 & 0xffffffffull)
                                    : (lane == L0 + 4 ? __popcll(t0 >> 32) + __popcll(t1 >> 32) : 0);
            }
          }
        }
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;
        const bool last = unit + 1 >= u1;
        int next_qt = cur_qt, next_et = cur_et;
        if (!last) um.at(unit + 1, next_qt, next_et);
        if (last || next_qt != cur_qt) {  // uniform: leave this query tile
          flush_rows(cur_qt);
          if (!last) load_rows(next_qt);
        }
        cur_qt = next_qt;
        cur_et = next_et;
      }
      if (more) swrite(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }
}

// ------------------------------------------------------------------- rows ----
// predict of arbitrary rows, one thread per row, from the raw tables: both chains restated with
// fmaf on the VALU -- tr_i over ascending j, then s over ascending i -- the MFMA's chains.
__global__ __launch_bounds__(128) void k_rescal_rows(const float* __restrict__ ent, const float* __restrict__ mats,
                                                     int64_t n_ent, int64_t n_rel, int dim,
                                                     const int64_t* __restrict__ hs, const int64_t* __restrict__ rs,
                                                     const int64_t* __restrict__ ts, int64_t n_rows, int pred_kind,
                                                     float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t h = hs[i], r = rs[i], t = ts[i];
  if (h < 0 || h >= n_ent || t < 0 || t >= n_ent || r < 0 || r >= n_rel) {
    out[i] = __builtin_nanf("");
    return;
  }
  const float* M = mats + r * ((int64_t)dim * dim);
  const float* xh = ent + h * dim;
  const float* xt = ent + t * dim;
  float s = 0.0f;
  for (int a = 0; a < dim; ++a) {
    const float* row = M + (int64_t)a * dim;
    float tr = 0.0f;
    for (int j = 0; j < dim; ++j) tr = __builtin_fmaf(row[j], xt[j], tr);
    s = __builtin_fmaf(xh[a], tr, s);
  }
  out[i] = apply_pred(pred_kind, 0.0f, s);
}

// ------------------------------------------------------------------ host ----
inline bool rs_dim(int dim) { return dim >= 1 && dim <= RS_MAX_DIM; }

struct RSWork {
  float *planes, *ent_km, *q_km, *list_v;
  int32_t* row_q;
};
int64_t rs_layout(RSWork& W, int64_t n_ent, int dim, int64_t n_tiles, int64_t n_used, int64_t n_entries, void* base) {
  const int64_t kp = rs_kp(dim), e_pad = round_up(n_ent > 0 ? n_ent : 1, TE);
  int64_t at = 0;
  auto carve = [&](int64_t bytes) {
    void* p = base ? (char*)base + at : nullptr;
    at += round_up(bytes, 256);
    return p;
  };
  W.planes = (float*)carve(n_used * kp * e_pad * 4);
  W.ent_km = (float*)carve(kp * e_pad * 4);
  W.q_km = (float*)carve(kp * n_tiles * TQ * 4);
  W.row_q = (int32_t*)carve(n_tiles * TQ * 4);
  W.list_v = (float*)carve((n_entries > 0 ? n_entries : 1) * 4);
  return at;
}

template <bool TC, int PK>
int rs_launch_sweep(hipStream_t st, const RSEval& P, const RSWork& W, const int32_t* tiles, int64_t n_tiles,
                    const float* thr, const uint32_t* type_head, const uint32_t* type_tail, int32_t* counts) {
  const int n_et = (int)(P.e_pad / TE), n_qt = (int)n_tiles;
  // the grid rule of the TransH / TransR sweeps: 16 short static ranges per resident slot, no more
  // workgroups than the busiest XCD group has units
  int g = 16 * resident_groups((const void*)k_sweep_rescal<TC, PK>, NT);
  const int64_t units = sweep_units(n_qt, n_et);
  if (units < g) g = (int)(units > 0 ? units : 1);
  hipLaunchKernelGGL((k_sweep_rescal<TC, PK>), dim3((unsigned)g), dim3(NT), 0, st, P, W.q_km, n_tiles * TQ, tiles,
                     n_qt, n_et, xcd_groups(g, n_et), thr, W.row_q, type_head, type_tail, (P.n_ent + 31) / 32,
                     counts);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_rescal_workspace(int64_t n_ent, int64_t n_rel, int dim, int64_t n_tiles, int64_t n_used,
                                         int64_t n_entries) {
  if (n_ent <= 0 || n_rel <= 0 || !rs_dim(dim) || n_tiles < 0 || n_used < 0 || n_entries < 0) return 0;
  RSWork W;
  return rs_layout(W, n_ent, dim, n_tiles, n_used, n_entries, nullptr);
}

extern "C" int mmre_rescal_evaluate(int model, int pred_kind, const float* d_ent, const float* d_rel_matrices,
                                    int64_t n_ent, int64_t n_rel, int dim, const int64_t* d_qh, const int64_t* d_qr,
                                    const int64_t* d_qt, const int8_t* d_qmode, int64_t n_query,
                                    const int32_t* d_perm, const int32_t* d_tiles, int64_t n_tiles,
                                    const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                                    const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                                    const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                                    int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                                    int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes,
                                    void* stream) {
  if (model != MMRE_RESCAL) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel_matrices || !d_qh || !d_qr || !d_qt || !d_qmode || !d_perm || !d_tiles || !d_used ||
      !d_rel_slot || !d_counts || !d_truth || !d_work)
    return MMRE_ERR_ARG;
  if (n_ent <= 0 || n_rel <= 0 || n_query <= 0 || n_tiles <= 0 || n_used <= 0 || n_used > n_rel) return MMRE_ERR_ARG;
  if (pred_kind != 0 && pred_kind != 2) return MMRE_ERR_ARG;
  if ((d_type_head == nullptr) != (d_type_tail == nullptr)) return MMRE_ERR_ARG;
  const bool grouped = d_grp_qoff != nullptr;
  if (grouped && (!d_grp_q || !d_filt_off || n_groups <= 0 || n_entries < 0 ||
                  (n_entries > 0 && (!d_filt_ids || !d_entry_q))))
    return MMRE_ERR_ARG;
  if (!grouped) n_entries = 0;
  if (!rs_dim(dim)) return MMRE_ERR_SHAPE;
  if (n_ent > (int64_t)INT32_MAX - 256 || n_query > (int64_t)INT32_MAX - 256 || n_tiles > (1 << 24))
    return MMRE_ERR_SHAPE;
  RSWork W;
  if (work_bytes < rs_layout(W, n_ent, dim, n_tiles, n_used, n_entries, d_work)) return MMRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = rs_kp(dim);
  const int64_t e_pad = round_up(n_ent, TE);
  hipLaunchKernelGGL(k_rs_ent_km, dim3((unsigned)std::min<int64_t>((kp * e_pad + 255) / 256, 1 << 20)), dim3(256), 0,
                     st, d_ent, n_ent, e_pad, dim, kp, W.ent_km);
  MMRE_CHECK_LAUNCH();
  // slot on y: consecutive workgroups share a relation's matrix and walk the entity table
  for (int64_t u = 0; u < n_used; u += 65535) {
    const int64_t nu = std::min<int64_t>(n_used - u, 65535);
    hipLaunchKernelGGL(k_rs_planes, dim3((unsigned)(e_pad / PL_COLS), (unsigned)nu), dim3(256), 0, st, d_ent,
                       d_rel_matrices, n_ent, e_pad, n_rel, dim, kp, d_used + u, nu, W.planes + u * kp * e_pad);
    MMRE_CHECK_LAUNCH();
  }
  RSEval P{d_ent, W.ent_km, W.planes, d_rel_slot, n_ent, e_pad, n_rel, n_used, n_query, dim, kp, d_qh, d_qr, d_qt,
           d_qmode};
  const bool tc = d_type_head != nullptr;
  const int64_t tasks = n_query + n_entries;
  const int64_t fc_grid = grouped ? std::min<int64_t>(n_groups, 1 << 20) : std::min<int64_t>((n_query + 63) / 64, 4096);
  hipLaunchKernelGGL(k_rs_queries, dim3((unsigned)n_tiles), dim3(TQ), 0, st, P, d_perm, d_tiles, n_tiles, W.q_km,
                     W.row_q);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rs_scores, dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st, P, pred_kind, d_entry_q,
                     d_filt_ids, n_entries, d_truth, W.list_v);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rs_filter_count, dim3((unsigned)fc_grid), dim3(64), 0, st, P, d_grp_qoff, d_grp_q, n_groups,
                     d_filt_off, d_filt_ids, W.list_v, n_entries, d_truth, d_type_head, d_type_tail,
                     (n_ent + 31) / 32, d_counts);
  MMRE_CHECK_LAUNCH();
  const int rs = with_bool(tc, [&](auto tc_) {
    constexpr bool TC = decltype(tc_)::value;
    return pred_kind == 0
               ? rs_launch_sweep<TC, 0>(st, P, W, d_tiles, n_tiles, d_truth, d_type_head, d_type_tail, d_counts)
               : rs_launch_sweep<TC, 2>(st, P, W, d_tiles, n_tiles, d_truth, d_type_head, d_type_tail, d_counts);
  });
  if (rs != MMRE_OK) return rs;
  return launch_finalize(st, d_counts, n_query, tc);  // filtered columns += raw columns
}

extern "C" int mmre_rescal_score_rows(int model, int pred_kind, const float* d_ent, const float* d_rel_matrices,
                                      int64_t n_ent, int64_t n_rel, int dim, const int64_t* d_h, const int64_t* d_r,
                                      const int64_t* d_t, int64_t n_rows, float* d_out, void* stream) {
  if (model != MMRE_RESCAL) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel_matrices || n_ent <= 0 || n_rel <= 0 || n_rows < 0) return MMRE_ERR_ARG;
  if (n_rows > 0 && (!d_h || !d_r || !d_t || !d_out)) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (!rs_dim(dim)) return MMRE_ERR_SHAPE;
  if (n_rows == 0) return MMRE_OK;
  hipLaunchKernelGGL(k_rescal_rows, dim3((unsigned)((n_rows + 127) / 128)), dim3(128), 0, (hipStream_t)stream, d_ent,
                     d_rel_matrices, n_ent, n_rel, dim, d_h, d_r, d_t, n_rows, pred_kind, d_out);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}
