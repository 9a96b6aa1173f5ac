// transr.hip -- TransR link prediction on MI355X: the relation projection on the matrix cores, the
// all-entity sweep over the projected planes with the fused rank epilogue, and predict for
// arbitrary rows (OpenKE/openke/module/model/TransR.py:37-103 under the Tester loop,
// Tester.py:70-91, Test.h:65-192).
//
// TransR moves an entity into the space of the query's relation with a dim_e x dim_r matrix,
// p(r, e) = normalize(e . M_r) (TransR.py:55-63, :40-44): a GEMM per relation, not a scalar pair
// per (relation, entity), so the staging threads of the sweep cannot make it. For every relation
// that occurs in the query set the prologue writes the projected table as a k-major plane
// P[slot][kp][e_pad] -- the sweep's own layout -- and every query tile of the sweep, which holds
// queries of ONE relation, stages its relation's plane as it is.
//
// Canonical arithmetic (TransR): f32. The projection is the one fused chain of the
// project, m_j = fma(e_{dim_e-1}, M[dim_e-1][j], ... fma(e_0, M[0][j], +0.0f)) in ascending i,
// because that is bit for bit what v_mfma_f32_32x32x2_f32 returns; k_transr_rows restates it with
// fmaf on the VALU. Everything after it is unfused, IEEE division and sqrtf, every sum one
// sequential chain in ascending k from 0.0f (TransH's th_q / th_step / th_final, restated here
// because transh.hip keeps them to itself). K rows padded with zeros leave the fused chain as it
// is: fma(0, 0, acc) = acc for every acc but -0, and a chain from +0.0f only reaches -0 after a
// product has underflowed.
//
// Kernels (one evaluation, one stream):
//   k_tr_relations     r_hat[R][kp] (normalised with norm_flag)
//   k_tr_project       P[slot] for every used relation: f32 MFMA, the row norm and the division
//                      in the epilogue
//   k_tr_queries       query vectors of the padded tile rows, gathered from the tile relation's plane
//   k_tr_scores        truth of every query and every listed entity of every filter group
//   k_tr_filter_count  one wave per filter group: counts = {0, -c, 0, -cc}
//   k_sweep_transr     128 x 128 units, 16 x 16 threads, 8 x 8 f32 accumulators, K in 8-row
//                      double-buffered LDS stages
//   k_transr_rows      predict of arbitrary (h, r, t) rows, one thread per row
// and, after the sweep, link.hip's finalize (launch_finalize: filtered columns += raw columns).
#include <algorithm>

#include "link_common.h"

namespace mmre {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR_MAX_DIM = 512;
__host__ __device__ inline int tr_kp(int dim) { return (int)round_up(dim, KC); }

// ------------------------------------------------------------ element functions ----
// F.normalize's denominator (TransR.py:41-43): max(sqrt(ss), 1e-12)
__device__ __forceinline__ float tr_den(float ss) {
  const float nr = sqrtf(ss);
  return nr < 1e-12f ? 1e-12f : nr;
}
// one element of the query vector from the projected anchor pa and r_hat (TransR.py:46-49):
// head_batch h + (r - t) -> q = -(r - t); tail_batch (h + r) - t -> q = h + r
__device__ __forceinline__ float tr_q(float pa, float rh, bool head) { return head ? -(rh - pa) : (pa + rh); }
template <bool L2>
__device__ __forceinline__ float tr_step(float s, float q, float p) {
  if constexpr (L2) {
    const float x = q - p;
    return s + x * x;
  } else {
    return s + fabsf(q - p);
  }
}
template <bool L2>
__device__ __forceinline__ float tr_final(float s) {
  if constexpr (L2) return sqrtf(s);
  else return s;
}

// ------------------------------------------------------------------ prologue ----
// One 64-thread workgroup per relation: r_hat = r / max(|r|, 1e-12) with norm_flag (TransR.py:42),
// else r; rows padded to kp with zeros. The norm is one sequential chain, by lane 0 from LDS.
__global__ __launch_bounds__(64) void k_tr_relations(const float* __restrict__ rel, int dim, int kp, int norm_flag,
                                                     float* __restrict__ r_hat) {
  extern __shared__ float lds[];  // [kp]
  __shared__ float s_den;
  const int64_t r = blockIdx.x;
  for (int k = threadIdx.x; k < kp; k += 64) lds[k] = k < dim ? rel[r * dim + k] : 0.0f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float ss = 0.0f;
    for (int k = 0; k < dim; ++k) ss = ss + lds[k] * lds[k];
    s_den = tr_den(ss);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kp; k += 64) r_hat[r * kp + k] = norm_flag ? lds[k] / s_den : lds[k];
}

// The projection. Workgroup (x, slot): PR_ROWS entity rows of the relation used[slot] over ALL
// dim_r columns, four waves. The columns go in chunks of PR_NC = four 32-wide MFMA tiles; wave w
// owns row tile w & 1 and the column tiles 2 (w >> 1), 2 (w >> 1) + 1 of the chunk: two f32x16
// accumulators that share the A operand. K runs in blocks of PR_KB rows through LDS -- A as
// sA[k][row] from the raw row-major entity table, B as sB[k][column] from the relation's raw
// transfer_matrix row -- the next block's values loaded into registers while the MFMAs of this one
// run. K ascends across blocks, across the instructions of a block and (the instruction's own
// order) inside an instruction; rows at or past dim_e are zeros in BOTH operands.
// A finished chunk goes to the LDS image m[j][row] (row stride PR_ST: the 32 columns of a wave's
// store hit 32 banks). After the last chunk thread `row` runs the norm's sequential chain over
// ascending j, and all threads divide and store to the k-major plane, 64 consecutive entities per
// row of it. Plane rows dim_r .. kp and the columns of entities at or past n_ent are zeros.
constexpr int PR_ROWS = 64, PR_NC = 128, PR_KB = 16, PR_SA = 68, PR_SB = 160, PR_ST = PR_ROWS + 1;
inline size_t pr_lds_bytes(int dim_r) {
  return ((size_t)dim_r * PR_ST + PR_KB * PR_SA + PR_KB * PR_SB + PR_ROWS) * sizeof(float);
}
template <bool NORM>
__global__ __launch_bounds__(256) void k_tr_project(const float* __restrict__ ent, const float* __restrict__ tmat,
                                                    int64_t n_ent, int64_t e_pad, int64_t n_rel, int dim_e, int dim_r,
                                                    int kp, const int32_t* __restrict__ used, int64_t n_used,
                                                    float* __restrict__ planes) {
  extern __shared__ float lds[];
  float* tile = lds;                              // [dim_r][PR_ST]
  float* sA = tile + (size_t)dim_r * PR_ST;       // [PR_KB][PR_SA]
  float* sB = sA + PR_KB * PR_SA;                 // [PR_KB][PR_SB]
  float* s_n = sB + PR_KB * PR_SB;                // [PR_ROWS]
  const int tid = threadIdx.x;
  const int64_t slot = blockIdx.y;
  const int64_t e0 = (int64_t)blockIdx.x * PR_ROWS;
  if (slot >= n_used || e0 + PR_ROWS > e_pad) return;  // uniform
  float* out = planes + slot * kp * e_pad;
  const int64_t r = used[slot];
  if (r < 0 || r >= n_rel) {  // uniform: a relation the tables do not hold gets a zero plane
    for (int idx = tid; idx < kp * PR_ROWS; idx += 256) out[(int64_t)(idx >> 6) * e_pad + e0 + (idx & 63)] = 0.0f;
    return;
  }
  const float* M = tmat + r * ((int64_t)dim_e * dim_r);

  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int rt = wave & 1, lc0 = (wave >> 1) * 64;  // row tile; first local column of the wave's two tiles
  // staging roles: A row a_row, k a_k .. a_k + 3; B column b_col, k b_k, b_k + 2, ..., b_k + 14
  const int a_row = tid >> 2, a_k = (tid & 3) * 4;
  const int b_col = tid & 127, b_k = tid >> 7;
  const int64_t a_e = e0 + a_row;
  const float* a_src = ent + a_e * dim_e;
  const bool a_in = a_e < n_ent;
  const int nkb = (dim_e + PR_KB - 1) / PR_KB;
  const bool a_vec = (dim_e & 3) == 0 && (reinterpret_cast<uintptr_t>(ent) & 15) == 0;

  for (int c0 = 0; c0 < dim_r; c0 += PR_NC) {
    const int j0 = c0 + lc0;
    const bool t0 = j0 < dim_r, t1 = j0 + 32 < dim_r;  // wave-uniform: tiles with a column to compute
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
    float ra[4], rb[8];
    auto gload = [&](int kb) {
      const int k0 = kb * PR_KB;
      if (a_vec) {  // uniform: the thread's four k are one aligned 16-B load (k0 + a_k + 3 < dim_e follows)
        const int k = k0 + a_k;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a_in && k < dim_e) v = *reinterpret_cast<const float4*>(a_src + k);
        ra[0] = v.x, ra[1] = v.y, ra[2] = v.z, ra[3] = v.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + a_k + u;
          ra[u] = (a_in && k < dim_e) ? a_src[k] : 0.0f;
        }
      }
      const int j = c0 + b_col;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + b_k + 2 * u;
        rb[u] = (k < dim_e && j < dim_r) ? M[(int64_t)k * dim_r + j] : 0.0f;
      }
    };
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
      __syncthreads();  // the block before is consumed
#pragma unroll
      for (int u = 0; u < 4; ++u) sA[(a_k + u) * PR_SA + a_row] = ra[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) sB[(b_k + 2 * u) * PR_SB + b_col] = rb[u];
      __syncthreads();
      if (kb + 1 < nkb) gload(kb + 1);
      if (t0) {
#pragma unroll
        for (int s = 0; s < PR_KB / 2; ++s) {
          const float a = sA[(2 * s + lh) * PR_SA + rt * 32 + li];
          const float b0 = sB[(2 * s + lh) * PR_SB + lc0 + li];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
          if (t1) {
            const float b1 = sB[(2 * s + lh) * PR_SB + lc0 + 32 + li];
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
          }
        }
      }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = rt * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
      if (j0 + li < dim_r) tile[(j0 + li) * PR_ST + row] = acc0[g];
      if (j0 + 32 + li < dim_r) tile[(j0 + 32 + li) * PR_ST + row] = acc1[g];
    }
  }
  __syncthreads();
  if constexpr (NORM) {
    if (tid < PR_ROWS) {
      // eight LDS reads in flight per round; the chain itself stays sequential in j
      float ss = 0.0f;
      int j = 0;
      for (; j + 8 <= dim_r; j += 8) {
        float m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) m[u] = tile[(j + u) * PR_ST + tid];
#pragma unroll
        for (int u = 0; u < 8; ++u) ss = ss + m[u] * m[u];
      }
      for (; j < dim_r; ++j) {
        const float m = tile[j * PR_ST + tid];
        ss = ss + m * m;
      }
      s_n[tid] = tr_den(ss);
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kp * PR_ROWS; idx += 256) {
    const int j = idx >> 6, row = idx & 63;
    float v = 0.0f;
    if (j < dim_r && e0 + row < n_ent) {
      v = tile[j * PR_ST + row];
      if constexpr (NORM) v = v / s_n[row];
    }
    out[(int64_t)j * e_pad + e0 + row] = v;
  }
}

// What the device kernels share about one evaluation.
struct TREval {
  const float* planes;      // [n_used][kp][e_pad] projected entities
  const float* r_hat;       // [n_rel][kp]
  const int32_t* rel_slot;  // [n_rel] -> the relation's plane, -1 for a relation without queries
  int64_t n_ent, e_pad, n_rel, n_used, n_query;
  int dim, kp;
  const int64_t *qh, *qr, *qt;
  const int8_t* qmode;
};

// (mode, relation, anchor, truth, slot) of query q, or false for ids outside the tables
struct TRQuery {
  bool head;
  int64_t r, anchor, truth, slot;
};
__device__ __forceinline__ bool tr_query(const TREval& P, int64_t q, TRQuery& Q) {
  if (q < 0 || q >= P.n_query) return false;
  const int64_t h = P.qh[q], t = P.qt[q];
  Q.r = P.qr[q];
  Q.head = P.qmode[q] == MMRE_HEAD_BATCH;
  Q.anchor = Q.head ? t : h;
  Q.truth = Q.head ? h : t;
  if (h < 0 || h >= P.n_ent || t < 0 || t >= P.n_ent || Q.r < 0 || Q.r >= P.n_rel) return false;
  Q.slot = P.rel_slot[Q.r];
  return Q.slot >= 0 && Q.slot < P.n_used;
}
// The score chain of one (anchor, candidate) pair, every operand from the stored plane
template <bool L2>
__device__ __forceinline__ float tr_pair(const TREval& P, const TRQuery& Q, int64_t cand) {
  const float* pl = P.planes + Q.slot * P.kp * P.e_pad;
  const float* rh = P.r_hat + Q.r * P.kp;
  float s = 0.0f;
  for (int k = 0; k < P.dim; ++k) {
    const float q = tr_q(pl[(int64_t)k * P.e_pad + Q.anchor], rh[k], Q.head);
    s = tr_step<L2>(s, q, pl[(int64_t)k * P.e_pad + cand]);
  }
  return tr_final<L2>(s);
}

// Query vectors of the padded tile rows, k-major q_km[kp][n_tiles * TQ], one thread per row; row_q:
// the row's query id in the caller's order (-1: padding, or a query / tile the tables do not hold).
__global__ __launch_bounds__(TQ) void k_tr_queries(TREval P, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ tiles, int64_t n_tiles,
                                                   float* __restrict__ q_km, int32_t* __restrict__ row_q) {
  const int64_t tile = blockIdx.x;
  const int64_t rel = tiles[3 * tile], first = tiles[3 * tile + 1], rows = tiles[3 * tile + 2];
  const int64_t q_pad = n_tiles * TQ, row = tile * TQ + threadIdx.x;
  TRQuery Q;
  int64_t q = -1;
  if (first >= 0 && rows >= 0 && rows <= TQ && first + rows <= P.n_query && (int64_t)threadIdx.x < rows) {
    q = perm[first + threadIdx.x];
    if (!tr_query(P, q, Q) || Q.r != rel) q = -1;
  }
  row_q[row] = (int32_t)q;
  if (q < 0) {
    for (int k = 0; k < P.kp; ++k) q_km[(int64_t)k * q_pad + row] = 0.0f;
    return;
  }
  const float* pl = P.planes + Q.slot * P.kp * P.e_pad + Q.anchor;
  const float* rh = P.r_hat + Q.r * P.kp;
  for (int k = 0; k < P.kp; ++k)
    q_km[(int64_t)k * q_pad + row] = k < P.dim ? tr_q(pl[(int64_t)k * P.e_pad], rh[k], Q.head) : 0.0f;
}

// ------------------------------------------------------- truth and filter pass ----
// One thread per chain: task t < n_query is the truth of query t -> thr[t]; task n_query + p is
// listed entity p of the filter CSR, scored for its group's representative query entry_q[p] ->
// list_v[p] (a group shares (mode, r, anchor): Test.h:85 `_find`). NaN marks what is never counted.
template <bool L2>
__global__ __launch_bounds__(256) void k_tr_scores(TREval P, int pred_kind, float margin,
                                                   const int32_t* __restrict__ entry_q,
                                                   const int32_t* __restrict__ ids, int64_t n_entries,
                                                   float* __restrict__ thr, float* __restrict__ list_v) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P.n_query + n_entries) return;
  TRQuery Q;
  if (t < P.n_query) {
    thr[t] = tr_query(P, t, Q) ? apply_pred(pred_kind, margin, tr_pair<L2>(P, Q, Q.truth)) : __builtin_nanf("");
    return;
  }
  const int64_t p = t - P.n_query;
  const int64_t j = ids[p];
  if (j < 0 || j >= P.n_ent || !tr_query(P, entry_q[p], Q)) {
    list_v[p] = __builtin_nanf("");
    return;
  }
  list_v[p] = apply_pred(pred_kind, margin, tr_pair<L2>(P, Q, j));
}

// One wave per filter group: the group's listed scores staged in LDS 64 at a time, every member
// (one per lane) counts those that beat its own truth (TransH's k_th_filter_count over TREval):
//   counts[.][q] = {0, -c, 0, -cc}, c = #{listed j != true(q) : pred(j) < thr[q]} (Test.h:85),
//   cc those the type constraint allows. grp_qoff == NULL: no filter, every query gets {0, 0, 0, 0}.
__global__ __launch_bounds__(64) void k_tr_filter_count(TREval P, const int64_t* __restrict__ grp_qoff,
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
    TRQuery G;
    const bool gv = tr_query(P, q0, G);
    const uint32_t* tm = (type_head && gv) ? (G.head ? type_head : type_tail) : nullptr;
    for (int64_t qc = qa; qc < qb; qc += 64) {
      const int64_t qi = qc + tid;
      int64_t q = qi < qb ? grp_q[qi] : -1;
      if (q >= nq) q = -1;
      const bool active = q >= 0;
      TRQuery Q;
      const bool qv = active && tr_query(P, q, Q);
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
template <bool TC>
struct TRSmem {
  float4 sq[2][KC][TQ / 4];
  float4 se[2][KC][TE / 4];
  float s_thr[2][TQ];
  int32_t s_true[2][TQ];
  int32_t s_q[2][TQ];
  int8_t s_head[2][TC ? TQ : 1];
  // type constraints: per unit (two in flight, by unit parity) the tile relation's head-side and
  // tail-side type words over the unit's 128 entity columns
  uint32_t s_tb[TC ? 2 : 1][2][4];
  // per-thread row counters of the query tile (off the VGPR budget)
  int32_t s_cnt[TC ? 2 : 1][8][NT];
};

// TransH's sweep geometry and epilogue (k_sweep_transh) over link_common.h's UnitMap: 256 threads
// as 16 (q) x 16 (e); a thread owns query rows {4tq..4tq+3, 64+4tq..} and entity columns
// {4te..4te+3, 64+4te..}: 64 f32 accumulators, one sequential k chain each. The loader runs one
// stage ahead of the compute and copies both operands as they are: the entity operand is the tile
// relation's projected plane. Per-row counts stay in the thread's LDS words until the workgroup
// leaves the query tile.
template <bool L2, bool TC, int PK>
__global__ __launch_bounds__(NT, 4) void k_sweep_transr(
    TREval P, const float* __restrict__ q_km, int64_t q_pad, const int32_t* __restrict__ tiles, int n_qt, int n_et,
    int n_groups, int pred_kind, float margin, const float* __restrict__ thr, const int32_t* __restrict__ row_q,
    const uint32_t* __restrict__ type_head, const uint32_t* __restrict__ type_tail, int64_t type_words,
    int32_t* __restrict__ counts) {
  __shared__ TRSmem<TC> sm;
  const int tid = threadIdx.x;
  const int tq = tid >> 4, te = tid & 15;
  const PredSel<PK> pred(pred_kind, margin);
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  const UnitMap um(grp, n_groups, n_qt, n_et);
  const int u0 = (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = (int)((int64_t)(gmem + 1) * um.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  const int kp = P.kp, nkc = kp / KC;
  const int64_t e_pad = P.e_pad, n_ent = P.n_ent, n_query = P.n_query;

  // the tile's relation, clamped to the tables (k_tr_queries emptied the rows of a tile they do not hold)
  auto tile_rel = [&](int qt, int64_t& rel, int64_t& slot) {
    rel = tiles[3 * (int64_t)qt];
    rel = rel < 0 ? 0 : (rel >= P.n_rel ? P.n_rel - 1 : rel);
    slot = P.rel_slot[rel];
    slot = slot < 0 ? 0 : (slot >= P.n_used ? P.n_used - 1 : slot);
  };
  auto load_meta = [&](int qt, int slot) {
    if (tid < TQ) {
      const int32_t q = row_q[(int64_t)qt * TQ + tid];
      const bool v = q >= 0 && q < n_query;
      bool head = false;
      int32_t tr = -1;
      if (v) {
        head = P.qmode[q] == MMRE_HEAD_BATCH;
        tr = (int32_t)(head ? P.qh[q] : P.qt[q]);
      }
      sm.s_thr[slot][tid] = v ? thr[q] : -INFINITY;
      sm.s_true[slot][tid] = tr;
      sm.s_q[slot][tid] = v ? q : -1;
      if constexpr (TC) sm.s_head[slot][tid] = head;
    }
  };

  // staging: stage row srow (one k), columns 4 sc4 .. 4 sc4 + 3 of both operands
  const int srow = tid >> 5, sc4 = tid & 31;
  float4 rq, re;
  uint32_t rt = 0u;    // type constraints: this thread's type word of the loader's unit (tid < 8)
  bool st_new = false;
  int ld_tpar = 1, st_par = 0, ep_par = 0;
  int ld_unit = u0, ld_kc = 0, ld_qt, ld_et;
  int64_t ld_rel = 0, ld_slot = 0;
  um.at(u0, ld_qt, ld_et);
  tile_rel(ld_qt, ld_rel, ld_slot);
  auto gload = [&]() {
    const int64_t e0 = (int64_t)ld_et * TE;
    if constexpr (TC) {
      if (ld_kc == 0) {  // the unit's first stage: its type words ride along
        ld_tpar ^= 1;
        st_par = ld_tpar;
        if (tid < 8) {
          const uint32_t* tm = ((tid >> 2) ? type_tail : type_head) + ld_rel * type_words;
          const int64_t w = (e0 >> 5) + (tid & 3);
          rt = w < type_words ? tm[w] : 0u;
        }
      }
      st_new = ld_kc == 0;
    }
    const int k = ld_kc * KC + srow;
    rq = *reinterpret_cast<const float4*>(q_km + (int64_t)k * q_pad + (int64_t)ld_qt * TQ + sc4 * 4);
    re = *reinterpret_cast<const float4*>(P.planes + (ld_slot * kp + k) * e_pad + e0 + sc4 * 4);
    if (++ld_kc == nkc) {
      ld_kc = 0;
      if (++ld_unit < u1) {
        const int prev_qt = ld_qt;
        um.at(ld_unit, ld_qt, ld_et);
        if (ld_qt != prev_qt) tile_rel(ld_qt, ld_rel, ld_slot);
      }
    }
  };
  auto swrite = [&](int buf) {
    if constexpr (TC) {
      if (st_new && tid < 8) sm.s_tb[TC ? st_par : 0][tid >> 2][tid & 3] = rt;
    }
    sm.sq[buf][srow][sc4] = rq;
    sm.se[buf][srow][sc4] = re;
  };

  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sm.s_cnt[0][i][tid] = 0;
    if constexpr (TC) sm.s_cnt[TC ? 1 : 0][i][tid] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
  }

  int cur_qt, cur_et;
  um.at(u0, cur_qt, cur_et);
  int slot = 0;
  load_meta(cur_qt, 0);
  gload();
  swrite(0);
  __syncthreads();

  int buf = 0;
  for (int unit = u0; unit < u1; ++unit) {
    for (int kc = 0; kc < nkc; ++kc) {
      const bool more = ld_unit < u1;
      if (more) gload();
#pragma unroll 2
      for (int kk = 0; kk < KC; ++kk) {
        const float4 a0 = sm.sq[buf][kk][tq], a1 = sm.sq[buf][kk][16 + tq];
        const float4 x0 = sm.se[buf][kk][te], x1 = sm.se[buf][kk][16 + te];
        const float qa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = tr_step<L2>(acc[i][j], qa[i], xv[j]);
      }
      if (kc == nkc - 1) {  // unit finished: rank epilogue
        const int ebase = cur_et * TE;
        uint32_t tbh = 0u, tbt = 0u;  // this thread's 8 type bits (bit j = column j), head / tail side
        if constexpr (TC) {
          const int sh = (te & 7) * 4, w = te >> 3;
          tbh = ((sm.s_tb[TC ? ep_par : 0][0][w] >> sh) & 15u) | (((sm.s_tb[TC ? ep_par : 0][0][2 + w] >> sh) & 15u) << 4);
          tbt = ((sm.s_tb[TC ? ep_par : 0][1][w] >> sh) & 15u) | (((sm.s_tb[TC ? ep_par : 0][1][2 + w] >> sh) & 15u) << 4);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
          const float th = sm.s_thr[slot][ql];
          const int32_t tr = sm.s_true[slot][ql];
          uint32_t tb = 0u;
          if constexpr (TC) tb = sm.s_head[slot][ql] ? tbh : tbt;
          int c = 0, cc = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int e = ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
            const float v = pred(tr_final<L2>(acc[i][j]));
            const bool better = (v < th) & (e != tr) & (e < n_ent);  // padded rows: th = -inf
            c += better;
            if constexpr (TC) cc += better & ((tb >> j) & 1u);
            acc[i][j] = 0.0f;
          }
          sm.s_cnt[0][i][tid] += c;
          if constexpr (TC) sm.s_cnt[TC ? 1 : 0][i][tid] += cc;
        }
        const bool last = unit + 1 >= u1;
        int next_qt = cur_qt, next_et = cur_et;
        if (!last) um.at(unit + 1, next_qt, next_et);
        if (last || next_qt != cur_qt) {  // uniform: flush this query tile's counts (raw columns)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            int c = sm.s_cnt[0][i][tid], cc = TC ? sm.s_cnt[TC ? 1 : 0][i][tid] : 0;
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) {
              c += __shfl_xor(c, sh);
              if constexpr (TC) cc += __shfl_xor(cc, sh);
            }
            const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
            const int32_t q = sm.s_q[slot][ql];
            if (te == 0 && q >= 0) {
              if (c) atomicAdd(&counts[q], c);
              if constexpr (TC) {
                if (cc) atomicAdd(&counts[2 * n_query + q], cc);
              }
            }
            sm.s_cnt[0][i][tid] = 0;
            if constexpr (TC) sm.s_cnt[TC ? 1 : 0][i][tid] = 0;
          }
          if (!last) {
            slot ^= 1;
            load_meta(next_qt, slot);  // visible after the stage's barrier below
          }
        }
        if constexpr (TC) ep_par ^= 1;
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
// predict of arbitrary rows, one thread per row, from the raw tables: both entities projected by
// the explicit fmaf chain in ascending i -- the MFMA's chain, restated on the VALU -- then the
// norms, r_hat and the score chain as the prologue and the sweep make them. With NORM the
// projection runs twice (once for the norms, once for the score) so that no thread keeps dim_r
// values. head != 0: the head_batch grouping h + (r - t), else (h + r) - t (TransR.py:46-49).
template <bool L2, bool NORM>
__global__ __launch_bounds__(128) void k_transr_rows(const float* __restrict__ ent, const float* __restrict__ rel,
                                                     const float* __restrict__ tmat, int64_t n_ent, int64_t n_rel,
                                                     int dim_e, int dim_r, const int64_t* __restrict__ hs,
                                                     const int64_t* __restrict__ rs, const int64_t* __restrict__ ts,
                                                     int64_t n_rows, int head, int pred_kind, float margin,
                                                     float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t h = hs[i], r = rs[i], t = ts[i];
  if (h < 0 || h >= n_ent || t < 0 || t >= n_ent || r < 0 || r >= n_rel) {
    out[i] = __builtin_nanf("");
    return;
  }
  const float* M = tmat + r * ((int64_t)dim_e * dim_r);
  const float* rr = rel + r * dim_r;
  const float* xa = ent + (head ? t : h) * dim_e;  // anchor
  const float* xc = ent + (head ? h : t) * dim_e;  // candidate
  auto project = [&](int j, float& ma, float& mc) {
    ma = mc = 0.0f;
    for (int k = 0; k < dim_e; ++k) {
      const float m = M[(int64_t)k * dim_r + j];
      ma = __builtin_fmaf(xa[k], m, ma);
      mc = __builtin_fmaf(xc[k], m, mc);
    }
  };
  float na = 1.0f, nc = 1.0f, dr = 1.0f;
  if constexpr (NORM) {
    float sa = 0.0f, sc = 0.0f, sr = 0.0f;
    for (int j = 0; j < dim_r; ++j) {
      float ma, mc;
      project(j, ma, mc);
      sa = sa + ma * ma;
      sc = sc + mc * mc;
      sr = sr + rr[j] * rr[j];
    }
    na = tr_den(sa);
    nc = tr_den(sc);
    dr = tr_den(sr);
  }
  float s = 0.0f;
  for (int j = 0; j < dim_r; ++j) {
    float pa, pc;
    project(j, pa, pc);
    if constexpr (NORM) {
      pa = pa / na;
      pc = pc / nc;
    }
    const float rh = NORM ? rr[j] / dr : rr[j];
    s = tr_step<L2>(s, tr_q(pa, rh, head != 0), pc);
  }
  out[i] = apply_pred(pred_kind, margin, tr_final<L2>(s));
}

// ------------------------------------------------------------------ host ----
inline bool tr_model(int m) { return m == MMRE_TRANSR_L1 || m == MMRE_TRANSR_L2; }
inline bool tr_dims(int dim_e, int dim_r) {
  return dim_e >= 1 && dim_e <= TR_MAX_DIM && dim_r >= 1 && dim_r <= TR_MAX_DIM;
}

struct TRWork {
  float *planes, *r_hat, *q_km, *list_v;
  int32_t* row_q;
};
int64_t tr_layout(TRWork& W, int64_t n_ent, int64_t n_rel, int dim_r, int64_t n_tiles, int64_t n_used,
                  int64_t n_entries, void* base) {
  const int64_t kp = tr_kp(dim_r), e_pad = round_up(n_ent > 0 ? n_ent : 1, TE);
  int64_t at = 0;
  auto carve = [&](int64_t bytes) {
    void* p = base ? (char*)base + at : nullptr;
    at += round_up(bytes, 256);
    return p;
  };
  W.planes = (float*)carve(n_used * kp * e_pad * 4);
  W.r_hat = (float*)carve(n_rel * kp * 4);
  W.q_km = (float*)carve(kp * n_tiles * TQ * 4);
  W.row_q = (int32_t*)carve(n_tiles * TQ * 4);
  W.list_v = (float*)carve((n_entries > 0 ? n_entries : 1) * 4);
  return at;
}

template <bool NORM>
int tr_launch_project(hipStream_t st, const float* d_ent, const float* d_tmat, int64_t n_ent, int64_t e_pad,
                      int64_t n_rel, int dim_e, int dim_r, int kp, const int32_t* d_used, int64_t n_used,
                      float* planes) {
  const size_t bytes = pr_lds_bytes(dim_r);
  MMRE_CHECK(hipFuncSetAttribute((const void*)k_tr_project<NORM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)bytes));
  // slot on y: consecutive workgroups share a relation's matrix and walk the entity table
  for (int64_t u = 0; u < n_used; u += 65535) {
    const int64_t nu = std::min<int64_t>(n_used - u, 65535);
    hipLaunchKernelGGL((k_tr_project<NORM>), dim3((unsigned)(e_pad / PR_ROWS), (unsigned)nu), dim3(256), bytes, st,
                       d_ent, d_tmat, n_ent, e_pad, n_rel, dim_e, dim_r, kp, d_used + u, nu,
                       planes + u * kp * e_pad);
    MMRE_CHECK_LAUNCH();
  }
  return MMRE_OK;
}

template <bool L2, bool TC, int PK>
int tr_launch_sweep(hipStream_t st, const TREval& P, const TRWork& W, const int32_t* tiles, int64_t n_tiles,
                    int pred_kind, float margin, const float* thr, const uint32_t* type_head,
                    const uint32_t* type_tail, int32_t* counts) {
  const int n_et = (int)(P.e_pad / TE), n_qt = (int)n_tiles;
  // 16 short static ranges per resident slot, as TransH's sweep; no more workgroups than the
  // busiest XCD group has units
  int g = 16 * resident_groups((const void*)k_sweep_transr<L2, TC, PK>, NT);
  const int64_t units = sweep_units(n_qt, n_et);
  if (units < g) g = (int)(units > 0 ? units : 1);
  hipLaunchKernelGGL((k_sweep_transr<L2, TC, PK>), dim3((unsigned)g), dim3(NT), 0, st, P, W.q_km, n_tiles * TQ, tiles,
                     n_qt, n_et, xcd_groups(g, n_et), pred_kind, margin, thr, W.row_q, type_head, type_tail,
                     (P.n_ent + 31) / 32, counts);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_transr_workspace(int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, int64_t n_tiles,
                                         int64_t n_used, int64_t n_entries) {
  if (n_ent <= 0 || n_rel <= 0 || !tr_dims(dim_e, dim_r) || n_tiles < 0 || n_used < 0 || n_entries < 0) return 0;
  TRWork W;
  return tr_layout(W, n_ent, n_rel, dim_r, n_tiles, n_used, n_entries, nullptr);
}

extern "C" int mmre_transr_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                    const float* d_rel, const float* d_transfer_matrix, int64_t n_ent, int64_t n_rel,
                                    int dim_e, int dim_r, const int64_t* d_qh, const int64_t* d_qr,
                                    const int64_t* d_qt, const int8_t* d_qmode, int64_t n_query,
                                    const int32_t* d_perm, const int32_t* d_tiles, int64_t n_tiles,
                                    const int32_t* d_used, int64_t n_used, const int32_t* d_rel_slot,
                                    const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                                    const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                                    int64_t n_entries, const uint32_t* d_type_head, const uint32_t* d_type_tail,
                                    int32_t* d_counts, float* d_truth, void* d_work, int64_t work_bytes,
                                    void* stream) {
  if (!tr_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_transfer_matrix || !d_qh || !d_qr || !d_qt || !d_qmode || !d_perm || !d_tiles ||
      !d_used || !d_rel_slot || !d_counts || !d_truth || !d_work)
    return MMRE_ERR_ARG;
  if (n_ent <= 0 || n_rel <= 0 || n_query <= 0 || n_tiles <= 0 || n_used <= 0 || n_used > n_rel) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 1) return MMRE_ERR_ARG;
  if ((d_type_head == nullptr) != (d_type_tail == nullptr)) return MMRE_ERR_ARG;
  const bool grouped = d_grp_qoff != nullptr;
  if (grouped && (!d_grp_q || !d_filt_off || n_groups <= 0 || n_entries < 0 ||
                  (n_entries > 0 && (!d_filt_ids || !d_entry_q))))
    return MMRE_ERR_ARG;
  if (!grouped) n_entries = 0;
  if (!tr_dims(dim_e, dim_r)) return MMRE_ERR_SHAPE;
  if (n_ent > (int64_t)INT32_MAX - 256 || n_query > (int64_t)INT32_MAX - 256 || n_tiles > (1 << 24))
    return MMRE_ERR_SHAPE;
  TRWork W;
  if (work_bytes < tr_layout(W, n_ent, n_rel, dim_r, n_tiles, n_used, n_entries, d_work)) return MMRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = tr_kp(dim_r);
  const int64_t e_pad = round_up(n_ent, TE);
  hipLaunchKernelGGL(k_tr_relations, dim3((unsigned)n_rel), dim3(64), kp * sizeof(float), st, d_rel, dim_r, kp,
                     norm_flag, W.r_hat);
  MMRE_CHECK_LAUNCH();
  const int rp = norm_flag ? tr_launch_project<true>(st, d_ent, d_transfer_matrix, n_ent, e_pad, n_rel, dim_e, dim_r,
                                                     kp, d_used, n_used, W.planes)
                           : tr_launch_project<false>(st, d_ent, d_transfer_matrix, n_ent, e_pad, n_rel, dim_e, dim_r,
                                                      kp, d_used, n_used, W.planes);
  if (rp != MMRE_OK) return rp;
  TREval P{W.planes, W.r_hat, d_rel_slot, n_ent, e_pad, n_rel, n_used, n_query, dim_r, kp, d_qh, d_qr, d_qt, d_qmode};
  const bool l2 = model == MMRE_TRANSR_L2, tc = d_type_head != nullptr;
  const int64_t tasks = n_query + n_entries;
  const int64_t fc_grid = grouped ? std::min<int64_t>(n_groups, 1 << 20) : std::min<int64_t>((n_query + 63) / 64, 4096);
  hipLaunchKernelGGL(k_tr_queries, dim3((unsigned)n_tiles), dim3(TQ), 0, st, P, d_perm, d_tiles, n_tiles, W.q_km,
                     W.row_q);
  MMRE_CHECK_LAUNCH();
  return with_bool(l2, [&](auto l2_) {
    constexpr bool L2 = decltype(l2_)::value;
    hipLaunchKernelGGL((k_tr_scores<L2>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st, P, pred_kind, margin,
                       d_entry_q, d_filt_ids, n_entries, d_truth, W.list_v);
    MMRE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tr_filter_count, dim3((unsigned)fc_grid), dim3(64), 0, st, P, d_grp_qoff, d_grp_q, n_groups,
                       d_filt_off, d_filt_ids, W.list_v, n_entries, d_truth, d_type_head, d_type_tail,
                       (n_ent + 31) / 32, d_counts);
    MMRE_CHECK_LAUNCH();
    const int rs = with_bool(tc, [&](auto tc_) {
      constexpr bool TC = decltype(tc_)::value;
      return pred_kind == 0 ? tr_launch_sweep<L2, TC, 0>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                         d_type_head, d_type_tail, d_counts)
                            : tr_launch_sweep<L2, TC, 1>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                         d_type_head, d_type_tail, d_counts);
    });
    if (rs != MMRE_OK) return rs;
    return launch_finalize(st, d_counts, n_query, tc);  // filtered columns += raw columns
  });
}

extern "C" int mmre_transr_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                      const float* d_rel, const float* d_transfer_matrix, int64_t n_ent,
                                      int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h, const int64_t* d_r,
                                      const int64_t* d_t, int64_t n_rows, int head_batch, float* d_out,
                                      void* stream) {
  if (!tr_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_transfer_matrix || n_ent <= 0 || n_rel <= 0 || n_rows < 0) return MMRE_ERR_ARG;
  if (n_rows > 0 && (!d_h || !d_r || !d_t || !d_out)) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (!tr_dims(dim_e, dim_r)) return MMRE_ERR_SHAPE;
  if (n_rows == 0) return MMRE_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n_rows + 127) / 128));
  return with_bool(model == MMRE_TRANSR_L2, [&](auto l2_) {
    return with_bool(norm_flag != 0, [&](auto nm_) {
      hipLaunchKernelGGL((k_transr_rows<decltype(l2_)::value, decltype(nm_)::value>), grid, dim3(128), 0, st, d_ent,
                         d_rel, d_transfer_matrix, n_ent, n_rel, dim_e, dim_r, d_h, d_r, d_t, n_rows, head_batch,
                         pred_kind, margin, d_out);
      MMRE_CHECK_LAUNCH();
      return (int)MMRE_OK;
    });
  });
}
