// transh.hip -- TransH link prediction on MI355X: the hyperplane-projected all-entity sweep with
// the fused rank epilogue, and predict for arbitrary rows (OpenKE/openke/module/model/
// TransH.py:52-115 under the Tester loop, Tester.py:70-91, Test.h:65-192).
//
// TransH projects an entity on the hyperplane of the query's relation, e_perp = e - (w_r . e) w_r
// (TransH.py:68-76), so an entity's sweep operand changes with the relation. The projected table
// is never materialised: per relation that occurs in the query set and per entity the prologue
// keeps the two scalars a(r, e) = e . w_r and n(r, e) = max(|e_perp|, 1e-12), every query tile of
// the sweep holds queries of ONE relation, and the staging threads turn the raw entity values
// into (e_k - a w_k) / n as they write LDS. The inner loop is TransE's f32 chain.
//
// Canonical arithmetic (TransH): f32, no contraction, IEEE division and sqrtf,
// every sum one sequential chain in ascending k from 0.0f. The sweep, the truth / filter pass and
// the rows kernel call the same element functions below, so a triple's score is one bit pattern
// wherever it is computed.
//
// Kernels (one evaluation, one stream):
//   k_th_relations     w_hat[R][kp] = F.normalize(norm_vector), r_hat[R][kp] (normalised with norm_flag)
//   k_th_an            (a, n)[used relation][entity] from the raw k-major planes
//   k_th_queries       query vectors of the padded tile rows, k-major, and the rows' query ids
//   k_th_scores        truth of every query and every listed entity of every filter group, one
//                      thread per chain
//   k_th_filter_count  one wave per filter group: counts = {0, -c, 0, -cc}
//   k_sweep_transh     128 x 128 units, 16 x 16 threads, 8 x 8 f32 accumulators, K in 8-row
//                      double-buffered LDS stages
//   k_transh_rows      predict of arbitrary (h, r, t) rows, one thread per row
// and, after the sweep, link.hip's finalize (launch_finalize: filtered columns += raw columns).
// The tile geometry, the type-bit lookup and the grid rules are the link sweeps' own
// (link_common.h).
#include <algorithm>

#include "link_common.h"

namespace mmre {
namespace {

// The tile geometry is the link sweeps' (link_common.h): TQ query rows per workgroup tile -- one
// relation per tile here -- x TE entities, KC K rows per LDS stage, NT threads.
__host__ __device__ inline int th_kp(int dim) { return (int)round_up(dim, KC); }

// ------------------------------------------------------------ element functions ----
// F.normalize's denominator (TransH.py:54-56, :69): max(sqrt(ss), 1e-12)
__device__ __forceinline__ float th_den(float ss) {
  const float nr = sqrtf(ss);
  return nr < 1e-12f ? 1e-12f : nr;
}
// one element of the projected entity: e_k - a w_k (multiply, then subtract), / n with norm_flag
template <bool NORM>
__device__ __forceinline__ float th_p(float e, float a, float w, float n) {
  const float p = e - a * w;
  if constexpr (NORM) return p / n;
  else return p;
}
// one element of the query vector from the projected anchor pa and r_hat (TransE's convention,
// TransH.py:61-64): head_batch h + (r - t) -> q = -(r - t); tail_batch (h + r) - t -> q = h + r
__device__ __forceinline__ float th_q(float pa, float rh, bool head) { return head ? -(rh - pa) : (pa + rh); }
template <bool L2>
__device__ __forceinline__ float th_step(float s, float q, float p) {
  if constexpr (L2) {
    const float x = q - p;
    return s + x * x;
  } else {
    return s + fabsf(q - p);
  }
}
template <bool L2>
__device__ __forceinline__ float th_final(float s) {
  if constexpr (L2) return sqrtf(s);
  else return s;
}

// The score chain of one (anchor, candidate) pair under relation vectors w (w_hat) and rh (r_hat):
// anchor = t and candidate = h for head_batch, anchor = h and candidate = t otherwise. aa / na and
// ac / nc: the anchor's and the candidate's (a, n).
template <bool L2, bool NORM>
__device__ __forceinline__ float th_chain(const float* __restrict__ anchor, const float* __restrict__ cand,
                                          const float* __restrict__ w, const float* __restrict__ rh, int dim,
                                          bool head, float aa, float na, float ac, float nc) {
  float s = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float wk = w[k];
    const float q = th_q(th_p<NORM>(anchor[k], aa, wk, na), rh[k], head);
    s = th_step<L2>(s, q, th_p<NORM>(cand[k], ac, wk, nc));
  }
  return th_final<L2>(s);
}

// ------------------------------------------------------------------ prologue ----
// One 64-thread workgroup per relation: w_hat = w / max(|w|, 1e-12) (TransH.py:69) and r_hat = r /
// max(|r|, 1e-12) with norm_flag (TransH.py:55), else r; rows padded to kp with zeros. The two
// norms are sequential chains, by lanes 0 and 1 from LDS.
__global__ __launch_bounds__(64) void k_th_relations(const float* __restrict__ norm_vec, const float* __restrict__ rel,
                                                     int dim, int kp, int norm_flag, float* __restrict__ w_hat,
                                                     float* __restrict__ r_hat) {
  extern __shared__ float lds[];  // [2][kp]
  __shared__ float s_den[2];
  const int64_t r = blockIdx.x;
  for (int k = threadIdx.x; k < kp; k += 64) {
    lds[k] = k < dim ? norm_vec[r * dim + k] : 0.0f;
    lds[kp + k] = k < dim ? rel[r * dim + k] : 0.0f;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* x = lds + threadIdx.x * kp;
    float ss = 0.0f;
    for (int k = 0; k < dim; ++k) ss = ss + x[k] * x[k];
    s_den[threadIdx.x] = th_den(ss);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kp; k += 64) {
    w_hat[r * kp + k] = lds[k] / s_den[0];
    r_hat[r * kp + k] = norm_flag ? lds[kp + k] / s_den[1] : lds[kp + k];
  }
}

// (a, n) of every entity column for AN_RB used relations per workgroup: a thread owns one column of
// the k-major planes (coalesced loads) and AN_RB pairs of chains, so a loaded value feeds AN_RB
// chains. Padded columns hold zeros: a = 0, n = 1e-12. Without norm_flag n is not read; 1 is stored.
constexpr int AN_RB = 4;
__global__ __launch_bounds__(256) void k_th_an(const float* __restrict__ ent_km, int64_t e_pad, int dim, int kp,
                                               const float* __restrict__ w_hat, const int32_t* __restrict__ used,
                                               int64_t n_used, int64_t n_rel, int norm_flag, float* __restrict__ an) {
  extern __shared__ float sw[];  // [AN_RB][kp]
  const int64_t u0 = (int64_t)blockIdx.y * AN_RB;
  for (int i = threadIdx.x; i < AN_RB * kp; i += 256) {
    const int64_t u = u0 + i / kp;
    int64_t r = u < n_used ? used[u] : -1;
    sw[i] = (r >= 0 && r < n_rel) ? w_hat[r * kp + i % kp] : 0.0f;
  }
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= e_pad) return;
  float a[AN_RB], ss[AN_RB];
#pragma unroll
  for (int j = 0; j < AN_RB; ++j) a[j] = ss[j] = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float x = ent_km[(int64_t)k * e_pad + e];
#pragma unroll
    for (int j = 0; j < AN_RB; ++j) a[j] = a[j] + x * sw[j * kp + k];
  }
  if (norm_flag) {
    for (int k = 0; k < dim; ++k) {
      const float x = ent_km[(int64_t)k * e_pad + e];
#pragma unroll
      for (int j = 0; j < AN_RB; ++j) {
        const float p = x - a[j] * sw[j * kp + k];
        ss[j] = ss[j] + p * p;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < AN_RB; ++j) {
    if (u0 + j >= n_used) break;
    an[(2 * (u0 + j)) * e_pad + e] = a[j];
    an[(2 * (u0 + j) + 1) * e_pad + e] = norm_flag ? th_den(ss[j]) : 1.0f;
  }
}

// What the device kernels share about one evaluation.
struct THEval {
  const float* ent_km;    // [kp][e_pad] raw
  const float* ent_rows;  // [n_ent][kp] raw, zero beyond dim
  const float* w_hat;     // [n_rel][kp]
  const float* r_hat;     // [n_rel][kp]
  const float* an;        // [n_used][2][e_pad]
  const int32_t* rel_slot;  // [n_rel] -> slot of the (a, n) table, -1 for a relation without queries
  int64_t n_ent, e_pad, n_rel, n_used, n_query;
  int dim, kp;
  const int64_t *qh, *qr, *qt;
  const int8_t* qmode;
};

// (mode, relation, anchor, truth, slot) of query q, or false for ids outside the tables
struct THQuery {
  bool head;
  int64_t r, anchor, truth, slot;
};
__device__ __forceinline__ bool th_query(const THEval& P, int64_t q, THQuery& Q) {
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
template <bool L2, bool NORM>
__device__ __forceinline__ float th_pair(const THEval& P, const THQuery& Q, int64_t cand) {
  const float* at = P.an + 2 * Q.slot * P.e_pad;
  return th_chain<L2, NORM>(P.ent_rows + Q.anchor * P.kp, P.ent_rows + cand * P.kp, P.w_hat + Q.r * P.kp,
                            P.r_hat + Q.r * P.kp, P.dim, Q.head, at[Q.anchor], at[P.e_pad + Q.anchor], at[cand],
                            at[P.e_pad + cand]);
}

// Query vectors of the padded tile rows, k-major q_km[kp][n_tiles * TQ], one thread per row; row_q:
// the row's query id in the caller's order (-1: padding, or a query / tile the tables do not hold).
template <bool NORM>
__global__ __launch_bounds__(TQ) void k_th_queries(THEval P, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ tiles, int64_t n_tiles,
                                                   float* __restrict__ q_km, int32_t* __restrict__ row_q) {
  const int64_t tile = blockIdx.x;
  const int64_t rel = tiles[3 * tile], first = tiles[3 * tile + 1], rows = tiles[3 * tile + 2];
  const int64_t q_pad = n_tiles * TQ, row = tile * TQ + threadIdx.x;
  THQuery Q;
  int64_t q = -1;
  if (first >= 0 && rows >= 0 && rows <= TQ && first + rows <= P.n_query && (int64_t)threadIdx.x < rows) {
    q = perm[first + threadIdx.x];
    if (!th_query(P, q, Q) || Q.r != rel) q = -1;
  }
  row_q[row] = (int32_t)q;
  if (q < 0) {
    for (int k = 0; k < P.kp; ++k) q_km[(int64_t)k * q_pad + row] = 0.0f;
    return;
  }
  const float* at = P.an + 2 * Q.slot * P.e_pad;
  const float aa = at[Q.anchor], na = at[P.e_pad + Q.anchor];
  const float* x = P.ent_rows + Q.anchor * P.kp;
  const float* w = P.w_hat + Q.r * P.kp;
  const float* rh = P.r_hat + Q.r * P.kp;
  for (int k = 0; k < P.kp; ++k)
    q_km[(int64_t)k * q_pad + row] = k < P.dim ? th_q(th_p<NORM>(x[k], aa, w[k], na), rh[k], Q.head) : 0.0f;
}

// ------------------------------------------------------- truth and filter pass ----
// One thread per chain: task t < n_query is the truth of query t -> thr[t]; task n_query + p is
// listed entity p of the filter CSR, scored for its group's representative query entry_q[p] ->
// list_v[p] (a group shares (mode, r, anchor): Test.h:85 `_find`). NaN marks what is never counted.
template <bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_th_scores(THEval P, int pred_kind, float margin,
                                                   const int32_t* __restrict__ entry_q,
                                                   const int32_t* __restrict__ ids, int64_t n_entries,
                                                   float* __restrict__ thr, float* __restrict__ list_v) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P.n_query + n_entries) return;
  THQuery Q;
  if (t < P.n_query) {
    thr[t] = th_query(P, t, Q) ? apply_pred(pred_kind, margin, th_pair<L2, NORM>(P, Q, Q.truth)) : __builtin_nanf("");
    return;
  }
  const int64_t p = t - P.n_query;
  const int64_t j = ids[p];
  if (j < 0 || j >= P.n_ent || !th_query(P, entry_q[p], Q)) {
    list_v[p] = __builtin_nanf("");
    return;
  }
  list_v[p] = apply_pred(pred_kind, margin, th_pair<L2, NORM>(P, Q, j));
}

// One wave per filter group: the group's listed scores staged in LDS 64 at a time, every member
// (one per lane) counts those that beat its own truth (link.hip's k_filter_count, restated):
//   counts[.][q] = {0, -c, 0, -cc}, c = #{listed j != true(q) : pred(j) < thr[q]} (Test.h:85),
//   cc those the type constraint allows. grp_qoff == NULL: no filter, every query gets {0, 0, 0, 0}.
__global__ __launch_bounds__(64) void k_th_filter_count(THEval P, const int64_t* __restrict__ grp_qoff,
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
    THQuery G;
    const bool gv = th_query(P, q0, G);
    const uint32_t* tm = (type_head && gv) ? (G.head ? type_head : type_tail) : nullptr;
    for (int64_t qc = qa; qc < qb; qc += 64) {
      const int64_t qi = qc + tid;
      int64_t q = qi < qb ? grp_q[qi] : -1;
      if (q >= nq) q = -1;
      const bool active = q >= 0;
      THQuery Q;
      const bool qv = active && th_query(P, q, Q);
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
// Work unit = (query tile) x (entity tile). XCD group g (workgroups g, g + G, ...: the ones the
// round-robin dispatch places on one XCD when the grid is a multiple of G = 8) owns n_et / G whole
// entity tiles for every query tile, query-tile major, then a 1 / G share of the leftover tiles'
// units; a workgroup sweeps one contiguous range of its group's units. This is link_common.h's
// UnitMap without its entity-major order, kept as a type of its own: with UnitMap (emajor left at
// its default) the four type-constrained k_sweep_transh instances allocate their SGPRs differently
// -- the same instructions on other registers -- and the sweep is held to its measured code.
struct THUnitMap {
  int m, r, ex0, el0, n_main, lo0, count;
  __device__ __forceinline__ THUnitMap(int grp, int n_groups, int n_qt, int n_et) {
    m = n_et / n_groups;
    r = n_et - m * n_groups;
    ex0 = grp * m;
    el0 = m * n_groups;
    n_main = n_qt * m;
    const int64_t left = (int64_t)n_qt * r;
    lo0 = (int)(left * grp / n_groups);
    count = n_main + (int)(left * (grp + 1) / n_groups) - lo0;
  }
  __device__ __forceinline__ void at(int i, int& qt, int& et) const {
    if (i < n_main) {
      qt = i / m;
      et = ex0 + i % m;
    } else {
      const int j = lo0 + (i - n_main);
      qt = j / r;
      et = el0 + j % r;
    }
  }
};

template <bool TC>
struct THSmem {
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

// 256 threads as 16 (q) x 16 (e); a thread owns query rows {4tq..4tq+3, 64+4tq..} and entity
// columns {4te..4te+3, 64+4te..}: 64 f32 accumulators, one sequential k chain each. The loader
// runs one stage ahead of the compute; it holds the unit's (a, n) of its four columns in registers
// and projects the raw entity values as it writes them to LDS. Per-row counts stay in the
// thread's LDS words until the workgroup leaves the query tile.
template <bool L2, bool TC, int PK, bool NORM>
__global__ __launch_bounds__(NT, 4) void k_sweep_transh(
    THEval P, const float* __restrict__ q_km, int64_t q_pad, const int32_t* __restrict__ tiles, int n_qt, int n_et,
    int n_groups, int pred_kind, float margin, const float* __restrict__ thr, const int32_t* __restrict__ row_q,
    const uint32_t* __restrict__ type_head, const uint32_t* __restrict__ type_tail, int64_t type_words,
    int32_t* __restrict__ counts) {
  __shared__ THSmem<TC> sm;
  const int tid = threadIdx.x;
  const int tq = tid >> 4, te = tid & 15;
  const PredSel<PK> pred(pred_kind, margin);
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  const THUnitMap um(grp, n_groups, n_qt, n_et);
  const int u0 = (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = (int)((int64_t)(gmem + 1) * um.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  const int kp = P.kp, nkc = kp / KC;
  const int64_t e_pad = P.e_pad, n_ent = P.n_ent, n_query = P.n_query;

  // the tile's relation, clamped to the tables (k_th_queries emptied the rows of a tile they do not hold)
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
  float4 la = {0.0f, 0.0f, 0.0f, 0.0f}, ln = {1.0f, 1.0f, 1.0f, 1.0f};  // the loader unit's (a, n) of its columns
  float rw = 0.0f;     // w_hat[k] of the pending stage
  uint32_t rt = 0u;    // type constraints: this thread's type word of the loader's unit (tid < 8)
  bool st_new = false;
  int ld_tpar = 1, st_par = 0, ep_par = 0;
  int ld_unit = u0, ld_kc = 0, ld_qt, ld_et;
  int64_t ld_rel = 0, ld_slot = 0;
  um.at(u0, ld_qt, ld_et);
  tile_rel(ld_qt, ld_rel, ld_slot);
  auto gload = [&]() {
    const int64_t e0 = (int64_t)ld_et * TE;
    if (ld_kc == 0) {  // the unit's first stage: its columns' (a, n) and type words ride along
      const float* at = P.an + 2 * ld_slot * e_pad + e0 + sc4 * 4;
      la = *reinterpret_cast<const float4*>(at);
      if constexpr (NORM) ln = *reinterpret_cast<const float4*>(at + e_pad);
      if constexpr (TC) {
        ld_tpar ^= 1;
        st_par = ld_tpar;
        if (tid < 8) {
          const uint32_t* tm = ((tid >> 2) ? type_tail : type_head) + ld_rel * type_words;
          const int64_t w = (e0 >> 5) + (tid & 3);
          rt = w < type_words ? tm[w] : 0u;
        }
      }
    }
    if constexpr (TC) st_new = ld_kc == 0;
    const int k = ld_kc * KC + srow;
    rq = *reinterpret_cast<const float4*>(q_km + (int64_t)k * q_pad + (int64_t)ld_qt * TQ + sc4 * 4);
    re = *reinterpret_cast<const float4*>(P.ent_km + (int64_t)k * e_pad + e0 + sc4 * 4);
    rw = P.w_hat[ld_rel * kp + k];
    if (++ld_kc == nkc) {
      ld_kc = 0;
      if (++ld_unit < u1) {
        const int prev_qt = ld_qt;
        um.at(ld_unit, ld_qt, ld_et);
        if (ld_qt != prev_qt) tile_rel(ld_qt, ld_rel, ld_slot);
      }
    }
  };
  // (la / ln are rewritten by gload only at a unit's first stage, which follows the swrite of the
  // unit before's last stage: every swrite sees its own unit's values)
  auto swrite = [&](int buf) {
    if constexpr (TC) {
      if (st_new && tid < 8) sm.s_tb[TC ? st_par : 0][tid >> 2][tid & 3] = rt;
    }
    sm.sq[buf][srow][sc4] = rq;
    float4 p;
    p.x = th_p<NORM>(re.x, la.x, rw, ln.x);
    p.y = th_p<NORM>(re.y, la.y, rw, ln.y);
    p.z = th_p<NORM>(re.z, la.z, rw, ln.z);
    p.w = th_p<NORM>(re.w, la.w, rw, ln.w);
    sm.se[buf][srow][sc4] = p;
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
          for (int j = 0; j < 8; ++j) acc[i][j] = th_step<L2>(acc[i][j], qa[i], xv[j]);
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
            const float v = pred(th_final<L2>(acc[i][j]));
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
// predict of arbitrary rows, one thread per row: w_hat and r_hat of the row's relation and (a, n)
// of both entities from the raw tables, by the chains of the prologue; then the score chain.
// head != 0: the head_batch grouping h + (r - t), else (h + r) - t (TransH.py:61-64).
template <bool L2, bool NORM>
__global__ __launch_bounds__(128) void k_transh_rows(const float* __restrict__ ent, const float* __restrict__ rel,
                                                     const float* __restrict__ norm_vec, int64_t n_ent,
                                                     int64_t n_rel, int dim, const int64_t* __restrict__ hs,
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
  const float* w = norm_vec + r * dim;
  const float* rr = rel + r * dim;
  float sw = 0.0f, sr = 0.0f;
  for (int k = 0; k < dim; ++k) sw = sw + w[k] * w[k];
  const float dw = th_den(sw);
  float dr = 1.0f;
  if constexpr (NORM) {
    for (int k = 0; k < dim; ++k) sr = sr + rr[k] * rr[k];
    dr = th_den(sr);
  }
  const float* xa = ent + (head ? t : h) * dim;  // anchor
  const float* xc = ent + (head ? h : t) * dim;  // candidate
  float aa = 0.0f, ac = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float wk = w[k] / dw;
    aa = aa + xa[k] * wk;
    ac = ac + xc[k] * wk;
  }
  float na = 1.0f, nc = 1.0f;
  if constexpr (NORM) {
    float sa = 0.0f, sc = 0.0f;
    for (int k = 0; k < dim; ++k) {
      const float wk = w[k] / dw;
      const float pa = xa[k] - aa * wk, pc = xc[k] - ac * wk;
      sa = sa + pa * pa;
      sc = sc + pc * pc;
    }
    na = th_den(sa);
    nc = th_den(sc);
  }
  float s = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float wk = w[k] / dw;
    const float rh = NORM ? rr[k] / dr : rr[k];
    const float q = th_q(th_p<NORM>(xa[k], aa, wk, na), rh, head != 0);
    s = th_step<L2>(s, q, th_p<NORM>(xc[k], ac, wk, nc));
  }
  out[i] = apply_pred(pred_kind, margin, th_final<L2>(s));
}

// ------------------------------------------------------------------ host ----
inline bool th_model(int m) { return m == MMRE_TRANSH_L1 || m == MMRE_TRANSH_L2; }

struct THWork {
  float *ent_km, *ent_rows, *w_hat, *r_hat, *an, *q_km, *list_v;
  int32_t* row_q;
};
int64_t th_layout(THWork& W, int64_t n_ent, int64_t n_rel, int dim, int64_t n_tiles, int64_t n_used,
                  int64_t n_entries, void* base) {
  const int64_t kp = th_kp(dim), e_pad = round_up(n_ent > 0 ? n_ent : 1, TE);
  int64_t at = 0;
  auto carve = [&](int64_t bytes) {
    void* p = base ? (char*)base + at : nullptr;
    at += round_up(bytes, 256);
    return p;
  };
  W.ent_km = (float*)carve(kp * e_pad * 4);
  W.ent_rows = (float*)carve(n_ent * kp * 4);
  W.w_hat = (float*)carve(n_rel * kp * 4);
  W.r_hat = (float*)carve(n_rel * kp * 4);
  W.an = (float*)carve(2 * n_used * e_pad * 4);
  W.q_km = (float*)carve(kp * n_tiles * TQ * 4);
  W.row_q = (int32_t*)carve(n_tiles * TQ * 4);
  W.list_v = (float*)carve((n_entries > 0 ? n_entries : 1) * 4);
  return at;
}

template <bool L2, bool TC, int PK, bool NORM>
int th_launch_sweep(hipStream_t st, const THEval& P, const THWork& W, const int32_t* tiles, int64_t n_tiles,
                    int pred_kind, float margin, const float* thr, const uint32_t* type_head,
                    const uint32_t* type_tail, int32_t* counts) {
  const int n_et = (int)(P.e_pad / TE), n_qt = (int)n_tiles;
  // 16 short static ranges per resident slot, as the link f32 sweep's (valu_grid, link_valu.hip);
  // no more workgroups than the busiest XCD group has units
  int g = 16 * resident_groups((const void*)k_sweep_transh<L2, TC, PK, NORM>, NT);
  const int64_t units = sweep_units(n_qt, n_et);
  if (units < g) g = (int)(units > 0 ? units : 1);
  hipLaunchKernelGGL((k_sweep_transh<L2, TC, PK, NORM>), dim3((unsigned)g), dim3(NT), 0, st, P, W.q_km, n_tiles * TQ,
                     tiles, n_qt, n_et, xcd_groups(g, n_et), pred_kind, margin, thr, W.row_q, type_head, type_tail,
                     (P.n_ent + 31) / 32, counts);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_transh_workspace(int64_t n_ent, int64_t n_rel, int dim, int64_t n_tiles, int64_t n_used,
                                         int64_t n_entries) {
  if (n_ent <= 0 || n_rel <= 0 || dim <= 0 || n_tiles < 0 || n_used < 0 || n_entries < 0) return 0;
  THWork W;
  return th_layout(W, n_ent, n_rel, dim, n_tiles, n_used, n_entries, nullptr);
}

extern "C" int mmre_transh_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                    const float* d_rel, const float* d_norm, int64_t n_ent, int64_t n_rel, int dim,
                                    const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                                    const int8_t* d_qmode, int64_t n_query, const int32_t* d_perm,
                                    const int32_t* d_tiles, int64_t n_tiles, const int32_t* d_used, int64_t n_used,
                                    const int32_t* d_rel_slot, const int64_t* d_grp_qoff, const int32_t* d_grp_q,
                                    int64_t n_groups, const int64_t* d_filt_off, const int32_t* d_filt_ids,
                                    const int32_t* d_entry_q, int64_t n_entries, const uint32_t* d_type_head,
                                    const uint32_t* d_type_tail, int32_t* d_counts, float* d_truth, void* d_work,
                                    int64_t work_bytes, void* stream) {
  if (!th_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_norm || !d_qh || !d_qr || !d_qt || !d_qmode || !d_perm || !d_tiles || !d_used ||
      !d_rel_slot || !d_counts || !d_truth || !d_work)
    return MMRE_ERR_ARG;
  if (n_ent <= 0 || n_rel <= 0 || n_query <= 0 || n_tiles <= 0 || n_used <= 0 || n_used > n_rel) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 1) return MMRE_ERR_ARG;
  if ((d_type_head == nullptr) != (d_type_tail == nullptr)) return MMRE_ERR_ARG;
  const bool grouped = d_grp_qoff != nullptr;
  if (grouped && (!d_grp_q || !d_filt_off || n_groups <= 0 || n_entries < 0 ||
                  (n_entries > 0 && (!d_filt_ids || !d_entry_q))))
    return MMRE_ERR_ARG;
  if (!grouped) n_entries = 0;
  if (dim <= 0) return MMRE_ERR_SHAPE;
  if (n_ent > (int64_t)INT32_MAX - 256 || n_query > (int64_t)INT32_MAX - 256 || n_tiles > (1 << 24))
    return MMRE_ERR_SHAPE;
  THWork W;
  if (work_bytes < th_layout(W, n_ent, n_rel, dim, n_tiles, n_used, n_entries, d_work)) return MMRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = th_kp(dim);
  const int64_t e_pad = round_up(n_ent, TE);
  // the raw k-major planes and the row-major copy: TransE's preparation without normalisation
  const int rc = mmre_link_prepare_entities(MMRE_TRANSE_L1, 0, d_ent, nullptr, n_ent, dim, W.ent_km, e_pad, W.ent_rows,
                                            stream);
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_th_relations, dim3((unsigned)n_rel), dim3(64), 2 * kp * sizeof(float), st, d_norm, d_rel, dim,
                     kp, norm_flag, W.w_hat, W.r_hat);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_th_an, dim3((unsigned)(e_pad / 256 + (e_pad % 256 != 0)), (unsigned)((n_used + AN_RB - 1) / AN_RB)),
                     dim3(256), AN_RB * kp * sizeof(float), st, W.ent_km, e_pad, dim, kp, W.w_hat, d_used, n_used,
                     n_rel, norm_flag, W.an);
  MMRE_CHECK_LAUNCH();
  THEval P{W.ent_km, W.ent_rows, W.w_hat, W.r_hat, W.an, d_rel_slot, n_ent, e_pad, n_rel, n_used, n_query,
           dim,      kp,         d_qh,    d_qr,    d_qt, d_qmode};
  const bool l2 = model == MMRE_TRANSH_L2, tc = d_type_head != nullptr;
  const int64_t tasks = n_query + n_entries;
  const int64_t fc_grid = grouped ? std::min<int64_t>(n_groups, 1 << 20) : std::min<int64_t>((n_query + 63) / 64, 4096);
  return with_bool(l2, [&](auto l2_) {
    return with_bool(norm_flag != 0, [&](auto nm_) {
      constexpr bool L2 = decltype(l2_)::value, NORM = decltype(nm_)::value;
      hipLaunchKernelGGL((k_th_queries<NORM>), dim3((unsigned)n_tiles), dim3(TQ), 0, st, P, d_perm, d_tiles, n_tiles,
                         W.q_km, W.row_q);
      MMRE_CHECK_LAUNCH();
      hipLaunchKernelGGL((k_th_scores<L2, NORM>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st, P, pred_kind,
                         margin, d_entry_q, d_filt_ids, n_entries, d_truth, W.list_v);
      MMRE_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_th_filter_count, dim3((unsigned)fc_grid), dim3(64), 0, st, P, d_grp_qoff, d_grp_q, n_groups,
                         d_filt_off, d_filt_ids, W.list_v, n_entries, d_truth, d_type_head, d_type_tail,
                         (n_ent + 31) / 32, d_counts);
      MMRE_CHECK_LAUNCH();
      const int rs = with_bool(tc, [&](auto tc_) {
        constexpr bool TC = decltype(tc_)::value;
        return pred_kind == 0 ? th_launch_sweep<L2, TC, 0, NORM>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                                 d_type_head, d_type_tail, d_counts)
                              : th_launch_sweep<L2, TC, 1, NORM>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                                 d_type_head, d_type_tail, d_counts);
      });
      if (rs != MMRE_OK) return rs;
      return launch_finalize(st, d_counts, n_query, tc);  // filtered columns += raw columns
    });
  });
}

extern "C" int mmre_transh_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                      const float* d_rel, const float* d_norm, int64_t n_ent, int64_t n_rel, int dim,
                                      const int64_t* d_h, const int64_t* d_r, const int64_t* d_t, int64_t n_rows,
                                      int head_batch, float* d_out, void* stream) {
  if (!th_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_norm || n_ent <= 0 || n_rel <= 0 || n_rows < 0) return MMRE_ERR_ARG;
  if (n_rows > 0 && (!d_h || !d_r || !d_t || !d_out)) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (dim <= 0) return MMRE_ERR_SHAPE;
  if (n_rows == 0) return MMRE_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n_rows + 127) / 128));
  return with_bool(model == MMRE_TRANSH_L2, [&](auto l2_) {
    return with_bool(norm_flag != 0, [&](auto nm_) {
      hipLaunchKernelGGL((k_transh_rows<decltype(l2_)::value, decltype(nm_)::value>), grid, dim3(128), 0, st, d_ent,
                         d_rel, d_norm, n_ent, n_rel, dim, d_h, d_r, d_t, n_rows, head_batch, pred_kind, margin, d_out);
      MMRE_CHECK_LAUNCH();
      return (int)MMRE_OK;
    });
  });
}

// =====================================================================================
// TransD (OpenKE/openke/module/model/TransD.py:78-155): the transfer projection
//   e_perp = normalize(e[:dim_r] + (e . e_p) r_p)                          (TransD.py:94-110)
// is TransH's staged element with another prologue: with s(e) = e . e_p over dim_e (relation-
// independent) the (a, n) table holds (-s(e), N(r, e)) and the w_hat table the RAW rel_transfer
// rows, so (e_k - a w_k) / n = (e_k + s rp_k) / N bit for bit ((-s) x == -(s x), y - (-z) == y + z).
// _transfer always normalises, so the NORM = true instances of k_th_queries, k_th_scores and
// k_sweep_transh run whatever norm_flag says; norm_flag adds _calc's second normalisation
// (TransD.py:79-82), folded into the one divisor N = n1 * n2, and r_hat.
//
// Canonical arithmetic (TransD): as TransH's -- f32, no contraction, IEEE division
// and sqrtf, every sum one sequential chain in ascending k from 0.0f.
//   s = sum_{k < dim_e} e_k ep_k ; a = -s ; u_k = e_k - a rp_k (k < dim_r) ; n1 = den(sum u_k u_k)
//   norm_flag: n2 = den(sum (u_k / n1)(u_k / n1)), N = n1 * n2 ; else N = n1 ; p_k = u_k / N
//
// New kernels:
//   k_td_relations  w[R][kp] = raw rel_transfer, r_hat[R][kp] as k_th_relations makes it
//   k_td_s          s[e] over dim_e from the raw (E, dim_e) tables
//   k_td_an         (-s, N)[used relation][entity] from the raw k-major planes (first dim_r columns)
//   k_transd_rows   predict of arbitrary (h, r, t) rows, one thread per row
namespace mmre {
namespace {

// One 64-thread workgroup per relation: w = the raw rel_transfer row, r_hat = r / max(|r|, 1e-12)
// with norm_flag (TransD.py:81), else r; rows padded to kp with zeros. The norm is one sequential
// chain, by lane 0 from LDS.
__global__ __launch_bounds__(64) void k_td_relations(const float* __restrict__ rel_transfer,
                                                     const float* __restrict__ rel, int dim, int kp, int norm_flag,
                                                     float* __restrict__ w, float* __restrict__ r_hat) {
  extern __shared__ float lds[];  // [kp]
  __shared__ float s_den;
  const int64_t r = blockIdx.x;
  for (int k = threadIdx.x; k < kp; k += 64) lds[k] = k < dim ? rel[r * dim + k] : 0.0f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float ss = 0.0f;
    for (int k = 0; k < dim; ++k) ss = ss + lds[k] * lds[k];
    s_den = th_den(ss);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kp; k += 64) {
    w[r * kp + k] = k < dim ? rel_transfer[r * dim + k] : 0.0f;
    r_hat[r * kp + k] = norm_flag ? lds[k] / s_den : lds[k];
  }
}

// s[e] = sum_{k < dim_e} ent[e][k] * ent_transfer[e][k] (TransD.py:100), one sequential chain per
// entity. A workgroup takes TD_SE entities: all 256 threads copy TD_SK-wide slices of both tables'
// rows to LDS (coalesced along k), then thread e < TD_SE extends its entity's chain over the slice
// (row stride TD_SK + 1: the 64 chains read 64 different banks). Columns n_ent .. e_pad get 0.
constexpr int TD_SE = 64, TD_SK = 32;
__global__ __launch_bounds__(256) void k_td_s(const float* __restrict__ ent, const float* __restrict__ ent_transfer,
                                              int64_t n_ent, int64_t e_pad, int dim_e, float* __restrict__ s) {
  __shared__ float sx[TD_SE][TD_SK + 1], sy[TD_SE][TD_SK + 1];
  const int64_t e0 = (int64_t)blockIdx.x * TD_SE;
  float acc = 0.0f;
  for (int k0 = 0; k0 < dim_e; k0 += TD_SK) {
    for (int i = threadIdx.x; i < TD_SE * TD_SK; i += 256) {
      const int row = i / TD_SK, col = i % TD_SK;
      const int64_t e = e0 + row;
      const bool in = e < n_ent && k0 + col < dim_e;
      sx[row][col] = in ? ent[e * dim_e + k0 + col] : 0.0f;
      sy[row][col] = in ? ent_transfer[e * dim_e + k0 + col] : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x < TD_SE) {
      const int nk = dim_e - k0 < TD_SK ? dim_e - k0 : TD_SK;
      for (int k = 0; k < nk; ++k) acc = acc + sx[threadIdx.x][k] * sy[threadIdx.x][k];
    }
    __syncthreads();  // the slice is read before the next one overwrites it
  }
  const int64_t e = e0 + threadIdx.x;
  if (threadIdx.x < TD_SE && e < e_pad) s[e] = e < n_ent ? acc : 0.0f;
}

// (-s, N) of every entity column for TD_RB used relations per workgroup, in k_th_an's shape: a
// thread owns one column of the k-major planes and TD_RB chains per pass, the relations' raw
// transfer rows in LDS. Pass 1: n1 = den(sum u u), u = x - a rp; with norm_flag pass 2: n2 =
// den(sum (u / n1)(u / n1)) and N = n1 * n2 (one multiply), else N = n1. Padded columns hold zeros
// and s = 0: u = 0, N = 1e-12 or 1e-24 -- finite, and the sweep never counts them.
// TD_RB is 2 where k_th_an's AN_RB is 4: pass 2 is bound by its IEEE division per element and
// relation, not by the plane loads a wider block saves (C2 shape, 29 relations: 92 us at 4, 69 at 2,
// 63 at 1; profiles/transd/README.md).
constexpr int TD_RB = 2;
__global__ __launch_bounds__(256) void k_td_an(const float* __restrict__ ent_km, int64_t e_pad, int dim, int kp,
                                               const float* __restrict__ w, const float* __restrict__ s,
                                               const int32_t* __restrict__ used, int64_t n_used, int64_t n_rel,
                                               int norm_flag, float* __restrict__ an) {
  extern __shared__ float sw[];  // [TD_RB][kp]
  const int64_t u0 = (int64_t)blockIdx.y * TD_RB;
  for (int i = threadIdx.x; i < TD_RB * kp; i += 256) {
    const int64_t u = u0 + i / kp;
    int64_t r = u < n_used ? used[u] : -1;
    sw[i] = (r >= 0 && r < n_rel) ? w[r * kp + i % kp] : 0.0f;
  }
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= e_pad) return;
  const float a = -s[e];
  float n1[TD_RB], ss[TD_RB];
#pragma unroll
  for (int j = 0; j < TD_RB; ++j) ss[j] = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float x = ent_km[(int64_t)k * e_pad + e];
#pragma unroll
    for (int j = 0; j < TD_RB; ++j) {
      const float u = x - a * sw[j * kp + k];
      ss[j] = ss[j] + u * u;
    }
  }
#pragma unroll
  for (int j = 0; j < TD_RB; ++j) {
    n1[j] = th_den(ss[j]);
    ss[j] = 0.0f;
  }
  if (norm_flag) {
    for (int k = 0; k < dim; ++k) {
      const float x = ent_km[(int64_t)k * e_pad + e];
#pragma unroll
      for (int j = 0; j < TD_RB; ++j) {
        const float v = (x - a * sw[j * kp + k]) / n1[j];
        ss[j] = ss[j] + v * v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TD_RB; ++j) {
    if (u0 + j >= n_used) break;
    an[(2 * (u0 + j)) * e_pad + e] = a;
    an[(2 * (u0 + j) + 1) * e_pad + e] = norm_flag ? n1[j] * th_den(ss[j]) : n1[j];
  }
}

// (a, N) of one entity row x (stride-1, dim_e values, transfer row xp) under the raw transfer row
// rp of a relation (dim_r values), by the chains of k_td_s and k_td_an.
template <bool NF>
__device__ __forceinline__ void td_an_row(const float* __restrict__ x, const float* __restrict__ xp,
                                          const float* __restrict__ rp, int dim_e, int dim_r, float& a, float& n) {
  float s = 0.0f;
  for (int k = 0; k < dim_e; ++k) s = s + x[k] * xp[k];
  a = -s;
  float ss = 0.0f;
  for (int k = 0; k < dim_r; ++k) {
    const float u = x[k] - a * rp[k];
    ss = ss + u * u;
  }
  const float n1 = th_den(ss);
  if constexpr (NF) {
    float s2 = 0.0f;
    for (int k = 0; k < dim_r; ++k) {
      const float v = (x[k] - a * rp[k]) / n1;
      s2 = s2 + v * v;
    }
    n = n1 * th_den(s2);
  } else {
    n = n1;
  }
}

// predict of arbitrary rows, one thread per row, from the raw tables (entity rows of stride
// dim_e, relation rows of stride dim_r): (a, N) of both entities and r_hat by the prologue's
// chains, then the sweep's score chain. NF: norm_flag. head != 0: the head_batch grouping
// h + (r - t), else (h + r) - t (TransD.py:87-90).
template <bool L2, bool NF>
__global__ __launch_bounds__(128) void k_transd_rows(const float* __restrict__ ent,
                                                     const float* __restrict__ ent_transfer,
                                                     const float* __restrict__ rel,
                                                     const float* __restrict__ rel_transfer, int64_t n_ent,
                                                     int64_t n_rel, int dim_e, int dim_r,
                                                     const int64_t* __restrict__ hs, const int64_t* __restrict__ rs,
                                                     const int64_t* __restrict__ ts, int64_t n_rows, int head,
                                                     int pred_kind, float margin, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t h = hs[i], r = rs[i], t = ts[i];
  if (h < 0 || h >= n_ent || t < 0 || t >= n_ent || r < 0 || r >= n_rel) {
    out[i] = __builtin_nanf("");
    return;
  }
  const float* rp = rel_transfer + r * dim_r;
  const float* rr = rel + r * dim_r;
  float dr = 1.0f;
  if constexpr (NF) {
    float sr = 0.0f;
    for (int k = 0; k < dim_r; ++k) sr = sr + rr[k] * rr[k];
    dr = th_den(sr);
  }
  const int64_t ia = head ? t : h, ic = head ? h : t;  // anchor, candidate
  const float* xa = ent + ia * dim_e;
  const float* xc = ent + ic * dim_e;
  float aa, na, ac, nc;
  td_an_row<NF>(xa, ent_transfer + ia * dim_e, rp, dim_e, dim_r, aa, na);
  td_an_row<NF>(xc, ent_transfer + ic * dim_e, rp, dim_e, dim_r, ac, nc);
  float s = 0.0f;
  for (int k = 0; k < dim_r; ++k) {
    const float wk = rp[k];
    const float rh = NF ? rr[k] / dr : rr[k];
    const float q = th_q(th_p<true>(xa[k], aa, wk, na), rh, head != 0);
    s = th_step<L2>(s, q, th_p<true>(xc[k], ac, wk, nc));
  }
  out[i] = apply_pred(pred_kind, margin, th_final<L2>(s));
}

inline bool td_model(int m) { return m == MMRE_TRANSD_L1 || m == MMRE_TRANSD_L2; }

// TransH's workspace at dim_r, then s[e_pad]
int64_t td_layout(THWork& W, float*& s, int64_t n_ent, int64_t n_rel, int dim_r, int64_t n_tiles, int64_t n_used,
                  int64_t n_entries, void* base) {
  const int64_t at = th_layout(W, n_ent, n_rel, dim_r, n_tiles, n_used, n_entries, base);
  s = base ? (float*)((char*)base + at) : nullptr;
  return at + round_up(round_up(n_ent > 0 ? n_ent : 1, TE) * 4, 256);
}

}  // namespace
}  // namespace mmre

extern "C" int64_t mmre_transd_workspace(int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, int64_t n_tiles,
                                         int64_t n_used, int64_t n_entries) {
  if (n_ent <= 0 || n_rel <= 0 || dim_r <= 0 || dim_e < dim_r || n_tiles < 0 || n_used < 0 || n_entries < 0) return 0;
  THWork W;
  float* s;
  return td_layout(W, s, n_ent, n_rel, dim_r, n_tiles, n_used, n_entries, nullptr);
}

extern "C" int mmre_transd_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                    const float* d_ent_transfer, const float* d_rel, const float* d_rel_transfer,
                                    const float* d_ent_narrow, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r,
                                    const int64_t* d_qh, const int64_t* d_qr, const int64_t* d_qt,
                                    const int8_t* d_qmode, int64_t n_query, const int32_t* d_perm,
                                    const int32_t* d_tiles, int64_t n_tiles, const int32_t* d_used, int64_t n_used,
                                    const int32_t* d_rel_slot, const int64_t* d_grp_qoff, const int32_t* d_grp_q,
                                    int64_t n_groups, const int64_t* d_filt_off, const int32_t* d_filt_ids,
                                    const int32_t* d_entry_q, int64_t n_entries, const uint32_t* d_type_head,
                                    const uint32_t* d_type_tail, int32_t* d_counts, float* d_truth, void* d_work,
                                    int64_t work_bytes, void* stream) {
  if (!td_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_ent_transfer || !d_rel || !d_rel_transfer || !d_ent_narrow || !d_qh || !d_qr || !d_qt ||
      !d_qmode || !d_perm || !d_tiles || !d_used || !d_rel_slot || !d_counts || !d_truth || !d_work)
    return MMRE_ERR_ARG;
  if (n_ent <= 0 || n_rel <= 0 || n_query <= 0 || n_tiles <= 0 || n_used <= 0 || n_used > n_rel) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 1) return MMRE_ERR_ARG;
  if ((d_type_head == nullptr) != (d_type_tail == nullptr)) return MMRE_ERR_ARG;
  const bool grouped = d_grp_qoff != nullptr;
  if (grouped && (!d_grp_q || !d_filt_off || n_groups <= 0 || n_entries < 0 ||
                  (n_entries > 0 && (!d_filt_ids || !d_entry_q))))
    return MMRE_ERR_ARG;
  if (!grouped) n_entries = 0;
  if (dim_r <= 0 || dim_e < dim_r) return MMRE_ERR_SHAPE;
  if (n_ent > (int64_t)INT32_MAX - 256 || n_query > (int64_t)INT32_MAX - 256 || n_tiles > (1 << 24))
    return MMRE_ERR_SHAPE;
  THWork W;
  float* s;
  if (work_bytes < td_layout(W, s, n_ent, n_rel, dim_r, n_tiles, n_used, n_entries, d_work)) return MMRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = th_kp(dim_r);
  const int64_t e_pad = round_up(n_ent, TE);
  // the raw k-major planes and the row-major copy of the first dim_r columns (TransD.py:62-68)
  const int rc = mmre_link_prepare_entities(MMRE_TRANSE_L1, 0, d_ent_narrow, nullptr, n_ent, dim_r, W.ent_km, e_pad,
                                            W.ent_rows, stream);
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_td_relations, dim3((unsigned)n_rel), dim3(64), kp * sizeof(float), st, d_rel_transfer, d_rel,
                     dim_r, kp, norm_flag, W.w_hat, W.r_hat);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_td_s, dim3((unsigned)((e_pad + TD_SE - 1) / TD_SE)), dim3(256), 0, st, d_ent, d_ent_transfer,
                     n_ent, e_pad, dim_e, s);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_td_an, dim3((unsigned)(e_pad / 256 + (e_pad % 256 != 0)), (unsigned)((n_used + TD_RB - 1) / TD_RB)),
                     dim3(256), TD_RB * kp * sizeof(float), st, W.ent_km, e_pad, dim_r, kp, W.w_hat, s, d_used, n_used,
                     n_rel, norm_flag, W.an);
  MMRE_CHECK_LAUNCH();
  THEval P{W.ent_km, W.ent_rows, W.w_hat, W.r_hat, W.an, d_rel_slot, n_ent, e_pad, n_rel, n_used, n_query,
           dim_r,    kp,         d_qh,    d_qr,    d_qt, d_qmode};
  const bool l2 = model == MMRE_TRANSD_L2, tc = d_type_head != nullptr;
  const int64_t tasks = n_query + n_entries;
  const int64_t fc_grid = grouped ? std::min<int64_t>(n_groups, 1 << 20) : std::min<int64_t>((n_query + 63) / 64, 4096);
  // from here on TransH's NORM = true kernels, unchanged: the staged element is (e - a w) / n
  return with_bool(l2, [&](auto l2_) {
    constexpr bool L2 = decltype(l2_)::value;
    hipLaunchKernelGGL((k_th_queries<true>), dim3((unsigned)n_tiles), dim3(TQ), 0, st, P, d_perm, d_tiles, n_tiles,
                       W.q_km, W.row_q);
    MMRE_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_th_scores<L2, true>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st, P, pred_kind,
                       margin, d_entry_q, d_filt_ids, n_entries, d_truth, W.list_v);
    MMRE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_th_filter_count, dim3((unsigned)fc_grid), dim3(64), 0, st, P, d_grp_qoff, d_grp_q, n_groups,
                       d_filt_off, d_filt_ids, W.list_v, n_entries, d_truth, d_type_head, d_type_tail,
                       (n_ent + 31) / 32, d_counts);
    MMRE_CHECK_LAUNCH();
    const int rs = with_bool(tc, [&](auto tc_) {
      constexpr bool TC = decltype(tc_)::value;
      return pred_kind == 0 ? th_launch_sweep<L2, TC, 0, true>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                               d_type_head, d_type_tail, d_counts)
                            : th_launch_sweep<L2, TC, 1, true>(st, P, W, d_tiles, n_tiles, pred_kind, margin, d_truth,
                                                               d_type_head, d_type_tail, d_counts);
    });
    if (rs != MMRE_OK) return rs;
    return launch_finalize(st, d_counts, n_query, tc);  // filtered columns += raw columns
  });
}

extern "C" int mmre_transd_score_rows(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                      const float* d_ent_transfer, const float* d_rel, const float* d_rel_transfer,
                                      int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h,
                                      const int64_t* d_r, const int64_t* d_t, int64_t n_rows, int head_batch,
                                      float* d_out, void* stream) {
  if (!td_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_ent_transfer || !d_rel || !d_rel_transfer || n_ent <= 0 || n_rel <= 0 || n_rows < 0)
    return MMRE_ERR_ARG;
  if (n_rows > 0 && (!d_h || !d_r || !d_t || !d_out)) return MMRE_ERR_ARG;
  if (pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (dim_r <= 0 || dim_e < dim_r) return MMRE_ERR_SHAPE;
  if (n_rows == 0) return MMRE_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n_rows + 127) / 128));
  return with_bool(model == MMRE_TRANSD_L2, [&](auto l2_) {
    return with_bool(norm_flag != 0, [&](auto nf_) {
      hipLaunchKernelGGL((k_transd_rows<decltype(l2_)::value, decltype(nf_)::value>), grid, dim3(128), 0, st, d_ent,
                         d_ent_transfer, d_rel, d_rel_transfer, n_ent, n_rel, dim_e, dim_r, d_h, d_r, d_t, n_rows,
                         head_batch, pred_kind, margin, d_out);
      MMRE_CHECK_LAUNCH();
      return (int)MMRE_OK;
    });
  });
}
