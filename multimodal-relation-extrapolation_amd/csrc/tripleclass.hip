// tripleclass.hip -- triple classification (Test.h:393-422 getNegTest / getTestBatch,
// Tester.py:93-151 get_best_threshlod / run_triple_classification): one corrupted copy of every
// test triple, model.predict on both, and the score threshold that separates them best.
//
// Three stages, each its own entry point, and mmre_tc_evaluate enqueues all of them:
//
//   k_tc_negatives  one thread per test triple. getNegTest draws thread 0's LCG exactly twice per
//                   triple (the coin `randd(0) % 1000 < 500`, then corrupt_head's / corrupt_tail's
//                   one rand_max), so triple i starts at lcg_jump(state, 2 i) and the serial loop
//                   of the reference is sampled in parallel, bit for bit. The corruption is
//                   sampler_openke.h's (Corrupt.h:7-83), looked up with key_block: test triples are
//                   not train rows, so there is no per-row block table to read.
//   k_tc_score      one wave per test triple scores the positive row and its negative with the
//                   row-wise chain of row_chain.h followed by apply_pred: bit for bit
//                   model.predict in 'normal' mode. A table row the two triples share (the
//                   relation and the kept entity: two of three) is loaded once.
//   k_tc_count / k_tc_best / k_tc_result   the threshold search without a sort. For a candidate c
//                   among the scores, P(c) = #{positives <= c}, A(c) = P(c) + #{negatives <= c};
//                   the accuracy of the rule `score <= c` is (2 P + F - A) / T (F negatives, T all),
//                   so the best c maximises the integer 2 P - A, the smallest such c winning. That
//                   is get_best_threshlod's walk over the sorted scores read at the end of each
//                   group of equal scores. Candidates sit in registers, the positive and the
//                   negative scores stream through LDS as separate arrays (the label is which
//                   array), one compare and one add per pair; counts meet in integer atomics and the
//                   winner in one 64-bit integer atomic max, so the result is the same every run.
//                   The cost is (n_pos + n_neg)^2 pairs: quadratic, and at FB15K237's 40,932 scores
//                   a fraction of a millisecond (profiles/tripleclass).
//
// NaN scores are never <= anything: they are classified negative, are no candidates, and are
// counted in n_nan. -0 and +0 are one group (reported as +0).
#include <math.h>

#include "dispatch.h"
#include "row_chain.h"
#include "sampler_openke.h"

namespace mmre {
namespace {

// ------------------------------------------------------------------------ negatives ----
struct TcNegArgs {
  const int64_t *head_hrt, *tail_hrt, *lef_head, *rig_head, *lef_tail, *rig_tail;
  int64_t train_total, n_ent;
  const int64_t *th, *tr, *tt;
  int64_t n;
  uint64_t state;
  int64_t *neg_h, *neg_t;
};

// corrupt_head / corrupt_tail for a kept entity that need not occur on that side of train. When it
// does not, Reader.h leaves lef = 0, rig = -1, Corrupt.h's searches give ll = -1, rr = 0 and the
// reference reads row -1; here: its modulus (n_ent - 2) and the draw returned unchanged, no read.
__device__ int64_t tc_corrupt(const int64_t* __restrict__ T, int col, const int64_t* __restrict__ lef,
                              const int64_t* __restrict__ rig, int64_t train_total, int64_t n_ent, uint64_t* st,
                              int64_t e, int64_t r) {
  const int64_t l0 = lef[e], r0 = rig[e];
  if (r0 < l0 || l0 < 0 || r0 >= train_total) return rand_max(st, n_ent - 2);
  int64_t ll, rr;
  key_block(T, 1, l0, r0, r, ll, rr);  // both inside [l0, r0]
  return corrupt_in_block(T, col, n_ent, st, ll, rr, T[3 * ll + col], T[3 * rr + col]);
}

__global__ __launch_bounds__(256) void k_tc_negatives(TcNegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int64_t h = a.th[i], r = a.tr[i], t = a.tt[i];
  if (h < 0 || h >= a.n_ent || t < 0 || t >= a.n_ent) {  // no such entity: reads no index row
    a.neg_h[i] = -1;
    a.neg_t[i] = -1;
    return;
  }
  uint64_t st = lcg_jump(a.state, 2ULL * (uint64_t)i);
  if (lcg_next(&st) % 1000ULL < 500ULL) {  // Test.h:404: corrupt_head returns a replacement TAIL
    a.neg_h[i] = h;
    a.neg_t[i] = tc_corrupt(a.head_hrt, 2, a.lef_head, a.rig_head, a.train_total, a.n_ent, &st, h, r);
  } else {
    a.neg_t[i] = t;
    a.neg_h[i] = tc_corrupt(a.tail_hrt, 0, a.lef_tail, a.rig_tail, a.train_total, a.n_ent, &st, t, r);
  }
}

// --------------------------------------------------------------------------- scores ----
constexpr int TC_WAVES = 4;  // test triples per 256-thread workgroup, one wave each
constexpr int TC_MAXDIM = 512;

struct TcScoreArgs {
  int norm_flag, pred_kind, dim;
  float margin, phase_denom;
  const float *ent, *ent_im, *rel, *rel_im;
  int64_t n_ent, n_rel;
  const int64_t *ph, *pr, *pt, *nh, *nr, *nt;
  int64_t n;
  float *pos, *neg;
};

// One table row as the score uses it, a[.] and b[.]:
//   TransE   a = x / |x| (norm_flag) or x                   DistMult a = x
//   ComplEx  a = re, b = im                                 RotatE   entity a = re, b = im;
//                                                                    relation a = sin, b = cos
template <int MODEL, int NC>
struct TcRow {
  float a[NC], b[NC];
};

template <int MODEL, int NC>
__device__ __forceinline__ void tc_normalise(TcRow<MODEL, NC>& X, int norm_flag) {
  if (!norm_flag) return;  // the raw row is the quotient
  const float n = row_norm(X.a);
#pragma unroll
  for (int c = 0; c < NC; ++c) X.a[c] = X.a[c] / n;
}

template <int MODEL, int NC>
__device__ __forceinline__ void tc_load_ent(TcRow<MODEL, NC>& X, const TcScoreArgs& A, int64_t e, int lane) {
  const int d = A.dim;
  if constexpr (MODEL == MMRE_TRANSE_L1 || MODEL == MMRE_TRANSE_L2) {
    vload(X.a, A.ent + e * d, d, lane);
    tc_normalise(X, A.norm_flag);
  } else if constexpr (MODEL == MMRE_DISTMULT) {
    vload(X.a, A.ent + e * d, d, lane);
  } else if constexpr (MODEL == MMRE_COMPLEX) {
    vload(X.a, A.ent + e * d, d, lane);
    vload(X.b, A.ent_im + e * d, d, lane);
  } else {
    vload(X.a, A.ent + e * 2 * d, d, lane);
    vload(X.b, A.ent + e * 2 * d + d, d, lane);
  }
}

template <int MODEL, int NC>
__device__ __forceinline__ void tc_load_rel(TcRow<MODEL, NC>& X, const TcScoreArgs& A, int64_t r, int lane) {
  const int d = A.dim;
  vload(X.a, A.rel + r * d, d, lane);
  if constexpr (MODEL == MMRE_TRANSE_L1 || MODEL == MMRE_TRANSE_L2) tc_normalise(X, A.norm_flag);
  else if constexpr (MODEL == MMRE_COMPLEX) vload(X.b, A.rel_im + r * d, d, lane);
  else if constexpr (MODEL == MMRE_ROTATE) vsincos(X.a, A.phase_denom, X.a, X.b);
}

// predict's value of the row (H, R, T)
template <int MODEL, int NC>
__device__ __forceinline__ float tc_predict(const TcRow<MODEL, NC>& H, const TcRow<MODEL, NC>& R,
                                            const TcRow<MODEL, NC>& T, const TcScoreArgs& A, int lane) {
  const float acc = lane_partial<NC>(A.dim, lane, [&](int c) {
    if constexpr (MODEL <= MMRE_DISTMULT) return row_term<MODEL>(H.a[c], R.a[c], T.a[c]);
    else return row_term<MODEL>(H.a[c], H.b[c], R.a[c], R.b[c], T.a[c], T.b[c]);
  });
  return row_finish(acc, MODEL == MMRE_TRANSE_L2, A.pred_kind, A.margin);
}

template <int MODEL, int NC>
__global__ __launch_bounds__(256) void k_tc_score(TcScoreArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * TC_WAVES + (threadIdx.x >> 6);
  if (i >= A.n) return;  // whole wave exits together
  const int64_t ph = A.ph[i], pr = A.pr[i], pt = A.pt[i];
  const int64_t nh = A.nh[i], nr = A.nr ? A.nr[i] : pr, nt = A.nt[i];
  const bool vp = ph >= 0 && ph < A.n_ent && pt >= 0 && pt < A.n_ent && pr >= 0 && pr < A.n_rel;
  const bool vn = nh >= 0 && nh < A.n_ent && nt >= 0 && nt < A.n_ent && nr >= 0 && nr < A.n_rel;
  // every branch below is on values the whole wave shares
  TcRow<MODEL, NC> H, R, T;
  float sp = NAN, sn = NAN;  // a triple with an id out of range reads nothing
  if (vp) {
    tc_load_ent(H, A, ph, lane);
    tc_load_rel(R, A, pr, lane);
    tc_load_ent(T, A, pt, lane);
    sp = tc_predict(H, R, T, A, lane);
  }
  if (vn) {  // the rows the negative shares with the positive stay in registers
    if (!vp || nh != ph) tc_load_ent(H, A, nh, lane);
    if (!vp || nr != pr) tc_load_rel(R, A, nr, lane);
    if (!vp || nt != pt) tc_load_ent(T, A, nt, lane);
    sn = tc_predict(H, R, T, A, lane);
  }
  if (lane == 0) {
    A.pos[i] = sp;
    A.neg[i] = sn;
  }
}

int run_scores(int model, const TcScoreArgs& A, hipStream_t st) {
  const dim3 grid((unsigned)((A.n + TC_WAVES - 1) / TC_WAVES)), block(64 * TC_WAVES);
  return with_model(model, [&](auto model_) {
    return with_nc<TC_MAXDIM / kWave>(nc_for_dim(A.dim, TC_MAXDIM / kWave), [&](auto nc_) {
      hipLaunchKernelGGL((k_tc_score<decltype(model_)::value, decltype(nc_)::value>), grid, block, 0, st, A);
    });
  });
}

// ----------------------------------------------------------------- threshold search ----
constexpr int TC_THREADS = 256;
constexpr int TC_CPT = 4;                        // candidates per thread, in registers
constexpr int TC_CAND = TC_THREADS * TC_CPT;     // candidates per workgroup
constexpr int TC_TILE = 1024;                    // scores per LDS tile
constexpr int64_t TC_TARGET_BLOCKS = 1024;       // workgroups to aim for
constexpr int64_t TC_MAX_SCORES = (int64_t)1 << 30;  // 2 P - A + T + 1 fits the key's high word

// workspace: [0] the best key (uint64), [16 ...) cnt_p[n], cnt_n[n] (int32), n = n_pos + n_neg
constexpr int64_t TC_WORK_HEAD = 16;

__device__ __forceinline__ float tc_candidate(const float* __restrict__ pos, int64_t n_pos,
                                              const float* __restrict__ neg, int64_t n_neg, int64_t c) {
  if (c < n_pos) return pos[c];
  return c < n_pos + n_neg ? neg[c - n_pos] : NAN;
}

// grid.x: blocks of TC_CAND candidates; grid.y: chunks of `chunk` scores, the positives' chunks
// first. Each workgroup adds, for its candidates, how many scores of its chunk are <= them.
__global__ __launch_bounds__(TC_THREADS) void k_tc_count(const float* __restrict__ pos, int64_t n_pos,
                                                         const float* __restrict__ neg, int64_t n_neg, int64_t chunk,
                                                         int64_t chunks_pos, int32_t* __restrict__ cnt_p,
                                                         int32_t* __restrict__ cnt_n) {
  __shared__ __attribute__((aligned(16))) float s[TC_TILE];
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * TC_CAND + tid;
  float cand[TC_CPT];
  int cnt[TC_CPT];
#pragma unroll
  for (int k = 0; k < TC_CPT; ++k) {
    cand[k] = tc_candidate(pos, n_pos, neg, n_neg, c0 + (int64_t)k * TC_THREADS);
    cnt[k] = 0;
  }
  const bool is_pos = (int64_t)blockIdx.y < chunks_pos;
  const float* __restrict__ src = is_pos ? pos : neg;
  const int64_t len = is_pos ? n_pos : n_neg;
  const int64_t begin = ((int64_t)blockIdx.y - (is_pos ? 0 : chunks_pos)) * chunk;
  const int64_t end = begin + chunk < len ? begin + chunk : len;
  for (int64_t t0 = begin; t0 < end; t0 += TC_TILE) {
#pragma unroll
    for (int j = 0; j < TC_TILE / TC_THREADS; ++j) {
      const int64_t i = t0 + j * TC_THREADS + tid;
      s[j * TC_THREADS + tid] = i < end ? src[i] : NAN;  // NaN: never <= a candidate
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < TC_TILE; j += 4) {
      const float4 v = *reinterpret_cast<const float4*>(&s[j]);  // one address: a broadcast read
#pragma unroll
      for (int k = 0; k < TC_CPT; ++k)
        cnt[k] += (int)(v.x <= cand[k]) + (int)(v.y <= cand[k]) + (int)(v.z <= cand[k]) + (int)(v.w <= cand[k]);
    }
    __syncthreads();
  }
  int32_t* __restrict__ out = is_pos ? cnt_p : cnt_n;
#pragma unroll
  for (int k = 0; k < TC_CPT; ++k) {
    const int64_t c = c0 + (int64_t)k * TC_THREADS;
    if (c < n_pos + n_neg && cnt[k]) atomicAdd(&out[c], cnt[k]);
  }
}

// The order-preserving integer image of a non-NaN float; -0 maps with +0.
__device__ __forceinline__ uint32_t tc_image(float c) {
  const uint32_t u = __float_as_uint(c + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tc_unimage(uint32_t m) {
  return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}

// key(c) = (2 P - A + T + 1) << 32 | ~image(c): the larger key is the better count, then the
// smaller candidate. 0 = no candidate.
__global__ __launch_bounds__(TC_THREADS) void k_tc_best(const float* __restrict__ pos, int64_t n_pos,
                                                        const float* __restrict__ neg, int64_t n_neg,
                                                        const int32_t* __restrict__ cnt_p,
                                                        const int32_t* __restrict__ cnt_n,
                                                        unsigned long long* __restrict__ best) {
  const int64_t c = (int64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  const float v = tc_candidate(pos, n_pos, neg, n_neg, c);
  unsigned long long key = 0;
  if (v == v) {
    const int64_t P = cnt_p[c], A = P + cnt_n[c];
    key = ((unsigned long long)(2 * P - A + n_pos + n_neg + 1) << 32) | (unsigned long long)(~tc_image(v));
  }
  uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    const uint32_t ohi = __shfl_xor(hi, sh), olo = __shfl_xor(lo, sh);
    const bool take = ohi > hi || (ohi == hi && olo > lo);
    hi = take ? ohi : hi;
    lo = take ? olo : lo;
  }
  key = ((unsigned long long)hi << 32) | lo;
  if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// out[0] = the threshold's float bits, out[1] = P = #{pos <= thr}, out[2] = A = P + #{neg <= thr},
// out[3] = NaN scores in both arrays. One workgroup.
__global__ __launch_bounds__(1024) void k_tc_result(const float* __restrict__ pos, int64_t n_pos,
                                                    const float* __restrict__ neg, int64_t n_neg,
                                                    const unsigned long long* __restrict__ best, float given,
                                                    int64_t* __restrict__ out) {
  __shared__ int s[3];
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  float thr = given;
  if (best) {
    const unsigned long long key = *best;
    thr = key ? tc_unimage(~(uint32_t)key) : NAN;
  }
  int p = 0, q = 0, nan = 0;
  for (int64_t i = threadIdx.x; i < n_pos; i += blockDim.x) {
    const float v = pos[i];
    p += v <= thr;
    nan += v != v;
  }
  for (int64_t i = threadIdx.x; i < n_neg; i += blockDim.x) {
    const float v = neg[i];
    q += v <= thr;
    nan += v != v;
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    p += __shfl_xor(p, sh);
    q += __shfl_xor(q, sh);
    nan += __shfl_xor(nan, sh);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s[0], p);
    atomicAdd(&s[1], q);
    atomicAdd(&s[2], nan);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (int64_t)__float_as_uint(thr);
    out[1] = s[0];
    out[2] = (int64_t)s[0] + s[1];
    out[3] = s[2];
  }
}

int check_negatives(const int64_t* head, const int64_t* tail, const int64_t* lh, const int64_t* rh, const int64_t* lt,
                    const int64_t* rt, int64_t train_total, int64_t n_ent, const int64_t* th, const int64_t* tr,
                    const int64_t* tt, int64_t n, const int64_t* neg_h, const int64_t* neg_t) {
  if (!head || !tail || !lh || !rh || !lt || !rt || train_total < 1 || n_ent < 3 || n < 0) return MMRE_ERR_ARG;
  if (n > (int64_t)INT32_MAX) return MMRE_ERR_SHAPE;
  if (n > 0 && (!th || !tr || !tt || !neg_h || !neg_t)) return MMRE_ERR_ARG;
  return MMRE_OK;
}

int check_scores(int model, int pred_kind, const float* ent, const float* ent_im, const float* rel,
                 const float* rel_im, int64_t n_ent, int64_t n_rel, int dim, float phase_denom, const int64_t* ph,
                 const int64_t* pr, const int64_t* pt, const int64_t* nh, const int64_t* nt, int64_t n,
                 const float* pos, const float* neg) {
  if (model < MMRE_TRANSE_L1 || model > MMRE_ROTATE) return MMRE_ERR_MODEL;
  if (dim < 1) return MMRE_ERR_ARG;
  if (dim > TC_MAXDIM) return MMRE_ERR_SHAPE;
  if (!ent || !rel || n_ent < 1 || n_rel < 1 || n < 0 || pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (model == MMRE_COMPLEX && (!ent_im || !rel_im)) return MMRE_ERR_ARG;
  if (model == MMRE_ROTATE && (phase_denom == 0.0f || phase_denom != phase_denom)) return MMRE_ERR_ARG;  // 0, NaN
  if (n > (int64_t)INT32_MAX) return MMRE_ERR_SHAPE;
  if (n > 0 && (!ph || !pr || !pt || !nh || !nt || !pos || !neg)) return MMRE_ERR_ARG;
  return MMRE_OK;
}

int check_threshold(const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int have_thr,
                    const int64_t* out, const void* work, int64_t work_bytes) {
  if (n_pos < 0 || n_neg < 0) return MMRE_ERR_ARG;
  if (n_pos > TC_MAX_SCORES || n_neg > TC_MAX_SCORES || n_pos + n_neg > TC_MAX_SCORES) return MMRE_ERR_SHAPE;
  if (n_pos + n_neg == 0) return MMRE_OK;
  if ((n_pos > 0 && !pos) || (n_neg > 0 && !neg) || !out) return MMRE_ERR_ARG;
  if (!have_thr) {
    if (!work) return MMRE_ERR_ARG;
    if (work_bytes < mmre_tc_threshold_workspace(n_pos, n_neg)) return MMRE_ERR_WORKSPACE;
  }
  return MMRE_OK;
}

int run_negatives(const TcNegArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_tc_negatives, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

int run_threshold(const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int have_thr, float thr,
                  int64_t* out, void* work, hipStream_t st) {
  const int64_t n = n_pos + n_neg;
  unsigned long long* best = nullptr;
  if (!have_thr) {
    best = (unsigned long long*)work;
    int32_t* cnt_p = (int32_t*)((char*)work + TC_WORK_HEAD);
    int32_t* cnt_n = cnt_p + n;
    MMRE_CHECK(hipMemsetAsync(work, 0, (size_t)mmre_tc_threshold_workspace(n_pos, n_neg), st));
    const int64_t gx = (n + TC_CAND - 1) / TC_CAND;
    const int64_t want = (TC_TARGET_BLOCKS + gx - 1) / gx;  // chunks of the score stream
    const int64_t chunk = round_up((n + want - 1) / want, TC_TILE);
    const int64_t chunks_pos = (n_pos + chunk - 1) / chunk, chunks_neg = (n_neg + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_tc_count, dim3((unsigned)gx, (unsigned)(chunks_pos + chunks_neg)), dim3(TC_THREADS), 0, st,
                       pos, n_pos, neg, n_neg, chunk, chunks_pos, cnt_p, cnt_n);
    MMRE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tc_best, dim3((unsigned)((n + TC_THREADS - 1) / TC_THREADS)), dim3(TC_THREADS), 0, st, pos,
                       n_pos, neg, n_neg, cnt_p, cnt_n, best);
    MMRE_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_tc_result, dim3(1), dim3(1024), 0, st, pos, n_pos, neg, n_neg, best, thr, out);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

TcScoreArgs score_args(int model, int norm_flag, int pred_kind, float margin, const float* ent, const float* ent_im,
                       const float* rel, const float* rel_im, int64_t n_ent, int64_t n_rel, int dim,
                       float phase_denom, const int64_t* ph, const int64_t* pr, const int64_t* pt, const int64_t* nh,
                       const int64_t* nr, const int64_t* nt, int64_t n, float* pos, float* neg) {
  TcScoreArgs A;
  A.norm_flag = (model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2) && norm_flag;
  A.pred_kind = pred_kind;
  A.dim = dim;
  A.margin = margin;
  A.phase_denom = phase_denom;
  A.ent = ent;
  A.ent_im = ent_im;
  A.rel = rel;
  A.rel_im = rel_im;
  A.n_ent = n_ent;
  A.n_rel = n_rel;
  A.ph = ph;
  A.pr = pr;
  A.pt = pt;
  A.nh = nh;
  A.nr = nr;
  A.nt = nt;
  A.n = n;
  A.pos = pos;
  A.neg = neg;
  return A;
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_tc_threshold_workspace(int64_t n_pos, int64_t n_neg) {
  if (n_pos < 0 || n_neg < 0 || n_pos > TC_MAX_SCORES || n_neg > TC_MAX_SCORES || n_pos + n_neg > TC_MAX_SCORES)
    return -1;
  return TC_WORK_HEAD + 2 * (n_pos + n_neg) * (int64_t)sizeof(int32_t);
}

extern "C" int mmre_tc_negatives(const int64_t* d_head_hrt, const int64_t* d_tail_hrt, const int64_t* d_lef_head,
                                 const int64_t* d_rig_head, const int64_t* d_lef_tail, const int64_t* d_rig_tail,
                                 int64_t train_total, int64_t n_ent, const int64_t* d_test_h,
                                 const int64_t* d_test_r, const int64_t* d_test_t, int64_t n, uint64_t state,
                                 int64_t* d_neg_h, int64_t* d_neg_t, void* stream) {
  const int rc = check_negatives(d_head_hrt, d_tail_hrt, d_lef_head, d_rig_head, d_lef_tail, d_rig_tail, train_total,
                                 n_ent, d_test_h, d_test_r, d_test_t, n, d_neg_h, d_neg_t);
  if (rc != MMRE_OK || n == 0) return rc;
  return run_negatives(TcNegArgs{d_head_hrt, d_tail_hrt, d_lef_head, d_rig_head, d_lef_tail, d_rig_tail, train_total,
                                 n_ent, d_test_h, d_test_r, d_test_t, n, state, d_neg_h, d_neg_t},
                       (hipStream_t)stream);
}

extern "C" int mmre_tc_scores(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                              const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                              int64_t n_rel, int dim, float phase_denom, const int64_t* d_pos_h,
                              const int64_t* d_pos_r, const int64_t* d_pos_t, const int64_t* d_neg_h,
                              const int64_t* d_neg_r, const int64_t* d_neg_t, int64_t n, float* d_pos_scores,
                              float* d_neg_scores, void* stream) {
  const int rc = check_scores(model, pred_kind, d_ent, d_ent_im, d_rel, d_rel_im, n_ent, n_rel, dim, phase_denom,
                              d_pos_h, d_pos_r, d_pos_t, d_neg_h, d_neg_t, n, d_pos_scores, d_neg_scores);
  if (rc != MMRE_OK || n == 0) return rc;
  return run_scores(model,
                    score_args(model, norm_flag, pred_kind, margin, d_ent, d_ent_im, d_rel, d_rel_im, n_ent, n_rel,
                               dim, phase_denom, d_pos_h, d_pos_r, d_pos_t, d_neg_h, d_neg_r, d_neg_t, n,
                               d_pos_scores, d_neg_scores),
                    (hipStream_t)stream);
}

extern "C" int mmre_tc_threshold(const float* d_pos_scores, int64_t n_pos, const float* d_neg_scores, int64_t n_neg,
                                 int have_threshold, float threshold, int64_t* d_out, void* d_work,
                                 int64_t work_bytes, void* stream) {
  const int rc = check_threshold(d_pos_scores, n_pos, d_neg_scores, n_neg, have_threshold, d_out, d_work, work_bytes);
  if (rc != MMRE_OK || n_pos + n_neg == 0) return rc;
  return run_threshold(d_pos_scores, n_pos, d_neg_scores, n_neg, have_threshold, threshold, d_out, d_work,
                       (hipStream_t)stream);
}

extern "C" int mmre_tc_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                                int64_t n_rel, int dim, float phase_denom, const int64_t* d_head_hrt,
                                const int64_t* d_tail_hrt, const int64_t* d_lef_head, const int64_t* d_rig_head,
                                const int64_t* d_lef_tail, const int64_t* d_rig_tail, int64_t train_total,
                                const int64_t* d_test_h, const int64_t* d_test_r, const int64_t* d_test_t, int64_t n,
                                uint64_t state, int have_threshold, float threshold, int64_t* d_neg_h,
                                int64_t* d_neg_t, float* d_pos_scores, float* d_neg_scores, int64_t* d_out,
                                void* d_work, int64_t work_bytes, void* stream) {
  int rc = check_scores(model, pred_kind, d_ent, d_ent_im, d_rel, d_rel_im, n_ent, n_rel, dim, phase_denom, d_test_h,
                        d_test_r, d_test_t, d_neg_h, d_neg_t, n, d_pos_scores, d_neg_scores);
  if (rc != MMRE_OK) return rc;
  rc = check_negatives(d_head_hrt, d_tail_hrt, d_lef_head, d_rig_head, d_lef_tail, d_rig_tail, train_total, n_ent,
                       d_test_h, d_test_r, d_test_t, n, d_neg_h, d_neg_t);
  if (rc != MMRE_OK) return rc;
  rc = check_threshold(d_pos_scores, n, d_neg_scores, n, have_threshold, d_out, d_work, work_bytes);
  if (rc != MMRE_OK || n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = run_negatives(TcNegArgs{d_head_hrt, d_tail_hrt, d_lef_head, d_rig_head, d_lef_tail, d_rig_tail, train_total,
                               n_ent, d_test_h, d_test_r, d_test_t, n, state, d_neg_h, d_neg_t},
                     st);
  if (rc != MMRE_OK) return rc;
  rc = run_scores(model,
                  score_args(model, norm_flag, pred_kind, margin, d_ent, d_ent_im, d_rel, d_rel_im, n_ent, n_rel, dim,
                             phase_denom, d_test_h, d_test_r, d_test_t, d_neg_h, nullptr, d_neg_t, n, d_pos_scores,
                             d_neg_scores),
                  st);
  if (rc != MMRE_OK) return rc;
  return run_threshold(d_pos_scores, n, d_neg_scores, n, have_threshold, threshold, d_out, d_work, st);
}
