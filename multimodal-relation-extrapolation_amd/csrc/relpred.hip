// relpred.hip -- relation prediction: every test pair (h, t) against every relation, ranks
// counted on the fly.
//
// Replaces, per evaluation, the reference's loop over the test triples (Test.h:55-62
// getRelBatch -> model.predict on the R rows (h, j, t) in 'normal' mode, TransE.py:62-110,
// DistMult.py:43-72, ComplEx.py:20-62, RotatE.py:45-91 -> a D2H copy -> testRel, Test.h:194-228):
// one wave per test triple keeps the pair's h and t rows (and whatever of the score depends
// on the pair alone) in registers, scores the true relation, then streams the relation rows and
// counts pred(j) < pred(r) as it goes. Nothing R-sized is staged, so any n_rel >= 1 works.
//
// The arithmetic is the row-wise chain of row_chain.h (the chain behind model.predict on this
// library). What is hoisted out of the (pair, relation) loop is the same operations on the same
// operands, done once: per pair h / |h| and t / |t| (TransE), the four products h* t* (ComplEx); per
// relation r / |r| (TransE, norm_flag) and sin / cos (RotatE), by a prologue into the workspace.
// So a prediction here and mmre_ns_forward's for the same row agree bit for bit, the fused
// evaluation and the reference-shaped loop (predict -> testRel) rank identically, and the tests
// are exact.
#include <math.h>

#include "dispatch.h"
#include "row_chain.h"

namespace mmre {
namespace {

constexpr int RP_WAVES = 4;  // test triples per 256-thread workgroup, one wave each
constexpr int RP_U = 4;      // relation rows in flight per wave
constexpr int RP_MAXDIM = 512;

struct RelArgs {
  int norm_flag, pred_kind, dim;
  float margin;
  const float *ent, *ent_im, *rel, *rel_im;
  const float* work;  // TransE + norm_flag: [R][d] normalised rows; RotatE: [R][2][d] sin, cos
  int64_t n_ent, n_rel;
  const int64_t *qh, *qr, *qt;
  int64_t n_query;
  const int64_t* filt_off;
  const int32_t* filt_ids;
  int32_t* counts;
  float *truth, *scores;
};

// Per-relation values, one wave per relation: r / |r| (TransE with norm_flag: the chain's norm)
// or sin / cos of r / phase_denom (RotatE).
__global__ __launch_bounds__(256) void k_rel_prep(int rotate, const float* __restrict__ rel, int64_t n_rel, int d,
                                                  float phase_denom, float* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * RP_WAVES + (threadIdx.x >> 6);
  if (j >= n_rel) return;  // whole wave exits together
  const float* rv = rel + j * d;
  if (rotate) {
    float* o = work + j * 2 * d;
    for (int k = lane; k < d; k += kWave) rel_sincos(rv[k], phase_denom, &o[k], &o[d + k]);
    return;
  }
  float c = 0.0f;
  for (int k = lane; k < d; k += kWave) c += rv[k] * rv[k];
  const float nr = norm_of_sq(wave_sum(c));
  for (int k = lane; k < d; k += kWave) work[j * d + k] = rv[k] / nr;
}

// What a pair contributes to every one of its R rows.
//   TransE   q0 = h / nh, q1 = t / nt          DistMult q0 = h, q1 = t
//   ComplEx  q0 = hr tr, q1 = hi ti, q2 = hr ti, q3 = hi tr
//   RotatE   q0 = h re, q1 = h im, q2 = t re, q3 = t im
template <int MODEL, int NC>
struct PairCtx {
  float q[4][NC];
};

template <int MODEL, int NC>
__device__ __forceinline__ void pair_load(PairCtx<MODEL, NC>& P, const RelArgs& A, int64_t h, int64_t t, int lane) {
  const int d = A.dim;
  if constexpr (MODEL == MMRE_TRANSE_L1 || MODEL == MMRE_TRANSE_L2) {
    vload(P.q[0], A.ent + h * d, d, lane);
    vload(P.q[1], A.ent + t * d, d, lane);
    float nh = 1.0f, nt = 1.0f;
    if (A.norm_flag) {
      nh = row_norm(P.q[0]);
      nt = row_norm(P.q[1]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      P.q[0][c] = P.q[0][c] / nh;
      P.q[1][c] = P.q[1][c] / nt;
    }
  } else if constexpr (MODEL == MMRE_DISTMULT) {
    vload(P.q[0], A.ent + h * d, d, lane);
    vload(P.q[1], A.ent + t * d, d, lane);
  } else if constexpr (MODEL == MMRE_COMPLEX) {
    float hr[NC], hi[NC], tr[NC], ti[NC];
    vload(hr, A.ent + h * d, d, lane);
    vload(hi, A.ent_im + h * d, d, lane);
    vload(tr, A.ent + t * d, d, lane);
    vload(ti, A.ent_im + t * d, d, lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      P.q[0][c] = hr[c] * tr[c];
      P.q[1][c] = hi[c] * ti[c];
      P.q[2][c] = hr[c] * ti[c];
      P.q[3][c] = hi[c] * tr[c];
    }
  } else {
    vload(P.q[0], A.ent + h * 2 * d, d, lane);
    vload(P.q[1], A.ent + h * 2 * d + d, d, lane);
    vload(P.q[2], A.ent + t * 2 * d, d, lane);
    vload(P.q[3], A.ent + t * 2 * d + d, d, lane);
  }
}

// This lane's partial of the row (pair, relation j).
template <int MODEL, int NC>
__device__ __forceinline__ float rel_partial(const PairCtx<MODEL, NC>& P, const RelArgs& A, int64_t j, int lane) {
  const int d = A.dim;
  float r0[NC], r1[NC];
  if constexpr (MODEL == MMRE_TRANSE_L1 || MODEL == MMRE_TRANSE_L2) {
    // without norm_flag the raw row is the quotient
    vload(r0, (A.norm_flag ? A.work : A.rel) + j * d, d, lane);
  } else if constexpr (MODEL == MMRE_DISTMULT) {
    vload(r0, A.rel + j * d, d, lane);
  } else if constexpr (MODEL == MMRE_COMPLEX) {
    vload(r0, A.rel + j * d, d, lane);
    vload(r1, A.rel_im + j * d, d, lane);
  } else {
    vload(r0, A.work + j * 2 * d, d, lane);      // sin
    vload(r1, A.work + j * 2 * d + d, d, lane);  // cos
  }
  return lane_partial<NC>(d, lane, [&](int c) {
    if constexpr (MODEL <= MMRE_DISTMULT) return row_term<MODEL>(P.q[0][c], r0[c], P.q[1][c]);
    else if constexpr (MODEL == MMRE_COMPLEX)
      return complex_term(P.q[0][c], P.q[1][c], P.q[2][c], P.q[3][c], r0[c], r1[c]);
    else return row_term<MODEL>(P.q[0][c], P.q[1][c], r0[c], r1[c], P.q[2][c], P.q[3][c]);
  });
}

template <int MODEL>
__device__ __forceinline__ float rel_finish(float acc, int pred_kind, float margin) {
  return row_finish(acc, MODEL == MMRE_TRANSE_L2, pred_kind, margin);
}

template <int MODEL, int NC>
__global__ __launch_bounds__(256) void k_rel_sweep(RelArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * RP_WAVES + (threadIdx.x >> 6);
  if (q >= A.n_query) return;  // whole wave exits together
  const int64_t R = A.n_rel;
  const int64_t h = A.qh[q], t = A.qt[q], r = A.qr[q];
  if (h < 0 || h >= A.n_ent || t < 0 || t >= A.n_ent || r < 0 || r >= R) {  // reads no table row
    if (lane == 0) {
      A.counts[q] = 0;
      A.counts[A.n_query + q] = 0;
      A.truth[q] = NAN;
    }
    if (A.scores)
      for (int64_t j = lane; j < R; j += kWave) A.scores[q * R + j] = NAN;
    return;
  }
  PairCtx<MODEL, NC> P;
  pair_load(P, A, h, t, lane);
  const float truth = rel_finish<MODEL>(rel_partial(P, A, r, lane), A.pred_kind, A.margin);
  // the listed (known) relations that beat the truth: what the filtered count leaves out
  int known = 0;
  if (A.filt_off) {
    const int64_t e = A.filt_off[q + 1];
    for (int64_t p = A.filt_off[q]; p < e; ++p) {
      const int64_t j = A.filt_ids[p];
      if (j < 0 || j >= R || j == r) continue;
      known += rel_finish<MODEL>(rel_partial(P, A, j, lane), A.pred_kind, A.margin) < truth;
    }
  }
  int raw = 0;
  for (int64_t j0 = 0; j0 < R; j0 += kWave) {
    const int nj = (int)(R - j0 < kWave ? R - j0 : kWave);
    float mine = 0.0f;  // lane l: pred(j0 + l)
    for (int u = 0; u < nj; u += RP_U) {
      float acc[RP_U];
#pragma unroll
      for (int v = 0; v < RP_U; ++v) {  // past the end: the last row again, kept by no lane
        const int64_t j = j0 + u + v < R ? j0 + u + v : R - 1;
        acc[v] = rel_partial(P, A, j, lane);
      }
#pragma unroll
      for (int v = 0; v < RP_U; ++v) {
        const float p = rel_finish<MODEL>(acc[v], A.pred_kind, A.margin);
        if (lane == u + v) mine = p;
      }
    }
    const int64_t j = j0 + lane;
    const bool valid = lane < nj;
    if (A.scores && valid) A.scores[q * R + j] = mine;
    raw += __popcll(__ballot(valid && j != r && mine < truth));  // strict <: ties, NaN never count
  }
  if (lane == 0) {
    A.counts[q] = raw;
    A.counts[A.n_query + q] = raw - known;
    A.truth[q] = truth;
  }
}

int launch_sweep(int model, const RelArgs& A, hipStream_t st) {
  const dim3 grid((unsigned)((A.n_query + RP_WAVES - 1) / RP_WAVES)), block(64 * RP_WAVES);
  return with_model(model, [&](auto model_) {
    return with_nc<RP_MAXDIM / kWave>(nc_for_dim(A.dim, RP_MAXDIM / kWave), [&](auto nc_) {
      hipLaunchKernelGGL((k_rel_sweep<decltype(model_)::value, decltype(nc_)::value>), grid, block, 0, st, A);
    });
  });
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_rel_workspace(int model, int64_t n_rel, int dim) {
  if (model < MMRE_TRANSE_L1 || model > MMRE_ROTATE || n_rel < 1 || dim < 1 || dim > RP_MAXDIM) return -1;
  const int64_t row = (int64_t)dim * (int64_t)sizeof(float);
  if (model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2) return n_rel * row;
  if (model == MMRE_ROTATE) return 2 * n_rel * row;
  return 0;
}

extern "C" int mmre_rel_evaluate(int model, int norm_flag, int pred_kind, float margin, const float* d_ent,
                                 const float* d_ent_im, const float* d_rel, const float* d_rel_im, int64_t n_ent,
                                 int64_t n_rel, int dim, float phase_denom, const int64_t* d_qh, const int64_t* d_qr,
                                 const int64_t* d_qt, int64_t n_query, const int64_t* d_filt_off,
                                 const int32_t* d_filt_ids, int32_t* d_counts, float* d_truth, float* d_scores,
                                 void* d_work, int64_t work_bytes, void* stream) {
  if (model < MMRE_TRANSE_L1 || model > MMRE_ROTATE) return MMRE_ERR_MODEL;
  if (dim < 1) return MMRE_ERR_ARG;
  if (dim > RP_MAXDIM) return MMRE_ERR_SHAPE;
  if (!d_ent || !d_rel || n_ent < 1 || n_rel < 1 || n_query < 0 || pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (model == MMRE_COMPLEX && (!d_ent_im || !d_rel_im)) return MMRE_ERR_ARG;
  if (model == MMRE_ROTATE && !(phase_denom != 0.0f)) return MMRE_ERR_ARG;  // 0 or NaN
  if ((d_filt_off == nullptr) != (d_filt_ids == nullptr)) return MMRE_ERR_ARG;
  if (n_rel > INT32_MAX || n_query > (int64_t)INT32_MAX) return MMRE_ERR_SHAPE;  // int32 ids; one grid
  if (n_query == 0) return MMRE_OK;
  if (!d_qh || !d_qr || !d_qt || !d_counts || !d_truth) return MMRE_ERR_ARG;
  const bool transe = model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2;
  const bool prep = model == MMRE_ROTATE || (transe && norm_flag);
  if (prep) {
    if (!d_work) return MMRE_ERR_ARG;
    if (work_bytes < mmre_rel_workspace(model, n_rel, dim)) return MMRE_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  RelArgs A;
  A.norm_flag = transe && norm_flag;
  A.pred_kind = pred_kind;
  A.dim = dim;
  A.margin = margin;
  A.ent = d_ent;
  A.ent_im = d_ent_im;
  A.rel = d_rel;
  A.rel_im = d_rel_im;
  A.work = (const float*)d_work;
  A.n_ent = n_ent;
  A.n_rel = n_rel;
  A.qh = d_qh;
  A.qr = d_qr;
  A.qt = d_qt;
  A.n_query = n_query;
  A.filt_off = d_filt_off;
  A.filt_ids = d_filt_ids;
  A.counts = d_counts;
  A.truth = d_truth;
  A.scores = d_scores;
  if (prep) {
    hipLaunchKernelGGL(k_rel_prep, dim3((unsigned)((n_rel + RP_WAVES - 1) / RP_WAVES)), dim3(64 * RP_WAVES), 0, st,
                       model == MMRE_ROTATE ? 1 : 0, d_rel, n_rel, dim, phase_denom, (float*)d_work);
    MMRE_CHECK_LAUNCH();
  }
  return launch_sweep(model, A, st);
}
