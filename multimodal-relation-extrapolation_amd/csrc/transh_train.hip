// transh_train.hip -- TransH negative-sampling training (OpenKE TransH.py:52-107 in 'normal' mode
// under strategy/NegativeSampling.py:23-32 + MarginLoss.py:24-28): the fused loss and its
// gradient into three dense tables (ent, rel, norm_vector), no float atomics, DESIGN.md §10h.
// Below it, the same step for TransD (four tables, six rows per triple) on the same index, scan,
// fill, relation and SGD kernels: the section headed "TransD".
//
// Arithmetic (the "TransH training chain"): f32, -ffp-contract=off, a row's element
// lane + 64 c in slot c, every sum a lane partial in increasing c then wave_sum (row_chain.h).
//   w^ = w / max(|w|, 1e-12)   a_e = e . w^   p_e = e - a_e w^           (e = h, t)
//   norm_flag: p^_e = p_e / max(|p_e|, 1e-12), r^ = r / max(|r|, 1e-12); else p^ = p, r^ = r
//   x = (p^_h + r^) - p^_t     s = sum |x| (L1) or sqrt(sum x^2) (L2)    forward = s or m - s
// Not the sequential-in-k chain of transh.hip: a training score need not be predict's bits.
//
// Backward, per row with g = d(loss)/d(score) (a model margin flips its sign):
//   gx = g sign(x) (L1) or g x / s, 0 where s = 0 (L2)
//   u_e = (+-gx - p^_e (p^_e . +-gx)) / |p_e|, +-gx / 1e-12 where clamped, +-gx without norm_flag
//   dh = u_h - (u_h . w^) w^, dt likewise;  dw^ = -(u_h . w^) h - a_h u_h - (u_t . w^) t - a_t u_t
//   dw = (dw^ - w^ (w^ . dw^)) / |w| or dw^ / 1e-12;  dr as u_e with r^ and |r|
//
// Forward (mmre_transh_ns_forward): one workgroup of four waves per positive b. Every wave holds
// the positive's context in registers (its rows, the unit normal, both projections, r^); rows
// j = wave, wave + 4, ... of [pos | neg_1 .. neg_K] (row b + j B) reuse whatever they share with it
// -- the relation (and with it the normal), a projected entity when relation and entity both
// match -- and load and project the rest, so any batch is scored right. Wave 0 then forms the
// positive's hinge partial from the K + 1 scores in LDS; k_th_reduce sums the partials in a
// fixed order.
//
// Gradient (mmre_transh_ns_grad): store-then-sum.
//   k_th_coef     d(loss)/d(score) of every row (k_ns_row_coef's margin rule), counters zeroed
//   k_th_records  same workgroup shape as the forward. Row i has four record slots 4 i + q
//                 (q = h, t, r, w). Contributions to a row the positive shares are summed on chip
//                 (registers in j order per wave, the four waves' sums in wave order through LDS)
//                 into the positive's slots 4 b + q; a negative's slot is written only for a row
//                 it does not share. Every record carries its rows' regulariser term, so the
//                 owners read records and never parameters. Keys: ekey[2 i + (0 | 1)] the entity
//                 of slots 4 i + (0 | 1) or -1, rkey[i] the relation of slots 4 i + (2, 3) or -1.
//   k_th_scan / k_th_fill   the entity table's inverted index (counts by integer atomics, one
//                 exclusive scan, lists filled in arrival order)
//   k_th_owner    entity rows: one wave per row orders its list by slot id and sums it. Relation
//                 and normal rows keep no list: wave (r, seg) scans rkey over batch rows
//                 [seg TH_SEG, (seg + 1) TH_SEG) with ballots, in order, and sums the matching
//                 record pairs into a partial
//   k_th_rel      one wave per relation adds its partials in segment order
// Every owner writes its whole gradient row (zeros without a record) and with lr != 0 also
// p <- fma(-lr, g, p). Every order is a function of the batch indices alone.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "row_chain.h"

namespace mmre {
namespace {

constexpr int TH_WPP = 4;       // waves per positive
constexpr int TH_MAXK = 512;    // negatives per positive
constexpr int TH_SEG = 1024;    // batch rows one relation-owner wave scans (why)
constexpr int TH_REGL = 16;     // list entries a lane keeps in registers: lists up to 1024 are ordered on chip
constexpr float TH_EPS = 1e-12f;

struct THArgs {
  const float* ent;
  const float* rel;
  const float* nv;
  int64_t n_ent, n_rel;
  int dim;
  const int64_t* h;
  const int64_t* t;
  const int64_t* r;
  int64_t B, K;
  float model_margin;
  int use_model_margin;
  float loss_margin, adv_t, regul_rate;
};

struct THWork {      // d_work carved (th_carve); every region starts on 8 bytes
  int64_t* elist;    // 2 N: the entity lists (slot ids), CSR by eoff
  int64_t* eoff;     // n_ent + 1
  float* part;       // 8 B: per positive hinge partial, sq h, sq t, sq r, sq w
  float* coef;       // N
  int32_t* rkey;     // N
  int32_t* ekey;     // 2 N
  int32_t* ecount;   // n_ent
  int32_t* ecur;     // n_ent
  int32_t* flag;     // n_rel * n_seg: the partial exists
  float* prel;       // n_rel * n_seg * 2 * dim: (rel, normal) partial pairs
  float* rec;        // 4 N * dim
  int64_t n_seg;
  int64_t floats;
};

THWork th_carve(float* base, int64_t B, int64_t K, int64_t n_ent, int64_t n_rel, int dim) {
  const int64_t N = B * (1 + K);
  THWork W;
  W.n_seg = (N + TH_SEG - 1) / TH_SEG;
  int64_t o = 0;
  auto take = [&](int64_t n_floats) {
    const int64_t at = o;
    o += round_up(n_floats, 2);
    return base + at;
  };
  W.elist = reinterpret_cast<int64_t*>(take(4 * N));
  W.eoff = reinterpret_cast<int64_t*>(take(2 * (n_ent + 1)));
  W.part = take(8 * B);
  W.coef = take(N);
  W.rkey = reinterpret_cast<int32_t*>(take(N));
  W.ekey = reinterpret_cast<int32_t*>(take(2 * N));
  W.ecount = reinterpret_cast<int32_t*>(take(n_ent));
  W.ecur = reinterpret_cast<int32_t*>(take(n_ent));
  W.flag = reinterpret_cast<int32_t*>(take(n_rel * W.n_seg));
  W.prel = take(n_rel * W.n_seg * 2 * dim);
  W.rec = take(4 * N * dim);
  W.floats = o;
  return W;
}

template <int NC>
__device__ __forceinline__ void vstore(float* __restrict__ row, const float (&v)[NC], int d, int lane) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + c * kWave;
    if (k < d) row[k] = v[c];
  }
}

template <int NC>
__device__ __forceinline__ float vdot(const float (&a)[NC], const float (&b)[NC]) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) s += a[c] * b[c];
  return wave_sum(s);
}

// A relation's side of a row: raw r and w, the unit normal, r^ and the two norms.
template <int NC>
struct RelCtx {
  float r[NC], w[NC], wh[NC], rh[NC];
  float nw, nr;  // |w|; |r| (1 without norm_flag)
};
// An entity projected on a relation's hyperplane.
template <int NC>
struct EntCtx {
  float e[NC], ph[NC];  // raw row; p^
  float a, np;          // e . w^; |p| (1 without norm_flag)
};

template <int NC, bool NORM>
__device__ __forceinline__ void load_rel(const THArgs& A, int64_t r, int lane, RelCtx<NC>& R) {
  vload(R.r, A.rel + r * A.dim, A.dim, lane);
  vload(R.w, A.nv + r * A.dim, A.dim, lane);
  R.nw = sqrtf(wave_sum(vsq(R.w)));
  const float cw = fmaxf(R.nw, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) R.wh[c] = R.w[c] / cw;
  R.nr = 1.0f;
  if constexpr (NORM) R.nr = sqrtf(wave_sum(vsq(R.r)));
  const float cr = fmaxf(R.nr, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) R.rh[c] = NORM ? R.r[c] / cr : R.r[c];
}

template <int NC, bool NORM>
__device__ __forceinline__ void load_ent(const THArgs& A, int64_t e, const RelCtx<NC>& R, int lane, EntCtx<NC>& E) {
  vload(E.e, A.ent + e * A.dim, A.dim, lane);
  E.a = vdot(E.e, R.wh);
#pragma unroll
  for (int c = 0; c < NC; ++c) E.ph[c] = E.e[c] - E.a * R.wh[c];
  E.np = 1.0f;
  if constexpr (NORM) {
    E.np = sqrtf(wave_sum(vsq(E.ph)));
    const float cp = fmaxf(E.np, TH_EPS);
#pragma unroll
    for (int c = 0; c < NC; ++c) E.ph[c] = E.ph[c] / cp;
  }
}

// x = (p^_h + r^) - p^_t and the raw score s (padding slots hold 0 in every operand: they add +0)
template <int NC, bool L2>
__device__ __forceinline__ float row_x(const EntCtx<NC>& H, const RelCtx<NC>& R, const EntCtx<NC>& T, float (&x)[NC]) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    x[c] = (H.ph[c] + R.rh[c]) - T.ph[c];
    acc += L2 ? x[c] * x[c] : fabsf(x[c]);
  }
  const float s = wave_sum(acc);
  return L2 ? sqrtf(s) : s;
}

// Row j of positive b: its ids, what it shares with the positive, and the contexts (the positive's
// copies or freshly loaded ones).
template <int NC, bool NORM>
struct RowCtx {
  RelCtx<NC> R;
  EntCtx<NC> H, T;
  int64_t h, t, r;
  bool same_r, same_h, same_t;
};
template <int NC, bool NORM>
__device__ __forceinline__ void load_row(const THArgs& A, int64_t i, int lane, int64_t pr, int64_t ph, int64_t pt,
                                         const RelCtx<NC>& PR, const EntCtx<NC>& PH, const EntCtx<NC>& PT,
                                         RowCtx<NC, NORM>& X) {
  X.h = A.h[i]; X.t = A.t[i]; X.r = A.r[i];
  X.same_r = X.r == pr;
  X.same_h = X.same_r && X.h == ph;
  X.same_t = X.same_r && X.t == pt;
  if (X.same_r) X.R = PR; else load_rel<NC, NORM>(A, X.r, lane, X.R);
  if (X.same_h) X.H = PH; else load_ent<NC, NORM>(A, X.h, X.R, lane, X.H);
  if (X.same_t) X.T = PT; else load_ent<NC, NORM>(A, X.t, X.R, lane, X.T);
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_th_forward(THArgs A, float* __restrict__ score, float* __restrict__ part) {
  __shared__ float s_sc[TH_MAXK + 1];
  __shared__ float s_sq[TH_WPP][4];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int64_t pr = A.r[b], ph = A.h[b], pt = A.t[b];
  RelCtx<NC> PR;
  EntCtx<NC> PH, PT;
  load_rel<NC, NORM>(A, pr, lane, PR);
  load_ent<NC, NORM>(A, ph, PR, lane, PH);
  load_ent<NC, NORM>(A, pt, PR, lane, PT);
  float sq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t j = w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    RowCtx<NC, NORM> X;
    load_row<NC, NORM>(A, i, lane, pr, ph, pt, PR, PH, PT, X);
    float x[NC];
    const float s = row_x<NC, L2>(X.H, X.R, X.T, x);
    const float f = A.use_model_margin ? A.model_margin - s : s;
    if (lane == 0) { score[i] = f; s_sc[j] = f; }
    if (A.regul_rate != 0.0f) {
      sq[0] += vsq(X.H.e); sq[1] += vsq(X.T.e); sq[2] += vsq(X.R.r); sq[3] += vsq(X.R.w);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float v = A.regul_rate != 0.0f ? wave_sum(sq[q]) : 0.0f;
    if (lane == 0) s_sq[w][q] = v;
  }
  __syncthreads();
  if (w != 0) return;
  // the positive's hinge partial: sum_j w_j max(p - n_j, -margin), w_j = softmax_j(-T n_j) or 1
  const float p = s_sc[0];
  float mx = -INFINITY, den = 0.0f;
  if (A.adv_t > 0.0f) {
    for (int64_t j = lane; j < A.K; j += kWave) mx = fmaxf(mx, -s_sc[1 + j] * A.adv_t);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
    for (int64_t j = lane; j < A.K; j += kWave) den += expf(-s_sc[1 + j] * A.adv_t - mx);
    den = wave_sum(den);
  }
  float loss = 0.0f;
  for (int64_t j = lane; j < A.K; j += kWave) {
    const float n = s_sc[1 + j];
    const float hinge = fmaxf(p - n, -A.loss_margin);
    loss += A.adv_t > 0.0f ? expf(-n * A.adv_t - mx) / den * hinge : hinge;
  }
  loss = wave_sum(loss);
  if (lane == 0) {
    float* o = part + b * 8;
    o[0] = loss;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[1 + q] = (s_sq[0][q] + s_sq[1][q]) + (s_sq[2][q] + s_sq[3][q]);
  }
}

// Fixed-order reduction of the per-positive partials by one workgroup: strided double sums per
// thread, butterfly wave sums, the four wave totals in a fixed order.
__global__ __launch_bounds__(256) void k_th_reduce(THArgs A, const float* __restrict__ part, float* __restrict__ loss) {
  __shared__ double red[5][4];
  double acc[5] = {0, 0, 0, 0, 0};
  for (int64_t b = threadIdx.x; b < A.B; b += 256) {
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] += (double)part[b * 8 + q];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc[q] += __shfl_xor(acc[q], s);
  }
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < 5; ++q) red[q][threadIdx.x >> 6] = acc[q];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[5];
  for (int q = 0; q < 5; ++q) t[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  const double Bd = (double)A.B, Kd = (double)A.K;
  double l = A.adv_t > 0.0f ? t[0] / Bd : t[0] / (Bd * Kd);
  l += (double)A.loss_margin;
  if (A.regul_rate != 0.0f) {
    const double nd = Bd * (1.0 + Kd) * (double)A.dim;
    l += (double)A.regul_rate * ((t[1] / nd + t[2] / nd + t[3] / nd + t[4] / nd) / 4.0);
  }
  loss[0] = (float)l;
}

// ------------------------------------------------------------------------------------------
// gradient
// ------------------------------------------------------------------------------------------

// d(loss)/d(score) of every row times the upstream gradient (k_ns_row_coef's margin rule: ties at
// the kink split the gradient, the self-adversarial weights are detached); the entity counters of
// this call zeroed.
__global__ __launch_bounds__(256) void k_th_coef(THArgs A, const float* __restrict__ score,
                                                  const float* __restrict__ grad_loss, float* __restrict__ coef,
                                                  int32_t* __restrict__ ecount, int32_t* __restrict__ ecur) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n_ent; i += (int64_t)gridDim.x * blockDim.x) {
    ecount[i] = 0;
    ecur[i] = 0;
  }
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= A.B) return;
  const float gl = grad_loss[0];
  const float p = score[b];
  float mx = -INFINITY, den = 0.0f;
  if (A.adv_t > 0.0f) {
    for (int64_t j = lane; j < A.K; j += kWave) mx = fmaxf(mx, -score[b + (j + 1) * A.B] * A.adv_t);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
    for (int64_t j = lane; j < A.K; j += kWave) den += expf(-score[b + (j + 1) * A.B] * A.adv_t - mx);
    den = wave_sum(den);
  }
  float gp = 0.0f;
  for (int64_t j = lane; j < A.K; j += kWave) {
    const float n = score[b + (j + 1) * A.B];
    const float x = p - n, m = -A.loss_margin;
    const float ind = x > m ? 1.0f : (x == m ? 0.5f : 0.0f);
    const float c = A.adv_t > 0.0f ? (expf(-n * A.adv_t - mx) / den) / (float)A.B : 1.0f / (float)(A.B * A.K);
    coef[b + (j + 1) * A.B] = -(c * ind) * gl;
    gp += c * ind;
  }
  gp = wave_sum(gp);
  if (lane == 0) coef[b] = gp * gl;
}

// The exact derivative of one row's score times g, with respect to its four raw rows (file header).
template <int NC, bool L2, bool NORM>
__device__ __forceinline__ void row_grad(const RowCtx<NC, NORM>& X, float g, float (&dH)[NC], float (&dT)[NC],
                                         float (&dR)[NC], float (&dW)[NC]) {
  float x[NC], gx[NC];
  const float s = row_x<NC, L2>(X.H, X.R, X.T, x);
#pragma unroll
  for (int c = 0; c < NC; ++c)
    gx[c] = L2 ? (s > 0.0f ? g * x[c] / s : 0.0f) : g * (float)((x[c] > 0.0f) - (x[c] < 0.0f));
  float uh[NC], ut[NC];
  if constexpr (NORM) {
    float a = 0.0f, b = 0.0f, e = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      a += X.H.ph[c] * gx[c];
      b += X.T.ph[c] * (-gx[c]);
      e += X.R.rh[c] * gx[c];
    }
    a = wave_sum(a); b = wave_sum(b); e = wave_sum(e);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uh[c] = X.H.np > TH_EPS ? (gx[c] - X.H.ph[c] * a) / X.H.np : gx[c] / TH_EPS;
      ut[c] = X.T.np > TH_EPS ? (-gx[c] - X.T.ph[c] * b) / X.T.np : -gx[c] / TH_EPS;
      dR[c] = X.R.nr > TH_EPS ? (gx[c] - X.R.rh[c] * e) / X.R.nr : gx[c] / TH_EPS;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) { uh[c] = gx[c]; ut[c] = -gx[c]; dR[c] = gx[c]; }
  }
  const float bh = vdot(uh, X.R.wh), bt = vdot(ut, X.R.wh);
  float dwh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dH[c] = uh[c] - bh * X.R.wh[c];
    dT[c] = ut[c] - bt * X.R.wh[c];
    dwh[c] = ((-(bh * X.H.e[c]) - X.H.a * uh[c]) - bt * X.T.e[c]) - X.T.a * ut[c];
  }
  const float q = vdot(X.R.wh, dwh);
#pragma unroll
  for (int c = 0; c < NC; ++c) dW[c] = X.R.nw > TH_EPS ? (dwh[c] - X.R.wh[c] * q) / X.R.nw : dwh[c] / TH_EPS;
}

template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_th_records(THArgs A, const float* __restrict__ coef,
                                                     const float* __restrict__ grad_loss, float reg_unit, THWork W) {
  __shared__ float s_acc[4][TH_WPP][NC * kWave];
  __shared__ int s_cnt[TH_WPP][4];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int d = A.dim;
  const float reg = reg_unit * grad_loss[0];  // the regulariser's weight per gathered row, times the upstream gradient
  const int64_t pr = A.r[b], ph = A.h[b], pt = A.t[b];
  RelCtx<NC> PR;
  EntCtx<NC> PH, PT;
  load_rel<NC, NORM>(A, pr, lane, PR);
  load_ent<NC, NORM>(A, ph, PR, lane, PH);
  load_ent<NC, NORM>(A, pt, PR, lane, PT);
  // This wave's sums for the positive's h, t, r, w rows, in j order, and how many rows each sums.
  // The regulariser joins a shared row once, at the end, as (reg * rows) * row: a negative that
  // repeats its positive then cancels it exactly, as it does in exact arithmetic.
  float acc[4][NC];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[q][c] = 0.0f;
  int cnt[4] = {0, 0, 0, 0};
  for (int64_t j = w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    float g = coef[i];
    const bool files = g != 0.0f || reg != 0.0f;  // else the row adds nothing anywhere
    int32_t kh = -1, kt = -1, kr = -1;
    if (files) {
      if (A.use_model_margin) g = -g;  // forward = m - s
      RowCtx<NC, NORM> X;
      load_row<NC, NORM>(A, i, lane, pr, ph, pt, PR, PH, PT, X);
      float dv[4][NC];
      row_grad<NC, L2, NORM>(X, g, dv[0], dv[1], dv[2], dv[3]);
      // slot q of row i: into the positive's sum when shared, else a record of its own
      auto put = [&](int q, bool shared, float (&v)[NC], const float (&raw)[NC]) {
        if (shared) {
          ++cnt[q];
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[q][c] += v[c];
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c) v[c] += reg * raw[c];
          vstore(W.rec + (4 * i + q) * d, v, d, lane);
        }
      };
      put(0, X.same_h, dv[0], X.H.e);
      put(1, X.same_t, dv[1], X.T.e);
      put(2, X.same_r, dv[2], X.R.r);
      put(3, X.same_r, dv[3], X.R.w);
      if (!X.same_h) kh = (int32_t)X.h;
      if (!X.same_t) kt = (int32_t)X.t;
      if (!X.same_r) kr = (int32_t)X.r;
    }
    if (j > 0 && lane == 0) {  // (row b's keys: below, once the positive's slots are known live)
      W.ekey[2 * i] = kh;
      W.ekey[2 * i + 1] = kt;
      W.rkey[i] = kr;
      if (kh >= 0) atomicAdd(&W.ecount[kh], 1);
      if (kt >= 0) atomicAdd(&W.ecount[kt], 1);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s_acc[q][w][lane + c * kWave] = acc[q][c];
    if (lane == 0) s_cnt[w][q] = cnt[q];
  }
  __syncthreads();
  // wave q adds the four waves' sums of slot q in wave order and writes the positive's record
  const int q = w;
  const int rows = (s_cnt[0][q] + s_cnt[1][q]) + (s_cnt[2][q] + s_cnt[3][q]);
  const bool any = rows > 0;
  if (any) {
    const float rw = reg * (float)rows;
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k = lane + c * kWave;
      const float raw = q == 0 ? PH.e[c] : q == 1 ? PT.e[c] : q == 2 ? PR.r[c] : PR.w[c];
      v[c] = (((s_acc[q][0][k] + s_acc[q][1][k]) + s_acc[q][2][k]) + s_acc[q][3][k]) + rw * raw;
    }
    vstore(W.rec + (4 * b + q) * d, v, d, lane);
  }
  if (lane == 0) {
    if (q == 0) { W.ekey[2 * b] = any ? (int32_t)ph : -1; if (any) atomicAdd(&W.ecount[ph], 1); }
    if (q == 1) { W.ekey[2 * b + 1] = any ? (int32_t)pt : -1; if (any) atomicAdd(&W.ecount[pt], 1); }
    if (q == 2) W.rkey[b] = any ? (int32_t)pr : -1;  // (slots 2 and 3 are live together)
  }
}

// eoff <- exclusive scan of ecount, by one workgroup: a contiguous run per thread, the runs' totals
// scanned inside each wave by shuffles, the sixteen wave totals by every thread.
__global__ __launch_bounds__(1024) void k_th_scan(const int32_t* __restrict__ ecount, int64_t n_ent,
                                                   int64_t* __restrict__ eoff) {
  __shared__ int64_t s_wave[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t per = (n_ent + 1023) / 1024;
  const int64_t lo = threadIdx.x * per, hi = lo + per < n_ent ? lo + per : n_ent;
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += ecount[i];
  int64_t incl = s;  // inclusive scan of the runs' totals over the wave
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int64_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == kWave - 1) s_wave[w] = incl;
  __syncthreads();
  int64_t run = incl - s, total = 0;
  for (int i = 0; i < 16; ++i) {
    if (i < w) run += s_wave[i];
    total += s_wave[i];
  }
  if (threadIdx.x == 0) eoff[n_ent] = total;
  for (int64_t i = lo; i < hi; ++i) {
    eoff[i] = run;
    run += ecount[i];
  }
}

// entity slot s = 2 i + (0 | 1) into its row's list, in arrival order (the owner orders it)
__global__ __launch_bounds__(256) void k_th_fill(THWork W, int64_t n_slots) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const int32_t key = W.ekey[s];
  if (key < 0) return;
  const int p = atomicAdd(&W.ecur[key], 1);
  W.elist[W.eoff[key] + p] = 4 * (s >> 1) + (s & 1);
}

__device__ __forceinline__ int64_t wave_min(int64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int64_t o = __shfl_xor(v, s);
    v = o < v ? o : v;
  }
  return v;
}

// g row -> the gradient table, and with lr != 0 the parameter row's plain SGD step
template <int NC>
__device__ __forceinline__ void owner_write(const float (&g)[NC], float* __restrict__ grad, float* __restrict__ par,
                                            float lr, bool touched, int d, int lane) {
  vstore(grad, g, d, lane);
  if (lr != 0.0f && touched) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k = lane + c * kWave;
      if (k < d) par[k] = __builtin_fmaf(-lr, g[c], par[k]);
    }
  }
}

// Workgroups [0, ent_blocks): one wave per entity row. The rest: one wave per (relation, segment).
template <int NC>
__global__ __launch_bounds__(256) void k_th_owner(THArgs A, THWork W, int64_t ent_blocks, float* ent, float lr,
                                                   float* __restrict__ grad_ent) {
  __shared__ int64_t s_ord[4][kWave];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = A.dim;
  const int64_t N = A.B * (1 + A.K);
  constexpr int64_t kNone = INT64_MAX;
  if ((int64_t)blockIdx.x < ent_blocks) {
    const int64_t e = (int64_t)blockIdx.x * 4 + w;
    if (e >= A.n_ent) return;
    const int64_t off = W.eoff[e], L = W.eoff[e + 1] - off;
    const int64_t* __restrict__ list = W.elist + off;
    float g[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) g[c] = 0.0f;
    if (L <= kWave) {  // rank the slot ids (they are distinct), then sum in rank order
      const int64_t x = lane < L ? list[lane] : kNone;
      int rank = 0;
      for (int m = 0; m < (int)L; ++m) rank += __shfl(x, m) < x ? 1 : 0;
      if (lane < L) s_ord[w][rank] = x;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int k = 0; k < (int)L; ++k) {
        float v[NC];
        vload(v, W.rec + s_ord[w][k] * d, d, lane);
#pragma unroll
        for (int c = 0; c < NC; ++c) g[c] += v[c];
      }
    } else {  // repeated selection of the next larger slot id
      const bool in_regs = L <= (int64_t)TH_REGL * kWave;
      int64_t mine[TH_REGL];
#pragma unroll
      for (int u = 0; u < TH_REGL; ++u) {
        const int64_t at = lane + (int64_t)u * kWave;
        mine[u] = in_regs && at < L ? list[at] : kNone;
      }
      int64_t cur = -1;
      for (int64_t k = 0; k < L; ++k) {
        int64_t best = kNone;
        if (in_regs) {
#pragma unroll
          for (int u = 0; u < TH_REGL; ++u) best = (mine[u] > cur && mine[u] < best) ? mine[u] : best;
        } else {
          for (int64_t at = lane; at < L; at += kWave) {
            const int64_t x = list[at];
            best = (x > cur && x < best) ? x : best;
          }
        }
        cur = wave_min(best);
        float v[NC];
        vload(v, W.rec + cur * d, d, lane);
#pragma unroll
        for (int c = 0; c < NC; ++c) g[c] += v[c];
      }
    }
    owner_write(g, grad_ent + e * d, ent + e * d, lr, L > 0, d, lane);
    return;
  }
  // relation side: the segment's rows of relation r, in row order
  const int64_t item = ((int64_t)blockIdx.x - ent_blocks) * 4 + w;
  if (item >= A.n_rel * W.n_seg) return;
  const int64_t r = item / W.n_seg, seg = item % W.n_seg;
  const int64_t lo = seg * TH_SEG, hi = lo + TH_SEG < N ? lo + TH_SEG : N;
  float gr[NC], gw[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gr[c] = gw[c] = 0.0f;
  bool found = false;
  for (int64_t base = lo; base < hi; base += kWave) {
    const int64_t i = base + lane;
    const bool hit = i < hi && (int64_t)W.rkey[i] == r;
    uint64_t m = __ballot(hit);
    found = found || m != 0;
    while (m) {
      const int64_t row = base + __builtin_ctzll(m);
      m &= m - 1;
      float a[NC], c2[NC];
      vload(a, W.rec + (4 * row + 2) * d, d, lane);
      vload(c2, W.rec + (4 * row + 3) * d, d, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) { gr[c] += a[c]; gw[c] += c2[c]; }
    }
  }
  if (lane == 0) W.flag[item] = found ? 1 : 0;
  if (found) {
    vstore(W.prel + item * 2 * d, gr, d, lane);
    vstore(W.prel + (item * 2 + 1) * d, gw, d, lane);
  }
}

// One wave per relation: its partial pairs added in segment order; both rows written.
template <int NC>
__global__ __launch_bounds__(256) void k_th_rel(THArgs A, THWork W, float* rel, float* nv, float lr,
                                                 float* __restrict__ grad_rel, float* __restrict__ grad_nv) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= A.n_rel) return;
  const int d = A.dim;
  float gr[NC], gw[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gr[c] = gw[c] = 0.0f;
  bool touched = false;
  for (int64_t base = 0; base < W.n_seg; base += kWave) {
    const int64_t s = base + lane;
    uint64_t m = __ballot(s < W.n_seg && W.flag[r * W.n_seg + s] != 0);
    touched = touched || m != 0;
    while (m) {
      const int64_t item = r * W.n_seg + base + __builtin_ctzll(m);
      m &= m - 1;
      float a[NC], c2[NC];
      vload(a, W.prel + item * 2 * d, d, lane);
      vload(c2, W.prel + (item * 2 + 1) * d, d, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) { gr[c] += a[c]; gw[c] += c2[c]; }
    }
  }
  owner_write(gr, grad_rel + r * d, rel + r * d, lr, touched, d, lane);
  owner_write(gw, grad_nv + r * d, nv + r * d, lr, touched, d, lane);
}

bool th_train_model(int model) { return model == MMRE_TRANSH_L1 || model == MMRE_TRANSH_L2; }

// the shapes the kernels have; the ids and the lists' offsets must fit their integer types
bool th_train_shape(int dim, int64_t neg) { return dim >= 1 && dim <= 8 * kWave && neg >= 1 && neg <= TH_MAXK; }
bool th_train_sizes(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel) {
  return batch >= 1 && n_ent >= 1 && n_rel >= 1 && n_ent <= INT32_MAX && n_rel <= INT32_MAX &&
         batch <= (int64_t)INT32_MAX / 8 / (1 + neg);
}

// f(NC, L2, NORM) for the model's instance
template <class F>
int th_dispatch(int model, int norm_flag, int dim, F&& f) {
  return with_nc<8>(nc_for_dim(dim, 8), [&](auto nc) {
    with_bool(model == MMRE_TRANSH_L2, [&](auto l2) {
      return with_bool(norm_flag != 0, [&](auto nm) {
        f(nc, l2, nm);
        return 0;
      });
    });
  });
}

// ==========================================================================================
// TransD (OpenKE TransD.py:94-147 in 'normal' mode): the same step for a model with two rows per
// entity (e, e_p of dim_e) and two per relation (r, r_p of dim_r <= dim_e). The "TransD training
// chain" (DESIGN.md §3), the conventions above, one NC = nc_for_dim(dim_e): relation-side rows are
// loaded zero past dim_r, so every vector of a row has dim_e's register shape.
//   s_e = e . e_p   u_e = e[:dim_r] + s_e r_p   u^_e = u_e / max(|u_e|, 1e-12)      (e = h, t)
//   norm_flag: u^_e <- u^_e / max(|u^_e|, 1e-12), r^ = r / max(|r|, 1e-12); else r^ = r
//   x = (u^_h + r^) - u^_t     s, forward and gx as TransH's
// Backward, v = +-gx:
//   norm_flag: v <- (v - u^ (u^ . v)) / |u^|, v / 1e-12 where clamped; du = v / max(|u|, 1e-12)
//              (where |u| > 1e-12 v is already normal to u^: the first normalise's projection
//              is collapsed; where it is clamped that normalise is linear)
//   else:      du = (v - u^ (u^ . v)) / |u|, v / 1e-12 where clamped
//   q = du . r_p   de = du (its first dim_r elements; it is 0 past them) + q e_p   de_p = q e
//   dr_p = s_h du_h + s_t du_t   dr as TransH's
// Records: row i owns 4 dim_e + 2 dim_r floats, [dh | dh_p | dt | dt_p | dr | dr_p]: entity slot
// 4 i + (0 | 1) of k_th_fill is the pair at (slot & 3) 2 dim_e of row slot >> 2. Keys, the inverted
// index, the relation segments and k_th_rel (rows of dim_r) are TransH's, unchanged.
// ==========================================================================================
struct TDArgs {
  THArgs A;  // ent, rel, nv = rel_transfer, dim = dim_e
  const float* ept;
  int dim_r;
};

__host__ __device__ inline int64_t td_row_floats(int dim_e, int dim_r) { return 4 * (int64_t)dim_e + 2 * (int64_t)dim_r; }

// THWork for TransD: part holds hinge, sq h, t, r, h_p, t_p, r_p (7 of 8); prel pairs of dim_r
THWork td_carve(float* base, int64_t B, int64_t K, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r) {
  const int64_t N = B * (1 + K);
  THWork W;
  W.n_seg = (N + TH_SEG - 1) / TH_SEG;
  int64_t o = 0;
  auto take = [&](int64_t n_floats) {
    const int64_t at = o;
    o += round_up(n_floats, 2);
    return base + at;
  };
  W.elist = reinterpret_cast<int64_t*>(take(4 * N));
  W.eoff = reinterpret_cast<int64_t*>(take(2 * (n_ent + 1)));
  W.part = take(8 * B);
  W.coef = take(N);
  W.rkey = reinterpret_cast<int32_t*>(take(N));
  W.ekey = reinterpret_cast<int32_t*>(take(2 * N));
  W.ecount = reinterpret_cast<int32_t*>(take(n_ent));
  W.ecur = reinterpret_cast<int32_t*>(take(n_ent));
  W.flag = reinterpret_cast<int32_t*>(take(n_rel * W.n_seg));
  W.prel = take(n_rel * W.n_seg * 2 * dim_r);
  W.rec = take(N * td_row_floats(dim_e, dim_r));
  W.floats = o;
  return W;
}

// A relation's side of a row: raw r and r_p (0 past dim_r), r^ and |r| (1 without norm_flag).
template <int NC>
struct TDRel {
  float r[NC], rp[NC], rh[NC];
  float nr;
};
// An entity transferred by a relation: raw e and e_p, the final u^, s = e . e_p, |u| and the
// second normalise's |u^| (1 without norm_flag).
template <int NC>
struct TDEnt {
  float e[NC], ep[NC], uh[NC];
  float s, nu, n2;
};

template <int NC, bool NORM>
__device__ __forceinline__ void td_load_rel(const TDArgs& D, int64_t r, int lane, TDRel<NC>& R) {
  vload(R.r, D.A.rel + r * D.dim_r, D.dim_r, lane);
  vload(R.rp, D.A.nv + r * D.dim_r, D.dim_r, lane);
  R.nr = 1.0f;
  if constexpr (NORM) R.nr = sqrtf(wave_sum(vsq(R.r)));
  const float cr = fmaxf(R.nr, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) R.rh[c] = NORM ? R.r[c] / cr : R.r[c];
}

template <int NC, bool NORM>
__device__ __forceinline__ void td_load_ent(const TDArgs& D, int64_t e, const TDRel<NC>& R, int lane, TDEnt<NC>& E) {
  vload(E.e, D.A.ent + e * D.A.dim, D.A.dim, lane);
  vload(E.ep, D.ept + e * D.A.dim, D.A.dim, lane);
  E.s = vdot(E.e, E.ep);
#pragma unroll
  for (int c = 0; c < NC; ++c) E.uh[c] = (lane + c * kWave < D.dim_r ? E.e[c] : 0.0f) + E.s * R.rp[c];
  E.nu = sqrtf(wave_sum(vsq(E.uh)));
  const float cu = fmaxf(E.nu, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) E.uh[c] = E.uh[c] / cu;
  E.n2 = 1.0f;
  if constexpr (NORM) {
    E.n2 = sqrtf(wave_sum(vsq(E.uh)));
    const float c2 = fmaxf(E.n2, TH_EPS);
#pragma unroll
    for (int c = 0; c < NC; ++c) E.uh[c] = E.uh[c] / c2;
  }
}

template <int NC, bool L2>
__device__ __forceinline__ float td_row_x(const TDEnt<NC>& H, const TDRel<NC>& R, const TDEnt<NC>& T, float (&x)[NC]) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    x[c] = (H.uh[c] + R.rh[c]) - T.uh[c];
    acc += L2 ? x[c] * x[c] : fabsf(x[c]);
  }
  const float s = wave_sum(acc);
  return L2 ? sqrtf(s) : s;
}

template <int NC>
struct TDRow {
  TDRel<NC> R;
  TDEnt<NC> H, T;
  int64_t h, t, r;
  bool same_r, same_h, same_t;
};
template <int NC, bool NORM>
__device__ __forceinline__ void td_load_row(const TDArgs& D, int64_t i, int lane, int64_t pr, int64_t ph, int64_t pt,
                                            const TDRel<NC>& PR, const TDEnt<NC>& PH, const TDEnt<NC>& PT,
                                            TDRow<NC>& X) {
  X.h = D.A.h[i]; X.t = D.A.t[i]; X.r = D.A.r[i];
  X.same_r = X.r == pr;
  X.same_h = X.same_r && X.h == ph;
  X.same_t = X.same_r && X.t == pt;
  if (X.same_r) X.R = PR; else td_load_rel<NC, NORM>(D, X.r, lane, X.R);
  if (X.same_h) X.H = PH; else td_load_ent<NC, NORM>(D, X.h, X.R, lane, X.H);
  if (X.same_t) X.T = PT; else td_load_ent<NC, NORM>(D, X.t, X.R, lane, X.T);
}

template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_tdt_forward(TDArgs D, float* __restrict__ score, float* __restrict__ part) {
  __shared__ float s_sc[TH_MAXK + 1];
  __shared__ float s_sq[TH_WPP][6];
  const THArgs& A = D.A;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int64_t pr = A.r[b], ph = A.h[b], pt = A.t[b];
  TDRel<NC> PR;
  TDEnt<NC> PH, PT;
  td_load_rel<NC, NORM>(D, pr, lane, PR);
  td_load_ent<NC, NORM>(D, ph, PR, lane, PH);
  td_load_ent<NC, NORM>(D, pt, PR, lane, PT);
  float sq[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t j = w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    TDRow<NC> X;
    td_load_row<NC, NORM>(D, i, lane, pr, ph, pt, PR, PH, PT, X);
    float x[NC];
    const float s = td_row_x<NC, L2>(X.H, X.R, X.T, x);
    const float f = A.use_model_margin ? A.model_margin - s : s;
    if (lane == 0) { score[i] = f; s_sc[j] = f; }
    if (A.regul_rate != 0.0f) {
      sq[0] += vsq(X.H.e); sq[1] += vsq(X.T.e); sq[2] += vsq(X.R.r);
      sq[3] += vsq(X.H.ep); sq[4] += vsq(X.T.ep); sq[5] += vsq(X.R.rp);
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const float v = A.regul_rate != 0.0f ? wave_sum(sq[q]) : 0.0f;
    if (lane == 0) s_sq[w][q] = v;
  }
  __syncthreads();
  if (w != 0) return;
  // the positive's hinge partial, as k_th_forward forms it
  const float p = s_sc[0];
  float mx = -INFINITY, den = 0.0f;
  if (A.adv_t > 0.0f) {
    for (int64_t j = lane; j < A.K; j += kWave) mx = fmaxf(mx, -s_sc[1 + j] * A.adv_t);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
    for (int64_t j = lane; j < A.K; j += kWave) den += expf(-s_sc[1 + j] * A.adv_t - mx);
    den = wave_sum(den);
  }
  float loss = 0.0f;
  for (int64_t j = lane; j < A.K; j += kWave) {
    const float n = s_sc[1 + j];
    const float hinge = fmaxf(p - n, -A.loss_margin);
    loss += A.adv_t > 0.0f ? expf(-n * A.adv_t - mx) / den * hinge : hinge;
  }
  loss = wave_sum(loss);
  if (lane == 0) {
    float* o = part + b * 8;
    o[0] = loss;
#pragma unroll
    for (int q = 0; q < 6; ++q) o[1 + q] = (s_sq[0][q] + s_sq[1][q]) + (s_sq[2][q] + s_sq[3][q]);
  }
}

// k_th_reduce for seven partials: the hinge and the six sums of squares (entity rows have dim_e
// elements, relation rows dim_r).
__global__ __launch_bounds__(256) void k_tdt_reduce(TDArgs D, const float* __restrict__ part, float* __restrict__ loss) {
  __shared__ double red[7][4];
  const THArgs& A = D.A;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t b = threadIdx.x; b < A.B; b += 256) {
#pragma unroll
    for (int q = 0; q < 7; ++q) acc[q] += (double)part[b * 8 + q];
  }
#pragma unroll
  for (int q = 0; q < 7; ++q) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc[q] += __shfl_xor(acc[q], s);
  }
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < 7; ++q) red[q][threadIdx.x >> 6] = acc[q];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[7];
  for (int q = 0; q < 7; ++q) t[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  const double Bd = (double)A.B, Kd = (double)A.K;
  double l = A.adv_t > 0.0f ? t[0] / Bd : t[0] / (Bd * Kd);
  l += (double)A.loss_margin;
  if (A.regul_rate != 0.0f) {
    const double ne = Bd * (1.0 + Kd) * (double)A.dim, nr = Bd * (1.0 + Kd) * (double)D.dim_r;
    l += (double)A.regul_rate * ((t[1] / ne + t[2] / ne + t[3] / nr + t[4] / ne + t[5] / ne + t[6] / nr) / 6.0);
  }
  loss[0] = (float)l;
}

// d(score)/d(u^) = v through the normalises to du, then to the entity's two rows (section header).
template <int NC, bool NORM, bool NEG>
__device__ __forceinline__ void td_ent_grad(const TDEnt<NC>& E, const TDRel<NC>& R, const float (&gx)[NC],
                                            float (&du)[NC], float (&dE)[NC], float (&dEp)[NC]) {
  float a = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) a += E.uh[c] * (NEG ? -gx[c] : gx[c]);
  a = wave_sum(a);
  const float cu = fmaxf(E.nu, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float v = NEG ? -gx[c] : gx[c];
    if constexpr (NORM) {
      const float y = E.n2 > TH_EPS ? (v - E.uh[c] * a) / E.n2 : v / TH_EPS;
      du[c] = y / cu;
    } else {
      du[c] = E.nu > TH_EPS ? (v - E.uh[c] * a) / E.nu : v / TH_EPS;
    }
  }
  const float q = vdot(du, R.rp);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dE[c] = du[c] + q * E.ep[c];
    dEp[c] = q * E.e[c];
  }
}

// The exact derivative of one row's score times g with respect to its six raw rows:
// dv[0 .. 5] = dh, dt, dh_p, dt_p, dr, dr_p.
template <int NC, bool L2, bool NORM>
__device__ __forceinline__ void td_row_grad(const TDRow<NC>& X, float g, float (&dv)[6][NC]) {
  float x[NC], gx[NC];
  const float s = td_row_x<NC, L2>(X.H, X.R, X.T, x);
#pragma unroll
  for (int c = 0; c < NC; ++c)
    gx[c] = L2 ? (s > 0.0f ? g * x[c] / s : 0.0f) : g * (float)((x[c] > 0.0f) - (x[c] < 0.0f));
  if constexpr (NORM) {
    float e = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) e += X.R.rh[c] * gx[c];
    e = wave_sum(e);
#pragma unroll
    for (int c = 0; c < NC; ++c) dv[4][c] = X.R.nr > TH_EPS ? (gx[c] - X.R.rh[c] * e) / X.R.nr : gx[c] / TH_EPS;
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) dv[4][c] = gx[c];
  }
  float duh[NC], dut[NC];
  td_ent_grad<NC, NORM, false>(X.H, X.R, gx, duh, dv[0], dv[2]);
  td_ent_grad<NC, NORM, true>(X.T, X.R, gx, dut, dv[1], dv[3]);
#pragma unroll
  for (int c = 0; c < NC; ++c) dv[5][c] = X.H.s * duh[c] + X.T.s * dut[c];
}

// slot q (h, t, h_p, t_p, r, r_p) of a row's record: its offset, and whose sharing decides it
__device__ __forceinline__ int64_t td_slot_off(int q, int de, int dr) {
  return q < 4 ? (int64_t)((q & 1) * 2 + (q >> 1)) * de : 4 * (int64_t)de + (q - 4) * dr;
}
__device__ __forceinline__ int td_slot_pair(int q) { return q < 4 ? (q & 1) : 2; }

template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_tdt_records(TDArgs D, const float* __restrict__ coef,
                                                      const float* __restrict__ grad_loss, float reg_ent,
                                                      float reg_rel, THWork W) {
  __shared__ float s_acc[6][TH_WPP][NC * kWave];
  __shared__ int s_cnt[TH_WPP][3];
  const THArgs& A = D.A;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int de = A.dim, dr = D.dim_r;
  const int64_t stride = td_row_floats(de, dr);
  const float gl = grad_loss[0];
  const float rege = reg_ent * gl, regr = reg_rel * gl;  // the regulariser's weight per gathered row
  const int64_t pr = A.r[b], ph = A.h[b], pt = A.t[b];
  TDRel<NC> PR;
  TDEnt<NC> PH, PT;
  td_load_rel<NC, NORM>(D, pr, lane, PR);
  td_load_ent<NC, NORM>(D, ph, PR, lane, PH);
  td_load_ent<NC, NORM>(D, pt, PR, lane, PT);
  // This wave's sums for the positive's six rows, in j order, and how many rows each pair sums
  // (h, t, r). The regulariser joins a shared row once, at the end, as in k_th_records.
  float acc[6][NC];
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[q][c] = 0.0f;
  int cnt[3] = {0, 0, 0};
  for (int64_t j = w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    float g = coef[i];
    const bool files = g != 0.0f || rege != 0.0f || regr != 0.0f;  // else the row adds nothing anywhere
    int32_t kh = -1, kt = -1, kr = -1;
    if (files) {
      if (A.use_model_margin) g = -g;  // forward = m - s
      TDRow<NC> X;
      td_load_row<NC, NORM>(D, i, lane, pr, ph, pt, PR, PH, PT, X);
      float dv[6][NC];
      td_row_grad<NC, L2, NORM>(X, g, dv);
      float* __restrict__ row = W.rec + i * stride;
      auto put = [&](int q, bool shared, float (&v)[NC], const float (&raw)[NC]) {
        if (shared) {
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[q][c] += v[c];
        } else {
          const float reg = q < 4 ? rege : regr;
#pragma unroll
          for (int c = 0; c < NC; ++c) v[c] += reg * raw[c];
          vstore(row + td_slot_off(q, de, dr), v, q < 4 ? de : dr, lane);
        }
      };
      put(0, X.same_h, dv[0], X.H.e);
      put(2, X.same_h, dv[2], X.H.ep);
      put(1, X.same_t, dv[1], X.T.e);
      put(3, X.same_t, dv[3], X.T.ep);
      put(4, X.same_r, dv[4], X.R.r);
      put(5, X.same_r, dv[5], X.R.rp);
      cnt[0] += X.same_h; cnt[1] += X.same_t; cnt[2] += X.same_r;
      if (!X.same_h) kh = (int32_t)X.h;
      if (!X.same_t) kt = (int32_t)X.t;
      if (!X.same_r) kr = (int32_t)X.r;
    }
    if (j > 0 && lane == 0) {  // (row b's keys: below, once the positive's slots are known live)
      W.ekey[2 * i] = kh;
      W.ekey[2 * i + 1] = kt;
      W.rkey[i] = kr;
      if (kh >= 0) atomicAdd(&W.ecount[kh], 1);
      if (kt >= 0) atomicAdd(&W.ecount[kt], 1);
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s_acc[q][w][lane + c * kWave] = acc[q][c];
  }
  if (lane == 0) { s_cnt[w][0] = cnt[0]; s_cnt[w][1] = cnt[1]; s_cnt[w][2] = cnt[2]; }
  __syncthreads();
  // wave w adds the four waves' sums of slots w and w + 4 in wave order and writes the positive's records
  float* __restrict__ row = W.rec + b * stride;
  for (int q = w; q < 6; q += TH_WPP) {
    const int p = td_slot_pair(q);
    const int rows = (s_cnt[0][p] + s_cnt[1][p]) + (s_cnt[2][p] + s_cnt[3][p]);
    if (rows == 0) continue;
    const float rw = (q < 4 ? rege : regr) * (float)rows;
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k = lane + c * kWave;
      const float raw = q == 0 ? PH.e[c] : q == 1 ? PT.e[c] : q == 2 ? PH.ep[c] : q == 3 ? PT.ep[c]
                      : q == 4 ? PR.r[c] : PR.rp[c];
      v[c] = (((s_acc[q][0][k] + s_acc[q][1][k]) + s_acc[q][2][k]) + s_acc[q][3][k]) + rw * raw;
    }
    vstore(row + td_slot_off(q, de, dr), v, q < 4 ? de : dr, lane);
  }
  if (w == 0 && lane == 0) {
    bool any[3];
    for (int p = 0; p < 3; ++p) any[p] = (s_cnt[0][p] + s_cnt[1][p]) + (s_cnt[2][p] + s_cnt[3][p]) > 0;
    W.ekey[2 * b] = any[0] ? (int32_t)ph : -1;
    W.ekey[2 * b + 1] = any[1] ? (int32_t)pt : -1;
    W.rkey[b] = any[2] ? (int32_t)pr : -1;
    if (any[0]) atomicAdd(&W.ecount[ph], 1);
    if (any[1]) atomicAdd(&W.ecount[pt], 1);
  }
}

// k_th_owner for record pairs. Workgroups [0, ent_blocks): one wave per entity sums its list's
// (e, e_p) pairs in increasing slot id and writes both rows. The rest: one wave per (relation,
// segment) sums the matching (r, r_p) pairs into a partial for k_th_rel. (The list ordering is
// k_th_owner's, repeated: factored into a helper both call, k_th_owner compiles to other code.)
template <int NC>
__global__ __launch_bounds__(256) void k_tdt_owner(TDArgs D, THWork W, int64_t ent_blocks, float* ent, float* ept,
                                                    float lr, float* __restrict__ grad_ent,
                                                    float* __restrict__ grad_ept) {
  __shared__ int64_t s_ord[4][kWave];
  const THArgs& A = D.A;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int de = A.dim, dr = D.dim_r;
  const int64_t stride = td_row_floats(de, dr);
  const int64_t N = A.B * (1 + A.K);
  constexpr int64_t kNone = INT64_MAX;
  if ((int64_t)blockIdx.x < ent_blocks) {
    const int64_t e = (int64_t)blockIdx.x * 4 + w;
    if (e >= A.n_ent) return;
    const int64_t off = W.eoff[e], L = W.eoff[e + 1] - off;
    const int64_t* __restrict__ list = W.elist + off;
    float g[NC], gp[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) g[c] = gp[c] = 0.0f;
    auto add = [&](int64_t slot) {
      const float* __restrict__ pair = W.rec + (slot >> 2) * stride + (slot & 3) * 2 * (int64_t)de;
      float a[NC], c2[NC];
      vload(a, pair, de, lane);
      vload(c2, pair + de, de, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) { g[c] += a[c]; gp[c] += c2[c]; }
    };
    if (L <= kWave) {  // rank the slot ids (they are distinct), then sum in rank order
      const int64_t x = lane < L ? list[lane] : kNone;
      int rank = 0;
      for (int m = 0; m < (int)L; ++m) rank += __shfl(x, m) < x ? 1 : 0;
      if (lane < L) s_ord[w][rank] = x;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int k = 0; k < (int)L; ++k) add(s_ord[w][k]);
    } else {  // repeated selection of the next larger slot id
      const bool in_regs = L <= (int64_t)TH_REGL * kWave;
      int64_t mine[TH_REGL];
#pragma unroll
      for (int u = 0; u < TH_REGL; ++u) {
        const int64_t at = lane + (int64_t)u * kWave;
        mine[u] = in_regs && at < L ? list[at] : kNone;
      }
      int64_t cur = -1;
      for (int64_t k = 0; k < L; ++k) {
        int64_t best = kNone;
        if (in_regs) {
#pragma unroll
          for (int u = 0; u < TH_REGL; ++u) best = (mine[u] > cur && mine[u] < best) ? mine[u] : best;
        } else {
          for (int64_t at = lane; at < L; at += kWave) {
            const int64_t x = list[at];
            best = (x > cur && x < best) ? x : best;
          }
        }
        cur = wave_min(best);
        add(cur);
      }
    }
    owner_write(g, grad_ent + e * de, ent + e * de, lr, L > 0, de, lane);
    owner_write(gp, grad_ept + e * de, ept + e * de, lr, L > 0, de, lane);
    return;
  }
  // relation side: the segment's rows of relation r, in row order
  const int64_t item = ((int64_t)blockIdx.x - ent_blocks) * 4 + w;
  if (item >= A.n_rel * W.n_seg) return;
  const int64_t r = item / W.n_seg, seg = item % W.n_seg;
  const int64_t lo = seg * TH_SEG, hi = lo + TH_SEG < N ? lo + TH_SEG : N;
  float gr[NC], gw[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gr[c] = gw[c] = 0.0f;
  bool found = false;
  for (int64_t base = lo; base < hi; base += kWave) {
    const int64_t i = base + lane;
    const bool hit = i < hi && (int64_t)W.rkey[i] == r;
    uint64_t m = __ballot(hit);
    found = found || m != 0;
    while (m) {
      const int64_t row = base + __builtin_ctzll(m);
      m &= m - 1;
      const float* __restrict__ pair = W.rec + row * stride + 4 * (int64_t)de;
      float a[NC], c2[NC];
      vload(a, pair, dr, lane);
      vload(c2, pair + dr, dr, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) { gr[c] += a[c]; gw[c] += c2[c]; }
    }
  }
  if (lane == 0) W.flag[item] = found ? 1 : 0;
  if (found) {
    vstore(W.prel + item * 2 * dr, gr, dr, lane);
    vstore(W.prel + (item * 2 + 1) * dr, gw, dr, lane);
  }
}

bool td_train_model(int model) { return model == MMRE_TRANSD_L1 || model == MMRE_TRANSD_L2; }
bool td_train_shape(int dim_e, int dim_r, int64_t neg) {
  return dim_r >= 1 && dim_r <= dim_e && th_train_shape(dim_e, neg);
}

TDArgs td_args(const float* ent, const float* ept, const float* rel, const float* rpt, int64_t n_ent, int64_t n_rel,
               int dim_e, int dim_r, const int64_t* h, const int64_t* t, const int64_t* r, int64_t batch, int64_t neg,
               float model_margin, int use_model_margin, float loss_margin, float adv_t, float regul_rate) {
  return TDArgs{THArgs{ent, rel, rpt, n_ent, n_rel, dim_e, h, t, r, batch, neg, model_margin, use_model_margin,
                       loss_margin, adv_t, regul_rate},
                ept, dim_r};
}

// f(NC, L2, NORM) for the model's instance; NC is dim_e's
template <class F>
int td_dispatch(int model, int norm_flag, int dim_e, F&& f) {
  return with_nc<8>(nc_for_dim(dim_e, 8), [&](auto nc) {
    with_bool(model == MMRE_TRANSD_L2, [&](auto l2) {
      return with_bool(norm_flag != 0, [&](auto nm) {
        f(nc, l2, nm);
        return 0;
      });
    });
  });
}

// ==========================================================================================
// TransR (OpenKE TransR.py:37-85 in 'normal' mode): the same step for a model that moves an entity
// into its relation's space with a dim_e x dim_r matrix. The matrix work -- the projection, the
// entity gradient and the matrix gradient -- is three grouped GEMMs on v_mfma_f32_32x32x2_f32 over
// a relation-major index of the batch's projection slots; everything per row stays VALU work in
// the conventions above, NC = nc_for_dim(dim_r).
//
// The "TransR training chain" (DESIGN.md §3): f32, -ffp-contract=off outside the MFMA, whose chain
// is fma in ascending i from +0 (transr.hip).
//   m_e = e . M_r    norm_flag: p_e = m_e / max(|m_e|, 1e-12), r^ = r / max(|r|, 1e-12); else p = m
//   x = (p_h + r^) - p_t     s, forward and gx as TransH's
// Backward: u_e = (+-gx - p_e (p_e . +-gx)) / |m_e|, +-gx / 1e-12 where clamped, +-gx without
// norm_flag; dr as TransH's; de = M_r u_e; dM_r = sum over the relation's slots of e (x) u_e.
// Regulariser: regul_rate S^2 with S = (mean h^2 + mean t^2 + mean r^2 + mean M_r^2) / 4 over the
// batch rows. The forward's reduction leaves S in the workspace; every gathered row r of a table
// with n elements per row then receives regul_rate 2 S (2 r / (4 N n)).
//
// Slots. Row i has two projection slots, 2 i (head) and 2 i + 1 (tail). A positive's slots are
// live; a negative's slot is live where it does not share (entity, relation) with its positive's
// slot of the same side -- TransH's sharing rule, so any batch is scored right. Live slots are
// numbered ("positions") relation-major, in slot order inside a relation: a function of the batch
// indices alone. P, U and D below are indexed by position.
//
// Forward (mmre_transr_ns_forward):
//   k_trt_zero     the counters of this call
//   k_trt_rank     one workgroup per TR_ISEG slots: a live slot's rank among the segment's earlier
//                  live slots of its relation, the segment's count per relation, rows per relation
//   k_trt_offsets  one workgroup: per relation the exclusive scan of its segment counts, and the
//                  scans over relations of slots, MFMA row tiles, dmat segments and dmat partials
//   k_trt_place    one wave per slot: its position, the position's entity and |e|^2
//   k_trt_gemm<0>  P = E_r M_r: workgroup (row tile, column chunk), surplus tiles exit
//   k_trt_frob     |M_r|_F^2 of every relation of the batch (with a regulariser)
//   k_trt_forward  one workgroup per positive as k_th_forward, from P
//   k_trt_reduce   the fixed-order reduction; loss and S
// Gradient (mmre_transr_ns_grad): k_th_coef; k_trt_back (u per live slot, shared slots summed on
// chip onto the positive's in j order; relation records and keys as k_th_records writes them);
// k_trt_gemm<1> (D = U_r M_r^T plus the regulariser's entity term); k_trt_dmat (E_r^T U_r per
// TR_DSEG-slot segment of a relation, slots in position order); k_th_scan, k_th_fill;
// k_trt_owner (entity rows from D in slot order); k_trt_relseg, k_trt_rel (relation rows as
// k_th_owner's relation side and k_th_rel, one row instead of a pair); k_trt_mat (segment tiles
// added in segment order, the regulariser, zeros for relations outside the batch, SGD).
// The parameter updates come last: every kernel before them reads the tables of the forward.
// ==========================================================================================
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR_TM = 32;       // slots per MFMA row tile
constexpr int TR_ISEG = 1024;   // slots one k_trt_rank workgroup ranks
constexpr int TR_DSEG = 1024;   // slots one k_trt_dmat workgroup sums

struct TRWork {
  THWork T;         // elist, eoff, part (hinge, sq h, sq t, sq r), coef, rkey, ekey, ecount, ecur, flag;
                    // prel: n_rel * n_seg rows of dim_r; rec: N relation records of dim_r
  int32_t* rank;    // 2 N: rank in (segment, relation), -1 for a slot that is not live
  int32_t* pos;     // 2 N: a live slot's position
  int32_t* pent;    // 2 N: a position's entity
  int32_t* scnt;    // 2 N: batch rows a position stands for (the gradient call)
  int32_t* segcnt;  // n_iseg * n_rel: slots of (segment, relation); after k_trt_offsets their exclusive scan over segments
  int32_t* nrows;   // n_rel: batch rows of the relation
  int32_t* roff;    // n_rel + 1: positions before the relation
  int32_t* toff;    // n_rel + 1: row tiles before it
  int32_t* soff;    // n_rel + 1: dmat segments before it
  int32_t* poff;    // n_rel + 1: dmat partial tiles before it (a relation of one segment has none)
  float* esq;       // 2 N: |e|^2 of a position's entity
  float* frob;      // n_rel
  float* regs;      // 2: S
  float* P;         // 2 N * dim_r
  float* U;         // 2 N * dim_r
  float* D;         // 2 N * dim_e
  float* dpart;     // n_dpart * dim_e * dim_r
  int64_t n_iseg, n_dpart;
  int64_t floats;
};

// upper bounds of what the device counts, from (B, K, n_rel) alone
inline int64_t tr_tile_bound(int64_t N, int64_t n_rel) { return 2 * N / TR_TM + (n_rel < 2 * N ? n_rel : 2 * N) + 1; }
inline int64_t tr_dseg_bound(int64_t N, int64_t n_rel) { return 2 * N / TR_DSEG + (n_rel < 2 * N ? n_rel : 2 * N) + 1; }
// a relation of c > TR_DSEG slots has ceil(c / TR_DSEG) < 2 c / TR_DSEG partials
inline int64_t tr_dpart_bound(int64_t N) { return 4 * N / TR_DSEG + 1; }

TRWork tr_carve(float* base, int64_t B, int64_t K, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r) {
  const int64_t N = B * (1 + K);
  TRWork W;
  THWork& T = W.T;
  T.n_seg = (N + TH_SEG - 1) / TH_SEG;
  W.n_iseg = (2 * N + TR_ISEG - 1) / TR_ISEG;
  W.n_dpart = tr_dpart_bound(N);
  int64_t o = 0;
  auto take = [&](int64_t n_floats) {  // every region starts on 16 bytes
    const int64_t at = o;
    o += round_up(n_floats, 4);
    return base + at;
  };
  auto take_i = [&](int64_t n) { return reinterpret_cast<int32_t*>(take(n)); };
  T.elist = reinterpret_cast<int64_t*>(take(4 * N));
  T.eoff = reinterpret_cast<int64_t*>(take(2 * (n_ent + 1)));
  T.part = take(8 * B);
  T.coef = take(N);
  T.rkey = take_i(N);
  T.ekey = take_i(2 * N);
  T.ecount = take_i(n_ent);
  T.ecur = take_i(n_ent);
  T.flag = take_i(n_rel * T.n_seg);
  T.prel = take(n_rel * T.n_seg * dim_r);
  T.rec = take(N * dim_r);
  W.rank = take_i(2 * N);
  W.pos = take_i(2 * N);
  W.pent = take_i(2 * N);
  W.scnt = take_i(2 * N);
  W.segcnt = take_i(W.n_iseg * n_rel);
  W.nrows = take_i(n_rel);
  W.roff = take_i(n_rel + 1);
  W.toff = take_i(n_rel + 1);
  W.soff = take_i(n_rel + 1);
  W.poff = take_i(n_rel + 1);
  W.esq = take(2 * N);
  W.frob = take(n_rel);
  W.regs = take(2);
  W.P = take(2 * N * dim_r);
  W.U = take(2 * N * dim_r);
  W.D = take(2 * N * dim_e);
  W.dpart = take(W.n_dpart * dim_e * dim_r);
  T.floats = W.floats = o;
  return W;
}

struct TRArgs {
  THArgs A;  // ent, rel, nv = transfer_matrix, dim = dim_r
  int dim_e;
};

// ---- index ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trt_zero(TRWork W, int64_t n_rel) {
  const int64_t n = W.n_iseg * n_rel;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    W.segcnt[i] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rel; i += (int64_t)gridDim.x * blockDim.x)
    W.nrows[i] = 0;
}

__global__ __launch_bounds__(TR_ISEG) void k_trt_rank(THArgs A, TRWork W) {
  __shared__ __attribute__((aligned(16))) int32_t s_key[TR_ISEG];
  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x, s = seg * TR_ISEG + tid, n_slots = 2 * A.B * (1 + A.K);
  int32_t key = -1;
  if (s < n_slots) {
    const int64_t i = s >> 1, b = i % A.B;
    const bool tail = (s & 1) != 0;
    const int64_t r = A.r[i], e = tail ? A.t[i] : A.h[i];
    const bool shared = i >= A.B && r == A.r[b] && e == (tail ? A.t[b] : A.h[b]);
    if (!shared) key = (int32_t)r;
    if (!tail) atomicAdd(&W.nrows[r], 1);
  }
  s_key[tid] = key;
  __syncthreads();
  if (s >= n_slots) return;
  int32_t rank = -1;
  if (key >= 0) {
    int before = 0, total = 0;
    const int4* k4 = reinterpret_cast<const int4*>(s_key);
    for (int m = 0; m < TR_ISEG / 4; ++m) {
      const int4 v = k4[m];
      const int h0 = v.x == key, h1 = v.y == key, h2 = v.z == key, h3 = v.w == key;
      total += (h0 + h1) + (h2 + h3);
      const int at = 4 * m;
      before += (h0 & (at < tid)) + (h1 & (at + 1 < tid)) + (h2 & (at + 2 < tid)) + (h3 & (at + 3 < tid));
    }
    rank = before;
    if (before == total - 1) W.segcnt[seg * A.n_rel + key] = total;  // the relation's last slot of the segment
  }
  W.rank[s] = rank;
}

// exclusive scan of v over the 1,024 threads of the workgroup, and the total
__device__ __forceinline__ int32_t tr_block_scan(int32_t v, int32_t* s_wave, int32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t incl = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int32_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == kWave - 1) s_wave[w] = incl;
  __syncthreads();
  int32_t run = incl - v;
  total = 0;
  for (int i = 0; i < 16; ++i) {
    if (i < w) run += s_wave[i];
    total += s_wave[i];
  }
  __syncthreads();
  return run;
}

__global__ __launch_bounds__(1024) void k_trt_offsets(TRWork W, int64_t n_rel) {
  __shared__ int32_t s_wave[16];
  int32_t c_r = 0, c_t = 0, c_s = 0, c_p = 0;  // the carries, the same in every thread
  for (int64_t base = 0; base < n_rel; base += 1024) {
    const int64_t r = base + threadIdx.x;
    int32_t c = 0;
    if (r < n_rel) {
      for (int64_t seg = 0; seg < W.n_iseg; ++seg) {
        const int32_t v = W.segcnt[seg * n_rel + r];
        W.segcnt[seg * n_rel + r] = c;
        c += v;
      }
    }
    const int32_t tiles = (c + TR_TM - 1) / TR_TM, segs = (c + TR_DSEG - 1) / TR_DSEG, parts = segs > 1 ? segs : 0;
    int32_t tot;
    const int32_t xr = tr_block_scan(c, s_wave, tot);
    const int32_t n_r = tot;
    const int32_t xt = tr_block_scan(tiles, s_wave, tot);
    const int32_t n_t = tot;
    const int32_t xs = tr_block_scan(segs, s_wave, tot);
    const int32_t n_s = tot;
    const int32_t xp = tr_block_scan(parts, s_wave, tot);
    if (r < n_rel) {
      W.roff[r] = c_r + xr;
      W.toff[r] = c_t + xt;
      W.soff[r] = c_s + xs;
      W.poff[r] = c_p + xp;
    }
    c_r += n_r; c_t += n_t; c_s += n_s; c_p += tot;
  }
  if (threadIdx.x == 0) {
    W.roff[n_rel] = c_r;
    W.toff[n_rel] = c_t;
    W.soff[n_rel] = c_s;
    W.poff[n_rel] = c_p;
  }
}

__global__ __launch_bounds__(256) void k_trt_place(TRArgs R, TRWork W) {
  const THArgs& A = R.A;
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= 2 * A.B * (1 + A.K)) return;
  const int32_t rk = W.rank[s];
  if (rk < 0) return;
  const int64_t i = s >> 1;
  const int64_t r = A.r[i], e = (s & 1) ? A.t[i] : A.h[i];
  const int32_t p = W.roff[r] + W.segcnt[(s / TR_ISEG) * A.n_rel + r] + rk;
  const float* __restrict__ row = A.ent + e * R.dim_e;
  float acc = 0.0f;  // element lane + 64 c in step c: row_chain.h's lane partial
  for (int k = lane; k < R.dim_e; k += kWave) acc += row[k] * row[k];
  acc = wave_sum(acc);
  if (lane == 0) {
    W.pos[s] = p;
    W.pent[p] = (int32_t)e;
    W.esq[p] = acc;
  }
}

// the relation of item t in the exclusive scan off[0 .. n_rel]: the last r with off[r] <= t
__device__ __forceinline__ int64_t tr_find(const int32_t* __restrict__ off, int64_t n_rel, int32_t t) {
  int64_t lo = 0, hi = n_rel;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// row[k .. k + 3] with zeros at and past n; vec: one aligned 16-byte load (n and k multiples of 4)
__device__ __forceinline__ void tr_ld4(float (&v)[4], const float* __restrict__ row, int k, int n, bool ok, bool vec) {
  v[0] = v[1] = v[2] = v[3] = 0.0f;
  if (!ok) return;
  if (vec) {
    if (k < n) {
      const float4 x = *reinterpret_cast<const float4*>(row + k);
      v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k + u < n) v[u] = row[k + u];
  }
}
inline bool tr_vec(const void* p, int n) { return (n & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the grouped GEMMs -----------------------------------------------------------------------
// Workgroup (row tile t, column chunk y): the TR_TM positions of tile t, all of one relation r,
// times TG_NC columns, wave w the 32 columns from 32 w. !TRANS: P = E M_r, A the gathered entity
// rows, K = dim_e, B[k][n] = M_r[k][n]. TRANS: D = U M_r^T, A the tile's rows of U, K = dim_r,
// B[k][n] = M_r[n][k], plus regw scnt e (the regulariser on a position's entity) in the epilogue.
// K runs in blocks of TG_KB through LDS, the next block's values loaded while this one's MFMAs run
// (k_tr_project's scheme); K ascends throughout; rows past K are zeros in both operands.
constexpr int TG_KB = 32, TG_NC = 128, TG_SA = TR_TM + 1, TG_SB = TG_NC + 1;
template <bool TRANS>
__global__ __launch_bounds__(256) void k_trt_gemm(TRWork W, const float* __restrict__ tmat,
                                                  const float* __restrict__ arows, const float* __restrict__ ent,
                                                  int64_t n_rel, int dim_e, int dim_r, bool a_vec, float reg_unit,
                                                  const float* __restrict__ grad_loss, float* __restrict__ out) {
  __shared__ float sA[TG_KB * TG_SA];
  __shared__ float sB[TG_KB * TG_SB];
  const int32_t t = blockIdx.x;
  if (t >= W.toff[n_rel]) return;  // uniform: a surplus tile
  const int64_t r = tr_find(W.toff, n_rel, t);
  const int32_t p0 = W.roff[r] + (t - W.toff[r]) * TR_TM;
  const int32_t left = W.roff[r + 1] - p0;
  const int nv = left < TR_TM ? left : TR_TM;
  const int Kd = TRANS ? dim_r : dim_e, Nc = TRANS ? dim_e : dim_r;
  const int c0 = blockIdx.y * TG_NC;
  const float* __restrict__ M = tmat + r * ((int64_t)dim_e * dim_r);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int a_row = tid >> 3, a_k = (tid & 7) * 4;
  const bool a_ok = a_row < nv;
  const float* __restrict__ a_src = arows;
  if (a_ok) a_src = arows + (TRANS ? (int64_t)(p0 + a_row) : (int64_t)W.pent[p0 + a_row]) * Kd;
  const bool active = c0 + wave * 32 < Nc;  // wave-uniform
  const int nkb = (Kd + TG_KB - 1) / TG_KB;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  float ra[4], rb[16];
  auto gload = [&](int kb) {
    const int k0 = kb * TG_KB;
    tr_ld4(ra, a_src, k0 + a_k, Kd, a_ok, a_vec);
    if constexpr (!TRANS) {
      const int n = c0 + (tid & 127);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + (tid >> 7) + 2 * u;
        rb[u] = (k < Kd && n < Nc) ? M[(int64_t)k * dim_r + n] : 0.0f;
      }
    } else {
      const int k = k0 + (tid & 31);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int n = c0 + (tid >> 5) + 8 * u;
        rb[u] = (k < Kd && n < Nc) ? M[(int64_t)n * dim_r + k] : 0.0f;
      }
    }
  };
  gload(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();  // the block before is consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) sA[(a_k + u) * TG_SA + a_row] = ra[u];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if constexpr (!TRANS) sB[((tid >> 7) + 2 * u) * TG_SB + (tid & 127)] = rb[u];
      else sB[(tid & 31) * TG_SB + (tid >> 5) + 8 * u] = rb[u];
    }
    __syncthreads();
    if (kb + 1 < nkb) gload(kb + 1);
    if (active) {
#pragma unroll
      for (int s = 0; s < TG_KB / 2; ++s) {
        const float a = sA[(2 * s + lh) * TG_SA + li];
        const float b = sB[(2 * s + lh) * TG_SB + wave * 32 + li];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
  }
  const int col = c0 + wave * 32 + li;
  if (col >= Nc) return;
  float regw = 0.0f;
  if constexpr (TRANS) {
    if (reg_unit != 0.0f) regw = (reg_unit * W.regs[0]) * grad_loss[0];
  }
  // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * lh;
    if (row >= nv) continue;
    const int64_t p = p0 + row;
    float v = acc[g];
    if constexpr (TRANS) {
      if (regw != 0.0f) v += (regw * (float)W.scnt[p]) * ent[(int64_t)W.pent[p] * dim_e + col];
    }
    out[p * Nc + col] = v;
  }
}

// dM: workgroup (segment sg, i tile, j chunk): the DM_M x DM_N tile at (i0, j0) of E^T U over the
// positions of segment sg of its relation, in position order, K blocks of DM_KB positions through
// LDS. Wave w: row tile w & 1, the two column tiles from 64 (w >> 1) (k_tr_project's shape). A
// relation of one segment writes its rows of the gradient table, any other its partial tile.
constexpr int DM_KB = 16, DM_M = 64, DM_N = 128, DM_SA = DM_M + 4, DM_SB = DM_N + 4;
__global__ __launch_bounds__(256) void k_trt_dmat(TRWork W, const float* __restrict__ ent, int64_t n_rel, int dim_e,
                                                  int dim_r, bool e_vec, bool u_vec, float* __restrict__ grad_mat) {
  __shared__ float sA[DM_KB * DM_SA];
  __shared__ float sB[DM_KB * DM_SB];
  const int32_t sg = blockIdx.x;
  if (sg >= W.soff[n_rel]) return;  // uniform: a surplus segment
  const int64_t r = tr_find(W.soff, n_rel, sg);
  const int32_t sr = sg - W.soff[r], nseg = W.soff[r + 1] - W.soff[r];
  const int32_t pb = W.roff[r] + sr * TR_DSEG;
  const int32_t pe = pb + TR_DSEG < W.roff[r + 1] ? pb + TR_DSEG : W.roff[r + 1];
  const int i0 = blockIdx.y * DM_M, j0 = blockIdx.z * DM_N;
  const int64_t msz = (int64_t)dim_e * dim_r;
  float* __restrict__ out = nseg == 1 ? grad_mat + r * msz : W.dpart + (int64_t)(W.poff[r] + sr) * msz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int rt = wave & 1, lc0 = (wave >> 1) * 64;
  const bool ta = i0 + rt * 32 < dim_e, t0 = j0 + lc0 < dim_r, t1 = j0 + lc0 + 32 < dim_r;  // wave-uniform
  const int ak = tid >> 4, ac = (tid & 15) * 4;
  const int bk = tid >> 5, bc = (tid & 31) * 4;
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
  float ra[4], rb[2][4];
  auto gload = [&](int32_t p0) {
    const int32_t pa = p0 + ak;
    const bool oka = pa < pe;
    tr_ld4(ra, oka ? ent + (int64_t)W.pent[pa] * dim_e : ent, i0 + ac, dim_e, oka, e_vec);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int32_t pu = p0 + bk + 8 * u;
      tr_ld4(rb[u], W.U + (int64_t)pu * dim_r, j0 + bc, dim_r, pu < pe, u_vec);
    }
  };
  gload(pb);
  for (int32_t p0 = pb; p0 < pe; p0 += DM_KB) {
    __syncthreads();  // the block before is consumed
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      sA[ak * DM_SA + ac + x] = ra[x];
      sB[bk * DM_SB + bc + x] = rb[0][x];
      sB[(bk + 8) * DM_SB + bc + x] = rb[1][x];
    }
    __syncthreads();
    if (p0 + DM_KB < pe) gload(p0 + DM_KB);
    if (ta && t0) {
#pragma unroll
      for (int s = 0; s < DM_KB / 2; ++s) {
        const float a = sA[(2 * s + lh) * DM_SA + rt * 32 + li];
        const float b0 = sB[(2 * s + lh) * DM_SB + lc0 + li];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        if (t1) {
          const float b1 = sB[(2 * s + lh) * DM_SB + lc0 + 32 + li];
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
      }
    }
  }
  const int j = j0 + lc0 + li;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int i = i0 + rt * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
    if (i >= dim_e) continue;
    if (j < dim_r) out[(int64_t)i * dim_r + j] = acc0[g];
    if (j + 32 < dim_r) out[(int64_t)i * dim_r + j + 32] = acc1[g];
  }
}

// One thread per element of the transfer_matrix gradient: a relation's segment tiles in segment
// order, the regulariser's regm rows M, zeros for a relation outside the batch; lr != 0: the step.
__global__ __launch_bounds__(256) void k_trt_mat(TRWork W, float* tmat, int dim_e, int dim_r, float reg_unit,
                                                 const float* __restrict__ grad_loss, float lr,
                                                 float* __restrict__ grad_mat) {
  const int64_t msz = (int64_t)dim_e * dim_r, chunks = (msz + 255) / 256;
  const int64_t r = blockIdx.x / chunks, idx = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (idx >= msz) return;
  const int32_t nseg = W.soff[r + 1] - W.soff[r];
  float g = 0.0f;
  if (nseg == 1) g = grad_mat[r * msz + idx];
  for (int32_t s = 0; nseg > 1 && s < nseg; ++s) g += W.dpart[(int64_t)(W.poff[r] + s) * msz + idx];
  if (nseg > 0) {
    if (reg_unit != 0.0f) g += (((reg_unit * W.regs[0]) * grad_loss[0]) * (float)W.nrows[r]) * tmat[r * msz + idx];
    if (lr != 0.0f) tmat[r * msz + idx] = __builtin_fmaf(-lr, g, tmat[r * msz + idx]);
  }
  grad_mat[r * msz + idx] = g;
}

// |M_r|_F^2 of a relation of the batch, by one workgroup in a fixed order
__global__ __launch_bounds__(256) void k_trt_frob(TRWork W, const float* __restrict__ tmat, int dim_e, int dim_r) {
  __shared__ float s_w[4];
  const int64_t r = blockIdx.x, msz = (int64_t)dim_e * dim_r;
  if (W.nrows[r] == 0) {  // uniform
    if (threadIdx.x == 0) W.frob[r] = 0.0f;
    return;
  }
  const float* __restrict__ M = tmat + r * msz;
  float acc = 0.0f;
  for (int64_t i = threadIdx.x; i < msz; i += 256) acc += M[i] * M[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) W.frob[r] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// ---- the row kernels ---------------------------------------------------------------------------
template <int NC>
struct TRRel {
  float r[NC], rh[NC];
  float nr;  // |r| (1 without norm_flag)
};
template <int NC>
struct TREnt {
  float ph[NC];
  float np;  // |m| (1 without norm_flag)
};

template <int NC, bool NORM>
__device__ __forceinline__ void tr_load_rel(const THArgs& A, int64_t r, int lane, TRRel<NC>& R) {
  vload(R.r, A.rel + r * A.dim, A.dim, lane);
  R.nr = 1.0f;
  if constexpr (NORM) R.nr = sqrtf(wave_sum(vsq(R.r)));
  const float cr = fmaxf(R.nr, TH_EPS);
#pragma unroll
  for (int c = 0; c < NC; ++c) R.rh[c] = NORM ? R.r[c] / cr : R.r[c];
}

template <int NC, bool NORM>
__device__ __forceinline__ void tr_load_ent(const THArgs& A, const float* __restrict__ P, int64_t p, int lane,
                                            TREnt<NC>& E) {
  vload(E.ph, P + p * A.dim, A.dim, lane);
  E.np = 1.0f;
  if constexpr (NORM) {
    E.np = sqrtf(wave_sum(vsq(E.ph)));
    const float cp = fmaxf(E.np, TH_EPS);
#pragma unroll
    for (int c = 0; c < NC; ++c) E.ph[c] = E.ph[c] / cp;
  }
}

template <int NC, bool L2>
__device__ __forceinline__ float tr_row_x(const TREnt<NC>& H, const TRRel<NC>& R, const TREnt<NC>& T, float (&x)[NC]) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    x[c] = (H.ph[c] + R.rh[c]) - T.ph[c];
    acc += L2 ? x[c] * x[c] : fabsf(x[c]);
  }
  const float s = wave_sum(acc);
  return L2 ? sqrtf(s) : s;
}

template <int NC>
struct TRRow {
  TRRel<NC> R;
  TREnt<NC> H, T;
  int64_t h, t, r;
  int32_t qh, qt;  // the positions its projections come from
  bool same_r, same_h, same_t;
};
// the positive of a workgroup: ids, positions, contexts
template <int NC>
struct TRPos {
  TRRel<NC> R;
  TREnt<NC> H, T;
  int64_t h, t, r;
  int32_t qh, qt;
};
template <int NC, bool NORM>
__device__ __forceinline__ void tr_load_pos(const THArgs& A, const TRWork& W, int64_t b, int lane, TRPos<NC>& Q) {
  Q.h = A.h[b]; Q.t = A.t[b]; Q.r = A.r[b];
  Q.qh = W.pos[2 * b]; Q.qt = W.pos[2 * b + 1];
  tr_load_rel<NC, NORM>(A, Q.r, lane, Q.R);
  tr_load_ent<NC, NORM>(A, W.P, Q.qh, lane, Q.H);
  tr_load_ent<NC, NORM>(A, W.P, Q.qt, lane, Q.T);
}
template <int NC, bool NORM>
__device__ __forceinline__ void tr_load_row(const THArgs& A, const TRWork& W, int64_t i, int lane, const TRPos<NC>& Q,
                                            TRRow<NC>& X) {
  X.h = A.h[i]; X.t = A.t[i]; X.r = A.r[i];
  X.same_r = X.r == Q.r;
  X.same_h = X.same_r && X.h == Q.h;
  X.same_t = X.same_r && X.t == Q.t;
  X.qh = X.same_h ? Q.qh : W.pos[2 * i];
  X.qt = X.same_t ? Q.qt : W.pos[2 * i + 1];
  if (X.same_r) X.R = Q.R; else tr_load_rel<NC, NORM>(A, X.r, lane, X.R);
  if (X.same_h) X.H = Q.H; else tr_load_ent<NC, NORM>(A, W.P, X.qh, lane, X.H);
  if (X.same_t) X.T = Q.T; else tr_load_ent<NC, NORM>(A, W.P, X.qt, lane, X.T);
}

// part[b]: the hinge partial, sq h, sq t, sq r of the positive's K + 1 rows
template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_trt_forward(THArgs A, TRWork W, float* __restrict__ score) {
  __shared__ float s_sc[TH_MAXK + 1];
  __shared__ float s_sq[TH_WPP][3];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  TRPos<NC> Q;
  tr_load_pos<NC, NORM>(A, W, b, lane, Q);
  float sqh = 0.0f, sqt = 0.0f, sqr = 0.0f;  // sqh, sqt: sums of whole rows' |e|^2; sqr: a lane partial
  for (int64_t j = w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    TRRow<NC> X;
    tr_load_row<NC, NORM>(A, W, i, lane, Q, X);
    float x[NC];
    const float s = tr_row_x<NC, L2>(X.H, X.R, X.T, x);
    const float f = A.use_model_margin ? A.model_margin - s : s;
    if (lane == 0) { score[i] = f; s_sc[j] = f; }
    if (A.regul_rate != 0.0f) {
      sqh += W.esq[X.qh]; sqt += W.esq[X.qt]; sqr += vsq(X.R.r);
    }
  }
  sqr = A.regul_rate != 0.0f ? wave_sum(sqr) : 0.0f;
  if (lane == 0) { s_sq[w][0] = sqh; s_sq[w][1] = sqt; s_sq[w][2] = sqr; }
  __syncthreads();
  if (w != 0) return;
  // the positive's hinge partial, as k_th_forward forms it
  const float p = s_sc[0];
  float mx = -INFINITY, den = 0.0f;
  if (A.adv_t > 0.0f) {
    for (int64_t j = lane; j < A.K; j += kWave) mx = fmaxf(mx, -s_sc[1 + j] * A.adv_t);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
    for (int64_t j = lane; j < A.K; j += kWave) den += expf(-s_sc[1 + j] * A.adv_t - mx);
    den = wave_sum(den);
  }
  float loss = 0.0f;
  for (int64_t j = lane; j < A.K; j += kWave) {
    const float n = s_sc[1 + j];
    const float hinge = fmaxf(p - n, -A.loss_margin);
    loss += A.adv_t > 0.0f ? expf(-n * A.adv_t - mx) / den * hinge : hinge;
  }
  loss = wave_sum(loss);
  if (lane == 0) {
    float* o = W.T.part + b * 8;
    o[0] = loss;
#pragma unroll
    for (int q = 0; q < 3; ++q) o[1 + q] = (s_sq[0][q] + s_sq[1][q]) + (s_sq[2][q] + s_sq[3][q]);
  }
}

// k_th_reduce for TransR: the hinge, the three row sums and sum_r rows_r |M_r|_F^2 over relations in
// strided order; loss = hinge + regul_rate S^2, and S for the gradient call.
__global__ __launch_bounds__(256) void k_trt_reduce(TRArgs R, TRWork W, float* __restrict__ loss) {
  __shared__ double red[5][4];
  const THArgs& A = R.A;
  double acc[5] = {0, 0, 0, 0, 0};
  for (int64_t b = threadIdx.x; b < A.B; b += 256) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += (double)W.T.part[b * 8 + q];
  }
  if (A.regul_rate != 0.0f)
    for (int64_t r = threadIdx.x; r < A.n_rel; r += 256) acc[4] += (double)W.nrows[r] * (double)W.frob[r];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc[q] += __shfl_xor(acc[q], s);
  }
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < 5; ++q) red[q][threadIdx.x >> 6] = acc[q];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[5];
  for (int q = 0; q < 5; ++q) t[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  const double Bd = (double)A.B, Kd = (double)A.K;
  double l = A.adv_t > 0.0f ? t[0] / Bd : t[0] / (Bd * Kd);
  l += (double)A.loss_margin;
  double S = 0.0;
  if (A.regul_rate != 0.0f) {
    const double n = Bd * (1.0 + Kd), ne = n * (double)R.dim_e, nr = n * (double)A.dim;
    S = (t[1] / ne + t[2] / ne + t[3] / nr + t[4] / (ne * (double)A.dim)) / 4.0;
    l += (double)A.regul_rate * (S * S);
  }
  loss[0] = (float)l;
  W.regs[0] = (float)S;
}

// d(s)/d(p_h), d(s)/d(p_t) and d(s)/d(r) of one row through the normalisations, times sg (-1 for a
// model margin, forward = m - s): the row's u_h, u_t and dr for a unit d(loss)/d(forward).
template <int NC, bool L2, bool NORM>
__device__ __forceinline__ void tr_unit_grad(const TREnt<NC>& H, const TRRel<NC>& R, const TREnt<NC>& T, float sg,
                                             float (&uh)[NC], float (&ut)[NC], float (&dR)[NC]) {
  float x[NC], gx[NC];
  const float s = tr_row_x<NC, L2>(H, R, T, x);
#pragma unroll
  for (int c = 0; c < NC; ++c)
    gx[c] = L2 ? (s > 0.0f ? sg * x[c] / s : 0.0f) : sg * (float)((x[c] > 0.0f) - (x[c] < 0.0f));
  if constexpr (NORM) {
    float a = 0.0f, bb = 0.0f, e = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      a += H.ph[c] * gx[c];
      bb += T.ph[c] * (-gx[c]);
      e += R.rh[c] * gx[c];
    }
    a = wave_sum(a); bb = wave_sum(bb); e = wave_sum(e);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uh[c] = H.np > TH_EPS ? (gx[c] - H.ph[c] * a) / H.np : gx[c] / TH_EPS;
      ut[c] = T.np > TH_EPS ? (-gx[c] - T.ph[c] * bb) / T.np : -gx[c] / TH_EPS;
      dR[c] = R.nr > TH_EPS ? (gx[c] - R.rh[c] * e) / R.nr : gx[c] / TH_EPS;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) { uh[c] = gx[c]; ut[c] = -gx[c]; dR[c] = gx[c]; }
  }
}

// u per live slot and the relation records. Same workgroup shape as the forward. The hinge term of
// negative j weighs (positive - negative j) by a_j = -coef[b + j B] (k_th_coef's positive
// coefficient is their sum, and is not read): a slot negative j shares with its positive gets
// a_j (u_pos - u_j), so a negative that repeats its positive, or scores through the same projections,
// cancels exactly, as it does in exact arithmetic; a slot of its own gets -a_j u_j, and the
// positive's a_j u_pos. The positive's sums are formed on chip (registers in j order per wave, the
// four waves' sums in wave order through LDS). Relation records: rec[i] of dim_r, the positive's
// carrying its shared rows, rkey[i]; the regulariser's relation term rides in them, rows counted
// as in k_th_records.
template <int NC, bool L2, bool NORM>
__global__ __launch_bounds__(256) void k_trt_back(THArgs A, TRWork W, const float* __restrict__ grad_loss,
                                                  float reg_unit) {
  __shared__ float s_acc[3][TH_WPP][NC * kWave];
  __shared__ int s_cnt[TH_WPP][3];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x;
  const int d = A.dim;
  const float reg = reg_unit != 0.0f ? (reg_unit * W.regs[0]) * grad_loss[0] : 0.0f;
  const float sg = A.use_model_margin ? -1.0f : 1.0f;
  TRPos<NC> Q;
  tr_load_pos<NC, NORM>(A, W, b, lane, Q);
  float pu[3][NC];  // the positive's unit u_h, u_t, dr
  tr_unit_grad<NC, L2, NORM>(Q.H, Q.R, Q.T, sg, pu[0], pu[1], pu[2]);
  float acc[3][NC];  // the positive's u_h, u_t, dr
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[q][c] = 0.0f;
  const int own = w == 0 ? 1 : 0;  // row b itself, counted by wave 0
  int cnt[3] = {own, own, own};
  for (int64_t j = w == 0 ? TH_WPP : w; j <= A.K; j += TH_WPP) {
    const int64_t i = b + j * A.B;
    const float a = -W.T.coef[i];
    TRRow<NC> X;
    tr_load_row<NC, NORM>(A, W, i, lane, Q, X);
    float nu[3][NC];
    tr_unit_grad<NC, L2, NORM>(X.H, X.R, X.T, sg, nu[0], nu[1], nu[2]);
    auto put = [&](int q, bool shared, float* __restrict__ rec, float regw) {  // regw: the regulariser on a record of its own
      if (shared) {
        ++cnt[q];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[q][c] += a * (pu[q][c] - nu[q][c]);
      } else {
        float v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          acc[q][c] += a * pu[q][c];
          v[c] = -a * nu[q][c];
          if (regw != 0.0f) v[c] += regw * X.R.r[c];
        }
        vstore(rec, v, d, lane);
      }
    };
    put(0, X.same_h, W.U + (int64_t)X.qh * d, 0.0f);
    put(1, X.same_t, W.U + (int64_t)X.qt * d, 0.0f);
    put(2, X.same_r, W.T.rec + i * d, reg);
    if (lane == 0) {  // (row b's keys: below)
      const int32_t kh = X.same_h ? -1 : (int32_t)X.h, kt = X.same_t ? -1 : (int32_t)X.t;
      W.T.ekey[2 * i] = kh;
      W.T.ekey[2 * i + 1] = kt;
      W.T.rkey[i] = X.same_r ? -1 : (int32_t)X.r;
      if (kh >= 0) { atomicAdd(&W.T.ecount[kh], 1); W.scnt[X.qh] = 1; }
      if (kt >= 0) { atomicAdd(&W.T.ecount[kt], 1); W.scnt[X.qt] = 1; }
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s_acc[q][w][lane + c * kWave] = acc[q][c];
    if (lane == 0) s_cnt[w][q] = cnt[q];
  }
  __syncthreads();
  // wave q < 3 adds the four waves' sums of slot q in wave order (row b itself is among them)
  if (w >= 3) return;
  const int q = w;
  const int rows = (s_cnt[0][q] + s_cnt[1][q]) + (s_cnt[2][q] + s_cnt[3][q]);
  float v[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + c * kWave;
    v[c] = ((s_acc[q][0][k] + s_acc[q][1][k]) + s_acc[q][2][k]) + s_acc[q][3][k];
    if (q == 2) v[c] += (reg * (float)rows) * Q.R.r[c];
  }
  const int32_t qp = q == 0 ? Q.qh : Q.qt;
  vstore(q == 2 ? W.T.rec + b * d : W.U + (int64_t)qp * d, v, d, lane);
  if (lane == 0) {
    if (q == 2) {
      W.T.rkey[b] = (int32_t)Q.r;
    } else {
      const int64_t e = q == 0 ? Q.h : Q.t;
      W.T.ekey[2 * b + q] = (int32_t)e;
      W.scnt[qp] = rows;
      atomicAdd(&W.T.ecount[e], 1);
    }
  }
}

// k_th_owner's entity side over D: one wave per entity orders its list by slot id and sums the
// positions' rows. (The list ordering is k_th_owner's, repeated, as in k_tdt_owner.)
template <int NC>
__global__ __launch_bounds__(256) void k_trt_owner(TRArgs R, TRWork W, float* ent, float lr,
                                                   float* __restrict__ grad_ent) {
  __shared__ int64_t s_ord[4][kWave];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int de = R.dim_e;
  constexpr int64_t kNone = INT64_MAX;
  const int64_t e = (int64_t)blockIdx.x * 4 + w;
  if (e >= R.A.n_ent) return;
  const int64_t off = W.T.eoff[e], L = W.T.eoff[e + 1] - off;
  const int64_t* __restrict__ list = W.T.elist + off;
  float g[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) g[c] = 0.0f;
  auto add = [&](int64_t entry) {  // k_th_fill's entry 4 i + (0 | 1) is slot 2 i + (0 | 1)
    const int64_t p = W.pos[2 * (entry >> 2) + (entry & 3)];
    float a[NC];
    vload(a, W.D + p * de, de, lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) g[c] += a[c];
  };
  if (L <= kWave) {  // rank the slot ids (they are distinct), then sum in rank order
    const int64_t x = lane < L ? list[lane] : kNone;
    int rank = 0;
    for (int m = 0; m < (int)L; ++m) rank += __shfl(x, m) < x ? 1 : 0;
    if (lane < L) s_ord[w][rank] = x;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = 0; k < (int)L; ++k) add(s_ord[w][k]);
  } else {  // repeated selection of the next larger slot id
    const bool in_regs = L <= (int64_t)TH_REGL * kWave;
    int64_t mine[TH_REGL];
#pragma unroll
    for (int u = 0; u < TH_REGL; ++u) {
      const int64_t at = lane + (int64_t)u * kWave;
      mine[u] = in_regs && at < L ? list[at] : kNone;
    }
    int64_t cur = -1;
    for (int64_t k = 0; k < L; ++k) {
      int64_t best = kNone;
      if (in_regs) {
#pragma unroll
        for (int u = 0; u < TH_REGL; ++u) best = (mine[u] > cur && mine[u] < best) ? mine[u] : best;
      } else {
        for (int64_t at = lane; at < L; at += kWave) {
          const int64_t x = list[at];
          best = (x > cur && x < best) ? x : best;
        }
      }
      cur = wave_min(best);
      add(cur);
    }
  }
  owner_write(g, grad_ent + e * de, ent + e * de, lr, L > 0, de, lane);
}

// k_th_owner's relation side for single records: wave (r, seg) sums rec[i] of the segment's rows
// with rkey[i] == r, in row order, into prel[item]
template <int NC>
__global__ __launch_bounds__(256) void k_trt_relseg(THArgs A, TRWork W) {
  const int lane = threadIdx.x & 63;
  const int d = A.dim;
  const int64_t N = A.B * (1 + A.K);
  const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= A.n_rel * W.T.n_seg) return;
  const int64_t r = item / W.T.n_seg, seg = item % W.T.n_seg;
  const int64_t lo = seg * TH_SEG, hi = lo + TH_SEG < N ? lo + TH_SEG : N;
  float gr[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gr[c] = 0.0f;
  bool found = false;
  for (int64_t base = lo; base < hi; base += kWave) {
    const int64_t i = base + lane;
    const bool hit = i < hi && (int64_t)W.T.rkey[i] == r;
    uint64_t m = __ballot(hit);
    found = found || m != 0;
    while (m) {
      const int64_t row = base + __builtin_ctzll(m);
      m &= m - 1;
      float a[NC];
      vload(a, W.T.rec + row * d, d, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) gr[c] += a[c];
    }
  }
  if (lane == 0) W.T.flag[item] = found ? 1 : 0;
  if (found) vstore(W.T.prel + item * d, gr, d, lane);
}

// k_th_rel for single rows: one wave per relation adds its partials in segment order
template <int NC>
__global__ __launch_bounds__(256) void k_trt_rel(THArgs A, TRWork W, float* rel, float lr, float* __restrict__ grad_rel) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= A.n_rel) return;
  const int d = A.dim;
  const int64_t n_seg = W.T.n_seg;
  float gr[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gr[c] = 0.0f;
  bool touched = false;
  for (int64_t base = 0; base < n_seg; base += kWave) {
    const int64_t s = base + lane;
    uint64_t m = __ballot(s < n_seg && W.T.flag[r * n_seg + s] != 0);
    touched = touched || m != 0;
    while (m) {
      const int64_t item = r * n_seg + base + __builtin_ctzll(m);
      m &= m - 1;
      float a[NC];
      vload(a, W.T.prel + item * d, d, lane);
#pragma unroll
      for (int c = 0; c < NC; ++c) gr[c] += a[c];
    }
  }
  owner_write(gr, grad_rel + r * d, rel + r * d, lr, touched, d, lane);
}

bool tr_train_model(int model) { return model == MMRE_TRANSR_L1 || model == MMRE_TRANSR_L2; }
bool tr_train_shape(int dim_e, int dim_r, int64_t neg) {
  return dim_e >= 1 && dim_e <= 8 * kWave && th_train_shape(dim_r, neg);
}

// f(NC, L2, NORM) for the model's instance; NC is dim_r's
template <class F>
int tr_dispatch(int model, int norm_flag, int dim_r, F&& f) {
  return with_nc<8>(nc_for_dim(dim_r, 8), [&](auto nc) {
    with_bool(model == MMRE_TRANSR_L2, [&](auto l2) {
      return with_bool(norm_flag != 0, [&](auto nm) {
        f(nc, l2, nm);
        return 0;
      });
    });
  });
}

}  // namespace
}  // namespace mmre

using namespace mmre;

extern "C" int mmre_transh_ns_supported(int model, int dim, int64_t neg) {
  return th_train_model(model) && th_train_shape(dim, neg) ? 1 : 0;
}

extern "C" int64_t mmre_transh_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim) {
  if (!th_train_shape(dim, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return -1;
  return th_carve(nullptr, batch, neg, n_ent, n_rel, dim).floats;
}

extern "C" int mmre_transh_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                                      const float* d_ent, const float* d_rel, const float* d_norm, int64_t n_ent,
                                      int64_t n_rel, int dim, const int64_t* d_h, const int64_t* d_t,
                                      const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin,
                                      float adv_temperature, float regul_rate, float* d_score, float* d_loss,
                                      float* d_work, void* stream) {
  if (!th_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_norm || !d_h || !d_t || !d_r || !d_score || !d_loss || !d_work) return MMRE_ERR_ARG;
  if (!th_train_shape(dim, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const THArgs A{d_ent, d_rel, d_norm, n_ent, n_rel, dim, d_h, d_t, d_r, batch, neg, model_margin,
                 use_model_margin, loss_margin, adv_temperature, regul_rate};
  const THWork W = th_carve(d_work, batch, neg, n_ent, n_rel, dim);
  const int rc = th_dispatch(model, norm_flag, dim, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_th_forward<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, A,
                       d_score, W.part);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_th_reduce, dim3(1), dim3(256), 0, st, A, W.part, d_loss);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_transh_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                                   float* d_rel, float* d_norm, int64_t n_ent, int64_t n_rel, int dim,
                                   const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch,
                                   int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                                   const float* d_score, const float* d_grad_loss, float* d_grad_ent,
                                   float* d_grad_rel, float* d_grad_norm, float* d_work, float lr, void* stream) {
  if (!th_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_norm || !d_h || !d_t || !d_r || !d_score || !d_grad_loss || !d_grad_ent ||
      !d_grad_rel || !d_grad_norm || !d_work)
    return MMRE_ERR_ARG;
  if (!th_train_shape(dim, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const THArgs A{d_ent, d_rel, d_norm, n_ent, n_rel, dim, d_h, d_t, d_r, batch, neg, model_margin,
                 use_model_margin, loss_margin, adv_temperature, regul_rate};
  const THWork W = th_carve(d_work, batch, neg, n_ent, n_rel, dim);
  const int64_t N = batch * (1 + neg);
  // d/d(row) of regul_rate (mean h^2 + mean t^2 + mean r^2 + mean w^2) / 4 is reg * row per
  // gathered row (k_th_records multiplies it by the upstream gradient, read on the device)
  const float reg = regul_rate != 0.0f ? (float)((double)regul_rate * 2.0 / (4.0 * (double)N * (double)dim)) : 0.0f;
  hipLaunchKernelGGL(k_th_coef, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, A, d_score, d_grad_loss, W.coef,
                     W.ecount, W.ecur);
  MMRE_CHECK_LAUNCH();
  int rc = th_dispatch(model, norm_flag, dim, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_th_records<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, A,
                       W.coef, d_grad_loss, reg, W);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_th_scan, dim3(1), dim3(1024), 0, st, W.ecount, n_ent, W.eoff);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_th_fill, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, st, W, 2 * N);
  MMRE_CHECK_LAUNCH();
  const int64_t ent_blocks = (n_ent + 3) / 4, rel_blocks = (n_rel * W.n_seg + 3) / 4;
  if (ent_blocks + rel_blocks > INT32_MAX) return MMRE_ERR_SHAPE;
  rc = with_nc<8>(nc_for_dim(dim, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_th_owner<decltype(nc)::value>), dim3((unsigned)(ent_blocks + rel_blocks)), dim3(256), 0, st, A, W,
                       ent_blocks, d_ent, lr, d_grad_ent);
  });
  if (rc != MMRE_OK) return rc;
  return with_nc<8>(nc_for_dim(dim, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_th_rel<decltype(nc)::value>), dim3((unsigned)((n_rel + 3) / 4)), dim3(256), 0, st, A, W, d_rel, d_norm,
                       lr, d_grad_rel, d_grad_norm);
  });
}

// ---- TransD ---------------------------------------------------------------------------------
extern "C" int mmre_transd_ns_supported(int model, int dim_e, int dim_r, int64_t neg) {
  return td_train_model(model) && td_train_shape(dim_e, dim_r, neg) ? 1 : 0;
}

extern "C" int64_t mmre_transd_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim_e,
                                            int dim_r) {
  if (!td_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return -1;
  return td_carve(nullptr, batch, neg, n_ent, n_rel, dim_e, dim_r).floats;
}

extern "C" int mmre_transd_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                                      const float* d_ent, const float* d_ent_transfer, const float* d_rel,
                                      const float* d_rel_transfer, int64_t n_ent, int64_t n_rel, int dim_e, int dim_r,
                                      const int64_t* d_h, const int64_t* d_t, const int64_t* d_r, int64_t batch,
                                      int64_t neg, float loss_margin, float adv_temperature, float regul_rate,
                                      float* d_score, float* d_loss, float* d_work, void* stream) {
  if (!td_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_ent_transfer || !d_rel || !d_rel_transfer || !d_h || !d_t || !d_r || !d_score || !d_loss || !d_work)
    return MMRE_ERR_ARG;
  if (!td_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const TDArgs D = td_args(d_ent, d_ent_transfer, d_rel, d_rel_transfer, n_ent, n_rel, dim_e, dim_r, d_h, d_t, d_r,
                           batch, neg, model_margin, use_model_margin, loss_margin, adv_temperature, regul_rate);
  const THWork W = td_carve(d_work, batch, neg, n_ent, n_rel, dim_e, dim_r);
  const int rc = td_dispatch(model, norm_flag, dim_e, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_tdt_forward<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, D,
                       d_score, W.part);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_tdt_reduce, dim3(1), dim3(256), 0, st, D, W.part, d_loss);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_transd_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                                   float* d_ent_transfer, float* d_rel, float* d_rel_transfer, int64_t n_ent,
                                   int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h, const int64_t* d_t,
                                   const int64_t* d_r, int64_t batch, int64_t neg, float loss_margin,
                                   float adv_temperature, float regul_rate, const float* d_score,
                                   const float* d_grad_loss, float* d_grad_ent, float* d_grad_ent_transfer,
                                   float* d_grad_rel, float* d_grad_rel_transfer, float* d_work, float lr,
                                   void* stream) {
  if (!td_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_ent_transfer || !d_rel || !d_rel_transfer || !d_h || !d_t || !d_r || !d_score || !d_grad_loss ||
      !d_grad_ent || !d_grad_ent_transfer || !d_grad_rel || !d_grad_rel_transfer || !d_work)
    return MMRE_ERR_ARG;
  if (!td_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel)) return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const TDArgs D = td_args(d_ent, d_ent_transfer, d_rel, d_rel_transfer, n_ent, n_rel, dim_e, dim_r, d_h, d_t, d_r,
                           batch, neg, model_margin, use_model_margin, loss_margin, adv_temperature, regul_rate);
  THArgs Ar = D.A;  // the relation tables' view, for k_th_rel: rows of dim_r
  Ar.dim = dim_r;
  const THWork W = td_carve(d_work, batch, neg, n_ent, n_rel, dim_e, dim_r);
  const int64_t N = batch * (1 + neg);
  // d/d(row) of regul_rate (the six means) / 6 is reg * row per gathered row: entity rows have dim_e
  // elements, relation rows dim_r (k_tdt_records multiplies by the upstream gradient on the device)
  const double unit = regul_rate != 0.0f ? (double)regul_rate * 2.0 / (6.0 * (double)N) : 0.0;
  const float reg_ent = (float)(unit / (double)dim_e), reg_rel = (float)(unit / (double)dim_r);
  hipLaunchKernelGGL(k_th_coef, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, D.A, d_score, d_grad_loss, W.coef,
                     W.ecount, W.ecur);
  MMRE_CHECK_LAUNCH();
  int rc = td_dispatch(model, norm_flag, dim_e, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_tdt_records<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, D,
                       W.coef, d_grad_loss, reg_ent, reg_rel, W);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_th_scan, dim3(1), dim3(1024), 0, st, W.ecount, n_ent, W.eoff);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_th_fill, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, st, W, 2 * N);
  MMRE_CHECK_LAUNCH();
  const int64_t ent_blocks = (n_ent + 3) / 4, rel_blocks = (n_rel * W.n_seg + 3) / 4;
  if (ent_blocks + rel_blocks > INT32_MAX) return MMRE_ERR_SHAPE;
  rc = with_nc<8>(nc_for_dim(dim_e, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_tdt_owner<decltype(nc)::value>), dim3((unsigned)(ent_blocks + rel_blocks)), dim3(256), 0, st, D, W,
                       ent_blocks, d_ent, d_ent_transfer, lr, d_grad_ent, d_grad_ent_transfer);
  });
  if (rc != MMRE_OK) return rc;
  return with_nc<8>(nc_for_dim(dim_r, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_th_rel<decltype(nc)::value>), dim3((unsigned)((n_rel + 3) / 4)), dim3(256), 0, st, Ar, W, d_rel,
                       d_rel_transfer, lr, d_grad_rel, d_grad_rel_transfer);
  });
}

// ---- TransR ---------------------------------------------------------------------------------
namespace mmre {
namespace {
TRArgs tr_args(const float* ent, const float* rel, const float* tmat, int64_t n_ent, int64_t n_rel, int dim_e,
               int dim_r, const int64_t* h, const int64_t* t, const int64_t* r, int64_t batch, int64_t neg,
               float model_margin, int use_model_margin, float loss_margin, float adv_t, float regul_rate) {
  return TRArgs{THArgs{ent, rel, tmat, n_ent, n_rel, dim_r, h, t, r, batch, neg, model_margin, use_model_margin,
                       loss_margin, adv_t, regul_rate},
                dim_e};
}
// the launch sizes below fit a grid's x
bool tr_train_grids(int64_t batch, int64_t neg, int64_t n_rel, int dim_e, int dim_r) {
  const int64_t N = batch * (1 + neg);
  const int64_t chunks = ((int64_t)dim_e * dim_r + 255) / 256;
  return tr_tile_bound(N, n_rel) <= INT32_MAX && n_rel <= INT32_MAX / chunks &&
         n_rel <= INT32_MAX / ((N + TH_SEG - 1) / TH_SEG);
}
}  // namespace
}  // namespace mmre

extern "C" int mmre_transr_ns_supported(int model, int dim_e, int dim_r, int64_t neg) {
  return tr_train_model(model) && tr_train_shape(dim_e, dim_r, neg) ? 1 : 0;
}

extern "C" int64_t mmre_transr_ns_workspace(int64_t batch, int64_t neg, int64_t n_ent, int64_t n_rel, int dim_e,
                                            int dim_r) {
  if (!tr_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel) ||
      !tr_train_grids(batch, neg, n_rel, dim_e, dim_r))
    return -1;
  return tr_carve(nullptr, batch, neg, n_ent, n_rel, dim_e, dim_r).floats;
}

extern "C" int mmre_transr_ns_forward(int model, int norm_flag, float model_margin, int use_model_margin,
                                      const float* d_ent, const float* d_rel, const float* d_transfer_matrix,
                                      int64_t n_ent, int64_t n_rel, int dim_e, int dim_r, const int64_t* d_h,
                                      const int64_t* d_t, const int64_t* d_r, int64_t batch, int64_t neg,
                                      float loss_margin, float adv_temperature, float regul_rate, float* d_score,
                                      float* d_loss, float* d_work, void* stream) {
  if (!tr_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_transfer_matrix || !d_h || !d_t || !d_r || !d_score || !d_loss || !d_work)
    return MMRE_ERR_ARG;
  if (!tr_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel) ||
      !tr_train_grids(batch, neg, n_rel, dim_e, dim_r))
    return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const TRArgs R = tr_args(d_ent, d_rel, d_transfer_matrix, n_ent, n_rel, dim_e, dim_r, d_h, d_t, d_r, batch, neg,
                           model_margin, use_model_margin, loss_margin, adv_temperature, regul_rate);
  const TRWork W = tr_carve(d_work, batch, neg, n_ent, n_rel, dim_e, dim_r);
  const int64_t N = batch * (1 + neg);
  hipLaunchKernelGGL(k_trt_zero, dim3(256), dim3(256), 0, st, W, n_rel);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trt_rank, dim3((unsigned)W.n_iseg), dim3(TR_ISEG), 0, st, R.A, W);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trt_offsets, dim3(1), dim3(1024), 0, st, W, n_rel);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trt_place, dim3((unsigned)((2 * N + 3) / 4)), dim3(256), 0, st, R, W);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_trt_gemm<false>), dim3((unsigned)tr_tile_bound(N, n_rel), (unsigned)((dim_r + TG_NC - 1) / TG_NC)),
                     dim3(256), 0, st, W, d_transfer_matrix, d_ent, d_ent, n_rel, dim_e, dim_r, tr_vec(d_ent, dim_e),
                     0.0f, (const float*)nullptr, W.P);
  MMRE_CHECK_LAUNCH();
  if (regul_rate != 0.0f) {
    hipLaunchKernelGGL(k_trt_frob, dim3((unsigned)n_rel), dim3(256), 0, st, W, d_transfer_matrix, dim_e, dim_r);
    MMRE_CHECK_LAUNCH();
  }
  const int rc = tr_dispatch(model, norm_flag, dim_r, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_trt_forward<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, R.A,
                       W, d_score);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL(k_trt_reduce, dim3(1), dim3(256), 0, st, R, W, d_loss);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_transr_ns_grad(int model, int norm_flag, float model_margin, int use_model_margin, float* d_ent,
                                   float* d_rel, float* d_transfer_matrix, int64_t n_ent, int64_t n_rel, int dim_e,
                                   int dim_r, const int64_t* d_h, const int64_t* d_t, const int64_t* d_r,
                                   int64_t batch, int64_t neg, float loss_margin, float adv_temperature,
                                   float regul_rate, const float* d_score, const float* d_grad_loss,
                                   float* d_grad_ent, float* d_grad_rel, float* d_grad_transfer_matrix, float* d_work,
                                   float lr, void* stream) {
  if (!tr_train_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_rel || !d_transfer_matrix || !d_h || !d_t || !d_r || !d_score || !d_grad_loss || !d_grad_ent ||
      !d_grad_rel || !d_grad_transfer_matrix || !d_work)
    return MMRE_ERR_ARG;
  if (!tr_train_shape(dim_e, dim_r, neg) || !th_train_sizes(batch, neg, n_ent, n_rel) ||
      !tr_train_grids(batch, neg, n_rel, dim_e, dim_r))
    return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const TRArgs R = tr_args(d_ent, d_rel, d_transfer_matrix, n_ent, n_rel, dim_e, dim_r, d_h, d_t, d_r, batch, neg,
                           model_margin, use_model_margin, loss_margin, adv_temperature, regul_rate);
  const TRWork W = tr_carve(d_work, batch, neg, n_ent, n_rel, dim_e, dim_r);
  const int64_t N = batch * (1 + neg);
  // d/d(x) of regul_rate S^2 is regul_rate 2 S (2 x / (4 N n)) = unit(n) S x per gathered row of n
  // elements (the kernels multiply by S and the upstream gradient, read on the device)
  const double unit = regul_rate != 0.0f ? (double)regul_rate / (double)N : 0.0;
  const float reg_ent = (float)(unit / (double)dim_e), reg_rel = (float)(unit / (double)dim_r);
  const float reg_mat = (float)(unit / ((double)dim_e * (double)dim_r));
  hipLaunchKernelGGL(k_th_coef, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, R.A, d_score, d_grad_loss, W.T.coef,
                     W.T.ecount, W.T.ecur);
  MMRE_CHECK_LAUNCH();
  int rc = tr_dispatch(model, norm_flag, dim_r, [&](auto nc, auto l2, auto nm) {
    hipLaunchKernelGGL((k_trt_back<decltype(nc)::value, decltype(l2)::value, decltype(nm)::value>), dim3((unsigned)batch), dim3(256), 0, st, R.A, W,
                       d_grad_loss, reg_rel);
  });
  if (rc != MMRE_OK) return rc;
  hipLaunchKernelGGL((k_trt_gemm<true>), dim3((unsigned)tr_tile_bound(N, n_rel), (unsigned)((dim_e + TG_NC - 1) / TG_NC)),
                     dim3(256), 0, st, W, d_transfer_matrix, W.U, d_ent, n_rel, dim_e, dim_r, tr_vec(W.U, dim_r), reg_ent,
                     d_grad_loss, W.D);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_trt_dmat,
                     dim3((unsigned)tr_dseg_bound(N, n_rel), (unsigned)((dim_e + DM_M - 1) / DM_M),
                          (unsigned)((dim_r + DM_N - 1) / DM_N)),
                     dim3(256), 0, st, W, d_ent, n_rel, dim_e, dim_r, tr_vec(d_ent, dim_e), tr_vec(W.U, dim_r),
                     d_grad_transfer_matrix);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_th_scan, dim3(1), dim3(1024), 0, st, W.T.ecount, n_ent, W.T.eoff);
  MMRE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_th_fill, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, st, W.T, 2 * N);
  MMRE_CHECK_LAUNCH();
  rc = with_nc<8>(nc_for_dim(dim_e, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_trt_owner<decltype(nc)::value>), dim3((unsigned)((n_ent + 3) / 4)), dim3(256), 0, st, R, W, d_ent, lr,
                       d_grad_ent);
  });
  if (rc != MMRE_OK) return rc;
  rc = with_nc<8>(nc_for_dim(dim_r, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_trt_relseg<decltype(nc)::value>), dim3((unsigned)((n_rel * W.T.n_seg + 3) / 4)), dim3(256), 0, st, R.A, W);
  });
  if (rc != MMRE_OK) return rc;
  rc = with_nc<8>(nc_for_dim(dim_r, 8), [&](auto nc) {
    hipLaunchKernelGGL((k_trt_rel<decltype(nc)::value>), dim3((unsigned)((n_rel + 3) / 4)), dim3(256), 0, st, R.A, W, d_rel, lr,
                       d_grad_rel);
  });
  if (rc != MMRE_OK) return rc;
  const int64_t chunks = ((int64_t)dim_e * dim_r + 255) / 256;
  hipLaunchKernelGGL(k_trt_mat, dim3((unsigned)(n_rel * chunks)), dim3(256), 0, st, W, d_transfer_matrix, dim_e, dim_r,
                     reg_mat, d_grad_loss, lr, d_grad_transfer_matrix);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}
