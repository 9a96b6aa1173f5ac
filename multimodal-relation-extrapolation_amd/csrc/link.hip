// link.hip -- link prediction on MI355X: the all-entity score sweep with a fused
// rank epilogue (replaces Tester.run_link_prediction's per-query loop,
// OpenKE/openke/config/Tester.py:70-91, with getHeadBatch/getTailBatch Test.h:36-53,
// model.predict and testHead/testTail Test.h:65-192).
//
// Data layout in HBM: the entity table and the query vectors are
// stored "k-major" -- plane[k][n] with n padded to 128 -- so that one K step of a
// 128-wide tile is a single contiguous 512-byte row: coalesced 16-B loads into LDS,
// conflict-free LDS reads, no transposes inside the hot loop.
//
// Kernels defined here (per evaluation, one stream):
//   k_prep_rows, k_prep_km_gated   table -> k-major plane + row-major copy (F.normalize for TransE
//                     norm_flag); the planes alone, gated on a device flag
//   k_prep_queries    (h, r, t, mode) -> k-major query vectors (+ truth ids)
//   k_truth_filter    pred(truth) per query (the sweep's arithmetic) and the filtered-rank
//                     correction, one workgroup per filter group (queries sharing a list)
//   k_filter_scores, k_filter_count   the grouped truth + filter pass, two phases
//   k_counts_finalize filtered columns += raw columns, after a sweep
//   k_sweep_mfma      DistMult/ComplEx: v_mfma_f32_32x32x2_f32, register-counter epilogue
//   k_bf3_*, k_sweep_bf3, k_sweep_bf3w   the split-bf16 MFMA filter in front of it
//   k_l1q_*, k_zero_words           TransE L1's integer filter: quantisation, probe, route
//   k_eval_*, k_heavy_rows          the fused TransE L1 evaluation
// Not here: the VALU sweep (k_sweep_valu: TransE L1/L2, RotatE and the integer filter's code
// sweeps, 49 of the engine's 102 kernels) is link_valu.hip, reached through launch_valu<OP>,
// launch_valu_grp<OP> and valu_grp_fills_grid. link_common.h holds what the two units share.
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "link_common.h"

namespace mmre {

// ------------------------------------------------------------------ prep ----
// Both prep kernels stage a block of rows through LDS (row stride kt+1: odd, so the
// per-row sequential reads and the column-wise k-major writes are bank-conflict free):
// global reads are contiguous row segments, global writes are contiguous in both the
// row-major and the k-major layout.

// Rows per LDS block for a row width kt: a power of two <= 16 (so it divides the 256
// threads; 64-B k-major write runs, ~900 workgroups at |E| = 14k) with <= 64 KB of LDS.
__host__ inline int stage_rows(int kt) {
  int rb = 16;
  while (rb > 1 && (int64_t)rb * (kt + 1) * 4 > 64 * 1024) rb >>= 1;
  return rb;
}

// Value k (< np*kp) of source row e in the plane layout [re 0..kp) [im kp..2kp).
__device__ __forceinline__ float plane_src(int model, const float* __restrict__ src, const float* __restrict__ src_im,
                                           int64_t e, int dim, int kp, int k) {
  const int pl = k >= kp;
  const int kk = k - pl * kp;
  if (kk >= dim) return 0.0f;
  if (model == MMRE_COMPLEX) return (pl ? src_im : src)[e * dim + kk];
  if (model == MMRE_ROTATE) return src[e * 2 * dim + pl * dim + kk];  // RotatE rows [re | im] (RotatE.py:48-49)
  return src[e * dim + kk];
}

// Thread layouts of the staging kernels (256 threads): row phases use 8 row slots x 32
// lanes along k (coalesced row segments, independent loads per thread); the k-major write
// uses rb lanes along the rows x 256/rb k slots (contiguous rb-float runs per k).
__device__ __forceinline__ void write_k_major(const float* lds, int ls, int rb, int kt, float* __restrict__ out,
                                              int64_t pad, int64_t r0) {
  const int i = threadIdx.x % rb, ks = threadIdx.x / rb, kstep = 256 / rb;
  const int64_t e = r0 + i;
  if (e >= pad) return;
#pragma unroll 4
  for (int k = ks; k < kt; k += kstep) out[(int64_t)k * pad + e] = lds[i * ls + k];
}

// Table rows -> (optional) k-major planes out_km[kt][pad] and row-major rows[n][rw]
// (rw <= kt). TransE with norm_flag: F.normalize(x, 2, -1) = x / max(||x||_2, 1e-12)
// (TransE.py:63-66), ||x|| from the canonical sequential sum of squares.
__device__ __forceinline__ void prep_rows_body(int model, int norm_flag, const float* __restrict__ src,
                                               const float* __restrict__ src_im, int64_t n, int dim, int kp, int rb,
                                               float* __restrict__ out_km, int64_t pad, float* __restrict__ rows,
                                               int rw, float* lds, float* s_norm) {
  const int kt = n_planes(model) * kp, ls = kt + 1;
  const int lane = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int64_t e0 = (int64_t)blockIdx.x * rb;
  for (int i = slot; i < rb; i += 8) {
    const int64_t e = e0 + i;
    float* x = lds + i * ls;
#pragma unroll 4
    for (int k = lane; k < kt; k += 32) x[k] = e < n ? plane_src(model, src, src_im, e, dim, kp, k) : 0.0f;
  }
  __syncthreads();
  const bool transe = model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2;
  if (transe && norm_flag) {
    if (threadIdx.x < rb) {
      const float* x = lds + threadIdx.x * ls;
      float ss = 0.0f;  // canonical sequential order; LDS reads batched 16 per round
      int k = 0;
      for (; k + 16 <= dim; k += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = x[k + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) ss = ss + v[u] * v[u];
      }
      for (; k < dim; ++k) ss = ss + x[k] * x[k];
      const float nr = sqrtf(ss);
      s_norm[threadIdx.x] = nr < 1e-12f ? 1e-12f : nr;
    }
    __syncthreads();
    for (int i = slot; i < rb; i += 8) {
      float* x = lds + i * ls;
      const float nr = s_norm[i];
      for (int k = lane; k < kt; k += 32) x[k] = x[k] / nr;
    }
    __syncthreads();
  }
  for (int i = slot; i < rb; i += 8) {
    const int64_t e = e0 + i;
    if (e >= n) break;
    const float* x = lds + i * ls;
#pragma unroll 4
    for (int k = lane; k < rw; k += 32) rows[e * rw + k] = x[k];
  }
  if (out_km) write_k_major(lds, ls, rb, kt, out_km, pad, e0);
}
__global__ __launch_bounds__(256) void k_prep_rows(int model, int norm_flag, const float* __restrict__ src,
                                                   const float* __restrict__ src_im, int64_t n, int dim, int kp,
                                                   int rb, float* __restrict__ out_km, int64_t pad,
                                                   float* __restrict__ rows, int rw) {
  extern __shared__ float lds[];
  __shared__ float s_norm[32];
  prep_rows_body(model, norm_flag, src, src_im, n, dim, kp, rb, out_km, pad, rows, rw, lds, s_norm);
}
// The k-major planes of a table whose row-major copy is the raw table itself (DistMult, d a
// multiple of 16: mmre_link_sweep_bf3_rows), gated: only when *gate != 0 -- the split-bf16
// filter's list overflowed and the exact f32 sweep that reads these planes is about to count.
__global__ __launch_bounds__(256) void k_prep_km_gated(const uint32_t* __restrict__ gate, int model,
                                                       const float* __restrict__ src, int64_t n, int dim, int kp,
                                                       int rb, float* __restrict__ out_km, int64_t pad) {
  extern __shared__ float lds[];
  __shared__ float s_norm[32];
  if (__builtin_amdgcn_readfirstlane(*gate) == 0u) return;
  prep_rows_body(model, 0, src, nullptr, n, dim, kp, rb, out_km, pad, nullptr, 0, lds, s_norm);
}

// Query vectors, one LDS block of rb queries: the anchor rows (t for head_batch, h for
// tail_batch) are copied from the prepared entity rows, combined element-wise with the
// relation row (rel = normalised relation rows for TransE norm_flag), written k-major.
__global__ __launch_bounds__(256) void k_prep_queries(int model, const float* __restrict__ ent_rows,
                                                      const float* __restrict__ rel, const float* __restrict__ rel_im,
                                                      int dim, int kp, int rb, float phase_denom,
                                                      const int64_t* __restrict__ qh, const int64_t* __restrict__ qr,
                                                      const int64_t* __restrict__ qt, const int8_t* __restrict__ qmode,
                                                      int64_t n_query, float* __restrict__ out, int64_t q_pad,
                                                      int32_t* __restrict__ qtrue, float* __restrict__ q_rows,
                                                      int rel_norm) {
  extern __shared__ float lds[];
  __shared__ int64_t s_anchor[32], s_rel[32];
  __shared__ int s_head[32];
  __shared__ float s_rnorm[32];
  const int np = n_planes(model);
  const int kt = np * kp, ls = kt + 1;
  const int lane = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int64_t q0 = (int64_t)blockIdx.x * rb;
  if (threadIdx.x < rb) {
    const int64_t q = q0 + threadIdx.x;
    int64_t a = -1, r = 0;
    int head = 0;
    if (q < n_query) {
      head = qmode[q] == MMRE_HEAD_BATCH;
      a = head ? qt[q] : qh[q];
      r = qr[q];
      qtrue[q] = (int32_t)(head ? qh[q] : qt[q]);
    }
    s_anchor[threadIdx.x] = a;
    s_rel[threadIdx.x] = r;
    s_head[threadIdx.x] = head;
    if (rel_norm) {  // TransE norm_flag: F.normalize of the relation row (TransE.py:63-66), in
                     // k_prep_rows' canonical order, so r / |r| is bit-identical to its output
      const float* rp = rel + r * dim;
      float ss = 0.0f;
      int k = 0;
      if ((dim & 3) == 0) {  // 16-B aligned rows: 64 values per round trip (a short latency chain)
        for (; k + 64 <= dim; k += 64) {
          float4 v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = reinterpret_cast<const float4*>(rp + k)[u];
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            ss = ss + v[u].x * v[u].x;
            ss = ss + v[u].y * v[u].y;
            ss = ss + v[u].z * v[u].z;
            ss = ss + v[u].w * v[u].w;
          }
        }
      }
      for (; k + 16 <= dim; k += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = rp[k + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) ss = ss + v[u] * v[u];
      }
      for (; k < dim; ++k) ss = ss + rp[k] * rp[k];
      const float nr = sqrtf(ss);
      s_rnorm[threadIdx.x] = nr < 1e-12f ? 1e-12f : nr;
    }
  }
  __syncthreads();
  for (int i = slot; i < rb; i += 8) {
    const int64_t a = s_anchor[i];
    float* x = lds + i * ls;
    const float* src = ent_rows + (a < 0 ? 0 : a) * kt;
#pragma unroll 4
    for (int k = lane; k < kt; k += 32) x[k] = a < 0 ? 0.0f : src[k];
  }
  __syncthreads();
  for (int i = slot; i < rb; i += 8) {
    float* x = lds + i * ls;
    const bool valid = s_anchor[i] >= 0;
    const int64_t r = s_rel[i];
    const bool head = s_head[i];
#pragma unroll 2
    for (int k = lane; k < kp; k += 32) {
      if (!valid || k >= dim) {
        x[k] = 0.0f;
        if (np == 2) x[kp + k] = 0.0f;
        continue;
      }
      if (model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2) {
        // head_batch: score = h + (r - t) -> q = -(r - t); tail_batch: (h + r) - t -> q = h + r
        // (TransE.py:71-74). |q - e| reproduces both element-wise bit-for-bit.
        const float b = rel_norm ? rel[r * dim + k] / s_rnorm[i] : rel[r * dim + k];
        x[k] = head ? -(b - x[k]) : (x[k] + b);
      } else if (model == MMRE_DISTMULT) {  // head: h*(r*t) ; tail: (h*r)*t  (DistMult.py:37-42)
        const float b = rel[r * dim + k];
        x[k] = head ? b * x[k] : x[k] * b;
      } else if (model == MMRE_COMPLEX) {  // ComplEx.py:20-27 regrouped by the candidate entity
        const float rr = rel[r * dim + k], ri = rel_im[r * dim + k];
        const float ar = x[k], ai = x[kp + k];  // anchor (t for head_batch, h for tail_batch)
        if (head) { x[k] = ar * rr + ai * ri; x[kp + k] = ai * rr - ar * ri; }
        else      { x[k] = ar * rr - ai * ri; x[kp + k] = ai * rr + ar * ri; }
      } else {  // RotatE (RotatE.py:51-72): rotate by the relation phase, regrouped per candidate
        float sn, cs;
        canon_sincos(rel[r * dim + k] / phase_denom, &sn, &cs);
        const float ar = x[k], ai = x[kp + k];
        if (head) { x[k] = cs * ar + sn * ai; x[kp + k] = cs * ai - sn * ar; }
        else      { x[k] = ar * cs - ai * sn; x[kp + k] = ar * sn + ai * cs; }
      }
    }
  }
  __syncthreads();
  write_k_major(lds, ls, rb, kt, out, q_pad, q0);
  if (q_rows) {  // row-major copy for the per-group loads of k_truth_filter
    for (int i = slot; i < rb; i += 8) {
      const int64_t q = q0 + i;
      if (q >= n_query) break;
      const float* x = lds + i * ls;
#pragma unroll 4
      for (int k = lane; k < kt; k += 32) q_rows[q * kt + k] = x[k];
    }
  }
}

// v_writelane_b32 with an immediate lane select (the lane must be a compile-time constant after
// unrolling: the switch folds away). Writes the wave-uniform s into lane `lane` of v.
template <int L>
__device__ __forceinline__ int writelane_c(int v, int s) {
  __asm__ volatile("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(L));
  return v;
}
__device__ __forceinline__ int writelane_imm(int v, int s, int lane) {
  switch (lane) {
    case 0: return writelane_c<0>(v, s);
    case 1: return writelane_c<1>(v, s);
    case 2: return writelane_c<2>(v, s);
    case 3: return writelane_c<3>(v, s);
    case 4: return writelane_c<4>(v, s);
    case 5: return writelane_c<5>(v, s);
    case 6: return writelane_c<6>(v, s);
    case 7: return writelane_c<7>(v, s);
    case 8: return writelane_c<8>(v, s);
    case 9: return writelane_c<9>(v, s);
    case 10: return writelane_c<10>(v, s);
    case 11: return writelane_c<11>(v, s);
    case 12: return writelane_c<12>(v, s);
    case 13: return writelane_c<13>(v, s);
    case 14: return writelane_c<14>(v, s);
    case 15: return writelane_c<15>(v, s);
    case 16: return writelane_c<16>(v, s);
    case 17: return writelane_c<17>(v, s);
    case 18: return writelane_c<18>(v, s);
    case 19: return writelane_c<19>(v, s);
    case 20: return writelane_c<20>(v, s);
    case 21: return writelane_c<21>(v, s);
    case 22: return writelane_c<22>(v, s);
    case 23: return writelane_c<23>(v, s);
    case 24: return writelane_c<24>(v, s);
    case 25: return writelane_c<25>(v, s);
    case 26: return writelane_c<26>(v, s);
    case 27: return writelane_c<27>(v, s);
    case 28: return writelane_c<28>(v, s);
    case 29: return writelane_c<29>(v, s);
    case 30: return writelane_c<30>(v, s);
    case 31: return writelane_c<31>(v, s);
    case 32: return writelane_c<32>(v, s);
    case 33: return writelane_c<33>(v, s);
    case 34: return writelane_c<34>(v, s);
    case 35: return writelane_c<35>(v, s);
    case 36: return writelane_c<36>(v, s);
    case 37: return writelane_c<37>(v, s);
    case 38: return writelane_c<38>(v, s);
    case 39: return writelane_c<39>(v, s);
    case 40: return writelane_c<40>(v, s);
    case 41: return writelane_c<41>(v, s);
    case 42: return writelane_c<42>(v, s);
    case 43: return writelane_c<43>(v, s);
    case 44: return writelane_c<44>(v, s);
    case 45: return writelane_c<45>(v, s);
    case 46: return writelane_c<46>(v, s);
    case 47: return writelane_c<47>(v, s);
    case 48: return writelane_c<48>(v, s);
    case 49: return writelane_c<49>(v, s);
    case 50: return writelane_c<50>(v, s);
    case 51: return writelane_c<51>(v, s);
    case 52: return writelane_c<52>(v, s);
    case 53: return writelane_c<53>(v, s);
    case 54: return writelane_c<54>(v, s);
    case 55: return writelane_c<55>(v, s);
    case 56: return writelane_c<56>(v, s);
    case 57: return writelane_c<57>(v, s);
    case 58: return writelane_c<58>(v, s);
    case 59: return writelane_c<59>(v, s);
    case 60: return writelane_c<60>(v, s);
    case 61: return writelane_c<61>(v, s);
    case 62: return writelane_c<62>(v, s);
    case 63: return writelane_c<63>(v, s);
    default: return v;
  }
}

// Two scores of the query vector sq against entity rows e1 and e2 at once (two independent
// canonical chains; their loads share the round trips): 32 floats of each row per round
// (RotatE: 16 re + 16 im of each). kp % 8 == 0.
template <int OP>
__device__ void pair_score2_lds(const float* __restrict__ ent_rows, const float* sq, int kp, int64_t e1, int64_t e2,
                                float* s1, float* s2) {
  constexpr int NP = (OP == 2 || OP == 4) ? 2 : 1;
  constexpr int W = (OP == 2) ? 16 : 32;  // floats of one plane per row per round
  const int kt = NP * kp;
  const float* r1 = ent_rows + e1 * (int64_t)kt;
  const float* r2 = ent_rows + e2 * (int64_t)kt;
  float a1 = 0.0f, a2 = 0.0f;
  const int kend = (OP == 2) ? kp : kt;  // RotatE walks k over one plane, pairing re/im
  int k0 = 0;
  for (; k0 + W <= kend; k0 += W) {
    float4 x1[W / 4], x2[W / 4], y1[OP == 2 ? W / 4 : 1], y2[OP == 2 ? W / 4 : 1];
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      x1[i] = *reinterpret_cast<const float4*>(r1 + k0 + 4 * i);
      x2[i] = *reinterpret_cast<const float4*>(r2 + k0 + 4 * i);
      if constexpr (OP == 2) {
        y1[i] = *reinterpret_cast<const float4*>(r1 + kp + k0 + 4 * i);
        y2[i] = *reinterpret_cast<const float4*>(r2 + kp + k0 + 4 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      const int k = k0 + 4 * i;
      if constexpr (OP == 2) {
        a1 = op_step<OP>(a1, sq[k + 0], sq[kp + k + 0], x1[i].x, y1[i].x);
        a2 = op_step<OP>(a2, sq[k + 0], sq[kp + k + 0], x2[i].x, y2[i].x);
        a1 = op_step<OP>(a1, sq[k + 1], sq[kp + k + 1], x1[i].y, y1[i].y);
        a2 = op_step<OP>(a2, sq[k + 1], sq[kp + k + 1], x2[i].y, y2[i].y);
        a1 = op_step<OP>(a1, sq[k + 2], sq[kp + k + 2], x1[i].z, y1[i].z);
        a2 = op_step<OP>(a2, sq[k + 2], sq[kp + k + 2], x2[i].z, y2[i].z);
        a1 = op_step<OP>(a1, sq[k + 3], sq[kp + k + 3], x1[i].w, y1[i].w);
        a2 = op_step<OP>(a2, sq[k + 3], sq[kp + k + 3], x2[i].w, y2[i].w);
      } else {
        a1 = op_step<OP>(a1, sq[k + 0], 0.0f, x1[i].x, 0.0f);
        a2 = op_step<OP>(a2, sq[k + 0], 0.0f, x2[i].x, 0.0f);
        a1 = op_step<OP>(a1, sq[k + 1], 0.0f, x1[i].y, 0.0f);
        a2 = op_step<OP>(a2, sq[k + 1], 0.0f, x2[i].y, 0.0f);
        a1 = op_step<OP>(a1, sq[k + 2], 0.0f, x1[i].z, 0.0f);
        a2 = op_step<OP>(a2, sq[k + 2], 0.0f, x2[i].z, 0.0f);
        a1 = op_step<OP>(a1, sq[k + 3], 0.0f, x1[i].w, 0.0f);
        a2 = op_step<OP>(a2, sq[k + 3], 0.0f, x2[i].w, 0.0f);
      }
    }
  }
  for (; k0 < kend; k0 += 8) {
    float x1[8], x2[8], y1[8], y2[8];
    *reinterpret_cast<float4*>(&x1[0]) = *reinterpret_cast<const float4*>(r1 + k0);
    *reinterpret_cast<float4*>(&x1[4]) = *reinterpret_cast<const float4*>(r1 + k0 + 4);
    *reinterpret_cast<float4*>(&x2[0]) = *reinterpret_cast<const float4*>(r2 + k0);
    *reinterpret_cast<float4*>(&x2[4]) = *reinterpret_cast<const float4*>(r2 + k0 + 4);
    if constexpr (OP == 2) {
      *reinterpret_cast<float4*>(&y1[0]) = *reinterpret_cast<const float4*>(r1 + kp + k0);
      *reinterpret_cast<float4*>(&y1[4]) = *reinterpret_cast<const float4*>(r1 + kp + k0 + 4);
      *reinterpret_cast<float4*>(&y2[0]) = *reinterpret_cast<const float4*>(r2 + kp + k0);
      *reinterpret_cast<float4*>(&y2[4]) = *reinterpret_cast<const float4*>(r2 + kp + k0 + 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float qb = (OP == 2) ? sq[kp + k0 + i] : 0.0f;
      a1 = op_step<OP>(a1, sq[k0 + i], qb, x1[i], (OP == 2) ? y1[i] : 0.0f);
      a2 = op_step<OP>(a2, sq[k0 + i], qb, x2[i], (OP == 2) ? y2[i] : 0.0f);
    }
  }
  *s1 = op_final<OP>(a1);
  *s2 = op_final<OP>(a2);
}

// Truth scores + filtered-rank correction, one 64-thread workgroup (one wave) per filter
// group. A filter group is a set of queries with the same (mode, r, anchor) -- the lookup
// key of Test.h:85's `_find` ((r, t) for head_batch, (h, r) for tail_batch) -- so its
// members share the query vector and the known-entity list. Per pass, lane i scores listed
// entity i of the pass and (first pass) the truth of member query i in one fused pair of
// chains, then every member counts the listed entities that beat its own truth:
//   thr[q]        = pred(true(q))                 (same arithmetic as the sweep)
//   counts[.][q]  = {0, -c, 0, -cc}, c = #{listed j != true(q) : pred(j) < thr[q]}
//                   (cc: those allowed by the type constraint); the sweep adds the raw counts.
// Groups of more than 64 queries are walked 64 at a time (FilterIndex.groups splits them).
// grp_qoff/grp_q == NULL: every query is its own group (off indexed by query).
constexpr int FT = 64;  // threads per filter workgroup = listed entities per pass
template <int OP>
__global__ __launch_bounds__(FT) void k_truth_filter(
    const float* __restrict__ ent_rows, int64_t n_ent, const float* __restrict__ q_km, int64_t q_pad, int kp,
    const float* __restrict__ q_rows, const int32_t* __restrict__ qtrue, const int64_t* __restrict__ qr,
    const int8_t* __restrict__ qmode, int64_t n_query, int pred_kind, float margin, const int64_t* __restrict__ grp_qoff,
    const int32_t* __restrict__ grp_q, int64_t n_groups, const int64_t* __restrict__ off,
    const int32_t* __restrict__ ids, const uint32_t* __restrict__ type_head, const uint32_t* __restrict__ type_tail,
    int64_t type_words, float* __restrict__ thr, int32_t* __restrict__ counts) {
  extern __shared__ float sq[];  // [NP * kp] query vector of the group
  __shared__ float s_v[FT];
  __shared__ int32_t s_id[FT];
  __shared__ uint8_t s_tb[FT];
  constexpr int NP = (OP == 2 || OP == 4) ? 2 : 1;
  const int tid = threadIdx.x;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t qa = grp_qoff ? grp_qoff[g] : g, qb = grp_qoff ? grp_qoff[g + 1] : g + 1;
    const int64_t la = off ? off[g] : 0, lb = off ? off[g + 1] : 0;
    const int64_t q0 = grp_q ? grp_q[qa] : qa;
    __syncthreads();  // previous group done with sq / s_*
    if (q_rows) {  // one contiguous row (the k-major column would touch one cache line per k)
      for (int k = tid; k < NP * kp; k += FT) sq[k] = q_rows[q0 * NP * kp + k];
    } else {
      for (int k = tid; k < NP * kp; k += FT) sq[k] = q_km[(int64_t)k * q_pad + q0];
    }
    const uint32_t* tm = type_head ? (qmode[q0] == MMRE_HEAD_BATCH ? type_head : type_tail) : nullptr;
    const int64_t r = qr[q0];
    __syncthreads();
    for (int64_t qc = qa; qc < qb; qc += FT) {
      const int64_t qi = qc + tid;
      const bool active = qi < qb;
      const int64_t q = active ? (grp_q ? grp_q[qi] : qi) : 0;
      const int32_t tr = active ? qtrue[q] : 0;
      float th = 0.0f;
      int c = 0, cc = 0;
      int64_t lc = la;
      bool first = true;
      do {  // at least one pass: the truth scores ride on the first
        const int nl = (int)((lb - lc) < FT ? (lb - lc) : FT);
        const int64_t j = tid < nl ? (int64_t)ids[lc + tid] : -1;
        const bool ok = j >= 0 && j < n_ent;
        float vt, vj;
        pair_score2_lds<OP>(ent_rows, sq, kp, tr, ok ? j : 0, &vt, &vj);
        if (first) {
          th = apply_pred(pred_kind, margin, vt);
          if (active) thr[q] = th;
        }
        s_id[tid] = ok ? (int32_t)j : -1;
        s_v[tid] = apply_pred(pred_kind, margin, vj);
        s_tb[tid] = (ok && tm) ? (uint8_t)type_bit(tm, type_words, r, j) : (uint8_t)0;
        __syncthreads();
        if (active) {
          for (int i = 0; i < nl; ++i) {
            const int32_t e = s_id[i];
            if (e >= 0 && e != tr && s_v[i] < th) {
              c += 1;
              cc += s_tb[i];
            }
          }
        }
        __syncthreads();  // s_* reuse
        lc += nl;
        first = false;
      } while (lc < lb);
      if (active) {
        counts[0 * n_query + q] = 0;
        counts[1 * n_query + q] = -c;
        counts[2 * n_query + q] = 0;
        counts[3 * n_query + q] = -cc;
      }
    }
  }
}

// --------------------------------------------- grouped truth + filter (2 phases) ---
// Phase 1, k_filter_scores: one lane per score task, all tasks of the evaluation in one
// flat launch (~1.3k waves at FB15K-237-ZS, resident at once): task t < n_query is the
// truth of query t -> thr[t]; task n_query + p is listed entity p of the filter CSR, scored
// with the query vector of its group's representative query entry_q[p] -> list_v[p].
// Both rows stream from global 32 floats per round (RotatE 16 re + 16 im).
template <int OP>
__device__ float row_score(const float* __restrict__ qv, const float* __restrict__ ev, int kp) {
  constexpr int W = (OP == 2) ? 16 : 32;  // 64 VGPRs of loads in flight per round
  const int kend = (OP == 2) ? kp : ((OP == 4) ? 2 * kp : kp);
  float acc = 0.0f;
  int k0 = 0;
  for (; k0 + W <= kend; k0 += W) {
    float4 a[W / 4], x[W / 4], b[OP == 2 ? W / 4 : 1], y[OP == 2 ? W / 4 : 1];
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      a[i] = *reinterpret_cast<const float4*>(qv + k0 + 4 * i);
      x[i] = *reinterpret_cast<const float4*>(ev + k0 + 4 * i);
      if constexpr (OP == 2) {
        b[i] = *reinterpret_cast<const float4*>(qv + kp + k0 + 4 * i);
        y[i] = *reinterpret_cast<const float4*>(ev + kp + k0 + 4 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      if constexpr (OP == 2) {
        acc = op_step<OP>(acc, a[i].x, b[i].x, x[i].x, y[i].x);
        acc = op_step<OP>(acc, a[i].y, b[i].y, x[i].y, y[i].y);
        acc = op_step<OP>(acc, a[i].z, b[i].z, x[i].z, y[i].z);
        acc = op_step<OP>(acc, a[i].w, b[i].w, x[i].w, y[i].w);
      } else {
        acc = op_step<OP>(acc, a[i].x, 0.0f, x[i].x, 0.0f);
        acc = op_step<OP>(acc, a[i].y, 0.0f, x[i].y, 0.0f);
        acc = op_step<OP>(acc, a[i].z, 0.0f, x[i].z, 0.0f);
        acc = op_step<OP>(acc, a[i].w, 0.0f, x[i].w, 0.0f);
      }
    }
  }
  for (; k0 < kend; k0 += 4) {  // kp % 8 == 0, so whole float4s remain
    const float4 a = *reinterpret_cast<const float4*>(qv + k0);
    const float4 x = *reinterpret_cast<const float4*>(ev + k0);
    if constexpr (OP == 2) {
      const float4 b = *reinterpret_cast<const float4*>(qv + kp + k0);
      const float4 y = *reinterpret_cast<const float4*>(ev + kp + k0);
      acc = op_step<OP>(acc, a.x, b.x, x.x, y.x);
      acc = op_step<OP>(acc, a.y, b.y, x.y, y.y);
      acc = op_step<OP>(acc, a.z, b.z, x.z, y.z);
      acc = op_step<OP>(acc, a.w, b.w, x.w, y.w);
    } else {
      acc = op_step<OP>(acc, a.x, 0.0f, x.x, 0.0f);
      acc = op_step<OP>(acc, a.y, 0.0f, x.y, 0.0f);
      acc = op_step<OP>(acc, a.z, 0.0f, x.z, 0.0f);
      acc = op_step<OP>(acc, a.w, 0.0f, x.w, 0.0f);
    }
  }
  return op_final<OP>(acc);
}

template <int OP>
__global__ __launch_bounds__(256) void k_filter_scores(const float* __restrict__ ent_rows, int64_t n_ent,
                                                       const float* __restrict__ q_rows, int kp,
                                                       const int32_t* __restrict__ qtrue, int64_t n_query,
                                                       int pred_kind, float margin, const int32_t* __restrict__ entry_q,
                                                       const int32_t* __restrict__ ids, int64_t n_entries,
                                                       float* __restrict__ thr, float* __restrict__ list_v) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_query + n_entries) return;
  const int64_t kt = (int64_t)((OP == 2 || OP == 4) ? 2 : 1) * kp;
  if (t < n_query) {
    thr[t] = apply_pred(pred_kind, margin, row_score<OP>(q_rows + t * kt, ent_rows + (int64_t)qtrue[t] * kt, kp));
    return;
  }
  const int64_t p = t - n_query;
  const int64_t j = ids[p];
  const int64_t vq = entry_q[p];
  if (j < 0 || j >= n_ent || vq < 0 || vq >= n_query) {
    list_v[p] = __builtin_nanf("");  // never < a threshold: an invalid id is not counted
    return;
  }
  list_v[p] = apply_pred(pred_kind, margin, row_score<OP>(q_rows + vq * kt, ent_rows + j * kt, kp));
}

// Phase 2, k_filter_count: one wave per filter group (queries sharing (mode, r, anchor),
// see mmre_link_truth_grouped); the group's listed scores are staged in LDS 64 at a time and
// every member query (one per lane) counts those that beat its own truth:
//   counts[.][q] = {0, -c, 0, -cc}, c = #{listed j != true(q) : pred(j) < thr[q]} (Test.h:85)
__global__ __launch_bounds__(64) void k_filter_count(const int64_t* __restrict__ grp_qoff,
                                                     const int32_t* __restrict__ grp_q, int64_t n_groups,
                                                     const int64_t* __restrict__ off, const int32_t* __restrict__ ids,
                                                     const float* __restrict__ list_v,
                                                     const int32_t* __restrict__ qtrue, const float* __restrict__ thr,
                                                     const int64_t* __restrict__ qr, const int8_t* __restrict__ qmode,
                                                     int64_t n_query, int64_t n_ent,
                                                     const uint32_t* __restrict__ type_head,
                                                     const uint32_t* __restrict__ type_tail, int64_t type_words,
                                                     int32_t* __restrict__ counts) {
  // staged list: id (-1 = invalid), score, type bit; read back 4 entries per LDS access
  __shared__ __attribute__((aligned(16))) int32_t s_id[64];
  __shared__ __attribute__((aligned(16))) float s_v[64];
  __shared__ __attribute__((aligned(16))) int32_t s_tb[64];
  const int tid = threadIdx.x;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t qa = grp_qoff[g], qb = grp_qoff[g + 1];
    const int64_t la = off[g], lb = off[g + 1];
    const int64_t q0 = grp_q[qa];
    const uint32_t* tm = type_head ? (qmode[q0] == MMRE_HEAD_BATCH ? type_head : type_tail) : nullptr;
    const int64_t r = qr[q0];
    for (int64_t qc = qa; qc < qb; qc += 64) {
      const int64_t qi = qc + tid;
      const bool active = qi < qb;
      const int64_t q = active ? grp_q[qi] : 0;
      const int32_t tr = active ? qtrue[q] : -1;
      const float th = active ? thr[q] : 0.0f;
      int c = 0, cc = 0;
      for (int64_t lc = la; lc < lb; lc += 64) {
        const int nl = (int)((lb - lc) < 64 ? (lb - lc) : 64);
        __syncthreads();  // s_* reuse
        {
          int32_t id = -1, tb = 0;
          float v = 0.0f;
          if (tid < nl) {
            const int64_t j = ids[lc + tid];
            if (j >= 0 && j < n_ent) {
              id = (int32_t)j;
              v = list_v[lc + tid];
              tb = tm ? (int32_t)type_bit(tm, type_words, r, j) : 0;
            }
          }
          s_id[tid] = id;  // entries nl..63 stay invalid: the loop below reads whole quads
          s_v[tid] = v;
          s_tb[tid] = tb;
        }
        __syncthreads();
        if (active) {
          for (int i = 0; i < nl; i += 4) {  // branch-free, 4 entries per LDS read
            const int4 e = *reinterpret_cast<const int4*>(&s_id[i]);
            const float4 v = *reinterpret_cast<const float4*>(&s_v[i]);
            const int4 t = *reinterpret_cast<const int4*>(&s_tb[i]);
            const int b0 = (e.x >= 0) & (e.x != tr) & (v.x < th);
            const int b1 = (e.y >= 0) & (e.y != tr) & (v.y < th);
            const int b2 = (e.z >= 0) & (e.z != tr) & (v.z < th);
            const int b3 = (e.w >= 0) & (e.w != tr) & (v.w < th);
            c += b0 + b1 + b2 + b3;
            cc += (b0 & t.x) + (b1 & t.y) + (b2 & t.z) + (b3 & t.w);
          }
        }
      }
      if (active) {
        counts[0 * n_query + q] = 0;
        counts[1 * n_query + q] = -c;
        counts[2 * n_query + q] = 0;
        counts[3 * n_query + q] = -cc;
      }
    }
  }
}

// Work units for a persistent grid whose P workgroups per XCD group run in lock-step windows
// (k_sweep_bf3, round 5): the group owns the contiguous entity tiles [e_lo, e_hi); a window is
// QB query tiles x EB entity tiles (QB x EB <= P), member m of the group always takes window
// position (m / EB, m % EB); windows advance along the entity tiles first, then to the next QB
// query tiles. The P concurrent units of a group therefore share QB query tiles (resident in the
// XCD's L2 for the whole entity pass) and EB entity tiles (each fetched once per window from
// HBM / MALL), instead of ~P different tiles of each operand (the contiguous ranges of UnitMap:
// at C5 every unit re-streamed both 128-KB operand tiles, 120 GB per launch). A member's unit i:
// query-block i / n_e, entity-block i % n_e (n_e = its entity windows): consecutive units of a
// workgroup keep their query tile, so counts flush once per query block.
struct BlockMap {
  int count, qin, ein, QB, EB, e_lo, n_e;
  __device__ __forceinline__ BlockMap(int grp, int n_groups, int member, int P, int n_qt, int n_et, int qb, int eb) {
    e_lo = (int)((int64_t)n_et * grp / n_groups);
    const int e_hi = (int)((int64_t)n_et * (grp + 1) / n_groups);
    const int m_e = e_hi - e_lo;
    QB = qb;
    EB = eb;
    qin = member / EB;
    ein = member - qin * EB;
    count = 0;
    n_e = 0;
    if (qin >= QB || m_e <= 0) return;
    n_e = ein < m_e ? (m_e - ein + EB - 1) / EB : 0;                  // entity windows holding its column
    const int n_q = qin < n_qt ? (n_qt - qin + QB - 1) / QB : 0;     // query windows holding its row
    count = n_q * n_e;
  }
  __device__ __forceinline__ void at(int i, int& qt, int& et) const {
    const int a = i / n_e, b = i - a * n_e;
    qt = a * QB + qin;
    et = e_lo + b * EB + ein;
  }
};

// filtered columns += raw columns (after the sweep): counts[1] = counts[0] + (minus the listed
// entities that beat the truth, written by the truth pass), likewise counts[3] from counts[2]
__global__ __launch_bounds__(256) void k_counts_finalize(int32_t* __restrict__ counts, int64_t n_query, int tc) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_query) return;
  counts[n_query + q] += counts[q];
  if (tc) counts[3 * n_query + q] += counts[2 * n_query + q];
}

// ---------------------------------------------------------- routed rows ---
// The per-query route's exact kernel: queries route_list[0 .. *route_n) against
// every entity of the slice, the canonical chain per pair (op_step<0>, k ascending over the kp
// rows from 0.0f), the sweep epilogue's three conditions, raw counts by integer atomics. The
// routed queries are few (C2: 122), so the 128 x 128 unit of the sweep left most of the machine
// idle and cost by the row tile; here a unit is HR_QB routed queries x HR_TE entity columns:
// a thread owns one column (the k-major loads coalesce along the entity axis) and HR_QB chains,
// so a loaded entity value feeds HR_QB chains. The query operand comes from the row-major
// q_rows through wave-uniform ids: scalar loads, no LDS stage. The host sizes the grid from the
// list's cap; the units come from the device's count, a workgroup without one leaves, and an
// inert route (count 0) changes nothing.
constexpr int HR_TE = 128;  // entity columns per unit (= TE: e_cols is whole units)
constexpr int HR_QB = 16;   // routed queries per unit
constexpr int HR_KU = 8;    // k rows per stage (= KC: kp is whole stages), the next stage's loads in flight
static_assert(HR_TE == TE && HR_KU == KC && HR_TE % 64 == 0 && HR_QB <= HR_TE, "routed rows' unit");
__global__ __launch_bounds__(HR_TE) void k_heavy_rows(
    const float* __restrict__ ent_km, int64_t e_pad, int64_t n_ent, int n_et, int e_base,
    const float* __restrict__ q_rows, int kp, const float* __restrict__ thr, const int32_t* __restrict__ qtrue,
    const int32_t* __restrict__ route_list, const uint32_t* __restrict__ route_n, int32_t* __restrict__ counts) {
  __shared__ int s_cnt[HR_TE / 64][HR_QB];
  const int tid = threadIdx.x;
  const int n_idx = __builtin_amdgcn_readfirstlane((int)*route_n);
  const int n_qb = (n_idx + HR_QB - 1) / HR_QB;
  const int64_t units = (int64_t)n_qb * n_et;
  // entity-tile major: neighbouring workgroups read the same columns
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int et = (int)(unit / n_qb), p0 = (int)(unit % n_qb) * HR_QB;
    // the unit's queries (uniform); a slot past the list repeats the unit's first query and
    // never counts (threshold -inf)
    const float* qp[HR_QB];
    float th[HR_QB];
    int32_t tr[HR_QB];
#pragma unroll
    for (int i = 0; i < HR_QB; ++i) {
      const bool v = p0 + i < n_idx;
      const int q = __builtin_amdgcn_readfirstlane(route_list[v ? p0 + i : p0]);
      qp[i] = q_rows + (int64_t)q * kp;
      th[i] = v ? thr[q] : -INFINITY;
      tr[i] = qtrue[q];
    }
    const int e = et * HR_TE + tid;
    const float* ep = ent_km + e;
    float acc[HR_QB];
#pragma unroll
    for (int i = 0; i < HR_QB; ++i) acc[i] = 0.0f;
    float ev[HR_KU], en[HR_KU];
#pragma unroll
    for (int u = 0; u < HR_KU; ++u) ev[u] = en[u] = ep[(int64_t)u * e_pad];
    for (int k0 = 0; k0 < kp; k0 += HR_KU) {
      if (k0 + HR_KU < kp) {
#pragma unroll
        for (int u = 0; u < HR_KU; ++u) en[u] = ep[(int64_t)(k0 + HR_KU + u) * e_pad];
      }
#pragma unroll
      for (int u = 0; u < HR_KU; ++u)
#pragma unroll
        for (int i = 0; i < HR_QB; ++i) acc[i] = op_step<0>(acc[i], qp[i][k0 + u], 0.0f, ev[u], 0.0f);
#pragma unroll
      for (int u = 0; u < HR_KU; ++u) ev[u] = en[u];
    }
    // the sweep epilogue's conditions; a wave's count per query is one ballot
#pragma unroll
    for (int i = 0; i < HR_QB; ++i) {
      const bool better = (op_final<0>(acc[i]) < th[i]) & (e + e_base != tr[i]) & (e < n_ent);
      const int c = __popcll(__ballot(better));
      if ((tid & 63) == 0) s_cnt[tid >> 6][i] = c;
    }
    __syncthreads();
    if (tid < HR_QB && p0 + tid < n_idx) {  // one add per (workgroup, query), raw column only
      int c = 0;
#pragma unroll
      for (int w = 0; w < HR_TE / 64; ++w) c += s_cnt[w][tid];
      if (c) atomicAdd(&counts[route_list[p0 + tid]], c);
    }
    __syncthreads();  // the next unit's ballots overwrite s_cnt
  }
}

// ------------------------------------------------------------ MFMA sweep ---
// DistMult / ComplEx: S = Q (queries x K) . E^T (K x entities) with the f32-input MFMA
// v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fma chain: the canonical order).
// Work units and the XCD-grouped split are the VALU sweep's (UnitMap): (query tile of 128) x
// (entity tile of 128). 4 waves as 2 (q) x 2 (e); each wave 64 x 64 = 2 x 2 blocks of 32 x 32
// accumulators. K goes through double-buffered LDS stages of KS rows, register-staged, the
// next stage's global loads issued at the top of the current one (scripts/probes/
// mfma_stage.hip: this beats LDS-DMA rings and a single 256 x 128 workgroup). The plain
// sweep runs KS = 16 at four 256-thread workgroups per CU (33 KB LDS, 112 VGPRs); the type-
// constrained / score-storing variants KS = 32 at two. Epilogue: each lane holds 32 query rows
// x 1 entity column of the 64 x 64 block and reads the rows' thresholds from LDS (b128 reads,
// once per unit). KS = 16: each row's 64 compares are counted by two ballots into a counter
// held by the lane of that row (one register for the wave's 64 rows); KS = 32: per-lane
// register counters for its 32 rows, reduced across the 32 column lanes. Either way the
// counts reach HBM only when the workgroup leaves the query tile. The truth needs no exclusion
// test: its score is bit-identical to the threshold (same canonical chain), so `< thr`
// rejects it.
typedef float floatx16 __attribute__((ext_vector_type(16)));

template <bool TC, bool STORE, int PK, int KS>
__global__ __launch_bounds__(NT, KS == 16 && !TC && !STORE ? 4 : 2) void k_sweep_mfma(
    const float* __restrict__ ent_km, int64_t e_pad, int64_t n_ent, const float* __restrict__ q_km,
    int64_t q_pad, int64_t n_query, int ktot, int n_et, int e_base, int n_groups, int pred_kind, float margin,
    const float* __restrict__ thr, const int64_t* __restrict__ qr, const int8_t* __restrict__ qmode,
    const uint32_t* __restrict__ type_head, const uint32_t* __restrict__ type_tail, int64_t type_words,
    int32_t* __restrict__ counts, float* __restrict__ scores, int emajor, const uint32_t* __restrict__ gate) {
  static_assert(KS == 16 || KS == 32, "stage of 16 or 32 K rows");
  if (gate != nullptr && *gate == 0u) return;  // the split-bf16 filter's fallback: runs only on its overflow
  // 16-row stages (33 KB of LDS) run 4 workgroups per CU: the row counters then live one row
  // per lane (ballot counts), which frees the 32 registers of per-lane row counters
  constexpr bool BAL = KS == 16;
  __shared__ float sq[2][KS][TQ];
  __shared__ float se[2][KS][TE];
  __shared__ int32_t s_rel[TC ? TQ : 1];
  __shared__ int8_t s_mode[TC ? TQ : 1];
  __shared__ __attribute__((aligned(16))) float s_th[2][TQ];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const PredSel<PK> pred(pred_kind, margin);
  const int wq = wave >> 1, we = wave & 1;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  const UnitMap um(grp, n_groups, (int)(q_pad / TQ), n_et, emajor != 0);
  const int u0 = (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = (int)((int64_t)(gmem + 1) * um.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  // stages of KS rows; with KS = 32 and K = 32 n + 16 (plane_rows: K is a multiple of 16) the
  // unit's last stage holds 16 rows (a uniform branch skips its upper half)
  const int nkc = (ktot + KS - 1) / KS;
  const bool half_tail = KS == 32 && (ktot % 32) != 0;

  // rows of this lane: ql(bi, r) = wq*64 + bi*32 + (r&3) + 8*(r>>2) + 4*lrow
  int tpar = 0;  // s_th slot of the current query tile
  // per-row counters of the current query tile. BAL: one row per lane, lane L holds wave row L
  // (tile row wq * 64 + L), each row's 64 compares counted by two ballots; else each lane
  // counts its own column of its 32 rows, reduced over the 32 column lanes at the flush
  int cntv = 0, cntv_tc = 0;
  int cnt[BAL ? 1 : 2][BAL ? 1 : 16], cnt_tc[TC && !BAL ? 2 : 1][TC && !BAL ? 16 : 1];
  auto row_of = [&](int bi, int r) { return wq * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow; };
  auto load_rows = [&](int qtile) {
    const int64_t q0 = (int64_t)qtile * TQ;
    // thresholds into the other s_th slot: visible after the stage's closing barrier, and the
    // slot's previous tile was left at least one stage ago
    tpar ^= 1;
    if (tid < TQ) {
      const int64_t q = q0 + tid;
      s_th[tpar][tid] = q < n_query ? thr[q] : -INFINITY;  // -inf: nothing beats a padded row
    }
    cntv = 0;
    cntv_tc = 0;
    if constexpr (!BAL) {
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          cnt[bi][r] = 0;
          if constexpr (TC) cnt_tc[bi][r] = 0;
        }
    }
    if constexpr (TC) {
      __syncthreads();  // previous tile's s_rel/s_mode readers are done
      if (tid < TQ) {
        const int64_t q = q0 + tid;
        s_rel[tid] = q < n_query ? (int32_t)qr[q] : 0;
        s_mode[tid] = q < n_query ? qmode[q] : 0;
      }
    }
  };
  auto flush_rows = [&](int qtile) {
    if constexpr (BAL) {  // each lane its row's count (both column waves add)
      const int64_t q = (int64_t)qtile * TQ + wq * 64 + lane;
      if (q < n_query) {
        if (cntv) atomicAdd(&counts[q], cntv);  // raw only (k_counts_finalize)
        if constexpr (TC) {
          if (cntv_tc) atomicAdd(&counts[2 * n_query + q], cntv_tc);
        }
      }
    } else {
      const int64_t q0 = (int64_t)qtile * TQ;
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int c = cnt[bi][r];
#pragma unroll
          for (int sh = 1; sh < 32; sh <<= 1) c += __shfl_xor(c, sh);  // the 32 column lanes
          int cc = 0;
          if constexpr (TC) {
            cc = cnt_tc[bi][r];
#pragma unroll
            for (int sh = 1; sh < 32; sh <<= 1) cc += __shfl_xor(cc, sh);
          }
          const int64_t q = q0 + row_of(bi, r);
          if (lcol == 0 && q < n_query) {
            if (c) atomicAdd(&counts[q], c);  // raw only (k_counts_finalize)
            if constexpr (TC) {
              if (cc) atomicAdd(&counts[2 * n_query + q], cc);
            }
          }
        }
    }
  };

  const int srow = tid >> 5, sc4 = tid & 31;  // rows srow + 8 i of the stage
  float4 rq0, rq1, re0, re1, rq2, rq3, re2, re3;  // named scalars, not an array: kept in VGPRs
  int ld_unit = u0, ld_kc = 0, ld_qt, ld_et;
  um.at(u0, ld_qt, ld_et);
  auto gload = [&]() {
    const int k = ld_kc * KS + srow;
    const float* qp = q_km + (int64_t)k * q_pad + (int64_t)ld_qt * TQ + sc4 * 4;
    const float* ep = ent_km + (int64_t)k * e_pad + (int64_t)ld_et * TE + sc4 * 4;
    rq0 = *reinterpret_cast<const float4*>(qp);
    rq1 = *reinterpret_cast<const float4*>(qp + 8 * q_pad);
    re0 = *reinterpret_cast<const float4*>(ep);
    re1 = *reinterpret_cast<const float4*>(ep + 8 * e_pad);
    if (KS == 32 && !(half_tail && ld_kc == nkc - 1)) {  // rows past K are never read
      rq2 = *reinterpret_cast<const float4*>(qp + 16 * q_pad);
      rq3 = *reinterpret_cast<const float4*>(qp + 24 * q_pad);
      re2 = *reinterpret_cast<const float4*>(ep + 16 * e_pad);
      re3 = *reinterpret_cast<const float4*>(ep + 24 * e_pad);
    }
    if (++ld_kc == nkc) {
      ld_kc = 0;
      if (++ld_unit < u1) um.at(ld_unit, ld_qt, ld_et);
    }
  };
  auto swrite = [&](int buf) {
    *reinterpret_cast<float4*>(&sq[buf][srow][sc4 * 4]) = rq0;
    *reinterpret_cast<float4*>(&sq[buf][srow + 8][sc4 * 4]) = rq1;
    *reinterpret_cast<float4*>(&se[buf][srow][sc4 * 4]) = re0;
    *reinterpret_cast<float4*>(&se[buf][srow + 8][sc4 * 4]) = re1;
    if constexpr (KS == 32) {
      *reinterpret_cast<float4*>(&sq[buf][srow + 16][sc4 * 4]) = rq2;
      *reinterpret_cast<float4*>(&sq[buf][srow + 24][sc4 * 4]) = rq3;
      *reinterpret_cast<float4*>(&se[buf][srow + 16][sc4 * 4]) = re2;
      *reinterpret_cast<float4*>(&se[buf][srow + 24][sc4 * 4]) = re3;
    }
  };

  floatx16 acc[2][2];
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

  int buf = 0;
  for (int unit = u0; unit < u1; ++unit) {
    for (int kc = 0; kc < nkc; ++kc) {
      const bool more = ld_unit < u1;
      if (more) gload();
      // the next stage's loads stay at the top of this one: hipcc otherwise sinks them to
      // their use at the stage's end and every stage waits a full L2 / MALL latency
      __builtin_amdgcn_sched_barrier(0);
      auto mfma_rows = [&](int k0) {  // 16 K rows = 8 k pairs from stage row k0
#pragma unroll
        for (int kp2 = 0; kp2 < 16; kp2 += 2) {
          const float a0 = sq[buf][k0 + kp2 + lrow][wq * 64 + lcol];
          const float a1 = sq[buf][k0 + kp2 + lrow][wq * 64 + 32 + lcol];
          const float b0 = se[buf][k0 + kp2 + lrow][we * 64 + lcol];
          const float b1 = se[buf][k0 + kp2 + lrow][we * 64 + 32 + lcol];
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
      };
      mfma_rows(0);
      if (KS == 32 && !(half_tail && kc == nkc - 1)) mfma_rows(16);
      if (kc == nkc - 1) {  // unit finished: rank epilogue
        const int64_t q0 = (int64_t)cur_qt * TQ;
        const int64_t ebase = (int64_t)cur_et * TE + we * 64;
        const int64_t e0 = ebase + lcol, e1 = ebase + 32 + lcol;
        const bool ev0 = e0 < n_ent, ev1 = e1 < n_ent;
        if constexpr (BAL) {
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
                const int ql = row_of(bi, r);
                const uint32_t* tm = s_mode[ql] == MMRE_HEAD_BATCH ? type_head : type_tail;
                const uint64_t t0 = __ballot(b0 && type_bit(tm, type_words, s_rel[ql], e0 + e_base));
                const uint64_t t1 = __ballot(b1 && type_bit(tm, type_words, s_rel[ql], e1 + e_base));
                cntv_tc += lane == L0 ? __popcll(t0 & 0xffffffffull) + __popcll(t1 & 0xffffffffull)
                                      : (lane == L0 + 4 ? __popcll(t0 >> 32) + __popcll(t1 >> 32) : 0);
              }
              if constexpr (STORE) {
                const int64_t q = q0 + row_of(bi, r);
                if (q < n_query) {
                  if (ev0) scores[q * n_ent + e0] = v0;
                  if (ev1) scores[q * n_ent + e1] = v1;
                }
              }
            }
          }
        } else {
          // the lane's 32 row thresholds, 8 LDS reads issued together (a read per compare
          // serialised 64 LDS latencies per unit); rows row_of(bi, 4i) .. + 3 are contiguous
          float tv[2][16];
#pragma unroll
          for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int r4 = 0; r4 < 16; r4 += 4) {
              const float4 t4 = *reinterpret_cast<const float4*>(&s_th[tpar][row_of(bi, r4)]);
              tv[bi][r4] = t4.x;
              tv[bi][r4 + 1] = t4.y;
              tv[bi][r4 + 2] = t4.z;
              tv[bi][r4 + 3] = t4.w;
            }
#pragma unroll
          for (int bj = 0; bj < 2; ++bj) {
            const int64_t e = bj ? e1 : e0;
            if (bj ? ev1 : ev0) {  // one exec mask per column block (lanes diverge in the last tile only)
#pragma unroll
              for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                  const float v = pred(acc[bi][bj][r]);
                  const bool better = v < tv[bi][r];
                  cnt[bi][r] += better;
                  if constexpr (TC) {
                    const int ql = row_of(bi, r);
                    const uint32_t* tm = s_mode[ql] == MMRE_HEAD_BATCH ? type_head : type_tail;
                    cnt_tc[bi][r] += better && type_bit(tm, type_words, s_rel[ql], e + e_base);
                  }
                  if constexpr (STORE) {
                    const int64_t q = q0 + row_of(bi, r);
                    if (q < n_query) scores[q * n_ent + e] = v;
                  }
                }
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

// ------------------------------------------------------ L1 integer filter ---
// M = max |x| over the query plane and the entity slice (non-finite values make M = inf),
// as float bits in hdr[0] (zeroed by the launch sequence just before), and per block the sum
// of |x| (finite x) into the partials at byte L1Q_PART -- the fallback test's mean |x|.
__global__ __launch_bounds__(256) void k_l1q_absmax(const float* __restrict__ q_km, int64_t q_pad,
                                                    const float* __restrict__ e_km, int64_t e_pad, int64_t e_cols,
                                                    int kp, uint32_t* __restrict__ work) {
  // work items (plane row r, column chunk y of 8) of both planes, strided over the blocks (no
  // index division per element); one atomic per block at most (same-address atomics serialize)
  float m = 0.0f, sa = 0.0f;
  for (int it = blockIdx.x; it < kp * 8; it += gridDim.x) {
    const int r = it >> 3;
    const int64_t st = 8 * (int64_t)blockDim.x, c0 = (int64_t)(it & 7) * blockDim.x + threadIdx.x;
    const float4* q4 = reinterpret_cast<const float4*>(q_km + (int64_t)r * q_pad);
#pragma unroll 4
    for (int64_t c = c0; c < q_pad / 4; c += st) {
      const float4 v = q4[c];
      const float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
      m = fmaxf(m, a);
      if (!(v.x - v.x == 0.0f && v.y - v.y == 0.0f && v.z - v.z == 0.0f && v.w - v.w == 0.0f)) m = INFINITY;
      else sa += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
    const float4* e4 = reinterpret_cast<const float4*>(e_km + (int64_t)r * e_pad);
#pragma unroll 4
    for (int64_t c = c0; c < e_cols / 4; c += st) {
      const float4 v = e4[c];
      const float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
      m = fmaxf(m, a);
      if (!(v.x - v.x == 0.0f && v.y - v.y == 0.0f && v.z - v.z == 0.0f && v.w - v.w == 0.0f)) m = INFINITY;
      else sa += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
    sa += __shfl_xor(sa, o);
  }
  __shared__ float s_m[4], s_s[4];
  if ((threadIdx.x & 63) == 0) {
    s_m[threadIdx.x >> 6] = m;
    s_s[threadIdx.x >> 6] = sa;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    reinterpret_cast<float*>(reinterpret_cast<char*>(work) + L1Q_PART)[blockIdx.x] = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
    // non-negative floats order as their bits; inf = no filter. Skip the atomic when the word
    // already holds at least m (a stale read only costs a redundant atomic).
    if (__float_as_uint(m) > __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(work, __float_as_uint(m));
  }
}

// The fallback test (every block of k_l1q_quant evaluates it identically; block 0 writes it):
// the code step is 2M / 65535 and a pair stays undecided when its score lies within ~1.03 K
// steps of its threshold, so the filter pays off while M is a modest multiple of the typical
// magnitude. M > ratio x mean|x| (one outlier value stretching the code range: every other value
// then lands in a few codes and most pairs would be rescored one at a time) or M non-finite
// -> the sweep runs the f32 path instead (same counts either way).
__device__ __forceinline__ bool l1q_fallback(const uint32_t* __restrict__ work, int n_part, double n_elem,
                                             float ratio) {
  __shared__ float s_p[4];
  const float* part = reinterpret_cast<const float*>(reinterpret_cast<const char*>(work) + L1Q_PART);
  float v = 0.0f;
  for (int i = threadIdx.x; i < n_part; i += blockDim.x) v += part[i];  // fixed order per thread
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = v;
  __syncthreads();
  const float sum = (s_p[0] + s_p[1]) + (s_p[2] + s_p[3]);
  const float mx = __uint_as_float(work[0]);
  if (!(mx < INFINITY)) return true;
  return (double)mx > (double)ratio * ((double)sum / n_elem);
}

// Codes of columns [c0, c0 + n) of a k-major float plane (kp rows, stride pad) into dword rows
// r < kw, Q(x) = rint((x + M) (2^BITS - 1) / 2M): BITS 16 packs Q(x[2r]) | Q(x[2r + 1]) << 16,
// BITS 8 the four codes Q(x[4r + h]) << 8h (k >= kp: code 0 in both planes).
// mode 0 (the first codes made): the fallback test decides between these codes and the f32
// sweep and writes the code-width word. mode 1 (the 16-bit codes after k_l1q_probe): made only
// while the f32 fallback is off and the probe counted more than probe_max undecided pairs; the
// first block writes L1Q_CODES16 (the other blocks read the word before or after that store
// and reach the same decision either way).
// Both planes in one launch: blockIdx.y 0 = the query plane, 1 = the entity slice.
struct L1QPlane {
  const float* km;  // k-major float plane, row stride pad
  int64_t pad, c0, n;  // columns [c0, c0 + n)
  uint32_t* out;    // code rows, row stride pad
};
template <int BITS>
__global__ __launch_bounds__(256) void k_l1q_quant(L1QPlane pq, L1QPlane pe, int kp, int kw,
                                                   uint32_t* __restrict__ work, int n_part, double n_elem,
                                                   float ratio, int mode, uint32_t probe_max) {
  const float* __restrict__ km = blockIdx.y ? pe.km : pq.km;
  const int64_t pad = blockIdx.y ? pe.pad : pq.pad, c0 = blockIdx.y ? pe.c0 : pq.c0, n = blockIdx.y ? pe.n : pq.n;
  uint32_t* __restrict__ out = blockIdx.y ? pe.out : pq.out;
  if (mode == 1) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(work[1]);
    if (w == L1Q_F32) return;
    if (w != L1Q_CODES16 && __builtin_amdgcn_readfirstlane(work[2]) <= probe_max) return;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) work[1] = L1Q_CODES16;
  } else {
    const bool fb = l1q_fallback(work, n_part, n_elem, ratio);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) work[1] = fb ? L1Q_F32 : (BITS == 8 ? L1Q_CODES8 : L1Q_CODES16);
    if (fb) return;
  }
  constexpr int PER = 32 / BITS;
  constexpr float LEVELS = BITS == 8 ? 255.0f : 65535.0f;
  const float mx = __uint_as_float(*work);
  const float inv = (mx > 0.0f && mx < INFINITY) ? LEVELS / (2.0f * mx) : 0.0f;
  const float off = (mx < INFINITY) ? mx : 0.0f;
  const int64_t total = (int64_t)kw * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int r = (int)(i / n);
    const int64_t c = c0 + i % n;
    uint32_t word = 0u;
#pragma unroll
    for (int h = 0; h < PER; ++h) {
      const int k = PER * r + h;
      float t = k < kp ? (km[(int64_t)k * pad + c] + off) * inv : 0.0f;
      t = t == t ? fminf(fmaxf(t, 0.0f), LEVELS) : 0.0f;
      word |= (uint32_t)rintf(t) << (BITS * h);
    }
    out[(int64_t)r * pad + c] = word;
  }
}

// The 8-bit codes (mode 0: the fallback test first, then the code-width word = 8-bit), written
// word row by word row like k_l1q_quant, plus one more row after the k values' words: with
// TIGHT (prediction = the score, no type masks, kt <= 1984) each column's quantization error
// sum E = sum_k |x_k - (delta code_k - M)| is reduced in the workgroup (32 columns x 8 row
// groups); a query row stores its bound 1.01 E + kt 2^-20 M (float rounding of the map and the
// sum) for the thresholds (q_l1c), an entity column stores o = ceil(bound / (delta (1 - l1f)))
// as four bytes summing to o in that row, so the sweep's own v_sad_u8 adds o to every pair's sum
// (the query's row is 0), and hdr[3] gets the slice's largest o. The pair's bound is then the
// two rows' error sums -- about K delta / 2 -- instead of 1.03 K delta.
template <bool TIGHT>
__global__ __launch_bounds__(256) void k_l1q_quant8(L1QPlane pq, L1QPlane pe, int kp, int kw, int kt,
                                                    uint32_t* __restrict__ work, int n_part, double n_elem,
                                                    float ratio, float* __restrict__ q_l1c) {
  const bool fb = l1q_fallback(work, n_part, n_elem, ratio);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) work[1] = fb ? L1Q_F32 : L1Q_CODES8;
  if (fb) return;
  const bool ent = blockIdx.y != 0;
  const float* __restrict__ km = ent ? pe.km : pq.km;
  const int64_t pad = ent ? pe.pad : pq.pad, c0 = ent ? pe.c0 : pq.c0, n = ent ? pe.n : pq.n;
  uint32_t* __restrict__ out = ent ? pe.out : pq.out;
  const float mx = __uint_as_float(*work);
  const float inv = (mx > 0.0f && mx < INFINITY) ? 255.0f / (2.0f * mx) : 0.0f;
  const float off = (mx < INFINITY) ? mx : 0.0f;
  const float delta = (mx > 0.0f && mx < INFINITY) ? (2.0f * mx) / 255.0f : 0.0f;  // l1q_delta's
  const float l1f = (float)(kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
  const int words = (kt + 3) >> 2;  // row `words`: the error offsets
  const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
  __shared__ float s_err[8][32];
  for (int64_t cb = (int64_t)blockIdx.x * 32; cb < n; cb += (int64_t)gridDim.x * 32) {  // uniform
    const bool live = cb + cl < n;
    const int64_t c = c0 + cb + cl;
    float err = 0.0f;
#pragma unroll 4
    for (int r = g; r < kw; r += 8) {  // 4 word rows' loads in flight per thread
      uint32_t word = 0u;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int k = 4 * r + h;
        if (live && k < kp) {
          const float x = km[(int64_t)k * pad + c];
          float t = (x + off) * inv;
          t = t == t ? fminf(fmaxf(t, 0.0f), 255.0f) : 0.0f;
          const float code = rintf(t);
          word |= (uint32_t)code << (8 * h);
          if constexpr (TIGHT) err += fabsf(x - (code * delta - off));
        }
      }
      if (live && !(TIGHT && r == words)) out[(int64_t)r * pad + c] = word;
    }
    if constexpr (TIGHT) {
      s_err[g][cl] = err;
      __syncthreads();
      if (g == 0 && live) {
        float e = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) e += s_err[i][cl];
        const float eb = __builtin_fmaf(e, 1.01f, (float)kt * 0x1p-20f * mx);
        uint32_t wv = 0u;
        if (!ent) {
          q_l1c[c] = eb;
        } else {
          // o <= 1020 (four bytes of 255) without the clamp ever acting: each element's code error
          // is at most delta / 2 (rounding to nearest; |x| <= M, so no value is clipped) plus the
          // float rounding of the map, so E <= kt delta / 2 (1 + 2^-20) and o <= 1.01 kt / 2 (1 +
          // 2^-16) + kt 2^-20 M / delta + 1 <= 0.506 kt + 1 = 1,005 at the host guard kt <= 1,984
          // (tests/test_sweep_filters_gpu.py::test_l1_tight_offsets_at_kt_1984 reads the largest o)
          uint32_t o = delta > 0.0f ? (uint32_t)ceilf(fminf(eb / (delta * (1.0f - l1f)) * (1.0f + 0x1p-17f), 1020.0f))
                                    : 0u;
          if (o) atomicMax(work + 3, o);
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const uint32_t b = o < 255u ? o : 255u;
            wv |= b << (8 * h);
            o -= b;
          }
        }
        out[(int64_t)words * pad + c] = wv;
      }
      __syncthreads();
    }
  }
}

// The code-width probe (runs when the 8-bit codes were made): L1Q_PROBE_Q workgroups, each one
// query column (evenly spaced over the queries) against L1Q_PROBE_E consecutive entity columns
// of the slice (the start spread over the slice), scored with the 8-bit codes; the pairs inside
// their query's undecided band (the epilogue's test in its float form) are counted into hdr[2].
// 512 queries x 256 entities: the undecided pairs concentrate on a few queries (C2: a sample of
// 64 queries read 0.19 % where the whole evaluation has 0.38 %), so many queries, short windows.
// The threshold: where the 8-bit sweep's rescoring stops paying. Spread over every query tile
// (C2 at N = 1, 0.38 %) the rescoring overlaps the other waves' sums and 8-bit wins (1.32 vs
// 1.62 ms); concentrated in a rank's share of a few relations it does not: 8-way C2 shares at
// 0.77 % / 1.18 % took 0.32 / 0.51 ms against 0.26 ms with 16-bit codes (profiles/r4).
constexpr int L1Q_PROBE_Q = 512, L1Q_PROBE_E = 256;
constexpr double L1Q_PROBE_FRAC = 0.006;  // undecided fraction of the sample above which 16-bit codes
// The probe's switch point in undecided pairs for a sample of n_slice entity columns -- ONE helper
// for both entry points (mmre_link_sweep_l1q and the fused mmre_link_evaluate_l1q), so that
// MMRE_L1_PROBE_FRAC (experiments) moves both alike and their code widths / stats agree.
static uint32_t l1q_probe_max(int64_t n_slice) {
  static const char* pf_env = getenv("MMRE_L1_PROBE_FRAC");
  const double pfrac = pf_env ? atof(pf_env) : L1Q_PROBE_FRAC;
  const int64_t sample = (int64_t)L1Q_PROBE_Q * std::min<int64_t>(L1Q_PROBE_E, n_slice);
  return (uint32_t)std::min(pfrac * (double)sample, 4.0e9);
}

__global__ __launch_bounds__(256) void k_l1q_probe(const uint32_t* __restrict__ uq, int64_t q_pad, int64_t n_query,
                                                   const uint32_t* __restrict__ ue, int64_t e_pad, int64_t n_slice,
                                                   int kw, int kt, const float* __restrict__ thr, int pred_kind,
                                                   float margin, uint32_t* __restrict__ work,
                                                   const float* __restrict__ q_l1c) {
  if (__builtin_amdgcn_readfirstlane(work[1]) != L1Q_CODES8) return;
  const PredSel<-1> pred(pred_kind, margin);
  const int64_t q = (int64_t)blockIdx.x * n_query / gridDim.x;
  const int64_t span = n_slice > L1Q_PROBE_E ? n_slice - L1Q_PROBE_E : 0;
  const int64_t c = (((int64_t)blockIdx.x * span / gridDim.x) & ~(int64_t)3) + 4 * threadIdx.x;  // 64 threads
  const float l1d = l1q_delta(work, 255.0f);
  const float l1f = (float)(kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
  const float l1c = __builtin_fmaf((float)kt * 1.03f, l1d, 0x1p-120f);
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  if (c < n_slice) {  // columns c .. c + 3 lie inside the slice's whole tiles
#pragma unroll 8
    for (int r = 0; r < kw; ++r) {
      const uint32_t a = uq[(int64_t)r * q_pad + q];
      const uint4 e = *reinterpret_cast<const uint4*>(ue + (int64_t)r * e_pad + c);
      acc[0] = __builtin_amdgcn_sad_u8(a, e.x, acc[0]);
      acc[1] = __builtin_amdgcn_sad_u8(a, e.y, acc[1]);
      acc[2] = __builtin_amdgcn_sad_u8(a, e.z, acc[2]);
      acc[3] = __builtin_amdgcn_sad_u8(a, e.w, acc[3]);
    }
  }
  const float th = thr[q];
  uint32_t und = 0u;
  if (q_l1c != nullptr) {  // the tight bound (prediction = the score): the sweep's integer test
    uint32_t t_sure, t_span;
    l1_int_thresholds(th, q_l1c[q] + 0x1p-120f, l1d, l1f, 2u * work[3], t_sure, t_span);
#pragma unroll
    for (int j = 0; j < 4; ++j) und += (uint32_t)((acc[j] - t_sure < t_span) & (c + j < n_slice));
  } else
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = (float)acc[j] * l1d;
    const float bnd = __builtin_fmaf(a, l1f, l1c);
    const float p1 = pred(a - bnd), p2 = pred(a + bnd);
    const bool fin = a < INFINITY;
    const bool sure = fin & (fmaxf(p1, p2) < th);
    const bool out = (fin & (fminf(p1, p2) >= th)) | (th != th);
    und += (uint32_t)(!sure & !out & (c + j < n_slice));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) und += __shfl_xor(und, o);
  if ((threadIdx.x & 63) == 0 && und) atomicAdd(work + 2, und);
}

// Zeroes n words: the filters' workspace headers at the start of each sweep. A kernel, not
// hipMemsetAsync: replayed from a captured hipGraph, the memset node of the 4,352-byte L1
// header left words 2-3 holding stale bytes (the probe's count read garbage and the graph's
// evaluations switched to the 16-bit codes), while eager runs were right.
__global__ __launch_bounds__(256) void k_zero_words(uint32_t* __restrict__ p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

// Sum of the undecided-pair slots, the code-width word, the rescoring guard's count and the largest
// error offset of the tight bound -> out[0..3] (mmre_link_l1q_stats).
__global__ void k_l1q_stats(const uint32_t* __restrict__ work, unsigned long long* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const unsigned long long* sl =
      reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(work) + 256);
  unsigned long long t = 0;
  for (int i = 0; i < L1Q_SLOTS; ++i) t += *reinterpret_cast<const uint32_t*>(sl + i * L1Q_SLOT_STRIDE);
  out[0] = t;
  out[1] = work[1];
  out[2] = work[4];
  out[3] = work[3];
}

static int l1q_rows(int dim) { return (int)round_up((plane_rows(MMRE_TRANSE_L1, dim) + 1) / 2, KC); }
// (+ 1: the entity error-offset row of the tight bound, k_l1q_quant8)
static int l1q_rows8(int dim) { return (int)round_up((plane_rows(MMRE_TRANSE_L1, dim) + 3) / 4 + 1, KC); }

// ------------------------------------------------- split-bf16 MFMA filter ---
// DistMult / ComplEx count-only sweeps through a filter with exact rescoring, as the VALU
// sweeps' (rot_bound, L1Q): every f32 plane value x is split into two bf16 values hi = bf16(x)
// and lo = bf16(x - hi) (round to nearest even), and the sweep computes
//     S' = Qhi . Ehi + Qhi . Elo + Qlo . Ehi
// on v_mfma_f32_32x32x16_bf16: three MFMAs of 16 k each per 32 x 32 block where the exact
// sweep issues eight v_mfma_f32_32x32x2_f32 of 2 k (16x the f32 rate per MFMA cycle,
// 5.3x per scored element). Bound on |S' - S|, S the canonical f32 fma chain (what the exact
// sweep and the truth kernels compute), P the exact dot product, with Sigma = sum |q_k||e_k|
// <= |q|_2 |e|_2 (Cauchy-Schwarz):
//   |P - T|  <= 3.02 x 2^-16 Sigma      T = the three products' exact sum; the dropped terms
//                                       are lo.lo + (hi+lo).r_e + r_q.e with |lo| <= 2^-8 (1+2^-8) |x|
//                                       and |r| = |x - hi - lo| <= 2^-16 |x| (bf16: 8-bit significand)
//   |T - S'| <= 3K x 2u (1 + 2^-7) Sigma   any order / grouping of the 3K exact bf16 products
//                                       summed with at most one rounding (RN or toward zero,
//                                       2u) per addition -- MFMA's internal summation order is
//                                       not documented, so no more is assumed
//   |S - P|  <= K u (1 + small) Sigma      the canonical chain (u = 2^-24)
// plus 2^-29 sqrt(K) |q||e| for the values |x| < 2^-60 the split sets to zero (norms are
// clamped to >= 2^-30). So B = cb |q|_2 |e|_2, cb = 1.02 (7K 2^-24 (1 + 2^-7) + 3.02 2^-16 +
// 2^-29 sqrt K) (computed on the host, the norms' own rounding inside the 2 %). A pair whose
// prediction is on the same side of its query's threshold at both ends of [S' - B, S' + B]
// is decided (apply_pred is monotone); every other valid pair -- the truth itself, near ties,
// any non-finite S' (an inf / NaN operand is split into a NaN hi) -- is appended to a pair
// list and rescored with the canonical chain from the row-major copies (k_bf3_rescore), so
// the counts are the exact sweep's bit for bit. ~2e-4 of the C3 pairs and 2e-5 of C5's land
// in the list. A list that overflows its capacity sets a flag on the device: the raw counts
// are reset and the exact f32 sweep runs instead (gated launches, no host round trip).
// Workspace: header (BF3_HDR bytes of 32-bit words: word 1 the overflow flag, word 4 the segment
// capacity, word 5 the path record of the sweep as launched (bits 0-15 the wide sweep's query
// tile, 0 for the 128 x 128 sweep; bit 16 the lock-step windows: Bf3Grid::blk), the list's append
// counters from word BF3_SEG_W0 on, one per 128-B line: segment s at BF3_SEG_W0 + 32 s, the shared
// half's at s = BF3_SEGS) | pair list (bf3_cap int2, padded to 16 B) | |q| (q_pad
// floats) | |e| (e_pad floats) | split query planes (K/16 blocks x q_pad rows x 64 B: hi[16] |
// lo[16]) | split entity planes (K/16 x e_pad x 64 B) | the wide sweep's operands (Bf3Work).
// The list: half of it cut into BF3_SEGS segments of cap / (2 BF3_SEGS) pairs, each with its own
// counter on a 128-B line of the header (32-bit words BF3_SEG_W0 + 32 s), the other half shared
// (its counter: segment index BF3_SEGS). A sweep workgroup b appends to segment b % BF3_SEGS and,
// once that is full, to the shared half (bf3_list). One counter for the whole list serialised
// every append chip-wide (~13 ns per same-address atomic): C3's 46 k listed pairs ~0.35 of a
// 0.74-ms sweep (a build with the decision pass compiled out ran 0.39 ms); the shared half keeps
// a burst of one workgroup (a non-finite row's pairs) from overflowing its segment. A full shared
// half sets the overflow flag (word 1): the exact sweep then counts, as for a full list before.
// A counter that wraps (> 4 G appends) cannot clear the flag its first overflow set.
constexpr int BF3_SEGS = 64;
constexpr int BF3_SEG_W0 = 64;
constexpr int BF3_HDR = 4 * (BF3_SEG_W0 + 32 * (BF3_SEGS + 1));
#ifndef BF3_WG_PER_CU
#define BF3_WG_PER_CU 3  // workgroups per CU the sweep is compiled for (168 VGPRs)
#endif
inline int64_t bf3_cap(int64_t q_pad, int64_t e_pad) {
  const char* cap_env = getenv("MMRE_BF3_CAP");  // tests: a tiny list forces the overflow fallback
  if (cap_env && atoll(cap_env) > 0) return atoll(cap_env);
  int64_t c = q_pad * e_pad / 512;
  c = c < (1 << 16) ? (1 << 16) : c;
  return c > (1 << 26) ? (1 << 26) : c;
}
typedef short bf16x8 __attribute__((ext_vector_type(8)));

// append one undecided pair to the calling workgroup's segment of the list, or to the shared
// half when the segment is full (see BF3_SEGS)
__device__ __forceinline__ void bf3_list(uint32_t* __restrict__ hdr, int2* __restrict__ pairs, int64_t cap, int2 p) {
  const int sgm = (int)(blockIdx.x & (BF3_SEGS - 1));
  const int64_t seg_cap = cap / (2 * BF3_SEGS);
  const uint32_t i = atomicAdd(hdr + BF3_SEG_W0 + 32 * sgm, 1u);
  if ((int64_t)i < seg_cap) {
    pairs[sgm * seg_cap + i] = p;
    return;
  }
  const uint32_t j = atomicAdd(hdr + BF3_SEG_W0 + 32 * BF3_SEGS, 1u);
  if ((int64_t)j < cap - BF3_SEGS * seg_cap) pairs[BF3_SEGS * seg_cap + j] = p;
  else hdr[1] = 1u;
}

__device__ __forceinline__ uint32_t bf16_rn_bits(float x) {  // finite x: round to nearest even
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// The split of 16 consecutive k values of one column into the 64-B block {hi[16], lo[16]}.
__device__ __forceinline__ void bf3_split_store(const float (&x)[16], uint4* __restrict__ o) {
  uint32_t hw[8], lw[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    uint32_t hb = 0u, lb = 0u;
    if (!(fabsf(x[j]) < INFINITY)) {
      hb = 0x7FC0u;  // inf / NaN: a NaN operand, every product NaN: the pair is undecided
    } else if (fabsf(x[j]) >= 0x1p-60f) {
      hb = bf16_rn_bits(x[j]);
      lb = bf16_rn_bits(x[j] - __uint_as_float(hb << 16));  // x - hi is exact (Sterbenz)
    }
    if (j & 1) { hw[j >> 1] |= hb << 16; lw[j >> 1] |= lb << 16; }
    else { hw[j >> 1] = hb; lw[j >> 1] = lb; }
  }
  o[0] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
  o[1] = make_uint4(hw[4], hw[5], hw[6], hw[7]);
  o[2] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
  o[3] = make_uint4(lw[4], lw[5], lw[6], lw[7]);
}

// One thread per (column c, 16-k block kb) of a k-major plane (K rows x pad, columns col0 + c):
// the split block out[kb][c] = {hi[16], lo[16]} (4 x 16 B). Consecutive threads take
// consecutive columns of one block: coalesced 64-B-per-thread reads and writes.
__global__ __launch_bounds__(256) void k_bf3_split(const float* __restrict__ km, int64_t pad, int64_t col0,
                                                   int64_t n_cols, int nkb, uint4* __restrict__ out,
                                                   int64_t out_pad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cols * nkb) return;
  const int kb = (int)(i / n_cols);
  const int64_t c = i - (int64_t)kb * n_cols;
  const float* src = km + col0 + c + (int64_t)kb * 16 * pad;
  float x[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) x[j] = src[(int64_t)j * pad];  // all in flight together
  bf3_split_store(x, out + ((int64_t)kb * out_pad + c) * 4);
}

// The split planes, norms and (wide sweep) 32-column norm maxima straight from a ROW-MAJOR
// table (mmre_link_sweep_bf3_rows: DistMult, whose row-major copy is the raw table itself, so
// no re-laid-out copy is written per evaluation): one read of the rows, one write of the split
// blocks. 256 threads = 32 rows x 8 lanes; lane j of a row takes its 16-k blocks j, j + 8, ...
// (8 lanes read 512 contiguous bytes of the row; for one block the 32 rows' 64-B outputs are
// contiguous). Same split as k_bf3_split, norms as k_bf3_norms / k_bf3_enorms (any summation
// order serves: the bound's 2 % slack covers the norm's rounding); rows past n_rows (the
// slice's last tile) are zero with norm 0.
__global__ __launch_bounds__(256) void k_bf3_split_rows(const float* __restrict__ rows, int64_t n_rows, int64_t r0,
                                                        int ktot, uint4* __restrict__ out, int64_t out_pad,
                                                        float* __restrict__ norms, float* __restrict__ bmax) {
  __shared__ float wm[4];
  const int i = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int64_t c = (int64_t)blockIdx.x * 32 + i;  // slice column
  const int64_t r = r0 + c;
  const bool valid = r < n_rows;
  const float* src = rows + (valid ? r : 0) * (int64_t)ktot;
  const int nkb = ktot / 16;
  float ss = 0.0f;
  for (int kb = j; kb < nkb; kb += 8) {
    float x[16];
    const float4* s4 = reinterpret_cast<const float4*>(src + kb * 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 v = valid ? s4[u] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      x[4 * u] = v.x; x[4 * u + 1] = v.y; x[4 * u + 2] = v.z; x[4 * u + 3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) ss = __builtin_fmaf(x[u], x[u], ss);
    bf3_split_store(x, out + ((int64_t)kb * out_pad + c) * 4);
  }
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  ss += __shfl_xor(ss, 4);
  const float nv = valid ? fmaxf(sqrtf(ss), 0x1p-30f) : 0.0f;
  if (j == 0) norms[c] = nv;
  if (bmax) {
    float m = nv;  // the 8 rows of this wave (lanes 0, 8, .., 56 hold distinct rows)
    m = fmaxf(m, __shfl_xor(m, 8));
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  }
}

// The bound's 2-norms, one wave per row of a row-major copy (rows r0 .. r0 + n_out - 1, K
// floats each; rows >= n_rows get 0 -- padding the sweep never counts): |x|_2 clamped to
// >= 2^-30, inf / NaN kept (the bound is then inf / NaN: undecided). Any summation order
// serves -- the bound's 2 % slack covers the norm's rounding.
// With thr_out (the query rows of the wide sweep, k_sweep_bf3w): also the padded per-row side
// data its DMA copies whole -- thr_out[i] = the threshold (-inf past the queries: nothing beats
// a padded row) and qb_out[i] = cb |q|.
__global__ __launch_bounds__(256) void k_bf3_norms(const float* __restrict__ rows, int64_t n_rows, int64_t r0,
                                                   int64_t n_out, int ktot, float* __restrict__ norms,
                                                   const float* __restrict__ thr_in, float* __restrict__ thr_out,
                                                   float* __restrict__ qb_out, float cb) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_out) return;
  const int64_t r = r0 + i;
  float ss = 0.0f;
  if (r < n_rows) {
    const float* x = rows + r * (int64_t)ktot;
    for (int k = lane; k < ktot; k += 64) ss = __builtin_fmaf(x[k], x[k], ss);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if (lane == 0) {
    const float nv = r < n_rows ? fmaxf(sqrtf(ss), 0x1p-30f) : 0.0f;
    norms[i] = nv;
    if (thr_out) {
      thr_out[i] = r < n_rows ? thr_in[r] : -INFINITY;
      qb_out[i] = cb * nv;
    }
  }
}

// The entity norms of the wide sweep: k_bf3_norms' rows (one wave per row, 8 rows per wave) and,
// per block of 32 consecutive columns, their largest norm (bmax[blockIdx.x]; NaN norms skipped by
// fmaxf -- such a row's S' is NaN, undecided whatever the bound), the bound factor of
// k_sweep_bf3w's thresholds.
__global__ __launch_bounds__(256) void k_bf3_enorms(const float* __restrict__ rows, int64_t n_rows, int64_t r0,
                                                    int64_t n_out, int ktot, float* __restrict__ norms,
                                                    float* __restrict__ bmax) {
  __shared__ float wm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ss[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) ss[t] = 0.0f;
  const int64_t rb = r0 + (int64_t)blockIdx.x * 32 + wave * 8;
  for (int k = lane; k < ktot; k += 64) {
    float x[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {  // the wave's 8 rows' loads in flight together (past the table: its last row, unused)
      const int64_t r = rb + t < n_rows ? rb + t : n_rows - 1;
      x[t] = rows[r * (int64_t)ktot + k];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) ss[t] = __builtin_fmaf(x[t], x[t], ss[t]);
  }
  float m = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int64_t i = (int64_t)blockIdx.x * 32 + wave * 8 + t;
    const int64_t r = r0 + i;
    float v = ss[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const float nv = r < n_rows ? fmaxf(sqrtf(v), 0x1p-30f) : 0.0f;
    if (lane == 0 && i < n_out) norms[i] = nv;
    if (i < n_out) m = fmaxf(m, nv);
  }
  if (lane == 0) wm[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

// The sweep: units, grid and staging as k_sweep_mfma's 16-row plain variant (4 workgroups per
// CU, ballot row counters), one split block (16 k) per stage: 8 KB per operand tile, read into
// LDS as 16-B chunks at position chunk ^ ((row >> 2) & 3) of the row's 64 B (the 32 lanes of
// an MFMA operand read hit 32 different 16-B bank groups: conflict-free).
template <int PK>
__global__ __launch_bounds__(NT, BF3_WG_PER_CU) void k_sweep_bf3(
    const uint4* __restrict__ ent_b, int64_t e_pad, int64_t n_ent, const uint4* __restrict__ q_b, int64_t q_pad,
    int64_t n_query, int nkb, int n_et, int e_base, int n_groups, int pred_kind, float margin,
    const float* __restrict__ thr, const float* __restrict__ qn, const float* __restrict__ en, float cb,
    int32_t* __restrict__ counts, uint32_t* __restrict__ hdr, int2* __restrict__ pairs, int64_t cap, int emajor,
    int blk_qb, int blk_eb) {
  __shared__ uint4 sq[2][TQ * 4];
  __shared__ uint4 se[2][TE * 4];
  __shared__ __attribute__((aligned(16))) float s_th[2][TQ];
  __shared__ __attribute__((aligned(16))) float s_qb[2][TQ];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const PredSel<PK> pred(pred_kind, margin);
  const int wq = wave >> 1, we = wave & 1;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  // blk_qb > 0: the lock-step window order (BlockMap, one unit range per member); else the
  // contiguous ranges of UnitMap
  const bool blocked = blk_qb > 0;
  const UnitMap um(grp, n_groups, (int)(q_pad / TQ), n_et, emajor != 0);
  const BlockMap bm(grp, n_groups, gmem, per_grp, (int)(q_pad / TQ), n_et, blocked ? blk_qb : 1, blocked ? blk_eb : 1);
  const int u0 = blocked ? 0 : (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = blocked ? bm.count : (int)((int64_t)(gmem + 1) * um.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  auto unit_at = [&](int i, int& qt, int& et) {
    if (blocked) bm.at(i, qt, et);
    else um.at(i, qt, et);
  };

  int tpar = 0;
  int cntv = 0;  // lane L: the count of wave row L (tile row wq * 64 + L) in the current query tile
  auto row_of = [&](int bi, int r) { return wq * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow; };
  auto load_rows = [&](int qtile) {
    const int64_t q0 = (int64_t)qtile * TQ;
    tpar ^= 1;
    if (tid < TQ) {
      const int64_t q = q0 + tid;
      s_th[tpar][tid] = q < n_query ? thr[q] : -INFINITY;  // -inf: nothing beats a padded row
      s_qb[tpar][tid] = q < n_query ? cb * qn[q] : 0.0f;
    }
    cntv = 0;
  };
  auto flush_rows = [&](int qtile) {
    const int64_t q = (int64_t)qtile * TQ + wq * 64 + lane;
    if (q < n_query && cntv) atomicAdd(&counts[q], cntv);  // raw only (k_counts_finalize)
  };
  auto sidx = [](int row, int c) { return row * 4 + (c ^ ((row >> 2) & 3)); };

  uint4 rq0, rq1, re0, re1;
  int ld_unit = u0, ld_kb = 0, ld_qt, ld_et;
  unit_at(u0, ld_qt, ld_et);
  auto gload = [&]() {
    const uint4* qp = q_b + ((int64_t)ld_kb * q_pad + (int64_t)ld_qt * TQ) * 4;
    const uint4* ep = ent_b + ((int64_t)ld_kb * e_pad + (int64_t)ld_et * TE) * 4;
    rq0 = qp[tid];
    rq1 = qp[tid + NT];
    re0 = ep[tid];
    re1 = ep[tid + NT];
    if (++ld_kb == nkb) {
      ld_kb = 0;
      if (++ld_unit < u1) unit_at(ld_unit, ld_qt, ld_et);
    }
  };
  auto swrite = [&](int buf) {
    const int r0 = tid >> 2, c = tid & 3;
    sq[buf][sidx(r0, c)] = rq0;
    sq[buf][sidx(r0 + 64, c)] = rq1;
    se[buf][sidx(r0, c)] = re0;
    se[buf][sidx(r0 + 64, c)] = re1;
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  int cur_qt, cur_et;
  unit_at(u0, cur_qt, cur_et);
  load_rows(cur_qt);
  gload();
  swrite(0);
  __syncthreads();

  int buf = 0;
  for (int unit = u0; unit < u1; ++unit) {
    for (int kb = 0; kb < nkb; ++kb) {
      const bool more = ld_unit < u1;
      if (more) gload();
      __builtin_amdgcn_sched_barrier(0);  // the next stage's loads stay at the top (k_sweep_mfma)
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int qrow = wq * 64 + i * 32 + lcol, ecol = we * 64 + i * 32 + lcol;
        ah[i] = __builtin_bit_cast(bf16x8, sq[buf][sidx(qrow, lrow)]);
        al[i] = __builtin_bit_cast(bf16x8, sq[buf][sidx(qrow, 2 + lrow)]);
        bh[i] = __builtin_bit_cast(bf16x8, se[buf][sidx(ecol, lrow)]);
        bl[i] = __builtin_bit_cast(bf16x8, se[buf][sidx(ecol, 2 + lrow)]);
      }
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[bi], bh[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[bi], bl[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[bi], bh[bj], acc[bi][bj], 0, 0, 0);
        }
      if (kb == nkb - 1) {  // unit finished: decide, count, list the undecided
        const int64_t q0 = (int64_t)cur_qt * TQ;
        const int64_t ebase = (int64_t)cur_et * TE + we * 64;
        const int64_t e0 = ebase + lcol, e1 = ebase + 32 + lcol;
        const bool ev0 = e0 < n_ent, ev1 = e1 < n_ent;
        const float ne0 = ev0 ? en[e0] : 0.0f, ne1 = ev1 ? en[e1] : 0.0f;
        const uint64_t evm[2] = {__ballot(ev0), __ballot(ev1)};
        // this unit's per-row counts, assembled lane by lane: row L0's count into lane L0 by
        // v_writelane (the popcounts are wave-uniform), one add into cntv at the end -- a
        // `lane == L0 ? c : ...` select per row made the compiler keep 32 lane-compare masks
        // live across the sweep (SGPR spills into VGPR lanes)
        // Per pair: the bound (one multiply), S' - B and S' + B, and three compares whose results
        // are the wave's masks (v_cmp into an SGPR pair: "beats at both ends", "beats at neither",
        // non-finite S'); what is counted and what is listed is 64-bit mask logic on the scalar
        // unit, per row and column block (round 4's per-lane booleans: ~21 VALU instructions per
        // pair at C5 -- as many issue cycles as the three MFMAs)
        int ctmp = 0;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int r4 = 0; r4 < 16; r4 += 4) {  // four rows' thresholds and bound factors per LDS read pair
            const float4 t4 = *reinterpret_cast<const float4*>(&s_th[tpar][row_of(bi, r4)]);
            const float4 b4 = *reinterpret_cast<const float4*>(&s_qb[tpar][row_of(bi, r4)]);
            const float tv[4] = {t4.x, t4.y, t4.z, t4.w}, qb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int r = r4; r < r4 + 4; ++r) {
            const uint64_t mnan = __ballot(tv[r - r4] != tv[r - r4]);  // a NaN threshold: nothing beats it
            uint64_t msure[2], mund[2];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
              const float s = acc[bi][bj][r];
              const float bnd = qb[r - r4] * (bj ? ne1 : ne0);
              uint64_t hi, lo;
              if constexpr (PK == 2) {
                // predict = -s: better iff S > -th. Rounding is monotone, so fl(s - B) > -th
                // implies s - B > -th (every S of the bracket beats the truth) and
                // fl(s + B) < -th implies s + B < -th (none does); a NaN S' or bound decides nothing
                const float nt = -tv[r - r4];
                hi = __ballot(s - bnd > nt);
                lo = __ballot(s + bnd < nt);
              } else {
                const float p1 = pred(s - bnd), p2 = pred(s + bnd);
                hi = __ballot(fmaxf(p1, p2) < tv[r - r4]);
                lo = __ballot(fminf(p1, p2) >= tv[r - r4]);
              }
              const uint64_t nf = __ballot(!__builtin_isfinite(s));  // inf and NaN: undecided
              msure[bj] = hi & ~nf & evm[bj];
              mund[bj] = evm[bj] & ~(msure[bj] | (lo & ~nf) | mnan);
            }
            const int L0 = bi * 32 + (r & 3) + 8 * (r >> 2);
            const int c_lo = __popcll(msure[0] & 0xffffffffull) + __popcll(msure[1] & 0xffffffffull);
            const int c_hi = __popcll(msure[0] >> 32) + __popcll(msure[1] >> 32);
            ctmp = writelane_imm(ctmp, c_lo, L0);
            ctmp = writelane_imm(ctmp, c_hi, L0 + 4);
            if (__builtin_expect((mund[0] | mund[1]) != 0ull, 0)) {  // rare (uniform): list the pair(s) for exact rescoring
              // (the row from an opaque lane id: recomputed here, not 32 row indices kept live)
              const int ol = vgpr_opaque(lane);
              const int64_t q = q0 + wq * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ol >> 5);
              if (q < n_query) {
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                  if (!((mund[bj] >> ol) & 1ull)) continue;
                  bf3_list(hdr, pairs, cap, make_int2((int)q, (int)((bj ? e1 : e0) + e_base)));
                }
              }
            }
          }
        }
        cntv += ctmp;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;
        const bool last = unit + 1 >= u1;
        int next_qt = cur_qt, next_et = cur_et;
        if (!last) unit_at(unit + 1, next_qt, next_et);
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

// The wide variant (round 5). k_sweep_bf3 stages one 16-k split block per barrier through
// registers at 128 x 128 per workgroup and decides each pair with a per-pair bound and mask
// logic on the scalar unit (~40 scalar + ~20 vector instructions per 64 pairs): at C5 it held
// ~0.33 of the bf16 MFMA peak, with the decision pass alone ~18 % of the time and the operand
// traffic from L2 (134 GB per launch) the rest of the ceiling. Here:
//  * a workgroup covers QT queries x 256 entities, waves of 64 queries x 128 entities
//    (QT = 128: 4 waves, two workgroups per CU; QT = 256: 8 waves, one per CU, 1.5x the MFMAs
//    per operand byte): 24 MFMAs per stage per wave for 12 ds_read_b128;
//  * stages are copied global -> LDS by the DMA path (global_load_lds_dwordx4: no staging
//    registers, no ds_write) into three buffers, two stages in flight across each barrier (a
//    counted s_waitcnt vmcnt, a raw s_barrier); the per-unit side data -- the entity tile's |e|,
//    the query tile's thresholds and bound factors cb |q| -- rides with the unit's first stage;
//  * the MFMA's A operand is the entity rows and B the queries, so a lane's accumulator values
//    all belong to two queries (its columns): per-lane thresholds in registers, per-lane counts
//    (one compare + one add-with-carry per 64 pairs), and the bound is taken per 32-entity
//    block -- B = cb |q| max|e| over the block -- folded into two thresholds per query,
//    T_hi >= -thr + B and T_lo <= -thr - B (one ulp outward of the rounded sums): S' > T_hi
//    beats the truth for every S within the bound, S' < T_lo for none, anything else (NaN S'
//    included: both compares fail) is undecided and listed. No S' is +-inf unless |q| max|e|
//    overflows, and then B and the thresholds are inf: the block's pairs are undecided
//    (conservative; an inf-norm row costs its block's 32 x n_query pairs on the list).
//    Per 64 pairs: two compares, one add, two scalar ORs for the per-block "any undecided"
//    flag; blocks with a flag are re-scanned for the list (rare: truths and near ties).
// LDS image of a stage: the query rows then the entity rows, 64 B each (hi[16] | lo[16]),
// 16-B chunk c of row r at slot 4 r + (c ^ ((r >> 2) & 3)) as k_sweep_bf3's (conflict-free
// operand reads); the DMA writes a wave-instruction's 1 KB lane-linearly, so the swizzle is
// applied to the source addresses.
constexpr int W3E = 256;
#ifndef W3_DEEP
#define W3_DEEP 0  // 1: four stage buffers at QT = 256 (three stages in flight; A/B)
#endif
#ifndef W3_PAIR
#define W3_PAIR 0  // 1: four stage buffers, one barrier per two stages (A/B)
#endif
template <int QT>
struct W3Geom {
  static constexpr int WAVES = QT / 32;                 // (QT / 64) x 2 waves
  static constexpr int NT = WAVES * 64;
  static constexpr int QB = QT * 64, STAGE = QB + W3E * 64;
  static constexpr int EPW = W3E * 64 / 1024 / WAVES;   // entity DMA instructions per wave and stage
  static constexpr int NDMA = 2 + EPW;                  // + two for the query rows
  static constexpr int SIDE = 1024 + 8 * QT;            // block max |e| [8] (1 KB piece) | threshold [QT] | cb |q| [QT]
  static constexpr int PIECES = SIDE / 1024;            // side DMA instructions (waves 0 .. PIECES - 1)
  static constexpr int NBUF = ((W3_DEEP && QT == 256) || W3_PAIR) ? 4 : 3;  // stage (and side) buffers
  static constexpr int LDS = NBUF * (STAGE + SIDE);
  static constexpr int WG_PER_CU = QT == 128 ? 2 : 1;
};

__device__ __forceinline__ void w3_glds(const void* src, char* lds_dst) {  // lds_dst wave-uniform
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
// wait until at most n of this wave's vector-memory operations are outstanding (n wave-uniform:
// the DMA instructions issued for the next stage, 0 / NDMA / NDMA + 1)
template <int NDMA>
__device__ __forceinline__ void w3_wait(int n) {
  if (n == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if (n == NDMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA + 1) : "memory");
}
template <int N>
__device__ __forceinline__ void w3_vmwait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void w3_wait_n(int n) {  // n wave-uniform, 0 .. 15 (a larger n: wait for all)
  switch (n) {
    case 1: w3_vmwait<1>(); break;
    case 2: w3_vmwait<2>(); break;
    case 3: w3_vmwait<3>(); break;
    case 4: w3_vmwait<4>(); break;
    case 5: w3_vmwait<5>(); break;
    case 6: w3_vmwait<6>(); break;
    case 7: w3_vmwait<7>(); break;
    case 8: w3_vmwait<8>(); break;
    case 9: w3_vmwait<9>(); break;
    case 10: w3_vmwait<10>(); break;
    case 11: w3_vmwait<11>(); break;
    case 12: w3_vmwait<12>(); break;
    case 13: w3_vmwait<13>(); break;
    case 14: w3_vmwait<14>(); break;
    case 15: w3_vmwait<15>(); break;
    default: w3_vmwait<0>(); break;
  }
}
__device__ __forceinline__ float w3_next_up(float x) {  // the next float above x (x not NaN, inf kept; selects)
  const uint32_t u = __float_as_uint(x);
  const uint32_t r = x == 0.0f ? 1u : (x > 0.0f ? u + 1u : u - 1u);  // +-0 -> the smallest subnormal
  return x == INFINITY ? x : __uint_as_float(r);
}

// BLK: the lock-step XCD windows (BlockMap) or contiguous ranges (UnitMap), a template parameter
// so that only one map's state lives in registers
template <int PK, int QT, bool BLK>
__global__ __launch_bounds__(W3Geom<QT>::NT, W3Geom<QT>::WG_PER_CU) void k_sweep_bf3w(
    const uint4* __restrict__ ent_b, int64_t e_pad, int64_t e_cols, int64_t n_ent, const uint4* __restrict__ q_b,
    int64_t q_pad, int64_t n_query, int nkb, int n_et, int e_base, int n_groups, const float* __restrict__ thr_pad,
    const float* __restrict__ qbf, const float* __restrict__ en /* block maxima */, int32_t* __restrict__ counts,
    uint32_t* __restrict__ hdr, int2* __restrict__ pairs, int64_t cap, int emajor, int blk_qb, int blk_eb) {
  static_assert(PK == 2, "the wide sweep folds the bound into thresholds on S (prediction = -S)");
  using G = W3Geom<QT>;
  __shared__ __attribute__((aligned(16))) char lds[G::LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave >> 1, we = wave & 1;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  const int n_qt = (int)(q_pad / QT);
  auto make_map = [&]() {
    if constexpr (BLK) return BlockMap(grp, n_groups, gmem, per_grp, n_qt, n_et, blk_qb, blk_eb);
    else return UnitMap(grp, n_groups, n_qt, n_et, emajor != 0);
  };
  const auto map = make_map();
  const int u0 = BLK ? 0 : (int)((int64_t)gmem * map.count / per_grp);
  const int u1 = BLK ? map.count : (int)((int64_t)(gmem + 1) * map.count / per_grp);
  if (u0 >= u1) return;  // uniform over the workgroup
  auto unit_at = [&](int i, int& qt, int& et) { map.at(i, qt, et); };
  auto sidx = [](int row, int c) { return row * 4 + (c ^ ((row >> 2) & 3)); };

  // the DMA cursor: the stage (unit, k block) whose copies are issued next, and its buffers.
  // Per lane, the source offsets (uint4 units) of its DMA rows are fixed: the query rows'
  // relative to the query tile, the entity rows' (clamped to the slice's last column) set once
  // per unit; a stage adds only the uniform k-block plane base (round 6: the per-stage 64-bit
  // address arithmetic had been ~30 VALU per wave and stage, plus SGPR spill traffic).
  const int sl = lane & 3;
  uint32_t qoff[2], erow[G::EPW], eoff[G::EPW];
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // query rows 32 wave .. + 31: two 1-KB instructions of 16 rows
    const int row = 16 * (wave * 2 + j) + (lane >> 2);
    qoff[j] = (uint32_t)(row * 4 + (sl ^ ((row >> 2) & 3)));
  }
#pragma unroll
  for (int j = 0; j < G::EPW; ++j) erow[j] = (uint32_t)(16 * (wave * G::EPW + j) + (lane >> 2));
  int ld_unit = u0, ld_kb = 0, ld_qt, ld_et, ld_buf = 0, ld_sbuf = 0;
  auto enter_unit = [&]() {  // the cursor's unit: its tiles and the entity rows' offsets
    unit_at(ld_unit, ld_qt, ld_et);
    const uint32_t c0 = (uint32_t)ld_et * W3E, last = (uint32_t)e_cols - 1u;
#pragma unroll
    for (int j = 0; j < G::EPW; ++j) {  // past the slice's columns: its last one
      const uint32_t er = c0 + erow[j] <= last ? c0 + erow[j] : last;
      eoff[j] = er * 4u + (uint32_t)(sl ^ ((erow[j] >> 2) & 3));
    }
  };
  enter_unit();
  auto issue = [&]() -> int {  // this wave's share of the cursor's stage; returns its instruction count
    if (ld_unit >= u1) return 0;
    char* sb = lds + ld_buf * G::STAGE;
    const int64_t q0 = (int64_t)ld_qt * QT;
    const uint4* qp = q_b + ((int64_t)ld_kb * q_pad + q0) * 4;
    const uint4* ep = ent_b + (int64_t)ld_kb * e_pad * 4;
#pragma unroll
    for (int j = 0; j < 2; ++j) w3_glds(qp + qoff[j], sb + (wave * 2 + j) * 1024);
#pragma unroll
    for (int j = 0; j < G::EPW; ++j) w3_glds(ep + eoff[j], sb + G::QB + (wave * G::EPW + j) * 1024);
    int n = G::NDMA;
    if (ld_kb == 0 && wave < G::PIECES) {  // the unit's side data, one 1-KB piece per wave
      char* sd = lds + G::NBUF * G::STAGE + ld_sbuf * G::SIDE + wave * 1024;
      const int64_t c0 = (int64_t)ld_et * W3E;
      const float* src;
      if (wave == 0) {  // the tile's 8 block maxima (lanes 0-1; the others re-read them)
        src = en + (c0 / 32 + 4 * (lane & 1) + 4 <= e_cols / 32 ? c0 / 32 + 4 * (lane & 1) : e_cols / 32 - 4);
      } else {  // [threshold | cb |q|] of the tile's QT queries
        const int f = (wave - 1) * 256 + 4 * lane;
        src = f < QT ? thr_pad + q0 + f : qbf + q0 + (f - QT);
      }
      w3_glds(src, sd);
      n = G::NDMA + 1;
    }
    ld_buf = ld_buf == G::NBUF - 1 ? 0 : ld_buf + 1;
    if (++ld_kb == nkb) {
      ld_kb = 0;
      ld_sbuf = ld_sbuf == G::NBUF - 1 ? 0 : ld_sbuf + 1;
      if (++ld_unit < u1) enter_unit();
    }
    return n;
  };

  // lane L: the count of query wq * 64 + j * 32 + (L & 31) of the current query tile over the
  // entity rows it holds (lanes L and L ^ 32 hold the same query)
  int cnt[2] = {0, 0};
  auto flush_rows = [&](int qtile) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = cnt[j] + __shfl_xor(cnt[j], 32);
      const int64_t q = (int64_t)qtile * QT + wq * 64 + j * 32 + lcol;
      if (lrow == 0 && q < n_query && c) atomicAdd(&counts[q], c);  // raw only (k_counts_finalize)
      cnt[j] = 0;
    }
  };

  floatx16 acc[4][2];  // [entity block][query block]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  // the decision pass of a finished unit; FULL: every entity of the wave's 128 is in the slice
  // (else the first nval are). Entity of (bi, r, lane): ebase + bi * 32 + (r & 3) + 8 (r >> 2) +
  // 4 lrow -- the lanes 0-31 / 32-63 halves of a register hold two entity rows, so a row's
  // validity is a wave-uniform half mask.
  // Thresholds of the lane's two queries against entity block bi (32 rows of the wave's 128):
  // B = cb |q| max |e| over the block (k_bf3_enorms: a NaN norm is skipped, and that row's S' is
  // NaN: undecided; blocks past the slice hold no counted row), T_hi >= nt + B,
  // T_lo <= nt - B one ulp outward of the rounded sums.
  // (branch-free: per-lane branches here cost exec-mask juggling on every unit)
  auto thresholds = [&](float nm, const float nt[2], const float qbv[2], float th[2], float tl[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float b = qbv[j] * nm, a = nt[j] + b, c = nt[j] - b;
      const bool nt_nan = nt[j] != nt[j];       // a NaN threshold: nothing beats it (decided)
      const bool bad = a != a || c != c;        // a NaN / inf bound (inf - inf): every pair undecided
      th[j] = nt_nan || bad ? INFINITY : w3_next_up(a);
      tl[j] = nt_nan ? INFINITY : (bad ? -INFINITY : -w3_next_up(-c));
    }
  };
  // the decision pass of a finished unit; FULL: every entity of the wave's 128 is in the slice
  // (else the first nval are). Entity of (bi, r, lane): ebase + bi * 32 + (r & 3) + 8 (r >> 2) +
  // 4 lrow -- the lanes 0-31 / 32-63 halves of a register hold two entity rows, so a row's
  // validity is a wave-uniform half mask. nt: -threshold of the lane's queries; qbv: cb |q|.
  auto decide = [&](auto full_tag, const float* s_bm, int64_t q0, int64_t ebase, int nval, float nt0, float nt1,
                    float qb0, float qb1) {
    constexpr bool FULL = decltype(full_tag)::value;
    // (opaque copies: the two instances' compares are not merged and hoisted above the branch
    // between them -- with all 256 masks live)
    const float nt[2] = {vgpr_opaque_f(nt0), vgpr_opaque_f(nt1)};
    const float qbv[2] = {vgpr_opaque_f(qb0), vgpr_opaque_f(qb1)};
    // the wave's four block maxima: one LDS read, held in SGPRs (wave-uniform)
    const float4 bm4 = *reinterpret_cast<const float4*>(&s_bm[we * 4]);
    auto rfl = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
    const float nmb[4] = {rfl(bm4.x), rfl(bm4.y), rfl(bm4.z), rfl(bm4.w)};
    uint64_t und[4][2];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
      float thi[2], tlo[2];
      thresholds(nmb[bi], nt, qbv, thi, tlo);
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        uint64_t u = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[bi][bj][r];
          bool h = s > thi[bj];
          uint64_t vm = ~0ull;
          if constexpr (!FULL) {
            const int row0 = bi * 32 + (r & 3) + 8 * (r >> 2);
            vm = (row0 < nval ? 0xffffffffull : 0ull) | (row0 + 4 < nval ? 0xffffffff00000000ull : 0ull);
            h = h && row0 + 4 * lrow < nval;
          }
          cnt[bj] += h ? 1 : 0;
          u |= vm & ~(__ballot(h) | __ballot(s < tlo[bj]));
          // consumed here, group by group: left alone the compiler hoists all 128 groups'
          // compares and re-associates the sums, keeping 256 masks live (SGPR spills)
          cnt[bj] = vgpr_opaque(cnt[bj]);
          u = sgpr_opaque64(u);
        }
        und[bi][bj] = u;
      }
    }
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
      if (__builtin_expect((und[bi][0] | und[bi][1]) != 0ull, 0)) {  // rare (uniform): list the undecided pairs
        // the thresholds recomputed from opaque copies: the compares are redone here, not the
        // pass's masks kept live (the compiler would merge the two)
        const float ntc[2] = {vgpr_opaque_f(nt[0]), vgpr_opaque_f(nt[1])};
        float th[2], tl[2];
        thresholds(nmb[bi], ntc, qbv, th, tl);
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
          if (und[bi][bj] == 0ull) continue;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float s = acc[bi][bj][r];
            const int row0 = bi * 32 + (r & 3) + 8 * (r >> 2);
            uint64_t um = ~(__ballot(s > th[bj]) | __ballot(s < tl[bj]));
            if constexpr (!FULL)
              um &= (row0 < nval ? 0xffffffffull : 0ull) | (row0 + 4 < nval ? 0xffffffff00000000ull : 0ull);
            if (um == 0ull) continue;  // uniform
            // (the lane's query and entity from an opaque lane id: recomputed here, not 64 indices
            // kept live across the sweep)
            const int ol = vgpr_opaque(lane);
            const int64_t q = q0 + wq * 64 + bj * 32 + (ol & 31);
            if (((um >> ol) & 1ull) && q < n_query)
              bf3_list(hdr, pairs, cap, make_int2((int)q, (int)(ebase + row0 + 4 * (ol >> 5) + e_base)));
          }
        }
      }
    }
  };

  issue();               // stage 0
  int nxt = issue();     // stage 1: the instructions still allowed in flight when stage 0 is read
  int nxt2 = (G::NBUF == 4 && !W3_PAIR) ? issue() : 0;  // (four buffers) stage 2 as well
  int g = 0;  // stages swept by this workgroup
  int cur_qt, cur_et;
  unit_at(u0, cur_qt, cur_et);
  int buf = 0, sbuf = 0;
  for (int unit = u0; unit < u1; ++unit) {
    for (int kb = 0; kb < nkb; ++kb) {
      if constexpr (W3_PAIR) {
        // one barrier per two stages: at an even stage every copy of this pair has landed
        // (nothing else is in flight), then the next pair's two stages are issued into the
        // buffers the previous pair was read from
        if ((g & 1) == 0) {
          w3_vmwait<0>();
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          issue();
          issue();
        }
      } else {
        if constexpr (G::NBUF == 4) w3_wait_n(nxt + nxt2);
        else w3_wait<G::NDMA>(nxt);  // this wave's copies of the stage have landed ...
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // ... and every wave's; every wave is done with the buffer refilled next
        asm volatile("" ::: "memory");
        if constexpr (G::NBUF == 4) {
          nxt = nxt2;
          nxt2 = issue();  // three stages ahead
        } else {
          nxt = issue();  // the stage after next, into the buffer read in the previous stage
        }
      }
      ++g;
      const uint4* sq = reinterpret_cast<const uint4*>(lds + buf * G::STAGE);
      const uint4* se = reinterpret_cast<const uint4*>(lds + buf * G::STAGE + G::QB);
      bf16x8 eh[4], el[4], qh[2], ql[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int erow = we * 128 + i * 32 + lcol;
        eh[i] = __builtin_bit_cast(bf16x8, se[sidx(erow, lrow)]);
        el[i] = __builtin_bit_cast(bf16x8, se[sidx(erow, 2 + lrow)]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int qrow = wq * 64 + j * 32 + lcol;
        qh[j] = __builtin_bit_cast(bf16x8, sq[sidx(qrow, lrow)]);
        ql[j] = __builtin_bit_cast(bf16x8, sq[sidx(qrow, 2 + lrow)]);
      }
#pragma unroll
      for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(eh[bi], qh[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(el[bi], qh[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(eh[bi], ql[bj], acc[bi][bj], 0, 0, 0);
        }
      buf = buf == G::NBUF - 1 ? 0 : buf + 1;
      if (kb == nkb - 1) {  // unit finished: decide, count, list the undecided
        const float* s_bm = reinterpret_cast<const float*>(lds + G::NBUF * G::STAGE + sbuf * G::SIDE);
        const float* s_th = s_bm + 256;
        const float* s_qb = s_th + QT;
        const int64_t q0 = (int64_t)cur_qt * QT;
        const int64_t ebase = (int64_t)cur_et * W3E + we * 128;
        float ntv[2], qbv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ql_ = wq * 64 + j * 32 + lcol;
          ntv[j] = -s_th[ql_];  // prediction -S beats the truth iff S > nt
          qbv[j] = s_qb[ql_];
        }
        if (ebase + 128 <= n_ent) decide(std::true_type{}, s_bm, q0, ebase, 128, ntv[0], ntv[1], qbv[0], qbv[1]);
        else decide(std::false_type{}, s_bm, q0, ebase, (int)(n_ent > ebase ? n_ent - ebase : 0), ntv[0], ntv[1],
                    qbv[0], qbv[1]);
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
          for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.0f;
        sbuf = sbuf == G::NBUF - 1 ? 0 : sbuf + 1;
        const bool last = unit + 1 >= u1;
        int next_qt = cur_qt, next_et = cur_et;
        if (!last) unit_at(unit + 1, next_qt, next_et);
        if (last || next_qt != cur_qt) flush_rows(cur_qt);  // uniform: leave this query tile
        cur_qt = next_qt;
        cur_et = next_et;
      }
    }
  }
}

// Overflowed list: reset the raw counts the filter sweep added (the truth pass left them 0);
// the gated f32 sweep that follows recounts them.
__global__ __launch_bounds__(256) void k_bf3_fallback_zero(const uint32_t* __restrict__ hdr,
                                                           int32_t* __restrict__ counts, int64_t n_query) {
  if (hdr[1] == 0u) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_query) counts[q] = 0;
}

// The listed pairs, one thread each: the canonical chain (acc = fma(e_k, q_k, acc), k in
// order -- the truth kernels' and the f32 MFMA's arithmetic) from the row-major copies, and
// the strict Test.h compare against the query's threshold.
template <int PK>
__global__ __launch_bounds__(256) void k_bf3_rescore(const uint32_t* __restrict__ hdr, const int2* __restrict__ pairs,
                                                     int64_t cap, const float* __restrict__ q_rows,
                                                     const float* __restrict__ ent_rows, int ktot, int pred_kind,
                                                     float margin, const float* __restrict__ thr,
                                                     int32_t* __restrict__ counts) {
  if (hdr[1] != 0u) return;  // overflow: the exact sweep counted everything
  const PredSel<PK> pred(pred_kind, margin);
  // gridDim.x / (BF3_SEGS + 1) workgroups per segment; segment BF3_SEGS: the shared half
  const int sgm = (int)(blockIdx.x % (BF3_SEGS + 1)), part = (int)(blockIdx.x / (BF3_SEGS + 1));
  const int parts = (int)(gridDim.x / (BF3_SEGS + 1));
  const int64_t seg_cap = cap / (2 * BF3_SEGS);
  const int64_t scap = sgm < BF3_SEGS ? seg_cap : cap - BF3_SEGS * seg_cap;
  const int64_t listed = hdr[BF3_SEG_W0 + 32 * sgm];
  const int64_t n = listed < scap ? listed : scap;
  const int2* seg = pairs + sgm * seg_cap;
  for (int64_t i = (int64_t)part * blockDim.x + threadIdx.x; i < n; i += (int64_t)parts * blockDim.x) {
    const int2 p = seg[i];
    const float4* a = reinterpret_cast<const float4*>(q_rows + (int64_t)p.x * ktot);
    const float4* b = reinterpret_cast<const float4*>(ent_rows + (int64_t)p.y * ktot);
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < ktot / 4; ++k) {
      const float4 x = b[k], y = a[k];
      acc = __builtin_fmaf(x.x, y.x, acc);
      acc = __builtin_fmaf(x.y, y.y, acc);
      acc = __builtin_fmaf(x.z, y.z, acc);
      acc = __builtin_fmaf(x.w, y.w, acc);
    }
    if (pred(acc) < thr[p.x]) atomicAdd(&counts[p.x], 1);
  }
}

// the list header zeroed, with word 4 = the segment capacity and word 5 = the path record (both
// read by k_bf3_stats)
__global__ __launch_bounds__(256) void k_bf3_hdr_init(uint32_t* __restrict__ hdr, int64_t cap, uint32_t path) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < BF3_HDR / 4; i += gridDim.x * blockDim.x)
    hdr[i] = i == 4 ? (uint32_t)(cap / (2 * BF3_SEGS)) : i == 5 ? path : 0u;
}

__global__ void k_bf3_stats(const uint32_t* __restrict__ hdr, unsigned long long* __restrict__ out) {
  // one wave: the pairs listed = the segments' kept appends + the shared half's appends (a full
  // segment's further appends are counted there; past the shared half's end: the fallback ran)
  const int64_t seg_cap = hdr[4];
  unsigned long long t = 0;
  if (threadIdx.x < BF3_SEGS) {
    const unsigned long long c = hdr[BF3_SEG_W0 + 32 * threadIdx.x];
    t = c < (unsigned long long)seg_cap ? c : (unsigned long long)seg_cap;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (threadIdx.x == 0) {
    out[0] = t + hdr[BF3_SEG_W0 + 32 * BF3_SEGS];
    out[1] = hdr[1];
    out[2] = hdr[BF3_SEG_W0 + 32 * BF3_SEGS];  // the shared half's appends
    out[3] = hdr[5];                           // the path record (k_bf3_hdr_init)
  }
}

// ---------------------------------------------------------------- launch ---
// An entry point fills one SweepCall (link_common.h), each kernel family has one launcher that takes
// it, run-time choices reach the template arguments through with_op / with_bool(s) (dispatch.h),
// grid rules are functions.

// Resident workgroups of a persistent sweep: the occupancy API's blocks per CU (capped at 4,
// the VGPR-limited residency of a 256-thread group at <= 128 VGPRs) x the device's CUs. Queried
// once per kernel and device: the fused evaluation asks on every call. (The one cache of every
// sweep, link_valu.hip's and TransH's included: link_common.h declares it.)
int resident_groups(const void* kernel, int threads) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, int>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lock(mu);
  const auto [it, fresh] = cache.try_emplace(std::make_tuple(kernel, threads, dev), 0);
  if (fresh) {
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, 0) != hipSuccess || per <= 0) per = 1;
    it->second = cus * std::min(per, 4);
  }
  return it->second;
}

// The sweep over entities [e_begin, e_end) of the table (e_begin a multiple of TE): the kernels
// see the slice (pointer offset by e_begin columns, row stride e_pad, n_slice ids) and add
// e_base back wherever an absolute id matters (truth exclusion, type-constraint bits).
static int sweep_slice(SweepCall& C, int64_t n_ent, int64_t e_begin, int64_t e_end, int kp) {
  if (e_begin < 0 || e_begin % TE || e_end <= e_begin || e_end > n_ent) return MMRE_ERR_ARG;
  C.ent += e_begin;
  C.kp = kp;
  C.e_base = (int)e_begin;
  C.n_slice = e_end - e_begin;
  C.n_et = (int)((C.n_slice + TE - 1) / TE);
  C.e_cols = round_up(e_end, TE) - e_begin;
  C.tw = (n_ent + 31) / 32;  // type bitsets span the whole table
  return MMRE_OK;
}
// the same call over other planes of kp rows (ent: the table's first column, as the ABI's)
static SweepCall planes(SweepCall C, const void* ent, const void* q, int kp) {
  C.ent = (const float*)ent + C.e_base;
  C.q = (const float*)q;
  C.kp = kp;
  return C;
}
static bool valid_model(int m) { return m >= MMRE_TRANSE_L1 && m <= MMRE_ROTATE; }
static int check_link_args(int model, const SweepCall& C, int64_t n_ent) {
  if (!valid_model(model)) return MMRE_ERR_MODEL;
  if (C.pred_kind < 0 || C.pred_kind > 4) return MMRE_ERR_ARG;
  if (!C.ent || !C.q || !C.q_true || !C.counts || !C.truth || !C.qmode || !C.qr) return MMRE_ERR_ARG;
  if (C.n_query <= 0 || n_ent <= 0 || C.e_pad < n_ent || C.e_pad % TE || C.q_pad < C.n_query || C.q_pad % TQ)
    return MMRE_ERR_ARG;
  if ((C.type_head == nullptr) != (C.type_tail == nullptr)) return MMRE_ERR_ARG;
  if (n_ent > (int64_t)INT32_MAX - 256) return MMRE_ERR_SHAPE;  // padded ids stay int32
  return MMRE_OK;
}

// Units entity-tile-major inside each XCD group when the entity planes outgrow the caches
// (> 64 MB; the 256 MB MALL also holds the query planes): a workgroup's consecutive units then
// share its entity tile (L2-resident) and sweep the query tiles, which stay MALL-resident, so
// the table streams from HBM about once instead of once per query tile (C5, a 1 GB table:
// 35.8 -> 34.5 ms on one box, 60 -> ~1 GB of entity reads per launch); C3's 20 MB planes keep
// the query-major order (0.979 vs 0.982 ms). MMRE_MFMA_EMAJOR (experiments): 0 / 1 force the order.
static int mfma_emajor(int64_t e_pad, int ktot) {
  static const char* env = getenv("MMRE_MFMA_EMAJOR");
  return env ? atoi(env) : ((double)e_pad * ktot * 4.0 > 64.0 * (1 << 20) ? 1 : 0);
}

int launch_finalize(hipStream_t st, int32_t* counts, int64_t n_query, bool tc) {
  hipLaunchKernelGGL(k_counts_finalize, dim3((unsigned)((n_query + 255) / 256)), dim3(256), 0, st, counts, n_query,
                     tc ? 1 : 0);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

// 16 units per workgroup, between lo = 1 (2 with 32-row stages) and 8 x the resident slots: short
// ranges let the dispatcher balance CUs of different speed (C5 1,024 / 4,096 groups: 35.1 / 34.3
// ms) while the few-unit C3 keeps ranges long enough to amortise each group's first stage (16-row
// stages at 4 / CU, C3: 1,024 groups 0.97 ms, 2,048 1.04, 4,096 1.02). Gated (the bf3 fallback):
// one residency round when shut.
static int mfma_grid(int res, bool ks32, bool gated, int64_t units) {
  const int64_t lo = ks32 ? 2LL * res : (int64_t)res;
  int g = (int)std::min<int64_t>(8LL * res, std::max<int64_t>(lo, units / 16)) & ~7;
  if (gated) g = (int)lo & ~7;
  return grid_override(g);
}

// The f32 MFMA sweep's launch (DistMult / ComplEx; C.kp = ktot). gate != NULL: every workgroup
// returns at once unless *gate != 0 (the split-bf16 filter's overflow fallback).
static int launch_mfma(const SweepCall& C, const uint32_t* gate, bool finalize) {
  // persistent XCD-grouped grid as for the VALU sweep, 2 workgroups per resident slot (MI355X,
  // KCM = 16: C3 1.20 / 1.24 / 1.22 / 1.24 ms and C5 36.5 / 36.5 / 36.5 / 36.6 ms at 1/2/3/4x)
  // K stages of 32 rows (a unit's last one 16 when K = 32 n + 16: C3 ComplEx 2 x 200): half the
  // per-stage staging and barriers per MFMA of 16-row stages (scripts/probes/mfma_stage.hip:
  // 0.79 -> 0.86 of the f32 MFMA peak, L2-resident or HBM-streamed alike)
  // The plain sweep (no type constraint, no score store) runs 16-row stages at 4 workgroups
  // per CU (33 KB of LDS, 112 VGPRs with the ballot row counters): C3 1.03 -> 0.97 ms, C5
  // 33.7 -> 33.0 ms against 32-row stages at 2 per CU; the TC / STORE variants keep 32-row
  // stages (their extra registers would spill at 4 per CU).
  static const char* ks_env = getenv("MMRE_MFMA_STAGE");  // experiments: 16 / 32 force the stage
  const int ks_force = ks_env ? atoi(ks_env) : 0;
  const bool ks32 = ks_force == 32 || (ks_force != 16 && (C.tc() || C.store()));
  const int emajor = mfma_emajor(C.e_pad, C.kp);
  // DistMult / ComplEx predict -s: compiled into the plain sweep's epilogue (one compare with a
  // negated operand per pair); other kinds and the TC / STORE variants decode it at run time
  const bool fast_pk = C.pred_kind == 2 && !C.tc() && !C.store();
  with_bools(C.tc(), C.store(), fast_pk, [&](auto tc_, auto st_, auto fast_) {
    return with_bool(ks32, [&](auto ks32_) {
      constexpr bool TC = decltype(tc_)::value, ST = decltype(st_)::value, FAST = decltype(fast_)::value;
      if constexpr (!(FAST && (TC || ST))) {  // the instances there are
        auto kernel = k_sweep_mfma<TC, ST, FAST ? 2 : -1, decltype(ks32_)::value ? 32 : 16>;
        const int g = mfma_grid(resident_groups((const void*)kernel, NT), ks32, gate != nullptr,
                                C.q_tiles() * (int64_t)C.n_et);
        hipLaunchKernelGGL(kernel, dim3((unsigned)g), dim3(NT), 0, C.st, C.ent, C.e_pad, C.n_slice, C.q, C.q_pad,
                           C.n_query, C.kp, C.n_et, C.e_base, xcd_groups(g, C.n_et), C.pred_kind, C.margin, C.truth,
                           C.qr, C.qmode, C.type_head, C.type_tail, C.tw, C.counts, C.scores, emajor, gate);
      }
      return MMRE_OK;
    });
  });
  MMRE_CHECK_LAUNCH();
  return finalize ? launch_finalize(C.st, C.counts, C.n_query, C.tc()) : MMRE_OK;
}

// ------------------------------------------ fused TransE L1 evaluation (round 5) ---
// mmre_link_evaluate_l1q: the whole count-only TransE L1 evaluation of a query set -- entity
// prep, query prep, truth scores, filter-list scores and counts, the L1 filter's quantization
// and code-width probe, the sweep -- in seven launches instead of thirteen, with what is
// independent fused into the same launch (block ranges of one grid doing different work):
//   K1 k_eval_prep        entity rows (normalised, k-major + row-major) | query rows, each
//                         query block normalising its own anchor and truth rows from the raw
//                         table (no dependency on the entity blocks), the truth scores; per
//                         block max |x| / sum |x| of the planes (plain stores); block 0 zeroes
//                         the filter header
//   K2 k_eval_quant_list  filter-list scores | 8-bit codes + the tight bound's error sums +
//                         16-bit codes, one read of the planes; every quantization block reduces
//                         K1's per-block statistics itself (same order: the same M everywhere),
//                         the first writes M and the codes / f32 word
//   K3 k_eval_count_probe filter counts, a wave per group | the code-width probe, a wave per
//                         sampled query (the last of its 128 blocks decides 8 vs 16 bits)
//   K4-K6                 the three gated sweeps (8-bit, 16-bit, f32; the code-width word
//                         names the one that counts); the two code sweeps are GROUPED (below);
//                         the f32 launch also carries the
//                         finalize (filtered += raw): each workgroup's slice when its gate is
//                         shut, the last workgroup's pass (ticket) when it is open
// Grouped code sweeps: a TransE query vector depends on (mode, r, anchor) alone, the filter
// groups' key, so every member of a group would sweep a bit-identical row of codes; only its
// threshold (its own truth's score) differs. The code sweeps therefore run one SAD chain per
// SWEEP ROW -- a group, cut into runs of <= L1Q_GS members -- and the rank epilogue compares each
// (row, entity) integer score against every member's thresholds (sweep_valu_body, GS > 0):
//   K1 block 0            the row map from the group offsets (rows per group, a block scan):
//                         row -> first member's position in grp_q, member count; the row totals
//                         (device words: the host never knows them)
//   K2                    quantizes ONE column per row (the first member's vector, read from its
//                         row-major copy) into the query-side code planes; the tight bound's
//                         q_l1c is per row; a block range writes the query -> row map and, per
//                         128-row tile, the largest member count (the slot loop's bound)
//   K3                    the probe samples the same queries as before and reads their codes
//                         through that map: the same decision
//   sweeps                work unit = (row tile) x (entity tile); per-query outputs unchanged.
// The member thresholds are computed by the sweep when it enters a row tile (load_meta_grp), not
// in K3 as per-tile tables: the code width -- which of the two threshold sets applies -- is only
// known when K3 ends. K1 still prepares and measures every query (q_km, q_rows, q_true, truth
// are outputs; M, the f32 decision and the code step stay what the separate path computes), and
// the f32 fallback sweeps per query.
// No cross-workgroup hand-off inside K1 / K2: grid-wide results pass at kernel boundaries.
// Measured on the way (MI355X, C2, per evaluation): a __threadfence() per K1 block (L2
// write-back of each block's freshly written rows) 163 us for K1; per-block partials read back by
// a ticket's last block ~30 us of serial sc1 loads; three same-address atomics per block
// (max, sum, ticket: ~3,100 blocks) 128 us -- same-address atomics serialise at ~13 ns each.
// Values are bit-identical to the separate path (same canonical chains in the same order):
// tests/test_eval_fused_gpu.py holds counts, truths and planes equal.
struct EvalL1 {
  const float* ent;      // raw entity table (n_ent, dim)
  const float* rel;      // raw relation table (n_rel, dim)
  int64_t n_ent;
  int dim, kp, norm, rb, rbq;  // rows per entity block, queries per query block (two row sets)
  const int64_t* qh;
  const int64_t* qr;
  const int64_t* qt;
  const int8_t* qmode;
  int64_t n_query;
  float* ent_km;
  int64_t e_pad;
  float* ent_rows;
  float* q_km;
  int64_t q_pad;
  float* q_rows;
  int32_t* q_true;
  float* truth;
  int64_t e_begin, e_cols;  // the swept slice (its columns feed M)
  int n_eblk, n_qblk;
  uint32_t* und_q;          // optional per-query rescored-pair counters (zeroed here)
  float* pstat;             // per K1 block: max |x|, sum |x|
  uint32_t* ticket;         // [1]: the probe's ticket
  uint32_t* hdr;            // the L1 filter header
  double n_elem;
  float ratio;
  // the grouped sweep's row map (block 0 of K1): each filter group, cut into runs of <= row_cap
  // members, gives the sweep rows -- row_off the run's first position in grp_q, row_cnt its
  // members; n_rows = {rows, rows padded to tiles} (tile_m, the largest count per 128-row tile, is K2's)
  const int64_t* grp_qoff;
  int64_t n_groups;
  int row_cap;   // 0: no row map (the ungrouped sweeps follow), the grid has no row-map block
  int32_t* row_off;
  int32_t* row_cnt;
  int32_t* tile_m;
  int32_t* n_rows;
  // the rows the map may hold: q_pad, or -- the grouped sweep's claim counters (L1Q::tq) live in
  // row_cnt's tail -- the host's bound on the rows, padded to tiles; aff_n words at aff, zeroed
  // here on every call (no launch or memset node of their own: graph replays and a second
  // evaluation slot's workspace need nothing more)
  int64_t row_lim;
  uint32_t* aff;
  int aff_n;
};

// canonical sum of squares over x[0..dim) (k ascending, LDS reads batched 16 per round) and
// F.normalize's clamp: the divisor k_prep_rows uses
__device__ __forceinline__ float canon_norm(const float* x, int dim) {
  float ss = 0.0f;
  int k = 0;
  for (; k + 16 <= dim; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = x[k + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) ss = ss + v[u] * v[u];
  }
  for (; k < dim; ++k) ss = ss + x[k] * x[k];
  const float nr = sqrtf(ss);
  return nr < 1e-12f ? 1e-12f : nr;
}

__device__ __forceinline__ void abs_stat(float v, float& mx, float& sa) {
  if (!(v - v == 0.0f)) mx = INFINITY;  // inf / NaN: no codes (the f32 sweep counts)
  else {
    mx = fmaxf(mx, fabsf(v));
    sa += fabsf(v);
  }
}

__global__ __launch_bounds__(256, 7) void k_eval_prep(EvalL1 P) {
  extern __shared__ float lds[];
  __shared__ float s_nrm[64];
  __shared__ int64_t s_a[32], s_t[32], s_r[32];
  __shared__ int s_head[32];
  __shared__ float s_m[4], s_s[4];
  const int kp = P.kp, kt = kp, ls = kt + 1, rb = P.rb, rbq = P.rbq, dim = P.dim;
  const int tid = threadIdx.x, lane = tid & 31, slot = tid >> 5;
  float mx = 0.0f, sa = 0.0f;
  if (P.row_cap > 0 && blockIdx.x == 0) {
    // ---- the row map, from the group offsets alone (first in dispatch order: it overlaps the
    // prep blocks). Thread t takes a contiguous run of groups: rows per run, a block scan, then
    // the rows written in group order -- any partition, any order; a group of n members gives
    // ceil(n / row_cap) rows, so rows <= queries.
    __shared__ int s_scan[256];
    const int cap = P.row_cap;
    const int64_t per = (P.n_groups + 255) / 256;
    const int64_t g0 = (int64_t)tid * per, g1 = g0 + per < P.n_groups ? g0 + per : P.n_groups;
    int nr = 0;
#pragma unroll 8
    for (int64_t g = g0; g < g1; ++g) {
      const int64_t n = P.grp_qoff[g + 1] - P.grp_qoff[g];
      nr += n > 0 ? (int)((n + cap - 1) / cap) : 0;
    }
    s_scan[tid] = nr;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = tid >= o ? s_scan[tid - o] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    int64_t row = s_scan[tid] - nr;
    const int64_t total = s_scan[255], rows_pad = total > 0 ? (total + TQ - 1) / TQ * TQ : TQ;
    for (int64_t g = g0; g < g1; ++g) {
      const int64_t a = P.grp_qoff[g], n = P.grp_qoff[g + 1] - a;
      for (int64_t j = 0; j < n && row < P.row_lim; j += cap, ++row) {
        P.row_off[row] = (int32_t)(a + j);
        P.row_cnt[row] = (int32_t)(n - j < cap ? n - j : cap);
      }
    }
    for (int64_t r = total + tid; r < rows_pad && r < P.row_lim; r += 256) {
      P.row_off[r] = 0;
      P.row_cnt[r] = 0;
    }
    if (tid == 0) {
      P.n_rows[0] = (int32_t)(total < P.row_lim ? total : P.row_lim);
      P.n_rows[1] = (int32_t)(rows_pad < P.row_lim ? rows_pad : P.row_lim);
    }
    return;
  }
  const int bx = (int)blockIdx.x - (P.row_cap > 0 ? 1 : 0);  // the prep blocks
  if (bx < P.n_eblk) {  // ---- entity rows (k_prep_rows for TransE)
    const int64_t e0 = (int64_t)bx * rb;
    for (int i = slot; i < rb; i += 8) {
      const int64_t e = e0 + i;
      float* x = lds + i * ls;
#pragma unroll 4
      for (int k = lane; k < kt; k += 32) x[k] = (e < P.n_ent && k < dim) ? P.ent[e * dim + k] : 0.0f;
    }
    __syncthreads();
    if (P.norm) {
      if (tid < rb) s_nrm[tid] = canon_norm(lds + tid * ls, dim);
      __syncthreads();
      for (int i = slot; i < rb; i += 8) {
        float* x = lds + i * ls;
        const float nr = s_nrm[i];
        for (int k = lane; k < kt; k += 32) x[k] = x[k] / nr;
      }
      __syncthreads();
    }
    const bool in_slice = e0 >= P.e_begin && e0 < P.e_begin + P.e_cols;
    for (int i = slot; i < rb; i += 8) {
      const int64_t e = e0 + i;
      const float* x = lds + i * ls;
      if (e < P.n_ent) {
#pragma unroll 4
        for (int k = lane; k < kt; k += 32) P.ent_rows[e * kt + k] = x[k];
      }
      if (in_slice && e < P.e_pad)
        for (int k = lane; k < kt; k += 32) abs_stat(x[k], mx, sa);
    }
    write_k_major(lds, ls, rb, kt, P.ent_km, P.e_pad, e0);
  } else {  // ---- query rows: q = h + r (tail) / -(r - t) (head), and the truth scores
    // Two dependent global rounds: the ids, then the anchor, truth and relation rows of every
    // query at once (into LDS); the norms and the combine work from LDS. (Reading the relation
    // row for its norm and again for the combine, each in its own dependent rounds, made a
    // block's latency ~27 us: K1 31.7 us for an 8-way share of C2.)
    const int64_t q0 = (int64_t)(bx - P.n_eblk) * rbq;
    float* y0 = lds + rbq * ls;      // the truth rows
    float* z0 = lds + 2 * rbq * ls;  // the relation rows
    if (tid < rbq) {
      const int64_t q = q0 + tid;
      int64_t a = -1, tr = -1, r = 0;
      int head = 0;
      if (q < P.n_query) {
        head = P.qmode[q] == MMRE_HEAD_BATCH;
        a = head ? P.qt[q] : P.qh[q];
        tr = head ? P.qh[q] : P.qt[q];
        r = P.qr[q];
        P.q_true[q] = (int32_t)tr;
        if (P.und_q) P.und_q[q] = 0u;
      }
      s_a[tid] = a;
      s_t[tid] = tr;
      s_r[tid] = r;
      s_head[tid] = head;
    }
    __syncthreads();
    for (int i = slot; i < rbq; i += 8) {
      const int64_t a = s_a[i], tr = s_t[i], r = s_r[i];
      float* x = lds + i * ls;
      float* y = y0 + i * ls;
      float* z = z0 + i * ls;
#pragma unroll 8
      for (int k = lane; k < kt; k += 32) {
        x[k] = (a >= 0 && k < dim) ? P.ent[a * dim + k] : 0.0f;
        y[k] = (tr >= 0 && k < dim) ? P.ent[tr * dim + k] : 0.0f;
        z[k] = (a >= 0 && k < dim) ? P.rel[r * dim + k] : 0.0f;
      }
    }
    __syncthreads();
    if (P.norm) {  // anchor, truth (k_prep_rows' canonical order) and relation rows
      // (k_prep_queries' order: the same k-ascending sum of squares and clamp)
      if (tid < 3 * rbq) s_nrm[tid] = canon_norm(lds + tid * ls, dim);  // x | y | z rows
      __syncthreads();
      for (int i = slot; i < 2 * rbq; i += 8) {
        float* x = lds + i * ls;
        const float nr = s_nrm[i];
        for (int k = lane; k < kt; k += 32) x[k] = x[k] / nr;
      }
      __syncthreads();
    }
    for (int i = slot; i < rbq; i += 8) {
      float* x = lds + i * ls;
      const float* z = z0 + i * ls;
      const bool valid = s_a[i] >= 0;
      const bool head = s_head[i];
      const float rn = P.norm ? s_nrm[2 * rbq + i] : 1.0f;
      for (int k = lane; k < kp; k += 32) {
        if (!valid || k >= dim) {
          x[k] = 0.0f;
          continue;
        }
        // head_batch: score = h + (r - t) -> q = -(r - t); tail_batch: (h + r) - t -> q = h + r
        const float b = P.norm ? z[k] / rn : z[k];
        x[k] = head ? -(b - x[k]) : (x[k] + b);
      }
    }
    __syncthreads();
    if (tid < rbq && q0 + tid < P.n_query) {  // the truth's score: the canonical chain, k ascending
      const float* x = lds + tid * ls;
      const float* y = y0 + tid * ls;
      float acc = 0.0f;
      int k = 0;
      for (; k + 8 <= kp; k += 8) {
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a[u] = x[k + u];
          b[u] = y[k + u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + fabsf(a[u] - b[u]);
      }
      for (; k < kp; ++k) acc = acc + fabsf(x[k] - y[k]);
      P.truth[q0 + tid] = acc;  // prediction = the score (TransE.py:104-110)
    }
    write_k_major(lds, ls, rbq, kt, P.q_km, P.q_pad, q0);
    for (int i = slot; i < rbq; i += 8) {
      const int64_t q = q0 + i;
      const float* x = lds + i * ls;
      if (q < P.n_query) {
#pragma unroll 4
        for (int k = lane; k < kt; k += 32) P.q_rows[q * kt + k] = x[k];
      }
      if (q < P.q_pad)
        for (int k = lane; k < kt; k += 32) abs_stat(x[k], mx, sa);
    }
  }
  // ---- the block's |x| statistics (K2 reduces them); block 0 zeroes the filter header's
  // counters (probe count, largest offset, guard, undecided slots) for K2 / K3 / the sweeps
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o));
    sa += __shfl_xor(sa, o);
  }
  if ((tid & 63) == 0) {
    s_m[tid >> 6] = mx;
    s_s[tid >> 6] = sa;
  }
  __syncthreads();
  if (tid == 0) {
    P.pstat[2 * bx] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    P.pstat[2 * bx + 1] = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
  }
  if (bx == 0) {
    for (int i = 2 + tid; i < L1Q_PART / 4; i += 256) P.hdr[i] = 0u;
    for (int i = tid; i < P.aff_n; i += 256) P.aff[i] = 0u;  // the grouped sweep's claim counters
  }
}

// The filter-list score of one entry (k_filter_scores' list task, TransE L1, prediction = the
// score): the canonical chain over kp floats, 64 floats of each row in flight per round.
__device__ __forceinline__ float l1_row_score64(const float* __restrict__ qv, const float* __restrict__ ev, int kp) {
  float acc = 0.0f;
  int k0 = 0;
  for (; k0 + 64 <= kp; k0 += 64) {
    float4 a[16], x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      a[i] = *reinterpret_cast<const float4*>(qv + k0 + 4 * i);
      x[i] = *reinterpret_cast<const float4*>(ev + k0 + 4 * i);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc = acc + fabsf(a[i].x - x[i].x);
      acc = acc + fabsf(a[i].y - x[i].y);
      acc = acc + fabsf(a[i].z - x[i].z);
      acc = acc + fabsf(a[i].w - x[i].w);
    }
  }
  for (; k0 < kp; k0 += 8) {  // kp % 8 == 0
    float4 a[2], x[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i] = *reinterpret_cast<const float4*>(qv + k0 + 4 * i);
      x[i] = *reinterpret_cast<const float4*>(ev + k0 + 4 * i);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      acc = acc + fabsf(a[i].x - x[i].x);
      acc = acc + fabsf(a[i].y - x[i].y);
      acc = acc + fabsf(a[i].z - x[i].z);
      acc = acc + fabsf(a[i].w - x[i].w);
    }
  }
  return acc;
}

struct EvalQuant {  // K2's quantization operands (k_l1q_quant8<TIGHT> + the 16-bit words)
  L1QPlane pq, pe;  // 8-bit planes
  uint32_t* out16q;
  uint32_t* out16e;
  int kw, k2, kt, n_blk;  // 8-bit word rows, 16-bit word rows, floats per row, blocks per plane
  int tight;
  float* q_l1c;
  // grouped sweep: the query-side planes hold one column per sweep ROW (its first member's
  // vector: every member's is bit-identical), q_l1c is per row, and the blocks after the
  // quantization blocks write the query -> row map (the probe's)
  const int32_t* row_off;
  const int32_t* row_cnt;
  const int32_t* grp_q;
  const int32_t* n_rows;
  int32_t* row_of_q;
  int32_t* tile_m;
};

__global__ __launch_bounds__(256, 4) void k_eval_quant_list(EvalL1 P, EvalQuant Q, const int32_t* __restrict__ ids,
                                                         const int32_t* __restrict__ entry_q, int64_t n_entries,
                                                         float* __restrict__ list_v, int n_lblk) {
  if ((int)blockIdx.x < n_lblk) {  // ---- filter-list scores (k_filter_scores' list tasks)
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_entries) return;
    const int64_t j = ids[p], vq = entry_q[p];
    if (j < 0 || j >= P.n_ent || vq < 0 || vq >= P.n_query) {
      list_v[p] = __builtin_nanf("");  // never < a threshold: an invalid id is not counted
      return;
    }
    list_v[p] = l1_row_score64(P.q_rows + vq * P.kp, P.ent_rows + j * P.kp, P.kp);
    return;
  }
  if ((int)blockIdx.x >= n_lblk + 2 * Q.n_blk) {  // ---- query -> sweep row, a thread per row
    // (+ the block's two row tiles' largest member counts, the sweep's slot-loop bounds)
    __shared__ int s_tm[2];
    if (threadIdx.x < 2) s_tm[threadIdx.x] = 0;
    __syncthreads();
    const int mb = (int)blockIdx.x - n_lblk - 2 * Q.n_blk;
    const int64_t row = (int64_t)mb * 256 + threadIdx.x;
    int n = 0;
    if (row < Q.n_rows[0]) {
      const int64_t a = Q.row_off[row];
      n = Q.row_cnt[row];
      for (int s = 0; s < n; ++s) {
        const int64_t q = Q.grp_q[a + s];
        if (q >= 0 && q < P.n_query) Q.row_of_q[q] = (int32_t)row;
      }
    }
    if (n > 0) atomicMax(&s_tm[threadIdx.x >> 7], n);
    __syncthreads();
    if (threadIdx.x < 2 && (int64_t)(2 * mb + threadIdx.x + 1) * TQ <= P.q_pad) Q.tile_m[2 * mb + threadIdx.x] = s_tm[threadIdx.x];
    return;
  }
  // ---- M and the codes / f32 decision from K1's per-block statistics: every quantization block
  // reduces them in the same order (the same M and decision everywhere, deterministic); the
  // first one publishes them in the header for K3 and the sweeps (the l1q_fallback test:
  // M non-finite, or M > ratio x mean |x|)
  __shared__ float s_rm[4], s_rs[4];
  {
    const int nst = P.n_eblk + P.n_qblk;
    float m = 0.0f, sm = 0.0f;
#pragma unroll 8
    for (int i = threadIdx.x; i < nst; i += 256) {
      const float2 v = reinterpret_cast<const float2*>(P.pstat)[i];
      m = fmaxf(m, v.x);
      sm += v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      m = fmaxf(m, __shfl_xor(m, o));
      sm += __shfl_xor(sm, o);
    }
    if ((threadIdx.x & 63) == 0) {
      s_rm[threadIdx.x >> 6] = m;
      s_rs[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
  }
  const float mx = fmaxf(fmaxf(s_rm[0], s_rm[1]), fmaxf(s_rm[2], s_rm[3]));
  const float msum = (s_rs[0] + s_rs[1]) + (s_rs[2] + s_rs[3]);
  const bool fb = !(mx < INFINITY) || (double)mx > (double)P.ratio * ((double)msum / P.n_elem);
  if ((int)blockIdx.x == n_lblk && threadIdx.x == 0) {
    P.hdr[0] = __float_as_uint(mx < INFINITY ? mx : INFINITY);
    P.hdr[1] = fb ? L1Q_F32 : L1Q_CODES8;
  }
  if (fb) return;  // the f32 sweep counts: no codes
  // ---- the codes: 8-bit words (+ the tight bound's error row) and 16-bit words in one pass
  const int b = (int)blockIdx.x - n_lblk;
  const bool ent = b >= Q.n_blk;
  const int bx = ent ? b - Q.n_blk : b;
  const L1QPlane& pl = ent ? Q.pe : Q.pq;
  const float* __restrict__ km = pl.km;
  const bool rows = !ent && Q.n_rows != nullptr;  // grouped: a column per sweep row
  const int64_t pad = pl.pad, c0 = pl.c0, n = rows ? (int64_t)Q.n_rows[1] : pl.n;
  uint32_t* __restrict__ out = pl.out;
  uint32_t* __restrict__ out16 = ent ? Q.out16e : Q.out16q;
  const int kp = P.kp, kw = Q.kw, k2 = Q.k2, kt = Q.kt;
  const float inv = (mx > 0.0f && mx < INFINITY) ? 255.0f / (2.0f * mx) : 0.0f;
  const float inv16 = (mx > 0.0f && mx < INFINITY) ? 65535.0f / (2.0f * mx) : 0.0f;
  const float off = (mx < INFINITY) ? mx : 0.0f;
  const float delta = (mx > 0.0f && mx < INFINITY) ? (2.0f * mx) / 255.0f : 0.0f;
  const float l1f = (float)(kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
  const int words = (kt + 3) >> 2;
  const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
  __shared__ float s_err[8][32];
  for (int64_t cb = (int64_t)bx * 32; cb < n; cb += (int64_t)Q.n_blk * 32) {  // uniform
    const bool live = cb + cl < n;
    const int64_t c = c0 + cb + cl;
    // the source column: the entity's own, or the row's first member (a padding row: zeros)
    int64_t cs = c;
    if (rows) cs = (live && c < Q.n_rows[0]) ? (int64_t)Q.grp_q[Q.row_off[c]] : -1;
    if (rows && cs >= P.n_query) cs = -1;
    float err = 0.0f;
    // four word rows of a thread in flight together (kw <= 64 word rows -- d <= 256 -- is two
    // load rounds instead of four; eight took 167 VGPRs), then coded in the same order as before
    for (int r0 = g; r0 < kw; r0 += 32) {
      float xv[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int k = 4 * (r0 + 8 * j) + h;
          xv[j][h] = (!rows && live && r0 + 8 * j < kw && k < kp) ? km[(int64_t)k * pad + c] : 0.0f;
        }
      if (rows) {  // a row's vector from its member's row-major copy (the same floats as the k-major
                   // plane's; 16 B per word row instead of four scattered dwords)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * (r0 + 8 * j);
          if (live && cs >= 0 && r0 + 8 * j < kw && k + 3 < kp) {
            const float4 v = *reinterpret_cast<const float4*>(P.q_rows + cs * kp + k);
            xv[j][0] = v.x;
            xv[j][1] = v.y;
            xv[j][2] = v.z;
            xv[j][3] = v.w;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r0 + 8 * j;
        if (r >= kw) break;
        uint32_t word = 0u, w16a = 0u, w16b = 0u;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int k = 4 * r + h;
          if (live && k < kp) {
            const float x = xv[j][h];
            float t = (x + off) * inv;
            t = t == t ? fminf(fmaxf(t, 0.0f), 255.0f) : 0.0f;
            const float code = rintf(t);
            word |= (uint32_t)code << (8 * h);
            if (Q.tight) err += fabsf(x - (code * delta - off));
            float t16 = (x + off) * inv16;
            t16 = t16 == t16 ? fminf(fmaxf(t16, 0.0f), 65535.0f) : 0.0f;
            const uint32_t c16 = (uint32_t)rintf(t16);
            if (h < 2) w16a |= c16 << (16 * h);
            else w16b |= c16 << (16 * (h - 2));
          }
        }
        if (live) {
          if (!(Q.tight && r == words)) out[(int64_t)r * pad + c] = word;
          if (2 * r < k2) out16[(int64_t)(2 * r) * pad + c] = w16a;
          if (2 * r + 1 < k2) out16[(int64_t)(2 * r + 1) * pad + c] = w16b;
        }
      }
    }
    if (Q.tight) {
      s_err[g][cl] = err;
      __syncthreads();
      uint32_t o_max = 0u;  // this chunk's largest entity offset (wave 0), one atomic per chunk
      if (g == 0 && live) {
        float e = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) e += s_err[i][cl];
        const float eb = __builtin_fmaf(e, 1.01f, (float)kt * 0x1p-20f * mx);
        uint32_t wv = 0u;
        if (!ent) {
          Q.q_l1c[c] = eb;
        } else {
          // (<= 1,005 at kt <= 1,984 without the clamp acting: see k_l1q_quant8)
          uint32_t o = delta > 0.0f ? (uint32_t)ceilf(fminf(eb / (delta * (1.0f - l1f)) * (1.0f + 0x1p-17f), 1020.0f))
                                    : 0u;
          o_max = o;
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const uint32_t bb = o < 255u ? o : 255u;
            wv |= bb << (8 * h);
            o -= bb;
          }
        }
        out[(int64_t)words * pad + c] = wv;
      }
      if (ent && threadIdx.x < 64) {  // uniform per wave: 32 lanes' offsets -> one atomicMax
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) o_max = max(o_max, (uint32_t)__shfl_xor((int)o_max, sh));
        if (threadIdx.x == 0 && o_max) atomicMax(P.hdr + 3, o_max);
      }
      __syncthreads();
    }
  }
}

// ---- the per-query route. A query whose truth ranks mid-table has a third to a half
// of the entities inside its 8-bit band; each of those pairs is rescored with the canonical chain at
// ~90 swept pairs' cost (MMRE_PAIR_COST), 30-50 code sweeps of the row, where an exact f32 sweep of
// the row costs ~4.3. K3's third block range scores every sweep row against one fixed sample of
// entity columns and flags a member whose band holds L1Q_HEAVY_FRAC of the sample or more;
// k_l1q_route_compact lists the flagged queries (query order, capped); the 8-bit sweeps leave a
// listed query out (load_meta / load_meta_grp) and k_heavy_rows counts it exactly. Counts are the
// same either way: the route only decides which exact method counts a query.
// The sample: four windows of 64 columns, their starts spread evenly over the slice (lane l: window
// l / 16, columns 4 (l % 16) .. + 3 of it) -- the same for every row, staged in LDS L1Q_HEAVY_KCH
// code rows at a time. (mmre.link.l1q_heavy_sample restates it.)
constexpr int L1Q_HEAVY_KCH = 16;
constexpr double L1Q_HEAVY_FRAC = 0.10;   // of the sampled columns (measured: DESIGN.md 4e)
constexpr double L1Q_HEAVY_ROW_COST = 4.3;  // an f32 row sweep in code sweeps (issue slots)
constexpr double L1Q_PAIR_COST = 90.0;      // a rescored pair in swept pairs (MMRE_PAIR_COST)
__host__ __device__ __forceinline__ int64_t l1q_heavy_col(int64_t n_slice, int lane) {
  const int64_t span = n_slice > 64 ? n_slice - 64 : 0;
  return ((span * (lane >> 4) / 3) & ~(int64_t)3) + 4 * (lane & 15);
}
static uint32_t l1q_heavy_sample(int64_t n_slice) {  // sampled columns inside the slice
  uint32_t n = 0;
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 4; ++j) n += l1q_heavy_col(n_slice, l) + j < n_slice;
  return n;
}
struct HeavyProbe {
  int n_blk;                 // blocks of the range (0: no route)
  int e_base;
  const int32_t* row_off;    // grouped: the row map (nullptr: a row per query)
  const int32_t* row_cnt;
  const int32_t* n_rows;
  uint8_t* flags;            // per query: its sampled band reached min_count
  uint32_t min_count;
};

// One block: the flag bytes -> the routed list (ascending query ids, the first `cap` flagged
// ones: a scan, no first-come atomics), the bytes rewritten as the routed map, the record in the
// header; a routed query's und_q entry becomes its f32 row's cost in rescored-pair units, so the
// sharding's weights stay a cost. Inert (nothing routed, bytes cleared) unless the 8-bit codes count.
__global__ __launch_bounds__(1024) void k_l1q_route_compact(uint32_t* __restrict__ hdr, uint8_t* __restrict__ flags,
                                                            int32_t* __restrict__ list, int64_t n_query, int64_t q_pad,
                                                            uint32_t cap, uint32_t* __restrict__ und_q, uint32_t und_cost,
                                                            uint32_t n_samp, uint32_t min_count) {
  __shared__ uint32_t s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool on = hdr[1] == L1Q_CODES8;
  // a thread's queries: a run of whole 16-byte words of the flag bytes (q_pad of them, a multiple
  // of 128), read as uint4 -- byte by byte the block's two passes were 22 us at C2, latency-bound
  const int64_t chunk = round_up((n_query + 1023) / 1024, 16);
  const int64_t a = min(q_pad, tid * chunk), b = min(q_pad, a + chunk);
  uint32_t n = 0u;
  if (on) {
#pragma unroll 4
    for (int64_t o = a; o < b; o += 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(flags + o);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) n += (uint32_t)((((w[j >> 2] >> (8 * (j & 3))) & 255u) != 0u) & (o + j < n_query));
    }
  }
  uint32_t inc = n;  // inclusive scan over the wave, then over the 16 waves
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    const uint32_t v = __shfl_up(inc, sh);
    if (lane >= sh) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t base = 0u, total = 0u;
  for (int w = 0; w < 16; ++w) {
    if (w < wv) base += s_w[w];
    total += s_w[w];
  }
  uint32_t pos = base + inc - n;
  for (int64_t o = a; o < b; o += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(flags + o);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool f = on & (((w[j >> 2] >> (8 * (j & 3))) & 255u) != 0u) & (o + j < n_query);
      const bool r = f && pos < cap;
      if (r) {
        list[pos] = (int32_t)(o + j);
        if (und_q) und_q[o + j] = und_cost;
        out[j >> 2] |= 1u << (8 * (j & 3));
      }
      pos += f;
    }
    *reinterpret_cast<uint4*>(flags + o) = make_uint4(out[0], out[1], out[2], out[3]);
  }
  if (tid == 0) {
    hdr[L1Q_ROUTE_W + 0] = total;
    hdr[L1Q_ROUTE_W + 1] = total < cap ? total : cap;
    hdr[L1Q_ROUTE_W + 2] = on ? n_samp : 0u;
    hdr[L1Q_ROUTE_W + 3] = on ? min_count : 0u;
  }
}

// route record -> out[0..3] (mmre_link_l1q_route_stats)
__global__ void k_l1q_route_stats(const uint32_t* __restrict__ work, unsigned long long* __restrict__ out) {
  if (threadIdx.x < 4) out[threadIdx.x] = work[L1Q_ROUTE_W + threadIdx.x];
}

// K3: filter counts (k_filter_count without type masks, one WAVE per filter group, four per
// block) | the code-width probe (k_l1q_probe's sample, one wave per sampled query: 128 blocks, so
// the probe's count and ticket take 128 same-address atomics each, not 512), whose last block
// turns the code-width word to the 16-bit codes when the sample's undecided fraction is over
// the threshold. force_bits 8 / 16 (MMRE_L1_BITS): no probe; 16 sets the word (unless f32).
// | the per-query route's probe (H.n_blk blocks, 0 without the route): every sweep row against the
// fixed sample of entity columns, a flag byte per member query (HeavyProbe, above).
__global__ __launch_bounds__(256) void k_eval_count_probe(
    const int64_t* __restrict__ grp_qoff, const int32_t* __restrict__ grp_q, int64_t n_groups, int n_cblk,
    const int64_t* __restrict__ off, const int32_t* __restrict__ ids, const float* __restrict__ list_v,
    const int32_t* __restrict__ qtrue, const float* __restrict__ thr, int64_t n_query, int64_t n_ent,
    int32_t* __restrict__ counts, const uint32_t* __restrict__ uq, int64_t q_pad, const uint32_t* __restrict__ ue,
    int64_t e_pad, int64_t n_slice, int kw, int kt, const float* __restrict__ q_l1c, uint32_t* __restrict__ hdr,
    uint32_t* __restrict__ ticket, uint32_t probe_max, int force_bits, const int32_t* __restrict__ row_of_q,
    HeavyProbe H) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_pblk = (int)gridDim.x - n_cblk - H.n_blk;  // the code-width probe's blocks
  if ((int)blockIdx.x >= n_cblk + n_pblk) {
    // ---- the per-query route's probe: 32 sweep rows per block, 8 per wave, a lane per four columns
    __shared__ uint4 s_e[L1Q_HEAVY_KCH][64];
    if (__builtin_amdgcn_readfirstlane(hdr[1]) != L1Q_CODES8 || force_bits == 16) return;  // no 8-bit sweep
    const int64_t n_r = H.n_rows ? (int64_t)H.n_rows[0] : n_query;
    const int64_t row0 = ((int64_t)blockIdx.x - n_cblk - n_pblk) * 32 + __builtin_amdgcn_readfirstlane(wv) * 8;
    if (row0 - __builtin_amdgcn_readfirstlane(wv) * 8 >= n_r) return;  // uniform over the block
    const int64_t c = l1q_heavy_col(n_slice, lane);
    uint32_t acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
    // Both operands of a chunk of code rows go through LDS, zero past the last row (|0 - 0| adds
    // nothing), so the chunk's 16 steps are unrolled with their LDS reads in flight. (Query words
    // read from HBM step by step, eight dependent-latency loads per step: K3 16 -> 71 us at C2.)
    __shared__ __attribute__((aligned(16))) uint32_t s_q[L1Q_HEAVY_KCH][32];
    const int64_t brow0 = row0 - __builtin_amdgcn_readfirstlane(wv) * 8;  // (32 rows of a block: inside q_pad)
    const int wq = __builtin_amdgcn_readfirstlane(wv) * 8;
    for (int r0 = 0; r0 < kw; r0 += L1Q_HEAVY_KCH) {
      __syncthreads();  // the previous chunk's reads are done
#pragma unroll
      for (int rr = wv; rr < L1Q_HEAVY_KCH; rr += 4) {  // (entry (rr, lane): the lane's own columns)
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + rr < kw && c < n_slice) v = *reinterpret_cast<const uint4*>(ue + (int64_t)(r0 + rr) * e_pad + c);
        s_e[rr][lane] = v;
      }
#pragma unroll
      for (int i = tid; i < L1Q_HEAVY_KCH * 32; i += 256) {
        const int rr = i >> 5;
        s_q[rr][i & 31] = r0 + rr < kw ? uq[(int64_t)(r0 + rr) * q_pad + brow0 + (i & 31)] : 0u;
      }
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < L1Q_HEAVY_KCH; ++rr) {
        const uint4 e = s_e[rr][lane];
        const uint4 a0 = *reinterpret_cast<const uint4*>(&s_q[rr][wq]);
        const uint4 a1 = *reinterpret_cast<const uint4*>(&s_q[rr][wq + 4]);
        const uint32_t a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          acc[i][0] = __builtin_amdgcn_sad_u8(a[i], e.x, acc[i][0]);
          acc[i][1] = __builtin_amdgcn_sad_u8(a[i], e.y, acc[i][1]);
          acc[i][2] = __builtin_amdgcn_sad_u8(a[i], e.z, acc[i][2]);
          acc[i][3] = __builtin_amdgcn_sad_u8(a[i], e.w, acc[i][3]);
        }
      }
    }
    // every member's own band (the sweep's thresholds: load_meta / load_meta_grp), its truth left out
    const float l1d = l1q_delta(hdr, 255.0f);
    const float l1f = (float)(kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
    const float l1c = __builtin_fmaf((float)kt * 1.03f, l1d, 0x1p-120f);
    const uint32_t om2 = q_l1c ? 2u * hdr[3] : 0u;
    // The wave's 8 rows x 8 member slots are its 64 lanes: lane l loads slot l % 8 of row l / 8 --
    // the map entry, the member, its threshold and truth, three dependent rounds once for all of
    // them (member after member they were ~20 serial round trips per wave: K3 16 -> 68 us at C2).
    // Then each member's thresholds are broadcast and its band counted over the 64 lanes' columns.
    const int mi = lane >> 3, ms = lane & 7;
    const int64_t mrow = row0 + mi;
    int64_t mq = -1;
    float rc = l1c;
    if (mrow < n_r) {
      const int cnt = H.row_cnt ? min(H.row_cnt[mrow], 8) : 1;
      if (ms < cnt) mq = H.row_off ? (int64_t)grp_q[(int64_t)H.row_off[mrow] + ms] : mrow;
      if ((uint64_t)mq >= (uint64_t)n_query) mq = -1;
      if (q_l1c) rc = q_l1c[mrow] + 0x1p-120f;
    }
    uint32_t m_ts = 0u, m_tw = 0u;
    int m_tr = -1;  // the truth's column of the slice (or outside it)
    if (mq >= 0) {
      l1_int_thresholds(thr[mq], rc, l1d, l1f, om2, m_ts, m_tw);
      const int64_t t = (int64_t)qtrue[mq] - H.e_base;
      m_tr = t >= 0 && t < n_slice ? (int)t : -1;
    }
    const int ci = (int)c;  // (columns are int32 ids: the entry point's check)
    uint32_t mine = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const uint32_t tw = (uint32_t)__builtin_amdgcn_readlane((int)m_tw, i * 8 + s);
        if (tw == 0u) continue;  // uniform: no member, or no band
        const uint32_t ts = (uint32_t)__builtin_amdgcn_readlane((int)m_ts, i * 8 + s);
        const int tr = __builtin_amdgcn_readlane(m_tr, i * 8 + s);
        uint32_t und = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          und += (uint32_t)__builtin_popcountll(
              __ballot((acc[i][j] - ts < tw) & ((int64_t)ci + j < n_slice) & (ci + j != tr)));
        if (lane == i * 8 + s) mine = und;
      }
    }
    if (mq >= 0) H.flags[mq] = mine >= H.min_count ? 1 : 0;
    return;
  }
  if ((int)blockIdx.x < n_cblk) {
    // the wave's own LDS slices: written and read by the same wave (wave barriers, no block sync)
    __shared__ __attribute__((aligned(16))) int32_t s_id[4][64];
    __shared__ __attribute__((aligned(16))) float s_v[4][64];
    for (int64_t g = (int64_t)blockIdx.x * 4 + wv; g < n_groups; g += (int64_t)n_cblk * 4) {
      const int64_t qa = grp_qoff[g], qb = grp_qoff[g + 1];
      const int64_t la = off[g], lb = off[g + 1];
      for (int64_t qc = qa; qc < qb; qc += 64) {
        const int64_t qi = qc + lane;
        const bool active = qi < qb;
        const int64_t q = active ? grp_q[qi] : 0;
        const int32_t tr = active ? qtrue[q] : -1;
        const float th = active ? thr[q] : 0.0f;
        int c = 0;
        for (int64_t lc = la; lc < lb; lc += 64) {
          const int nl = (int)((lb - lc) < 64 ? (lb - lc) : 64);
          int32_t id = -1;
          float v = 0.0f;
          if (lane < nl) {
            const int64_t j = ids[lc + lane];
            if (j >= 0 && j < n_ent) {
              id = (int32_t)j;
              v = list_v[lc + lane];
            }
          }
          __builtin_amdgcn_wave_barrier();  // the previous round's reads are done
          s_id[wv][lane] = id;  // entries nl..63 stay invalid: the loop below reads whole quads
          s_v[wv][lane] = v;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          if (active) {
            for (int i = 0; i < nl; i += 4) {  // branch-free, 4 entries per LDS read
              const int4 e = *reinterpret_cast<const int4*>(&s_id[wv][i]);
              const float4 vv = *reinterpret_cast<const float4*>(&s_v[wv][i]);
              c += ((e.x >= 0) & (e.x != tr) & (vv.x < th)) + ((e.y >= 0) & (e.y != tr) & (vv.y < th)) +
                   ((e.z >= 0) & (e.z != tr) & (vv.z < th)) + ((e.w >= 0) & (e.w != tr) & (vv.w < th));
            }
          }
        }
        if (active) {
          counts[0 * n_query + q] = 0;
          counts[1 * n_query + q] = -c;
          counts[2 * n_query + q] = 0;
          counts[3 * n_query + q] = 0;
        }
      }
    }
    return;
  }
  // ---- the probe
  const uint32_t w = __builtin_amdgcn_readfirstlane(hdr[1]);
  if (force_bits != 0) {
    if (force_bits == 16 && w != L1Q_F32 && blockIdx.x == (unsigned)n_cblk && tid == 0) hdr[1] = L1Q_CODES16;
    return;
  }
  if (w != L1Q_CODES8) return;  // the f32 fallback: no codes to probe
  const int pb = ((int)blockIdx.x - n_cblk) * 4 + wv, n_pb = n_pblk * 4;
  const int64_t q = (int64_t)pb * n_query / n_pb;
  // the same sampled queries as the separate path's probe; their codes and error sums sit in
  // their sweep row's column (row_of_q: the grouped planes)
  const int64_t qc = row_of_q ? (int64_t)row_of_q[q] : q;
  const int64_t span = n_slice > L1Q_PROBE_E ? n_slice - L1Q_PROBE_E : 0;
  const int64_t c = (((int64_t)pb * span / n_pb) & ~(int64_t)3) + 4 * lane;
  const float l1d = l1q_delta(hdr, 255.0f);
  const float l1f = (float)(kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
  const float l1c = __builtin_fmaf((float)kt * 1.03f, l1d, 0x1p-120f);
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  if (c < n_slice) {
#pragma unroll 8
    for (int r = 0; r < kw; ++r) {
      const uint32_t a = uq[(int64_t)r * q_pad + qc];
      const uint4 e = *reinterpret_cast<const uint4*>(ue + (int64_t)r * e_pad + c);
      acc[0] = __builtin_amdgcn_sad_u8(a, e.x, acc[0]);
      acc[1] = __builtin_amdgcn_sad_u8(a, e.y, acc[1]);
      acc[2] = __builtin_amdgcn_sad_u8(a, e.z, acc[2]);
      acc[3] = __builtin_amdgcn_sad_u8(a, e.w, acc[3]);
    }
  }
  uint32_t t_sure, t_span;
  l1_int_thresholds(thr[q], (q_l1c ? q_l1c[qc] : l1c) + (q_l1c ? 0x1p-120f : 0.0f), l1d, l1f, q_l1c ? 2u * hdr[3] : 0u,
                    t_sure, t_span);
  uint32_t und = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) und += (uint32_t)((acc[j] - t_sure < t_span) & (c + j < n_slice));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) und += __shfl_xor(und, o);
  __shared__ uint32_t s_und[4];
  __shared__ uint32_t s_last;
  if (lane == 0) s_und[wv] = und;
  __syncthreads();
  if (tid == 0) {  // the block's count, then the ticket (the hand-off of K1's table row 1: atomics, vmcnt(0))
    const uint32_t bu = (s_und[0] + s_und[1]) + (s_und[2] + s_und[3]);
    if (bu) __hip_atomic_fetch_add(hdr + 2, bu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(&ticket[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             (uint32_t)n_pblk - 1;
  }
  __syncthreads();
  if (s_last && tid == 0) {
    const uint32_t total = __hip_atomic_load(hdr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (total > probe_max) hdr[1] = L1Q_CODES16;
    ticket[1] = 0u;
  }
}

}  // namespace mmre

using namespace mmre;

extern "C" int64_t mmre_link_k(int model, int dim) { return (int64_t)n_planes(model) * plane_rows(model, dim); }
extern "C" int64_t mmre_link_pad(int64_t n) { return round_up(n > 0 ? n : 1, 128); }

struct Carver {  // carves consecutive regions out of a workspace; a NULL base only adds the sizes up
  char* base;
  int64_t off = 0;
  template <class T>
  T* take(int64_t bytes) {
    off += bytes;
    return base ? reinterpret_cast<T*>(base + off - bytes) : nullptr;
  }
};

extern "C" int mmre_link_prepare_entities(int model, int norm_flag, const float* d_ent, const float* d_ent_im,
                                          int64_t n_ent, int dim, float* d_ent_km, int64_t e_pad, float* d_ent_rows,
                                          void* stream) {
  if (!valid_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent || !d_ent_km || !d_ent_rows || n_ent <= 0 || dim <= 0 || e_pad < n_ent || e_pad % TE) return MMRE_ERR_ARG;
  if (model == MMRE_COMPLEX && !d_ent_im) return MMRE_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int kp = plane_rows(model, dim), kt = n_planes(model) * kp;
  const int rb = stage_rows(kt);
  const size_t lds = sizeof(float) * (size_t)rb * (kt + 1);
  if (lds > 64 * 1024) return MMRE_ERR_SHAPE;
  hipLaunchKernelGGL(k_prep_rows, dim3((unsigned)((e_pad + rb - 1) / rb)), dim3(256), lds, st, model, norm_flag, d_ent,
                     d_ent_im, n_ent, dim, kp, rb, d_ent_km, e_pad, d_ent_rows, kt);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_link_prepare_queries(int model, int norm_flag, const float* d_ent_rows, const float* d_rel,
                                         const float* d_rel_im, int64_t n_ent, int64_t n_rel, int dim,
                                         float phase_denom, const int64_t* d_qh, const int64_t* d_qr,
                                         const int64_t* d_qt, const int8_t* d_qmode, int64_t n_query,
                                         float* d_q_km, int64_t q_pad, int32_t* d_q_true, float* d_rel_work,
                                         float* d_q_rows, void* stream) {
  if (!valid_model(model)) return MMRE_ERR_MODEL;
  if (!d_ent_rows || !d_rel || !d_qh || !d_qr || !d_qt || !d_qmode || !d_q_km || !d_q_true) return MMRE_ERR_ARG;
  if (n_query <= 0 || q_pad < n_query || q_pad % TQ || dim <= 0 || n_ent <= 0 || n_rel <= 0) return MMRE_ERR_ARG;
  if (model == MMRE_COMPLEX && !d_rel_im) return MMRE_ERR_ARG;
  if (model == MMRE_ROTATE && !(phase_denom != 0.0f)) return MMRE_ERR_ARG;
  const bool transe = model == MMRE_TRANSE_L1 || model == MMRE_TRANSE_L2;
  if (transe && norm_flag && !d_rel_work) return MMRE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = plane_rows(model, dim), kt = n_planes(model) * kp;
  // TransE norm_flag: each query block normalises its relation rows itself (no separate
  // relation-prep launch; d_rel_work stays part of the ABI as caller-provided scratch)
  const int rel_norm = (transe && norm_flag) ? 1 : 0;
  const int rb = stage_rows(kt);
  const size_t lds = sizeof(float) * (size_t)rb * (kt + 1);
  if (lds > 64 * 1024) return MMRE_ERR_SHAPE;
  hipLaunchKernelGGL(k_prep_queries, dim3((unsigned)((q_pad + rb - 1) / rb)), dim3(256), lds, st, model, d_ent_rows,
                     d_rel, d_rel_im, dim, kp, rb, phase_denom, d_qh, d_qr, d_qt, d_qmode, n_query, d_q_km, q_pad,
                     d_q_true, d_q_rows, rel_norm);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_link_truth_grouped(int model, int pred_kind, float margin, const float* d_ent_rows, int64_t n_ent,
                                       const float* d_q_rows, const int32_t* d_q_true, const int64_t* d_qr,
                                       const int8_t* d_qmode, int64_t n_query, int dim, const int64_t* d_grp_qoff,
                                       const int32_t* d_grp_q, int64_t n_groups, const int64_t* d_filt_off,
                                       const int32_t* d_filt_ids, const int32_t* d_entry_q, int64_t n_entries,
                                       const uint32_t* d_type_head, const uint32_t* d_type_tail,
                                       float* d_list_scores, int32_t* d_counts, float* d_truth, void* stream) {
  if (!valid_model(model)) return MMRE_ERR_MODEL;
  if (pred_kind < 0 || pred_kind > 4) return MMRE_ERR_ARG;
  if (!d_ent_rows || !d_q_rows || !d_q_true || !d_qr || !d_qmode || !d_counts || !d_truth) return MMRE_ERR_ARG;
  if (!d_grp_qoff || !d_grp_q || !d_filt_off) return MMRE_ERR_ARG;
  if (n_query <= 0 || n_ent <= 0 || dim <= 0 || n_groups <= 0 || n_groups > n_query || n_entries < 0)
    return MMRE_ERR_ARG;
  if (n_entries > 0 && (!d_filt_ids || !d_entry_q || !d_list_scores)) return MMRE_ERR_WORKSPACE;
  if ((d_type_head == nullptr) != (d_type_tail == nullptr)) return MMRE_ERR_ARG;
  if (n_ent >= (int64_t)INT32_MAX || n_query >= (int64_t)INT32_MAX) return MMRE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int kp = plane_rows(model, dim);
  const int64_t tasks = n_query + n_entries;  // k_filter_scores: a thread per truth and per list entry
  with_op(op_of_model(model), [&](auto op_) {
    hipLaunchKernelGGL((k_filter_scores<decltype(op_)::value>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st,
                       d_ent_rows, n_ent, d_q_rows, kp, d_q_true, n_query, pred_kind, margin, d_entry_q, d_filt_ids,
                       n_entries, d_truth, d_list_scores);
    return MMRE_OK;
  });
  MMRE_CHECK_LAUNCH();
  const unsigned blocks = (unsigned)(n_groups < (1 << 20) ? n_groups : (1 << 20));
  hipLaunchKernelGGL(k_filter_count, dim3(blocks), dim3(64), 0, st, d_grp_qoff, d_grp_q, n_groups, d_filt_off,
                     d_filt_ids, d_list_scores, d_q_true, d_truth, d_qr, d_qmode, n_query, n_ent, d_type_head,
                     d_type_tail, (n_ent + 31) / 32, d_counts);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_link_truth(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                               int64_t e_pad, const float* d_ent_rows, const float* d_q_km, const int32_t* d_q_true,
                               const int64_t* d_qr, const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim,
                               const int64_t* d_filt_off, const int32_t* d_filt_ids, const uint32_t* d_type_head,
                               const uint32_t* d_type_tail, int32_t* d_counts, float* d_truth, void* stream) {
  const SweepCall C{nullptr, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin, d_truth, d_q_true, d_qr,
                    d_qmode, d_type_head, d_type_tail, d_counts};
  int rc = check_link_args(model, C, n_ent);
  if (rc) return rc;
  if (!d_ent_rows) return MMRE_ERR_ARG;
  if ((d_filt_off == nullptr) != (d_filt_ids == nullptr)) return MMRE_ERR_ARG;
  const int kp = plane_rows(model, dim);
  rc = with_op(op_of_model(model), [&](auto op_) -> int {
    constexpr int OP = decltype(op_)::value, NP = (OP == 2 || OP == 4) ? 2 : 1;
    const size_t lds = sizeof(float) * (size_t)NP * kp;
    if (lds > 64 * 1024) return MMRE_ERR_SHAPE;
    const unsigned blocks = (unsigned)(n_query < (1 << 20) ? n_query : (1 << 20));
    hipLaunchKernelGGL((k_truth_filter<OP>), dim3(blocks), dim3(FT), lds, (hipStream_t)stream, d_ent_rows, n_ent,
                       d_q_km, q_pad, kp, nullptr, d_q_true, d_qr, d_qmode, n_query, pred_kind, margin, nullptr, nullptr,
                       n_query, d_filt_off, d_filt_ids, d_type_head, d_type_tail, (n_ent + 31) / 32, d_truth, d_counts);
    return MMRE_OK;
  });
  if (rc) return rc;
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

// mmre_link_sweep / mmre_link_sweep_range: the exact sweep of the model's own planes.
static int sweep_impl(int model, SweepCall C, int64_t n_ent, int64_t e_begin, int64_t e_end, int dim) {
  if (int rc = check_link_args(model, C, n_ent); rc) return rc;
  const int k = mfma_model(model) ? (int)mmre_link_k(model, dim) : plane_rows(model, dim);
  if (int rc = sweep_slice(C, n_ent, e_begin, e_end, k); rc) return rc;
  if (C.scores && (e_begin != 0 || e_end != n_ent)) return MMRE_ERR_ARG;  // score rows are whole-table
  return with_op(op_of_model(model), [&](auto op_) -> int {
    constexpr int OP = decltype(op_)::value;
    if constexpr (OP <= 2) return launch_valu<OP>(C);
    else return launch_mfma(C, nullptr, true);
  });
}

extern "C" int mmre_link_sweep(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                               int64_t e_pad, const float* d_q_km, const int32_t* d_q_true, const int64_t* d_qr,
                               const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim,
                               const uint32_t* d_type_head, const uint32_t* d_type_tail, int32_t* d_counts,
                               const float* d_truth, float* d_scores, void* stream) {
  if (n_ent <= 0) return MMRE_ERR_ARG;
  return sweep_impl(model, {(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin, d_truth,
                            d_q_true, d_qr, d_qmode, d_type_head, d_type_tail, d_counts, d_scores}, n_ent, 0, n_ent,
                    dim);
}

extern "C" int mmre_link_sweep_range(int model, int pred_kind, float margin, const float* d_ent_km, int64_t n_ent,
                                     int64_t e_pad, int64_t e_begin, int64_t e_end, const float* d_q_km,
                                     const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode,
                                     int64_t n_query, int64_t q_pad, int dim, const uint32_t* d_type_head,
                                     const uint32_t* d_type_tail, int32_t* d_counts, const float* d_truth,
                                     void* stream) {
  return sweep_impl(model, {(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin, d_truth,
                            d_q_true, d_qr, d_qmode, d_type_head, d_type_tail, d_counts, nullptr}, n_ent, e_begin,
                    e_end, dim);
}

// ------------------------------------------------ the TransE L1 integer filter ---
// The L1Q workspace: header | 16-bit code planes, queries then entities (k2 rows of q_pad / e_pad
// words) | 8-bit code planes (k4 rows) | the tight bound's error sums (q_pad floats).
struct L1QWork {
  int k2, k4;
  uint32_t *hdr, *uq, *ue, *vq, *ve;
  float* q_l1c;
};
static int64_t l1q_layout(L1QWork& W, int dim, int64_t e_pad, int64_t q_pad, void* base) {
  Carver w{(char*)base};
  W.k2 = l1q_rows(dim);
  W.k4 = l1q_rows8(dim);
  W.hdr = w.take<uint32_t>(L1Q_HDR);
  W.uq = w.take<uint32_t>(4 * (int64_t)W.k2 * q_pad);
  W.ue = w.take<uint32_t>(4 * (int64_t)W.k2 * e_pad);
  W.vq = w.take<uint32_t>(4 * (int64_t)W.k4 * q_pad);
  W.ve = w.take<uint32_t>(4 * (int64_t)W.k4 * e_pad);
  W.q_l1c = w.take<float>(4 * q_pad);
  return w.off;
}

extern "C" int64_t mmre_link_l1q_workspace(int dim, int64_t e_pad, int64_t q_pad) {
  if (dim <= 0 || e_pad <= 0 || q_pad <= 0) return 0;
  L1QWork W;
  return l1q_layout(W, dim, e_pad, q_pad, nullptr);
}

extern "C" int mmre_link_l1q_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream) {
  if (!d_work || !d_out || work_bytes < L1Q_HDR) return MMRE_ERR_ARG;
  hipLaunchKernelGGL(k_l1q_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)d_work,
                     (unsigned long long*)d_out);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

static float l1q_ratio() {  // fallback ratio M / mean|x| (MMRE_L1Q_RATIO: experiments; <= 0 forces the fallback)
  static const char* env = getenv("MMRE_L1Q_RATIO");
  return env ? (float)atof(env) : 128.0f;
}
// code width (MMRE_L1_BITS: experiments and tests, read per call): 8 / 16 forces it, otherwise the
// 8-bit codes unless the probe finds their band too wide for this data
static int l1q_bits() {
  const char* env = getenv("MMRE_L1_BITS");
  return env ? atoi(env) : 0;
}
// (C: the f32 call; TransE L1 has one plane, kt = kp)
static L1Q l1q_operands(const L1QWork& W, const SweepCall& C, const float* q_rows, const float* ent_rows, bool tight,
                        uint32_t* und_q) {
  L1Q l1{q_rows, ent_rows, W.hdr, (unsigned long long*)((char*)W.hdr + 256), C.q, C.ent, C.kp,
         C.kp, nullptr, tight ? W.q_l1c : nullptr, W.hdr + 4, und_q};
  l1.wq = l1q_work_counters(W.hdr);
  return l1;
}

extern "C" int mmre_link_sweep_l1q(int pred_kind, float margin, const float* d_ent_km, const float* d_ent_rows,
                                   int64_t n_ent, int64_t e_pad, int64_t e_begin, int64_t e_end, const float* d_q_km,
                                   const float* d_q_rows, const int32_t* d_q_true, const int64_t* d_qr,
                                   const int8_t* d_qmode, int64_t n_query, int64_t q_pad, int dim,
                                   const uint32_t* d_type_head, const uint32_t* d_type_tail, int32_t* d_counts,
                                   const float* d_truth, void* d_work, int64_t work_bytes, void* stream) {
  SweepCall C{(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin, d_truth,
              d_q_true, d_qr, d_qmode, d_type_head, d_type_tail, d_counts};
  if (int rc = check_link_args(MMRE_TRANSE_L1, C, n_ent); rc) return rc;
  L1QWork W;
  if (!d_ent_rows || !d_q_rows || !d_work || work_bytes < mmre_link_l1q_workspace(dim, e_pad, q_pad))
    return MMRE_ERR_WORKSPACE;
  l1q_layout(W, dim, e_pad, q_pad, d_work);
  const int kp = plane_rows(MMRE_TRANSE_L1, dim), kt = n_planes(MMRE_TRANSE_L1) * kp;
  if (int rc = sweep_slice(C, n_ent, e_begin, e_end, kp); rc) return rc;
  hipStream_t st = C.st;
  const float ratio = l1q_ratio();
  const int n_abs = std::min(kp * 8, L1Q_MAX_BLOCKS);
  const double n_elem = (double)kp * (double)(q_pad + C.e_cols);
  const int bits = l1q_bits();
  hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(256), 0, st, W.hdr, L1Q_PART / 4);
  hipLaunchKernelGGL(k_l1q_absmax, dim3((unsigned)n_abs), dim3(256), 0, st, d_q_km, q_pad, C.ent, e_pad, C.e_cols, kp,
                     W.hdr);
  const L1QPlane p8q{d_q_km, q_pad, 0, q_pad, W.vq}, p8e{d_ent_km, e_pad, e_begin, C.e_cols, W.ve};
  const L1QPlane p16q{d_q_km, q_pad, 0, q_pad, W.uq}, p16e{d_ent_km, e_pad, e_begin, C.e_cols, W.ue};
  // the tight per-pair bound (k_l1q_quant8): prediction = the score, no type masks (their sweep
  // keeps the uniform bound), and error offsets that fit one code row (kt <= 1984);
  // MMRE_L1_TIGHT=0 keeps the uniform bound (A/B; read per call: tests switch it)
  const char* tight_env = getenv("MMRE_L1_TIGHT");
  const bool tight = pred_kind == 0 && d_type_head == nullptr && kt <= 1984 && !(tight_env && tight_env[0] == '0');
  if (bits != 16)
    with_bool(tight, [&](auto tight_) {
      hipLaunchKernelGGL(k_l1q_quant8<decltype(tight_)::value>, dim3(2048, 2), dim3(256), 0, st, p8q, p8e, kp, W.k4, kt,
                         W.hdr, n_abs, n_elem, ratio, W.q_l1c);
      return MMRE_OK;
    });
  if (bits == 0)
    hipLaunchKernelGGL(k_l1q_probe, dim3(L1Q_PROBE_Q), dim3(L1Q_PROBE_E / 4), 0, st, W.vq, q_pad, n_query,
                       W.ve + e_begin, e_pad, C.n_slice, W.k4, kt, d_truth, pred_kind, margin, W.hdr,
                       tight ? W.q_l1c : nullptr);
  if (bits == 0 || bits == 16)  // after the probe: it decides whether these codes count
    hipLaunchKernelGGL(k_l1q_quant<16>, dim3(1024, 2), dim3(256), 0, st, p16q, p16e, kp, W.k2, W.hdr, n_abs, n_elem,
                       ratio, bits == 0 ? 1 : 0, bits == 0 ? l1q_probe_max(C.n_slice) : 0u);
  MMRE_CHECK_LAUNCH();
  const L1Q l1 = l1q_operands(W, C, d_q_rows, d_ent_rows, tight, nullptr);
  // the gated sweeps: the one the code-width word names counts, the others' workgroups leave
  int rc = bits != 16 ? launch_valu<6>(planes(C, W.ve, W.vq, W.k4), l1, false) : MMRE_OK;
  if (rc) return rc;
  // after the 8-bit sweep the 16-bit one rarely counts: gated at its top (one flag load per
  // workgroup, 4 workgroups per resident slot) like the f32 fallback below
  L1Q l16 = l1;
  if (bits == 0) l16.gate = W.hdr + 1;
  if (bits != 8 && (rc = launch_valu<5>(planes(C, W.ue, W.uq, W.k2), l16, false))) return rc;
  // the fallback: the exact f32 sweep of the float planes, gated on the flag k_l1q_quant wrote
  // (its workgroups return at once when the codes were used)
  L1Q gate{};
  gate.gate = W.hdr + 1;
  return launch_valu<0>(C, gate, true);
}

// ------------------------------------------------------ split-bf16 MFMA filter ---
// The lock-step window QB x EB for P workgroups per XCD group (BlockMap): about 8 query tiles
// (MMRE_BF3_QB) by P / QB entity tiles, evened out so the last window along each axis is not
// mostly empty (C5: P 96, 64 query tiles, 976 entity tiles per group -> 8 x 12; C3: 89 x 12-13
// -> 7 x 13).
static void bf3_window(int P, int n_qt, int m_e, int& q, int& e) {
  static const char* qb_env = getenv("MMRE_BF3_QB");
  q = std::max(1, std::min(qb_env ? atoi(qb_env) : 8, std::min(P, n_qt)));
  e = std::max(1, std::min(P / q, m_e));
  const int ne = (m_e + e - 1) / e;      // windows along the entity tiles, then even them out
  e = (m_e + ne - 1) / ne;
  q = std::max(1, std::min(P / e, n_qt));
  const int nq = (n_qt + q - 1) / q;
  q = (n_qt + nq - 1) / nq;
}

// The grid of k_sweep_bf3 / k_sweep_bf3w over q_tiles x n_tiles units: g_ranges workgroups with
// contiguous unit ranges, or -- blocked, the planes overflow the caches -- one resident wave of
// workgroups (res) stepping through lock-step windows bq x be; the windows are those of the grid
// actually launched (MMRE_SWEEP_GRID: a multiple of 8).
struct Bf3Grid { int g, bq, be; bool blk; };
static Bf3Grid bf3_grid(int g_ranges, int res, bool blocked, int q_tiles, int n_tiles) {
  Bf3Grid G{g_ranges, 0, 0, blocked && n_tiles >= 8 && res % 8 == 0};
  if (G.blk) G.g = res;
  G.g = grid_override(G.g);
  if (G.blk) {
    G.g = std::max(8, G.g & ~7);
    bf3_window(G.g / 8, q_tiles, n_tiles / 8, G.bq, G.be);
  }
  return G;
}

// The split-bf16 workspace (the comment above BF3_HDR), then the wide sweep's padded thresholds and
// bound factors (q_pad floats each) and its 32-column block maxima of |e| (e_pad / 32 floats).
struct Bf3Work {
  int64_t cap;
  uint32_t* hdr;
  int2* pairs;
  uint4 *qb, *eb;
  float *qn, *en, *thr_pad, *qbf, *ebm;
};
static int64_t bf3_layout(Bf3Work& W, int64_t ktot, int64_t e_pad, int64_t q_pad, void* base) {
  Carver w{(char*)base};
  W.cap = bf3_cap(q_pad, e_pad);
  W.hdr = w.take<uint32_t>(BF3_HDR);
  W.pairs = w.take<int2>((8 * W.cap + 15) & ~(int64_t)15);  // (an odd MMRE_BF3_CAP: the planes stay 16-B aligned)
  W.qn = w.take<float>(4 * q_pad);
  W.en = w.take<float>(4 * e_pad);
  W.qb = w.take<uint4>(4 * ktot * q_pad);
  W.eb = w.take<uint4>(4 * ktot * e_pad);
  W.thr_pad = w.take<float>(4 * q_pad);
  W.qbf = w.take<float>(4 * q_pad);
  W.ebm = w.take<float>(4 * (e_pad / 32));
  return w.off;
}

extern "C" int64_t mmre_link_bf3_workspace(int model, int dim, int64_t e_pad, int64_t q_pad) {
  if (!mfma_model(model) || dim <= 0 || e_pad <= 0 || q_pad <= 0) return 0;
  Bf3Work W;
  return bf3_layout(W, (int64_t)n_planes(model) * plane_rows(model, dim), e_pad, q_pad, nullptr);
}

extern "C" int mmre_link_bf3_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream) {
  if (!d_work || !d_out || work_bytes < BF3_HDR) return MMRE_ERR_ARG;
  hipLaunchKernelGGL(k_bf3_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)d_work,
                     (unsigned long long*)d_out);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

// The wide sweep's launch (prediction -S only): a persistent grid of resident workgroups, the
// lock-step windows where the planes overflow the caches (as k_sweep_bf3's), else contiguous
// unit ranges.
template <int QT>
static Bf3Grid grid_bf3w(const SweepCall& C, bool blocked) {
  using G = W3Geom<QT>;
  const int n_etw = (int)((C.n_slice + W3E - 1) / W3E);
  const int res = resident_groups((const void*)k_sweep_bf3w<2, QT, true>, G::NT);
  const int64_t units = (C.q_pad / QT) * (int64_t)n_etw;
  const int g_ranges = (int)std::min<int64_t>(8LL * res, std::max<int64_t>((int64_t)res, units / 16)) & ~7;
  return bf3_grid(g_ranges, res, blocked, (int)(C.q_pad / QT), n_etw);
}
template <int QT>
static void launch_bf3w(const SweepCall& C, const Bf3Work& W, int nkb, int emajor, const Bf3Grid& B) {
  using G = W3Geom<QT>;
  const int n_etw = (int)((C.n_slice + W3E - 1) / W3E);
  const int g = std::max(1, B.g);
  with_bool(B.blk, [&](auto blk_) {
    hipLaunchKernelGGL((k_sweep_bf3w<2, QT, decltype(blk_)::value>), dim3((unsigned)g), dim3(G::NT), 0, C.st, W.eb,
                       C.e_pad, C.e_cols, C.n_slice, W.qb, C.q_pad, C.n_query, nkb, n_etw, C.e_base,
                       xcd_groups(g, n_etw), W.thr_pad, W.qbf, W.ebm, C.counts, W.hdr, W.pairs, W.cap, emajor, B.bq,
                       B.be);
    return MMRE_OK;
  });
}

// The 128 x 128 sweep's launch: whole rounds of the resident capacity, ~3 units per workgroup --
// static ranges of ~12 units left the list-heavy units' workgroups last (C3, 8,900 units at 768
// resident: 4 rounds 0.454 ms against 0.479 for one, profiles/r6) -- or the lock-step windows.
template <int PK>
static Bf3Grid grid_bf3(const SweepCall& C, bool blocked) {
  const int res = resident_groups((const void*)k_sweep_bf3<PK>, NT);
  const int64_t units = C.q_tiles() * (int64_t)C.n_et;
  const int64_t rounds = std::max<int64_t>(1, std::min<int64_t>(8, units / (3LL * res)));
  return bf3_grid((int)(rounds * res) & ~7, res, blocked, (int)C.q_tiles(), C.n_et);
}
template <int PK>
static void launch_bf3(const SweepCall& C, const Bf3Work& W, int nkb, float cb, int emajor, const Bf3Grid& B) {
  hipLaunchKernelGGL((k_sweep_bf3<PK>), dim3((unsigned)B.g), dim3(NT), 0, C.st, W.eb, C.e_pad, C.n_slice, W.qb, C.q_pad,
                     C.n_query, nkb, C.n_et, C.e_base, xcd_groups(B.g, C.n_et), C.pred_kind, C.margin, C.truth, W.qn,
                     W.en, cb, C.counts, W.hdr, W.pairs, W.cap, emajor, B.bq, B.be);
}

// mmre_link_sweep_bf3 / _rows. rows_src: the entity split planes, norms and block maxima come from
// the row-major table d_ent_rows in one pass (k_bf3_split_rows), and d_ent_km is written only by
// the gated overflow fallback, right before the exact f32 sweep that reads it.
static int sweep_bf3_impl(int model, SweepCall C, float* d_ent_km, const float* d_ent_rows, const float* d_q_rows,
                          int64_t n_ent, int64_t e_begin, int64_t e_end, int dim, void* d_work, int64_t work_bytes,
                          bool rows_src) {
  if (!mfma_model(model)) return MMRE_ERR_MODEL;
  if (int rc = check_link_args(model, C, n_ent); rc) return rc;
  const int64_t e_pad = C.e_pad, q_pad = C.q_pad;
  if (!d_ent_rows || !d_q_rows || !d_work || work_bytes < mmre_link_bf3_workspace(model, dim, e_pad, q_pad))
    return MMRE_ERR_WORKSPACE;
  const int kp = plane_rows(model, dim);
  const int ktot = n_planes(model) * kp;  // a multiple of 16 (plane_rows)
  if (int rc = sweep_slice(C, n_ent, e_begin, e_end, ktot); rc) return rc;
  C.qr = nullptr, C.qmode = nullptr, C.tw = 0;  // no type masks: the fallback's f32 sweep is passed none of these
  hipStream_t st = C.st;
  Bf3Work W;
  bf3_layout(W, ktot, e_pad, q_pad, d_work);
  // bound coefficient (see k_sweep_bf3's header): 1.02 (7K 2^-24 (1 + 2^-7) + 3.02 2^-16 + 2^-29 sqrt K)
  const double K = (double)ktot;
  const float cb = (float)(1.02 * (7.0 * K * std::ldexp(1.0, -24) * (1.0 + std::ldexp(1.0, -7)) +
                                   3.02 * std::ldexp(1.0, -16) + std::ldexp(1.0, -29) * std::sqrt(K)));
  static_assert(BF3_SEGS == 64, "k_bf3_stats sums one segment per lane of a wave");
  const int emajor = mfma_emajor(e_pad, ktot);
  // the wide sweep (k_sweep_bf3w, prediction -S) where the planes overflow the caches (C5: 15.9
  // -> 14.5 ms per evaluation); on cache-resident planes the 128 x 128 one is faster (C3: 0.74 vs
  // 0.86-0.88 ms -- its per-pair bound lists fewer pairs than the wide sweep's per-tile one on
  // trained tables, whose norms vary); MMRE_BF3_WIDE=1 / 0 forces either (tests, A/B)
  const char* wide_env = getenv("MMRE_BF3_WIDE");  // read per call: tests switch it
  const bool wide = C.pred_kind == 2 && (wide_env ? wide_env[0] != '0' : emajor != 0);
  const char* qt_env = getenv("MMRE_BF3_QT");  // the wide sweep's query tile, 256 or 128
  const int wide_qt = !wide ? 0 : (q_pad % 256 == 0 && (qt_env ? atoi(qt_env) : 256) == 256) ? 256 : 128;
  // the lock-step windows pay where the planes overflow the caches (C5, 1 GB: 16.45 -> 16.24 ms);
  // on planes that stay L2 / MALL resident the contiguous ranges are faster (C3, 20 MB: 0.75 vs
  // 0.85 ms, profiles/r5) -- the emajor threshold; MMRE_BF3_BLOCKED=0 / 1 forces either (tests, A/B)
  const char* blk_env = getenv("MMRE_BF3_BLOCKED");  // read per call, as MMRE_BF3_WIDE
  const bool blocked = blk_env ? blk_env[0] != '0' : emajor != 0;
  // the sweep's grid, decided here so that the header records the path as launched (word 5)
  const Bf3Grid B = wide_qt == 256   ? grid_bf3w<256>(C, blocked)
                    : wide_qt == 128 ? grid_bf3w<128>(C, blocked)
                    : C.pred_kind == 2 ? grid_bf3<2>(C, blocked)
                                       : grid_bf3<-1>(C, blocked);
  hipLaunchKernelGGL(k_bf3_hdr_init, dim3((BF3_HDR / 4 + 255) / 256), dim3(256), 0, st, W.hdr, W.cap,
                     (uint32_t)wide_qt | (B.blk ? 1u << 16 : 0u));
  const int nkb = ktot / 16;
  hipLaunchKernelGGL(k_bf3_split, dim3((unsigned)((q_pad * nkb + 255) / 256)), dim3(256), 0, st, C.q, q_pad,
                     (int64_t)0, q_pad, nkb, W.qb, q_pad);
  if (!rows_src)
    hipLaunchKernelGGL(k_bf3_split, dim3((unsigned)((C.e_cols * nkb + 255) / 256)), dim3(256), 0, st, d_ent_km, e_pad,
                       e_begin, C.e_cols, nkb, W.eb, e_pad);
  hipLaunchKernelGGL(k_bf3_norms, dim3((unsigned)((q_pad + 3) / 4)), dim3(256), 0, st, d_q_rows, C.n_query, (int64_t)0,
                     q_pad, ktot, W.qn, C.truth, wide ? W.thr_pad : nullptr, W.qbf, cb);
  if (rows_src)  // split planes, norms and block maxima in one read of the rows (e_cols: whole tiles)
    hipLaunchKernelGGL(k_bf3_split_rows, dim3((unsigned)(C.e_cols / 32)), dim3(256), 0, st, d_ent_rows, n_ent, e_begin,
                       ktot, W.eb, e_pad, W.en, wide ? W.ebm : nullptr);
  else if (wide)
    hipLaunchKernelGGL(k_bf3_enorms, dim3((unsigned)((C.e_cols + 31) / 32)), dim3(256), 0, st, d_ent_rows, n_ent,
                       e_begin, C.e_cols, ktot, W.en, W.ebm);
  else
    hipLaunchKernelGGL(k_bf3_norms, dim3((unsigned)((C.e_cols + 3) / 4)), dim3(256), 0, st, d_ent_rows, n_ent, e_begin,
                       C.e_cols, ktot, W.en, nullptr, nullptr, nullptr, 0.0f);
  MMRE_CHECK_LAUNCH();
  return with_bool(C.pred_kind == 2, [&](auto fast_) -> int {
    constexpr int PK = decltype(fast_)::value ? 2 : -1;  // -S compiled into the epilogue, or decoded
    if constexpr (PK == 2) {  // (the wide sweep has no other epilogue)
      if (!wide) launch_bf3<PK>(C, W, nkb, cb, emajor, B);
      else if (wide_qt == 256) launch_bf3w<256>(C, W, nkb, emajor, B);
      else launch_bf3w<128>(C, W, nkb, emajor, B);
    } else {
      launch_bf3<PK>(C, W, nkb, cb, emajor, B);
    }
    MMRE_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_bf3_fallback_zero), dim3((unsigned)((C.n_query + 255) / 256)), dim3(256), 0, st, W.hdr,
                       C.counts, C.n_query);
    if (rows_src) {  // the fallback's k-major planes, only when it runs
      const int rb = stage_rows(ktot);
      hipLaunchKernelGGL(k_prep_km_gated, dim3((unsigned)((C.e_cols + rb - 1) / rb)), dim3(256),
                         sizeof(float) * (size_t)rb * (ktot + 1), st, W.hdr + 1, model,
                         d_ent_rows + e_begin * (int64_t)ktot, C.n_slice, dim, kp, rb, d_ent_km + e_begin, e_pad);
    }
    const int r = launch_mfma(C, W.hdr + 1, false);  // the exact sweep, gated on the overflow flag
    if (r) return r;
    hipLaunchKernelGGL((k_bf3_rescore<PK>), dim3(16 * (BF3_SEGS + 1)), dim3(256), 0, st, W.hdr, W.pairs, W.cap,
                       d_q_rows, d_ent_rows, ktot, C.pred_kind, C.margin, C.truth, C.counts);
    MMRE_CHECK_LAUNCH();
    return launch_finalize(st, C.counts, C.n_query, false);
  });
}

extern "C" int mmre_link_sweep_bf3(int model, int pred_kind, float margin, const float* d_ent_km,
                                   const float* d_ent_rows, int64_t n_ent, int64_t e_pad, int64_t e_begin,
                                   int64_t e_end, const float* d_q_km, const float* d_q_rows,
                                   const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode,
                                   int64_t n_query, int64_t q_pad, int dim, int32_t* d_counts, const float* d_truth,
                                   void* d_work, int64_t work_bytes, void* stream) {
  return sweep_bf3_impl(model, {(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin,
                                d_truth, d_q_true, d_qr, d_qmode, nullptr, nullptr, d_counts},
                        const_cast<float*>(d_ent_km), d_ent_rows, d_q_rows, n_ent, e_begin, e_end, dim, d_work,
                        work_bytes, false);
}

extern "C" int mmre_link_sweep_bf3_rows(int model, int pred_kind, float margin, const float* d_ent_rows,
                                        int64_t n_ent, int64_t e_pad, int64_t e_begin, int64_t e_end,
                                        float* d_ent_km, const float* d_q_km, const float* d_q_rows,
                                        const int32_t* d_q_true, const int64_t* d_qr, const int8_t* d_qmode,
                                        int64_t n_query, int64_t q_pad, int dim, int32_t* d_counts,
                                        const float* d_truth, void* d_work, int64_t work_bytes, void* stream) {
  // the row-major table must be the plane layout itself: DistMult with d a multiple of 16 (K = d)
  if (model != MMRE_DISTMULT || plane_rows(model, dim) != dim) return MMRE_ERR_SHAPE;
  if (!d_ent_rows || !d_ent_km || (reinterpret_cast<uintptr_t>(d_ent_rows) & 15)) return MMRE_ERR_ARG;
  return sweep_bf3_impl(model, {(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, pred_kind, margin,
                                d_truth, d_q_true, d_qr, d_qmode, nullptr, nullptr, d_counts}, d_ent_km, d_ent_rows,
                        d_q_rows, n_ent, e_begin, e_end, dim, d_work, work_bytes, true);
}

// ---------------------------------------- fused TransE L1 evaluation (round 5) ---
// K1's blocks: rb entity rows, or rb / 2 queries with their truth rows (two row sets): the
// same LDS, 16 rows of kt + 1 floats at C2 (12.9 KB)
static int eval_rb(int kp) { return stage_rows(kp); }
static int eval_rbq(int kp) { return std::max(1, eval_rb(kp) / 2); }
// The fused evaluation's workspace: the L1Q workspace | tickets (256 bytes, zero before the first call:
// the caller zeroes the workspace once; words 8-9 the row counts K1's block 0 writes) | K1's per-block
// statistics | the grouped sweep's row map (q_pad each: rows <= queries) and tile_m (per query tile).
struct EvalWork {
  L1QWork q;
  uint32_t* ticket;
  int32_t* n_rows;
  float* pstat;
  int32_t *row_off, *row_cnt, *row_of_q, *tile_m;
};
static int64_t eval_layout(EvalWork& W, int dim, int64_t e_pad, int64_t q_pad, void* base) {
  Carver w{(char*)base, l1q_layout(W.q, dim, e_pad, q_pad, base)};
  const int kp = plane_rows(MMRE_TRANSE_L1, dim);
  const int64_t blocks = (e_pad + eval_rb(kp) - 1) / eval_rb(kp) + (q_pad + eval_rbq(kp) - 1) / eval_rbq(kp);
  W.ticket = w.take<uint32_t>(256);
  W.n_rows = base ? (int32_t*)W.ticket + 8 : nullptr;
  W.pstat = w.take<float>(round_up(8 * blocks, 256));
  W.row_off = w.take<int32_t>(4 * q_pad);
  W.row_cnt = w.take<int32_t>(4 * q_pad);
  W.row_of_q = w.take<int32_t>(4 * q_pad);
  W.tile_m = w.take<int32_t>(round_up(4 * (q_pad / TQ), 256));
  return w.off;
}

extern "C" int64_t mmre_link_evaluate_l1q_workspace(int dim, int64_t e_pad, int64_t q_pad) {
  if (dim <= 0 || e_pad <= 0 || q_pad <= 0) return 0;
  EvalWork W;
  return eval_layout(W, dim, e_pad, q_pad, nullptr);
}

// The per-query route's storage: K1's pstat region, dead once K2 has reduced it (the workspace does
// not grow) -- q_pad flag bytes (K3's probe; then the routed map), then the routed list in what is
// left. The cap: n_query / 16 (at least 1), or what the list holds.
struct RouteStore {
  uint8_t* flags;
  int32_t* list;
  int64_t cap_store, cap;
};
static RouteStore route_store(float* pstat, int dim, int64_t e_pad, int64_t q_pad, int64_t n_query) {
  const int kp = plane_rows(MMRE_TRANSE_L1, dim);
  const int64_t blocks = (e_pad + eval_rb(kp) - 1) / eval_rb(kp) + (q_pad + eval_rbq(kp) - 1) / eval_rbq(kp);
  const int64_t bytes = round_up(8 * blocks, 256);  // eval_layout's
  RouteStore R{(uint8_t*)pstat, (int32_t*)((char*)pstat + q_pad), std::max<int64_t>(0, (bytes - q_pad) / 4), 0};
  R.cap = std::min(R.cap_store, std::max<int64_t>(1, n_query / 16));
  return R;
}
extern "C" int64_t mmre_link_l1q_route_cap(int dim, int64_t e_pad, int64_t q_pad, int64_t n_query) {
  if (dim <= 0 || e_pad <= 0 || q_pad <= 0 || n_query <= 0 || n_query > q_pad || e_pad % TE || q_pad % TQ) return 0;
  return route_store(nullptr, dim, e_pad, q_pad, n_query).cap;
}

extern "C" int mmre_link_l1q_route_stats(const void* d_work, int64_t work_bytes, uint64_t* d_out, void* stream) {
  if (!d_work || !d_out || work_bytes < L1Q_HDR) return MMRE_ERR_ARG;
  hipLaunchKernelGGL(k_l1q_route_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)d_work,
                     (unsigned long long*)d_out);
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

extern "C" int mmre_link_evaluate_l1q(int norm_flag, const float* d_ent, int64_t n_ent, const float* d_rel,
                                      int64_t n_rel, int dim, const int64_t* d_qh, const int64_t* d_qr,
                                      const int64_t* d_qt, const int8_t* d_qmode, int64_t n_query,
                                      const int64_t* d_grp_qoff, const int32_t* d_grp_q, int64_t n_groups,
                                      const int64_t* d_filt_off, const int32_t* d_filt_ids, const int32_t* d_entry_q,
                                      int64_t n_entries, int64_t e_begin, int64_t e_end, float* d_ent_km,
                                      int64_t e_pad, float* d_ent_rows, float* d_q_km, int64_t q_pad, float* d_q_rows,
                                      int32_t* d_q_true, float* d_list_scores, int32_t* d_counts, float* d_truth,
                                      uint32_t* d_undecided_q, void* d_work, int64_t work_bytes, void* stream) {
  if (!d_ent || !d_rel || !d_qh || !d_qr || !d_qt || !d_qmode || !d_ent_km || !d_ent_rows || !d_q_km || !d_q_rows ||
      !d_q_true || !d_counts || !d_truth || !d_grp_qoff || !d_grp_q || !d_filt_off)
    return MMRE_ERR_ARG;
  if (n_ent <= 0 || n_rel <= 0 || dim <= 0 || n_query <= 0 || n_groups <= 0 || n_groups > n_query || n_entries < 0)
    return MMRE_ERR_ARG;
  if (e_pad < n_ent || e_pad % TE || q_pad < n_query || q_pad % TQ) return MMRE_ERR_ARG;
  const int kp = plane_rows(MMRE_TRANSE_L1, dim), kt = kp;
  // the f32 call (prediction = the score, no type masks); the code sweeps run over planes() of it
  SweepCall C{(hipStream_t)stream, d_ent_km, e_pad, d_q_km, q_pad, n_query, 0, 0.0f, d_truth, d_q_true, d_qr, d_qmode};
  C.counts = d_counts;
  if (int rc = sweep_slice(C, n_ent, e_begin, e_end, kp); rc) return rc;
  if (n_entries > 0 && (!d_filt_ids || !d_entry_q || !d_list_scores)) return MMRE_ERR_WORKSPACE;
  if (n_ent > (int64_t)INT32_MAX - 256 || n_query >= (int64_t)INT32_MAX) return MMRE_ERR_SHAPE;
  EvalWork W;
  if (!d_work || work_bytes < eval_layout(W, dim, e_pad, q_pad, d_work)) return MMRE_ERR_WORKSPACE;
  hipStream_t st = C.st;
  const int rb = eval_rb(kp), rbq = eval_rbq(kp);
  const size_t lds1 = sizeof(float) * (size_t)std::max(rb, 3 * rbq) * (kt + 1);
  if (lds1 > 64 * 1024) return MMRE_ERR_SHAPE;
  const L1QWork& WQ = W.q;
  // Grouped or not. The grouped sweep shares a SAD chain among a row's members but pays for it:
  // K1's row-map block and K2's map blocks on every call, a longer unit per row, fewer units.
  // It runs when the rows (bounded from the group count: a group of n members is ceil(n / 8)
  // rows) (a) give every resident workgroup a unit -- a small evaluation is bound by its longest
  // workgroup and by launch latencies, C1 -- and (b) are few enough against the queries
  // (L1Q_GROUP_FRAC, measured: DESIGN.md 4d). Otherwise the call is the ungrouped one: no row
  // map, a column per query, the per-query sweeps. MMRE_GROUP_CAP=1..8 (A/B, tests) forces the
  // grouped sweep with that many members per row at most.
  const char* cap_env = getenv("MMRE_GROUP_CAP");
  int row_cap = cap_env ? std::min(L1Q_GS, std::max(1, atoi(cap_env))) : L1Q_GS;
  if (!cap_env) {
    const int64_t rows8 = std::min<int64_t>(n_query, n_groups + n_query / L1Q_GS);
    if (!valu_grp_fills_grid(rows8, C.n_et) || (double)rows8 > L1Q_GROUP_FRAC * (double)n_query) row_cap = 0;
  }
  const bool grouped = row_cap > 0;
  const int64_t rows_max = grouped ? std::min<int64_t>(n_query, n_groups + n_query / row_cap) : n_query;
  // The grouped sweep's row-tile-affine claims (sweep_valu_body) need 8 x l1q_affine_stride
  // zeroed words per call. The workspace does not grow for them: the row map holds at most
  // rows_max rows, padded to a tile, so the words of row_cnt past that bound are dead (k_eval_prep
  // is held to the bound, every reader to the row count), and the counters are its last words --
  // whole 128-B lines, q_pad and the stride being multiples of 32 words. Where the bound leaves no
  // such tail (a row per query) the sweep keeps the group's sequential counter.
  // MMRE_SWEEP_AFFINE=0: the sequential counter (A/B, tests; read per call).
  const char* aff_env = getenv("MMRE_SWEEP_AFFINE");
  const int64_t aff_words = 8LL * l1q_affine_stride(q_pad), rows_lim = round_up(rows_max, TQ);
  const bool affine = grouped && !(aff_env && aff_env[0] == '0') && q_pad - rows_lim >= aff_words;
  uint32_t* aff = affine ? (uint32_t*)W.row_cnt + (q_pad - aff_words) : nullptr;
  static const char* tight_env = getenv("MMRE_L1_TIGHT");  // (once per process here)
  const int bits = l1q_bits();
  const bool tight = kt <= 1984 && !(tight_env && tight_env[0] == '0');
  EvalL1 P{};
  P.ent = d_ent;
  P.rel = d_rel;
  P.n_ent = n_ent;
  P.dim = dim;
  P.kp = kp;
  P.norm = norm_flag ? 1 : 0;
  P.rb = rb;
  P.rbq = rbq;
  P.qh = d_qh;
  P.qr = d_qr;
  P.qt = d_qt;
  P.qmode = d_qmode;
  P.n_query = n_query;
  P.ent_km = d_ent_km;
  P.e_pad = e_pad;
  P.ent_rows = d_ent_rows;
  P.q_km = d_q_km;
  P.q_pad = q_pad;
  P.q_rows = d_q_rows;
  P.q_true = d_q_true;
  P.truth = d_truth;
  P.e_begin = e_begin;
  P.e_cols = C.e_cols;
  P.n_eblk = (int)((e_pad + rb - 1) / rb);
  P.n_qblk = (int)((q_pad + rbq - 1) / rbq);
  P.pstat = W.pstat;
  P.und_q = d_undecided_q;
  P.ticket = W.ticket;
  P.hdr = WQ.hdr;
  P.n_elem = (double)kp * (double)(q_pad + C.e_cols);
  P.ratio = l1q_ratio();
  P.grp_qoff = d_grp_qoff;
  P.n_groups = n_groups;
  P.row_cap = row_cap;
  P.row_off = W.row_off;
  P.row_cnt = W.row_cnt;
  P.tile_m = W.tile_m;
  P.n_rows = W.n_rows;
  P.row_lim = affine ? rows_lim : q_pad;
  P.aff = aff;
  P.aff_n = affine ? (int)aff_words : 0;
  // K1: the row map (block 0, grouped) | prep + truths + |x| statistics
  hipLaunchKernelGGL(k_eval_prep, dim3((unsigned)((grouped ? 1 : 0) + P.n_eblk + P.n_qblk)), dim3(256), lds1, st, P);
  MMRE_CHECK_LAUNCH();
  // K2: list scores | codes (8-bit words + error row, 16-bit words)
  EvalQuant Q{};
  Q.pq = L1QPlane{d_q_km, q_pad, 0, q_pad, WQ.vq};
  Q.pe = L1QPlane{d_ent_km, e_pad, e_begin, C.e_cols, WQ.ve};
  Q.out16q = WQ.uq;
  Q.out16e = WQ.ue;
  Q.kw = WQ.k4;
  Q.k2 = WQ.k2;
  Q.kt = kt;
  const int n_lblk = (int)((n_entries + 255) / 256);
  // quantization blocks per plane: the list blocks and both planes' blocks resident at once (one
  // round: 2 x 512 + the list blocks took two at an 8-way share of C2, 23 us)
  Q.n_blk = (int)std::min<int64_t>(512, std::max<int64_t>(64, (resident_groups((const void*)k_eval_quant_list, 256) -
                                                              n_lblk) / 2));
  Q.tight = tight ? 1 : 0;
  Q.q_l1c = WQ.q_l1c;  // per sweep row (grouped), per query
  Q.row_off = W.row_off;
  Q.row_cnt = W.row_cnt;
  Q.grp_q = d_grp_q;
  Q.n_rows = grouped ? W.n_rows : nullptr;
  Q.row_of_q = W.row_of_q;
  Q.tile_m = W.tile_m;
  const int n_mblk = grouped ? (int)((rows_max + 255) / 256) : 0;  // the query -> row map, tile_m: a thread per row
  hipLaunchKernelGGL(k_eval_quant_list, dim3((unsigned)(n_lblk + 2 * Q.n_blk + n_mblk)), dim3(256), 0, st, P, Q, d_filt_ids,
                     d_entry_q, n_entries, d_list_scores, n_lblk);
  MMRE_CHECK_LAUNCH();
  // The per-query route: when the sweep's units fill the resident grid -- grouping's
  // own test: a small evaluation is launch-bound, and three more launches cost it more than its
  // rescoring -- and the 8-bit codes may count by the probe's own choice. MMRE_L1_HEAVY=0 / 1: off /
  // on at any size; MMRE_L1_HEAVY_MIN: the sampled-pair count that flags; MMRE_L1_HEAVY_CAP: the
  // list's cap (A/B, tests).
  const RouteStore R = route_store(W.pstat, dim, e_pad, q_pad, n_query);
  const char* heavy_env = getenv("MMRE_L1_HEAVY");
  bool heavy = bits != 16 && R.cap > 0;
  if (heavy && heavy_env) heavy = atoi(heavy_env) != 0;
  else if (heavy) {  // (the grouping rule's bound on the rows, whichever sweep MMRE_GROUP_CAP forces)
    const int64_t rows8 = std::min<int64_t>(n_query, n_groups + n_query / L1Q_GS);
    // (a forced code width, MMRE_L1_BITS, is an A/B hook: its record stays the plain sweep's)
    heavy = bits == 0 && valu_grp_fills_grid(rows8, C.n_et);
  }
  HeavyProbe H{};
  uint32_t route_cap = 0;
  if (heavy) {
    const char* min_env = getenv("MMRE_L1_HEAVY_MIN");
    const char* cap_env2 = getenv("MMRE_L1_HEAVY_CAP");
    const uint32_t n_samp = l1q_heavy_sample(C.n_slice);
    H.n_blk = (int)((rows_max + 31) / 32);
    H.e_base = C.e_base;
    H.row_off = grouped ? W.row_off : nullptr;
    H.row_cnt = grouped ? W.row_cnt : nullptr;
    H.n_rows = grouped ? W.n_rows : nullptr;
    H.flags = R.flags;
    H.min_count = min_env ? (uint32_t)std::min<long long>(std::max(0LL, atoll(min_env)), UINT32_MAX)
                          : std::max<uint32_t>(1u, (uint32_t)std::ceil(L1Q_HEAVY_FRAC * (double)n_samp));
    route_cap = (uint32_t)(cap_env2 ? std::min<long long>(std::max(0LL, atoll(cap_env2)), R.cap_store) : R.cap);
  }
  // K3: filter counts | the code-width probe | the route's probe
  const int n_cblk = (int)std::min<int64_t>((n_groups + 3) / 4, 65536);  // four groups (waves) per block
  const uint32_t probe_max = l1q_probe_max(C.n_slice);
  hipLaunchKernelGGL(k_eval_count_probe, dim3((unsigned)(n_cblk + L1Q_PROBE_Q / 4 + H.n_blk)), dim3(256), 0, st,
                     d_grp_qoff, d_grp_q, n_groups, n_cblk, d_filt_off, d_filt_ids, d_list_scores, d_q_true, d_truth,
                     n_query, n_ent, d_counts, WQ.vq, q_pad, WQ.ve + e_begin, e_pad, C.n_slice, WQ.k4, kt,
                     tight ? WQ.q_l1c : nullptr, WQ.hdr, W.ticket, probe_max, bits == 8 || bits == 16 ? bits : 0,
                     grouped ? W.row_of_q : nullptr, H);
  MMRE_CHECK_LAUNCH();
  if (heavy) {  // after the width decision: the routed list, the routed map and the record
    const double cost = std::ceil(L1Q_HEAVY_ROW_COST * (double)C.n_slice / L1Q_PAIR_COST);
    hipLaunchKernelGGL(k_l1q_route_compact, dim3(1), dim3(1024), 0, st, WQ.hdr, R.flags, R.list, n_query, q_pad,
                       route_cap, d_undecided_q, (uint32_t)cost, l1q_heavy_sample(C.n_slice), H.min_count);
    MMRE_CHECK_LAUNCH();
  }
  // the sweeps: the one the code-width word names counts, the others' workgroups leave
  L1Q l1 = l1q_operands(WQ, C, d_q_rows, d_ent_rows, tight, d_undecided_q);
  if (grouped) {
    l1.row_off = W.row_off;
    l1.row_cnt = W.row_cnt;
    l1.grp_q = d_grp_q;
    l1.tile_m = W.tile_m;
    l1.n_rows = W.n_rows;
    l1.tq = aff;
  }
  if (heavy) l1.routed = R.flags;
  L1Q l16 = l1;
  l16.gate = WQ.hdr + 1;
  const SweepCall C8 = planes(C, WQ.ve, WQ.vq, WQ.k4), C16 = planes(C, WQ.ue, WQ.uq, WQ.k2);
  // the 8-bit sweep (it leaves unless the word names the 8-bit codes) and the gated 16-bit one
  // (one launch for both widths was tried: with both SAD loops in one kernel the allocator
  // spilled 58-81 VGPRs): a sweep per query, the separate path's launches, or grouped, a SAD
  // chain per sweep row, ranked against each member
  int rc = grouped ? launch_valu_grp<6>(C8, l1, rows_max) : launch_valu<6>(C8, l1, false);
  if (!rc) rc = grouped ? launch_valu_grp<5>(C16, l16, rows_max) : launch_valu<5>(C16, l16, false);
  if (rc) return rc;
  // the routed queries' exact kernel, before the launch that carries the finalize: the grid from
  // the cap (eight two-wave workgroups per CU at most; a workgroup walks the units of its stride),
  // the units from the device's count (workgroups without a unit leave at once)
  if (heavy && route_cap > 0) {
    const int64_t units = (((int64_t)route_cap + HR_QB - 1) / HR_QB) * C.n_et;
    const int g = (int)std::max<int64_t>(
        1, std::min<int64_t>(2 * (int64_t)resident_groups((const void*)k_heavy_rows, HR_TE), units));
    hipLaunchKernelGGL(k_heavy_rows, dim3((unsigned)g), dim3(HR_TE), 0, st, C.ent, C.e_pad, C.n_slice, C.n_et, C.e_base,
                       d_q_rows, C.kp, C.truth, C.q_true, (const int32_t*)R.list,
                       (const uint32_t*)(WQ.hdr + L1Q_ROUTE_W + 1), C.counts);
    MMRE_CHECK_LAUNCH();
  }
  // the f32 fallback, gated on the word; it also carries the finalize (filtered += raw)
  L1Q gate{};
  gate.gate = WQ.hdr + 1;
  gate.fin_counts = d_counts;
  gate.fin_n = n_query;
  gate.fin_ticket = WQ.hdr + 6;
  return launch_valu<0>(C, gate, false);
}
