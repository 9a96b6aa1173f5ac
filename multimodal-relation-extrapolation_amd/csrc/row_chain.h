// row_chain.h -- the row-wise score chain: one wave scores one triple (h, r, t).
//
// This is the arithmetic behind model.predict and the training forward on this library
// (DESIGN.md §3), written once. Kernels that use it agree bit for bit on the same row, so ranks
// and thresholds computed from them are exact. The contract:
//   - element lane + 64 c of a row sits in slot c of the lane's register row, 0 past the end;
//   - a lane's partial adds its terms in increasing c, starting from 0;
//   - the row's score is the xor-butterfly wave_sum of the partials;
//   - TransE divides h, r and t by max(sqrt(wave_sum(x^2)), 1e-12) before (h + r) - t, and by
//     1.0f, exactly, without norm_flag: the raw row is then the quotient;
//   - RotatE rotates by canon_sincos(r / phase_denom).
// A kernel may hoist any of these operations out of a loop (relpred.hip: per pair, per relation),
// share a row between triples (tripleclass.hip, ns.hip) or read the elements from memory instead
// of registers (ns.hip row_score): the same operations on the same operands, in this order.
// Users: ns.hip (row_score, the TransE and the generic forward), relpred.hip, tripleclass.hip.
// Not the fused TransE step (ns_fused_body: its own reduction) nor the link sweeps
// (link.hip, link_valu.hip, transh.hip: k-major tiles, one sequential chain per pair).
#pragma once
#include "mmre_common.h"

namespace mmre {

template <int NC>
struct Vec {
  float v[NC];  // element lane + 64 c of the row in v[c] (zero past the row's end)
};

template <int NC>
__device__ __forceinline__ void vload(float (&v)[NC], const float* __restrict__ row, int d, int lane) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + c * kWave;
    v[c] = k < d ? row[k] : 0.0f;
  }
}

// This lane's sum of squares of a register row (padding adds +0: the sum is unchanged).
template <int NC>
__device__ __forceinline__ float vsq(const float (&v)[NC]) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) s += v[c] * v[c];
  return s;
}

// TransE's divisor from a row's wave-summed squares. Without norm_flag no norm is formed: the
// divisor is exactly 1.0f, and a kernel may skip the division.
__device__ __forceinline__ float norm_of_sq(float sq) { return fmaxf(sqrtf(sq), 1e-12f); }
template <int NC>
__device__ __forceinline__ float row_norm(const float (&v)[NC]) {
  return norm_of_sq(wave_sum(vsq(v)));
}

// RotatE: sin and cos of one relation element, and of a register row (s may be r itself).
__device__ __forceinline__ void rel_sincos(float r, float phase_denom, float* s, float* c) {
  canon_sincos(r / phase_denom, s, c);
}
template <int NC>
__device__ __forceinline__ void vsincos(const float (&r)[NC], float phase_denom, float (&s)[NC], float (&c)[NC]) {
#pragma unroll
  for (int i = 0; i < NC; ++i) rel_sincos(r[i], phase_denom, &s[i], &c[i]);
}

// ComplEx's term from the four entity products hr tr, hi ti, hr ti, hi tr (relpred.hip forms them
// once per pair) and the relation's re, im.
__device__ __forceinline__ float complex_term(float hrtr, float hiti, float hrti, float hitr, float rr, float ri) {
  return hrtr * rr + hiti * rr + hrti * ri - hitr * ri;
}

// The per-element term of MODEL from the halves a, b of H, R and T. TransE, DistMult: a alone
// (TransE's operands already divided by their norms). ComplEx: a = re, b = im. RotatE: entities
// a = re, b = im; relation a = sin, b = cos.
template <int MODEL>
__device__ __forceinline__ float row_term(float ha, float hb, float ra, float rb, float ta, float tb) {
  if constexpr (MODEL == MMRE_TRANSE_L1 || MODEL == MMRE_TRANSE_L2) {
    const float x = (ha + ra) - ta;
    return MODEL == MMRE_TRANSE_L1 ? fabsf(x) : x * x;
  } else if constexpr (MODEL == MMRE_DISTMULT) {
    return (ha * ra) * ta;
  } else if constexpr (MODEL == MMRE_COMPLEX) {
    return complex_term(ha * ta, hb * tb, ha * tb, hb * ta, ra, rb);
  } else {
    const float re = ha * rb - hb * ra - ta;
    const float im = ha * ra + hb * rb - tb;
    return sqrtf(re * re + im * im);
  }
}
template <int MODEL>  // the one-half models
__device__ __forceinline__ float row_term(float h, float r, float t) {
  static_assert(MODEL <= MMRE_DISTMULT, "ComplEx and RotatE rows have two halves");
  return row_term<MODEL>(h, 0.0f, r, 0.0f, t, 0.0f);
}

// This lane's partial of a row of d elements: term(c) for c = 0 .. NC - 1, in that order. With
// d = 64 NC every slot adds: the same bits when the rows are zero past their end, where every
// model's term is +0 (ns.hip's register forwards, which spare the compares).
template <int NC, class Term>
__device__ __forceinline__ float lane_partial(int d, int lane, Term&& term) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float x = term(c);
    acc = lane + c * kWave < d ? acc + x : acc;  // a lane adds only the elements it owns
  }
  return acc;
}

// partial -> the row's raw score s (TransE L2: its square root) -> predict's value, or with
// pred_kind 0 / 4 the training forward's s / model_margin - s.
__device__ __forceinline__ float row_finish(float partial, bool l2, int pred_kind, float margin) {
  float s = wave_sum(partial);
  if (l2) s = sqrtf(s);
  return apply_pred(pred_kind, margin, s);
}

}  // namespace mmre
