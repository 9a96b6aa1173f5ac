// link_common.h -- what link.hip and link_valu.hip share (and transh.hip uses for its own sweep):
// the tile geometry and the plane layout, the score operators, the work-unit map, the integer
// filter's operand struct L1Q, the host's SweepCall with the grid rules, and the declarations of
// the launchers that cross the two units.
//
// No kernel is defined here. Every kernel instance lives in exactly one unit and is named -- to
// launch it or to ask its occupancy -- in that unit alone; another unit reaches it through the
// owning unit's host launcher (declared at the end of this file). A kernel emitted into two code
// objects of one library would be registered twice.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "dispatch.h"

namespace mmre {

typedef float f32x2 __attribute__((ext_vector_type(2)));  // a v_pk_*_f32 operand pair

constexpr int TQ = 128;   // queries per workgroup tile
constexpr int TE = 128;   // entities per workgroup tile
constexpr int KC = 8;     // K rows per LDS stage
constexpr int NT = 256;   // threads per workgroup

// rows per plane: TransE/DistMult use one plane of plane_rows(model, d) rows;
// ComplEx/RotatE use two planes (re, im) of plane_rows(model, d) rows each.
// DistMult/ComplEx planes are padded to whole 16-row LDS stages of the MFMA sweep (zero rows
// add exact zeros to the fma chain; a 32-row stage measured slower: C3 1.27 vs 1.18 ms, C5
// 37.9 vs 36.6 ms at 248 VGPRs); TransE/RotatE to the VALU sweep's 8.
constexpr int KS_MFMA = 16;
__host__ __device__ inline int n_planes(int model) { return (model == MMRE_COMPLEX || model == MMRE_ROTATE) ? 2 : 1; }
__host__ __device__ inline bool mfma_model(int model) { return model == MMRE_DISTMULT || model == MMRE_COMPLEX; }
// MFMA planes: K = n_planes x plane_rows a multiple of 16 (ComplEx d = 200: 2 x 200, no padding)
inline int plane_rows(int model, int dim) {
  return (int)round_up(dim, !mfma_model(model) ? KC : KS_MFMA / n_planes(model));
}

// A value the compiler cannot see through: what is computed from it is computed where it is
// used, not hoisted out of a loop into a register (or scratch) kept live across the loop.
__device__ __forceinline__ int vgpr_opaque(int x) {
  __asm__ volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float vgpr_opaque_f(float x) {
  __asm__ volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint64_t sgpr_opaque64(uint64_t x) {
  __asm__ volatile("" : "+s"(x));
  return x;
}
__device__ __forceinline__ uint32_t sgpr_opaque(uint32_t x) {
  __asm__ volatile("" : "+s"(x));
  return x;
}
__device__ __forceinline__ int sgpr_opaque(int x) {
  __asm__ volatile("" : "+s"(x));
  return x;
}

// ------------------------------------------------------------ score ops ----
// OP: 0 TransE L1, 1 TransE L2, 2 RotatE, 3 DistMult, 4 ComplEx, 5 / 6 TransE L1 on 16-bit /
// 8-bit codes (the integer filter; acc carries a uint32 in float bits). One k step.
template <int OP>
__device__ __forceinline__ float op_step(float acc, float qa, float qb, float x, float y) {
  if constexpr (OP == 0) {
    return acc + fabsf(qa - x);
  } else if constexpr (OP == 1) {
    float d = qa - x;
    return acc + d * d;
  } else if constexpr (OP == 2) {
    float dr = qa - x, di = qb - y;
    return acc + sqrtf(__builtin_fmaf(di, di, dr * dr));
  } else if constexpr (OP == 5) {  // TransE L1 integer filter: two 16-bit codes per dword
    return __uint_as_float(__builtin_amdgcn_sad_u16(__float_as_uint(qa), __float_as_uint(x), __float_as_uint(acc)));
  } else if constexpr (OP == 6) {  // TransE L1 integer filter: four 8-bit codes per dword
    return __uint_as_float(__builtin_amdgcn_sad_u8(__float_as_uint(qa), __float_as_uint(x), __float_as_uint(acc)));
  } else {
    return __builtin_fmaf(x, qa, acc);
  }
}
template <int OP>
__device__ __forceinline__ float op_final(float acc) {
  if constexpr (OP == 1) return sqrtf(acc);
  else return acc;
}
// RotatE's |(dr, di)| = sqrt(v), v = fma(di, di, dr*dr), correctly rounded, for the sweep's inner
// loop, in full-rate f32 arithmetic only: y = v_rsq_f32(v), s = v*y, h = y/2, then one
// Newton step s + (v - s*s)*h in fma form. Checked exhaustively on MI355X against IEEE
// sqrtf over every float input (scripts/probes/sqrt_candidates.hip): exact for all
// v in [2^-96, FLT_MAX]; it is not for v = 0, v < 2^-96 or v = inf, so the caller tracks
// min(v) and the accumulators' NaN-ness and recomputes such a (rare) tile with sqrtf.
__device__ __forceinline__ float rot_mag(float v, float y) {  // y = v_rsq_f32(v)
  const float s = v * y, h = 0.5f * y;
  const float e = __builtin_fmaf(-s, s, v);
  return __builtin_fmaf(e, h, s);
}
constexpr float kRotMin = 0x1p-96f;

// RotatE's fast filter (the plain and type-constrained sweeps; the score-storing sweep keeps
// the exact chain): the inner loop takes the raw v_sqrt_f32, which is within 1 ulp of the
// correctly rounded sqrtf on every normal input and within 2^-63 on denormal ones
// (scripts/probes/sqrt_ulp.hip, exhaustive on MI355X). Both chains add non-negative terms in
// the same order, so with S' the fast sum and S the canonical one
//   |S' - S| <= sum_k |m'_k - m_k| + the two chains' rounding errors
//            <= (kp + 1) 2^-23 S' (1 + small) + kp 2^-63,
// and rot_bound() returns a bound above that. A pair whose prediction is on the same side of
// the threshold at both ends of [S' - B, S' + B] (every apply_pred kind is monotone in S) is
// decided; the few others (~2e-4 of the pairs on the C4 tables) and any non-finite S' are
// rescored exactly by rot_exact (IEEE sqrtf, the canonical chain), so the counts are the
// canonical ones bit for bit.
__device__ __forceinline__ float rot_bound(float s, int kp) {
  const float f = (float)(kp + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
  return __builtin_fmaf(s, f, (float)kp * 0x1p-62f);
}
__device__ __forceinline__ float rot_exact(const float* __restrict__ q_km, int64_t q_pad, int64_t q,
                                        const float* __restrict__ ent_km, int64_t e_pad, int64_t e, int kp) {
  float acc = 0.0f;
#pragma unroll 8
  for (int k = 0; k < kp; ++k)
    acc = op_step<2>(acc, q_km[(int64_t)k * q_pad + q], q_km[(int64_t)(kp + k) * q_pad + q],
                     ent_km[(int64_t)k * e_pad + e], ent_km[(int64_t)(kp + k) * e_pad + e]);
  return acc;
}

// TransE L1's integer filter (count-only sweeps, mmre_link_sweep_l1q). The k-major planes are
// quantized once per evaluation to 16-bit codes Q(x) = rint((x + M) * 65535 / 2M), M the
// largest |x| over both planes, two consecutive k per dword, and the sweep's inner loop is
// one v_sad_u16 per two elements (|a.lo - b.lo| + |a.hi - b.hi| + acc: half rate, i.e. one
// issue slot per element against two for sub + add-with-abs; scripts/probes/sad_rate.hip).
// delta * sum|Qq - Qe| is within K delta (1 + small) of the real sum |q - e| (each code is off
// by at most 1/2 + the float rounding of the map), and the canonical f32 chain is within
// (K + 1) 2^-24 S of it, so B = 1.03 K delta + (K + 4) 2^-23 S' bounds |S' - S|; decided /
// undecided pairs as for RotatE (rot_bound), the undecided rescored exactly from the
// row-major copies (l1_exact_rows: the canonical chain, acc + |q_k - e_k| in k order).
// M non-finite (an inf / NaN anywhere in the planes): delta = inf, every pair is undecided.
// Round 4: the default code width is 8 bits -- four k per dword, ONE v_sad_u8 per four elements
// at the issue cost of one v_sad_u16 (scripts/probes/sad8_rate.hip: 4.4 vs 4.7 SIMD-cycles per
// wave-instruction), i.e. half the inner loop -- with the same bound at delta = 2M / 255 (a band
// 257x wider: 0.38 % of the trained C2 pairs undecided, scripts/probes/transe_quant_frac.py).
// Whether that band pays depends on the data (how many scores sit that close to the
// thresholds: xavier-init tables, whose truths rank mid-table, put tens of percent there), so
// k_l1q_probe counts the undecided pairs of a fixed sample with the 8-bit codes and, over
// L1Q_PROBE_FRAC of it, the 16-bit codes are made and swept instead. The choice is one device
// word (hdr[1]); the three sweeps (8-bit, 16-bit, f32) are launched gated on it, and the one it
// names counts -- no host round trip.
// Workspace header (L1Q_HDR bytes before the code planes): word 0 = bits of M, word 1 = the
// code-width word (L1Q_CODES8 / L1Q_F32 / L1Q_CODES16), word 2 = the probe's undecided pairs,
// L1Q_SLOTS undecided-pair counters (uint64, L1Q_SLOT_STRIDE apart: separate cache lines) from
// byte 256, the absmax blocks' partial sums of |x| from byte L1Q_PART. Zeroed up to L1Q_PART by
// the launch sequence. The 16-bit planes follow the header, then the 8-bit planes.
constexpr uint32_t L1Q_CODES8 = 0u, L1Q_F32 = 1u, L1Q_CODES16 = 2u;
constexpr int L1Q_HDR = 8192;
constexpr int L1Q_SLOTS = 16;
constexpr int L1Q_SLOT_STRIDE = 32;  // uint64 units = 256 B
constexpr int L1Q_PART = 256 + L1Q_SLOTS * L1Q_SLOT_STRIDE * 8;
constexpr int L1Q_MAX_BLOCKS = 512;
struct L1Q {
  const float* q_rows;     // (queries, kt) row-major query vectors
  const float* ent_rows;   // (whole table, kt) row-major entity rows
  const uint32_t* hdr;     // workspace header: hdr[0] bits of M, hdr[1] code-width word, hdr[2] probe count
  unsigned long long* undecided;  // counter slots
  const float* q_f;        // fallback: the f32 k-major planes (query, entity slice) and their rows
  const float* ent_f;
  int kp_f;
  int kt;                  // floats per row (the canonical chain's length, padding rows are 0)
  const uint32_t* gate;    // gated launches: run only if *gate is the sweep's code-width word (L1Q_F32 for the f32 sweep)
  const float* q_l1c;      // 8-bit codes, tight bound: per query row sum |eps_q| (upper bound); nullptr: uniform bound
  uint32_t* guard;         // hdr[4]: pairs the rescoring refused (query or entity id out of range; must stay 0)
  uint32_t* und_q;         // optional per-query count of rescored pairs (cost calibration of the sharding)
  int32_t* fin_counts;     // gated f32 launch of the fused evaluation: the finalize (filtered += raw) rides
  int64_t fin_n;           // on it -- every workgroup's slice when the gate is shut, the last workgroup's
  uint32_t* fin_ticket;    // pass after the sweep when it is open (fin_counts nullptr: a separate launch)
  uint32_t* wq;            // dynamic unit scheduling: one zeroed work counter per XCD group (nullptr: static ranges)
  // grouped sweep (the fused evaluation; k_eval_prep's row map): sweep row -> its first member's
  // position in grp_q and its member count; per row tile the largest count; [0] rows, [1] rows
  // padded to whole tiles. q_l1c is then per ROW, and the code planes hold one column per row.
  const int32_t* row_off;
  const int32_t* row_cnt;
  const int32_t* grp_q;
  const int32_t* tile_m;
  const int32_t* n_rows;
  // per-query route (the fused evaluation): the 8-bit sweeps leave out a query whose
  // byte in `routed` is set (nullptr: no route); k_heavy_rows counts the routed list's queries
  // instead
  const uint8_t* routed;
  // grouped sweep, row-tile-affine claims (l1q_affine_stride): per XCD group a hint word and one
  // claim counter per row tile, zeroed by k_eval_prep (nullptr: the group's sequential counter, wq)
  uint32_t* tq;
  const uint32_t* route_n;    // (unused since k_heavy_rows takes the list itself; kept so that the
                              // sweeps' kernel argument, and with it their code, stays as measured)
};
// Header words of the route's record (zeroed with the header by K1, written by k_l1q_route_compact):
// flagged queries, routed queries (k_heavy_rows' query count), sampled columns, flag threshold
constexpr int L1Q_ROUTE_W = 8;
// The sweeps' dynamic-scheduling work counters (L1Q::wq): one per XCD group, each on a 128-B
// line of its own -- the second half of an undecided-pair counter slot (L1Q_SLOT_STRIDE bytes
// apart from byte 256; the slot's counter uses its first 8 bytes) -- zeroed with the header
// before every evaluation (k_zero_words / k_eval_prep). (Eight counters on one line serialised
// every claim of the grid on that line: C2 sweep 1.03 -> 2.33 ms.) MMRE_SWEEP_DYN=0: the
// static contiguous unit ranges (A/B).
constexpr int L1Q_WQ_STRIDE = L1Q_SLOT_STRIDE * 2;  // uint32 words between two groups' counters
inline uint32_t* l1q_work_counters(const uint32_t* hdr) {
  static_assert(L1Q_SLOTS >= 8 && L1Q_SLOT_STRIDE * 8 >= 256, "a 128-B half slot per XCD group");
  static const char* env = getenv("MMRE_SWEEP_DYN");
  return (env && env[0] == '0') ? nullptr : const_cast<uint32_t*>(hdr) + (256 + 128) / 4;
}
// The grouped sweep's row-tile-affine claims (L1Q::tq; sweep_valu_body's claim_affine): per XCD
// group a block of l1q_affine_stride words, whole 128-B lines of its own -- word 0 the group's
// hint (every row tile below it is exhausted; it only rises), word 1 + t the claims made on row
// tile t. Sized from q_pad, which host and device both know (the device's row tiles are at most
// q_pad / TQ). The host finds the 8 blocks in the tail of the row map's row_cnt, which nothing
// reads or writes past the rows' bound (mmre_link_evaluate_l1q), and k_eval_prep zeroes them.
__host__ __device__ inline int l1q_affine_stride(int64_t q_pad) { return (int)((1 + q_pad / TQ + 31) / 32 * 32); }
__device__ __forceinline__ float l1q_delta(const uint32_t* absmax, float levels) {
  const float m = __uint_as_float(*absmax);
  return m == 0.0f ? 0.0f : (m < INFINITY ? (2.0f * m) / levels : INFINITY);
}
// Integer thresholds of the L1 filter for one query row (prediction = the score): with a = delta
// S_int, |S - a| <= l1f a + l1c, so S_int < x = (th - l1c) / (delta (1 + l1f)) gives S < th and
// S_int >= y = (th + l1c) / (delta (1 - l1f)) gives S >= th; x, y shrunk / grown by 2^-18 against
// the float rounding of their own computation. With the tight 8-bit bound the accumulator also
// holds the entity's error offset o_e (its code row `words`: S_int + o_e), l1c is the query's own
// error sum, and o_e >= sum |eps_e| / (delta (1 - l1f)): S_int + o_e < t_sure proves S < th and
// S_int + o_e >= t_out + 2 o_max proves S >= th (o_max: the largest offset of the slice).
__device__ __forceinline__ void l1_int_thresholds(float th, float l1c, float l1d, float l1f, uint32_t omax2,
                                                  uint32_t& t_sure, uint32_t& t_span) {
  uint32_t ts = 0u, to = 0xFFFFFFFFu;
  if (l1d < INFINITY) {
    const float x = (th - l1c) / (l1d * (1.0f + l1f)) * (1.0f - 0x1p-18f);
    const float y = (th + l1c) / (l1d * (1.0f - l1f)) * (1.0f + 0x1p-18f);
    ts = x > 0.0f ? (uint32_t)floorf(fminf(x, 0x1p31f)) : 0u;
    to = y > 0.0f ? (uint32_t)ceilf(fminf(y, 0x1p31f)) : 0u;
    // y <= 0 or NaN (a padding query row's -inf threshold, a NaN truth): no pair beats it, no
    // band -- the offsets must not open one (a band there sent padding rows to the rescoring)
    if (to != 0u) to = to + omax2 < to ? 0xFFFFFFFFu : to + omax2;
  }
  t_sure = ts;
  t_span = to > ts ? to - ts : 0u;
}

// (U float4 pairs in flight per round: 5, or 3 inside the grouped sweep's slot loop, where the
// tile's 64 accumulators stay live across the rescoring: 4 and 5 spilled 16 VGPRs there)
template <int U = 5>
__device__ __forceinline__ float l1_exact_rows(const float* __restrict__ q, const float* __restrict__ e, int kt) {
  const float4* q4 = reinterpret_cast<const float4*>(q);
  const float4* e4 = reinterpret_cast<const float4*>(e);
  float acc = 0.0f;
#pragma unroll U
  for (int k = 0; k < kt / 4; ++k) {
    const float4 a = q4[k], b = e4[k];
    acc = acc + fabsf(a.x - b.x);
    acc = acc + fabsf(a.y - b.y);
    acc = acc + fabsf(a.z - b.z);
    acc = acc + fabsf(a.w - b.w);
  }
  return acc;
}

__host__ __device__ inline int op_of_model(int model) {
  return model == MMRE_TRANSE_L1 ? 0 : model == MMRE_TRANSE_L2 ? 1 : model == MMRE_ROTATE ? 2
         : model == MMRE_DISTMULT ? 3 : 4;
}

__device__ __forceinline__ bool type_bit(const uint32_t* __restrict__ mask, int64_t words, int64_t r, int64_t e) {
  return (mask[r * words + (e >> 5)] >> (e & 31)) & 1u;
}
// The type bits of a VALU-sweep thread's 8 entity columns for relation r: columns 0-3 are ids
// e0 .. e0 + 3, columns 4-7 e0 + 64 .. e0 + 67 (e0 a multiple of 4: each group of four lies in
// one 32-bit word); bit j = column j. Two loads per query row instead of one per pair, and no
// per-pair branch (the per-pair `better && type_bit(...)` kept ~100 VGPRs of masks and
// addresses live in the type-constrained sweeps: they spilled). Columns at or past e_end: 0.
__device__ __forceinline__ uint32_t type_bits8(const uint32_t* __restrict__ mask, int64_t words, int64_t r, int e0,
                                               int e_end) {
  const uint32_t* row = mask + r * words;
  const uint32_t lo = e0 < e_end ? (row[e0 >> 5] >> (e0 & 31)) & 15u : 0u;
  const uint32_t hi = e0 + 64 < e_end ? (row[(e0 + 64) >> 5] >> (e0 & 31)) & 15u : 0u;
  return lo | (hi << 4);
}

// The grouped sweep of the fused evaluation (ValuSmemGrp and launch_valu_grp, link_valu.hip)
constexpr int L1Q_GS = 8;  // member slots per sweep row: 8 KB + 2 KB per slot = 36 KB, four workgroups per CU
// The grouped sweep runs when the host's bound on the sweep rows is at most this share of the
// queries (mmre_link_evaluate_l1q). C2, 1-unit claims: rows at 0.373 / 0.448 / 0.620 / 1.0 of the
// queries (caps 8 / 4 / 2 / 1) 0.709 / 0.807 / 0.915 / 1.268 ms against the ungrouped 0.980: the
// break-even is near 0.69 of the true rows, which the bound overstates by up to 1/8.
constexpr double L1Q_GROUP_FRAC = 0.6;

// ------------------------------------------------------- work-unit map ---
// Work unit = (query tile of TQ) x (entity tile of TE). XCD group g (workgroups g, g + G,
// g + 2G, ...: the ones round-robin dispatch places on one XCD when the grid is a multiple of
// G = 8) owns m = n_et / G whole entity tiles for every query tile (query-tile major, so its
// L2 keeps streaming the same 1/G of the table and a workgroup leaves a query tile rarely),
// then a 1/G share of the n_et % G leftover tiles' units. Every group gets the same number of
// units +-1, so no XCD runs a whole extra round of units (C3: 100 entity tiles = 8 x 12 + 4;
// whole-tile groups of 12 and 13 left the 13-tile XCDs 10 units per workgroup against 8.7).
struct UnitMap {
  int m, r, ex0, el0, n_main, lo0, count, nq;
  bool emajor;  // entity-tile-major order inside the group (consecutive units share an entity tile)
  __device__ __forceinline__ UnitMap(int grp, int n_groups, int n_qt, int n_et, bool emajor_ = false) {
    nq = n_qt;
    emajor = emajor_;
    m = n_et / n_groups;
    r = n_et - m * n_groups;
    ex0 = grp * m;
    el0 = m * n_groups;  // first leftover entity tile
    n_main = n_qt * m;
    const int64_t left = (int64_t)n_qt * r;
    lo0 = (int)(left * grp / n_groups);
    count = n_main + (int)(left * (grp + 1) / n_groups) - lo0;
  }
  // unit i (< count) of the group -> (query tile, entity tile)
  __device__ __forceinline__ void at(int i, int& qt, int& et) const {
    if (i < n_main) {
      if (emajor) {
        qt = i % nq;
        et = ex0 + i / nq;
      } else {
        qt = i / m;
        et = ex0 + i % m;
      }
    } else {
      const int j = lo0 + (i - n_main);
      qt = j / r;
      et = el0 + j % r;
    }
  }
};

// ------------------------------------------------------------------ host ---
// Host functions here are inline, not static: one that reads an experiment variable once (a static
// local) reads it once per process, not once per unit. Hidden: none of this is part of the
// library's surface.
#pragma GCC visibility push(hidden)

// What every sweep launcher needs. An entry point fills the first part from its ABI arguments
// (ent: the table's k-major planes), check_link_args validates it, sweep_slice() the rest (link.hip).
struct SweepCall {
  hipStream_t st;
  const float* ent;
  int64_t e_pad;
  const float* q;
  int64_t q_pad, n_query;
  int pred_kind;
  float margin;
  const float* truth;
  const int32_t* q_true;
  const int64_t* qr;
  const int8_t* qmode;
  const uint32_t *type_head, *type_tail;  // both or neither
  int32_t* counts;
  float* scores;
  // sweep_slice: ent now at the first column of the slice [e_base, e_base + n_slice) -- e_cols
  // columns in n_et whole tiles; kp K rows of the planes (ktot for the MFMA sweeps); tw type words
  int kp, n_et, e_base;
  int64_t n_slice, e_cols, tw;
  bool tc() const { return type_head != nullptr; }
  bool store() const { return scores != nullptr; }
  int64_t q_tiles() const { return q_pad / TQ; }
};

// Work units (query tile x entity tile) of an XCD-grouped sweep: the busiest group's (UnitMap) x 8.
inline int64_t sweep_units(int64_t q_tiles, int n_et) {
  return n_et >= 8 ? 8 * q_tiles * ((n_et + 7) / 8) : q_tiles * n_et;
}
inline int xcd_groups(int g, int n_et) { return (g % 8 == 0 && n_et >= 8) ? 8 : 1; }  // of a grid of g workgroups
// MMRE_SWEEP_GRID (experiments): a number = that many persistent workgroups; "tiles" = the
// caller's tile grid, where it has one (the VALU sweep)
inline int grid_override(int g, int tiles = 0) {
  static const char* env = getenv("MMRE_SWEEP_GRID");
  if (env && env[0] == 't' && tiles > 0) return tiles;
  return (env && env[0] >= '1' && env[0] <= '9') ? atoi(env) : g;
}

// ------------------------------------------------------------- launchers ---
// Each is defined in the unit that owns its kernels. The templates are instantiated explicitly
// there for the operators listed, so no other unit instantiates a kernel by calling one.

// link.hip. Resident workgroups of a persistent grid of `kernel` (the caller's own kernel); the
// cache and its mutex exist once.
int resident_groups(const void* kernel, int threads);
// k_counts_finalize: filtered columns += raw columns, after a sweep
int launch_finalize(hipStream_t st, int32_t* counts, int64_t n_query, bool tc);

// link_valu.hip: k_sweep_valu. OP 0, 1, 2, 5, 6 / the grouped sweep, OP 5, 6.
template <int OP>
int launch_valu(const SweepCall& C, const L1Q& l1 = {}, bool finalize = true);
template <int OP>
int launch_valu_grp(const SweepCall& C, L1Q l1, int64_t rows_max);
// Do `rows` sweep rows over n_et entity tiles give every resident workgroup of the grouped sweep a
// unit? (the fused evaluation's rule for grouping and for the per-query route)
bool valu_grp_fills_grid(int64_t rows, int n_et);

#pragma GCC visibility pop

}  // namespace mmre
