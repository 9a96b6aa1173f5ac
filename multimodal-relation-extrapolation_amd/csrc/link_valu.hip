// link_valu.hip -- the VALU sweep of the link-prediction engine (link.hip): TransE L1 / L2 and
// RotatE on f32 planes (OP 0 - 2) and TransE L1's integer filter on 16- / 8-bit codes (OP 5 / 6),
// ungrouped or grouped (GS = L1Q_GS, the fused evaluation's sweep rows).
//
// Kernels defined here: k_sweep_valu<OP, TC, STORE, PK, DYNC, GS>, every instance of it and
// nothing else -- they are about half of the library's link kernels and its longest compile.
// Other units reach them through launch_valu<OP> and launch_valu_grp<OP> (explicitly
// instantiated at the end of this file) and ask valu_grp_fills_grid about the grouped sweep's
// resident grid; none of them names k_sweep_valu.
#include "link_common.h"

namespace mmre {

// ------------------------------------------------------------ VALU sweep ---
// Work unit = (query tile of 128) x (entity tile of 128); units are ordered query-tile
// major and split into equal contiguous ranges over a persistent grid sized to the
// resident capacity (4 workgroups per CU), so no tail round is left half empty.
// Within a unit: 256 threads as 16 (q) x 16 (e); each thread owns queries
// {4tq..4tq+3, 64+4tq..} and entities {4te..4te+3, 64+4te..}: 64 fp32 accumulators, one
// sequential k chain each (the canonical order). K is staged through LDS in
// double-buffered steps of 8 rows (16 B per thread per plane per operand). Per-query
// counts stay in registers until the workgroup moves to the next query tile.
// LDS of one VALU-sweep workgroup. A struct declared once in the kernel, so that the L1
// filter's kernel and its f32 fallback path (the same kernel, one uniform branch) share it.
// Grouped sweep (the fused evaluation, GS > 0): a sweep row is one query VECTOR shared by up to GS
// member queries; per member slot and row of the tile, the member's integer thresholds, its query
// id (-1: no member) and its count accumulator (flushed when the workgroup leaves the row tile).
// Single-buffered: the flush / reload sits between two workgroup barriers. An empty base for
// GS = 0, so the ungrouped instantiations keep their LDS to the byte.
template <int GS>
struct ValuSmemGrp {
  uint32_t g_ts[GS][TQ];
  uint32_t g_tw[GS][TQ];
  int32_t g_mq[GS][TQ];
  uint32_t g_acc[GS][TQ];
};
template <>
struct ValuSmemGrp<0> {};
// k_sweep_valu's DYNC (units per claim of the dynamically scheduled instances: 1, 2, 4) for the
// grouped sweep's row-tile-affine 1-unit claims (sweep_valu_body)
constexpr int DYNC_AFFINE = 8;
// Workgroups that start on one row tile. C2 (103 row tiles x 13 units per XCD group, 128 workgroups
// per group), ms per evaluation against the sequential counter's 0.596: 1 (a tile each) 0.68 -- a
// row tile's codes then have one reader, and every unit fetches them from beyond the L2 -- 2
// 0.607, 4 0.577, 13 (a unit each) 0.64 (profiles/grouped_affine).
constexpr int L1Q_AFFINE_SHARE = 4;

template <int NPL, bool TC, bool LIST, int GS = 0>
struct ValuSmem : ValuSmemGrp<GS> {
  float4 sq[2][NPL][KC][TQ / 4];
  float4 se[2][NPL][KC][TE / 4];
  float s_thr[2][GS ? 1 : TQ];
  int32_t s_true[2][GS ? 1 : TQ];
  int32_t s_rel[2][TC ? TQ : 1];
  int8_t s_mode[2][TC ? TQ : 1];
  // per-thread counters (off the VGPR budget); 16-bit with type constraints, so that the wave
  // lists fit beside them at four workgroups per CU (a thread adds <= 8 per unit and row; the
  // sweep flushes every unit where a query tile could hold more than 8,190 of a workgroup's units)
  std::conditional_t<TC, uint16_t, int32_t> s_cnt[TC ? 2 : 1][GS ? 1 : 8][GS ? 1 : NT];
  uint32_t s_unc[NT / 64];           // undecided pairs per wave (the L1 filter's counter)
  uint32_t s_ts[2][GS ? 1 : TQ];     // L1 filter, prediction = score: per query row, the integer
  uint32_t s_tw[2][GS ? 1 : TQ];     // thresholds t_sure and t_out - t_sure (load_meta)
  int s_unit;                        // dynamic scheduling: the unit after the one being swept
  // type constraints: per unit (two in flight, by unit parity), the type words of its 128 query
  // rows over its 128 entity columns -- words 0, 2, 1, 3 of the tile, so a thread's two words
  // (columns 4te.., 64 + 4te..) are one 8-B read -- staged with the unit's first stage
  uint32_t s_tb[TC ? 2 : 1][TC ? TQ : 1][4];
  int2 s_pairs[LIST ? NT / 64 : 1][LIST ? 128 : 1];  // L1 filter: each wave's undecided (query, entity) pairs
};

// The sweep body. Counts go to the raw columns only (counts[0][q], counts[2][q]); the filtered
// columns (initialised to minus the listed entities that beat the truth by the truth pass)
// receive them in k_counts_finalize, one coalesced pass after the sweep (half the atomics).
template <int OP, bool TC, bool STORE, int PK, int NPL, int DYNC, int GS = 0>
__device__ __forceinline__ void sweep_valu_body(
    ValuSmem<NPL, TC, (OP == 5 || OP == 6), GS>& sm, const float* __restrict__ ent_km, int64_t e_pad, int64_t n_ent,
    const float* __restrict__ q_km, int64_t q_pad, int64_t n_query, int kp, int n_et, int e_base, int n_groups,
    int pred_kind, float margin, const float* __restrict__ thr, const int32_t* __restrict__ qtrue,
    const int64_t* __restrict__ qr, const int8_t* __restrict__ qmode, const uint32_t* __restrict__ type_head,
    const uint32_t* __restrict__ type_tail, int64_t type_words, int32_t* __restrict__ counts,
    float* __restrict__ scores, const L1Q& l1) {
  static_assert(NPL == ((OP == 2) ? 2 : 1), "planes");
  // filters: RotatE's raw-sqrt sum (rot_bound / rot_exact), TransE L1's 16-bit codes (L1Q)
  constexpr bool L1F = OP == 5 || OP == 6;  // TransE L1's integer filter (16- / 8-bit codes)
  constexpr bool w8 = OP == 6;
  constexpr bool FAST = (OP == 2 || L1F) && !STORE;
  // grouped sweep: one SAD chain per sweep row (a query vector), ranked against each member's
  // thresholds in turn (the slot loop of the epilogue); see ValuSmemGrp and k_eval_prep's row map
  constexpr bool GRP = GS > 0;
  static_assert(!GRP || (L1F && PK == 0 && !TC && !STORE), "the grouped sweep is the plain integer filter's");
  auto& sq = sm.sq;
  auto& se = sm.se;
  auto& s_thr = sm.s_thr;
  auto& s_true = sm.s_true;
  auto& s_rel = sm.s_rel;
  auto& s_mode = sm.s_mode;
  auto& s_cnt = sm.s_cnt;

  const int tid = threadIdx.x;
  const int tq = tid >> 4, te = tid & 15;
  const PredSel<PK> pred(pred_kind, margin);
  // XCD-aware split (UnitMap): the group's units split evenly over its workgroups, each a
  // contiguous range -- or, with l1.wq (dynamic scheduling, a persistent grid), member m takes
  // unit m of its group first and every further unit from the group's work counter. The loader
  // runs one stage ahead of the compute and enters unit U at the top of compute stage nkc - 2 of
  // the unit before; one stage later thread 0 claims U's successor and publishes it in LDS (its
  // wave waits for the reply there; the other waves of the CU run on), and the loader reads it
  // when it leaves U, >= 1 barrier later. (Holding the reply in a register across the stage
  // instead made it loop-carried: 160 B of scratch per lane.) Units of uneven cost (the
  // rescoring of undecided pairs) balance themselves instead of leaving a tail of workgroups.
  const int grp = blockIdx.x % n_groups, gmem = blockIdx.x / n_groups;
  const int per_grp = gridDim.x / n_groups;
  // (grouped: the row tiles, known on the device only)
  const int n_qt = GRP ? __builtin_amdgcn_readfirstlane(l1.n_rows[GRP ? 1 : 0]) / TQ : (int)(q_pad / TQ);
  const UnitMap um(grp, n_groups, n_qt, n_et);
  const int nkc = kp / KC;
  // (compiled per mode and chunk: a runtime choice between the modes, or a runtime chunk size,
  // kept values of both live across the loop -- 160-168 B of scratch per lane; the host passes
  // l1.wq only with nkc >= 2)
  constexpr bool dyn = DYNC > 0;
  // dynamic scheduling claims chunks of consecutive units (the units of a group are query-tile
  // major: a chunk mostly keeps its query tile, so its counts flush and its query metadata loads
  // once, not at every unit): 4 when a workgroup sweeps many units, 1 for a rank's small share
  // (valu_grid; C2 N = 1, per evaluation: chunks of 1 / 2 / 4 / 8 / 16 units 1.053 / 1.007 /
  // 0.975 / 0.997 / 1.017 ms; 8-way shares: 1 or 2 best)
  constexpr int ch_log2 = DYNC == DYNC_AFFINE ? 0 : DYNC >= 4 ? 2 : DYNC >= 2 ? 1 : 0;
  constexpr int ch_mask = (1 << ch_log2) - 1;
  int u0 = dyn ? gmem << ch_log2 : (int)((int64_t)gmem * um.count / per_grp);
  const int u1 = dyn ? um.count : (int)((int64_t)(gmem + 1) * um.count / per_grp);
  // DYNC_AFFINE (grouped, 1-unit claims, l1.tq): row-tile-affine claims. The sequential counter hands a
  // workgroup a unit ~per_grp units on, ten row tiles later at C2, so every claim paid the flush
  // / reload of the epilogue; here a claim (thread 0) takes the next unclaimed unit of row tile t
  // in this XCD group -- its m main units, then its run of the group's leftover units, one counter
  // over both (l1q_affine_stride) -- and, that tile exhausted, of the lowest row tile that has
  // one: from the group's hint on, raising the hint past every tile it finds exhausted (a value
  // read from the hint has only exhausted tiles below it, so hint = t + 1 after tile t = hint
  // failed keeps that). It never waits for another workgroup: a round takes a unit or moves to a
  // higher tile, and the claim is um.count (no unit) once the hint reaches the row tiles' count.
  // The unit indices are UnitMap's; counts are integer sums, so the order of units is free.
  // (an instance of its own, not a runtime choice beside the sequential counter: with both
  // claims in one kernel the 8-bit instance spilled 8 VGPRs, 20 B of scratch per lane)
  constexpr bool AFF = DYNC == DYNC_AFFINE;
  static_assert(!AFF || GRP, "affine claims are the grouped sweep's");
  auto claim_affine = [&](int t) -> int {
    uint32_t* base = l1.tq + grp * l1q_affine_stride(q_pad);
    const int lo1 = um.lo0 + (um.count - um.n_main);  // the end of the group's leftover run
    bool hinted = false;
    for (;;) {  // (one lane runs this: the replies go to SGPRs, the rounds are scalar code)
      const int c = __builtin_amdgcn_readfirstlane((int)atomicAdd(&base[1 + t], 1u));
      if (c < um.m) return t * um.m + c;
      const int j = max(um.lo0, t * um.r) + (c - um.m);
      if (j < min(lo1, (t + 1) * um.r)) return um.n_main + (j - um.lo0);
      const int old = __builtin_amdgcn_readfirstlane((int)atomicMax(&base[0], hinted ? (uint32_t)(t + 1) : 0u));
      const int h = hinted ? max(old, t + 1) : old;
      hinted = true;
      if (h >= n_qt) return um.count;
      t = h;
    }
  };
  if constexpr (AFF) {
    // the first unit is a claim like any other, on row tile (gmem / L1Q_AFFINE_SHARE) % n_qt (the
    // members spread over the tiles, a few to a tile) -- after the gate: a shut launch must claim none
    if (__builtin_amdgcn_readfirstlane(l1.hdr[1]) != (w8 ? L1Q_CODES8 : L1Q_CODES16)) return;
    if (threadIdx.x == 0) sm.s_unit = claim_affine((gmem / L1Q_AFFINE_SHARE) % n_qt);
    __syncthreads();
    u0 = __builtin_amdgcn_readfirstlane(sm.s_unit);  // (overwritten after the first stage's barrier)
  }
  if (u0 >= u1) return;  // uniform over the workgroup

  // L1 filter constants (uniform): code step, bound slope and offset
  float l1d = 0.0f, l1f = 0.0f, l1c = 0.0f;
  if constexpr (L1F) {
    l1d = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(l1q_delta(l1.hdr, w8 ? 255.0f : 65535.0f))));
    l1f = (float)(l1.kt + 4) * 0x1p-23f * (1.0f + 0x1p-8f);
    l1c = __builtin_fmaf((float)l1.kt * 1.03f, l1d, 0x1p-120f);
  }

  // load_meta and the count flush run once per query tile; what they compute from tid and the
  // filter constants is recomputed there from opaque copies (vgpr_opaque / sgpr_opaque), not
  // hoisted by the compiler into per-lane values kept live across the sweep (that kept ~21 of
  // them in scratch: a scratch store of ~90 B per lane at every wave's start)
  auto load_meta = [&](int qtile, int slot) {
    const int tid = vgpr_opaque(threadIdx.x);
    if (tid < TQ) {
      const int64_t q = (int64_t)qtile * TQ + tid;
      const bool v = q < n_query;
      const float th = v ? thr[q] : -INFINITY;
      s_thr[slot][tid] = th;
      s_true[slot][tid] = v ? qtrue[q] : -1;
      if constexpr (L1F && PK == 0) {
        // prediction = the score: the filter decides in the integer domain. With a = delta *
        // S_int, |S - a| <= l1f a + l1c, so S_int < x = (th - l1c) / (delta (1 + l1f)) gives
        // S < th and S_int >= y = (th + l1c) / (delta (1 - l1f)) gives S >= th; x, y are shrunk /
        // grown by 2^-18 against the float rounding of their own computation. Once per query
        // row and query tile, not per unit.
        uint32_t t_sure, t_span;
        const bool tight = w8 && l1.q_l1c != nullptr;
        const int ktm = sgpr_opaque(l1.kt);
        const float md = __uint_as_float(sgpr_opaque(__float_as_uint(l1d)));
        const float mf = (float)(ktm + 4) * 0x1p-23f * (1.0f + 0x1p-8f);  // = l1f
        const float mc = __builtin_fmaf((float)ktm * 1.03f, md, 0x1p-120f);  // = l1c
        l1_int_thresholds(th, tight ? (v ? l1.q_l1c[q] : 0.0f) + 0x1p-120f : mc, md, mf, tight ? 2u * l1.hdr[3] : 0u,
                          t_sure, t_span);
        if constexpr (w8) {
          // a routed query (k_heavy_rows counts it): no sure pair, no band, as a padding row
          if (l1.routed != nullptr && v && l1.routed[q]) t_sure = t_span = 0u;
        }
        sm.s_ts[slot][tid] = t_sure;
        sm.s_tw[slot][tid] = t_span;
      }
      if constexpr (TC) {
        s_rel[slot][tid] = v ? (int32_t)qr[q] : 0;
        s_mode[slot][tid] = v ? qmode[q] : 0;
      }
    }
  };

  // Grouped: the row tile's member slots. Entry idx = slot * TQ + row is always thread idx % NT's
  // (here and in the flush), so reload and flush need no barrier between them. A slot without a
  // member (or a padding row) gets t_sure = t_span = 0: it neither counts nor lists a pair.
  // Returns the tile's slot count (uniform).
  auto load_meta_grp = [&](int qtile) -> int {
    int m = 0;
    if constexpr (GRP) {
      const int tid = vgpr_opaque(threadIdx.x);
      m = min(__builtin_amdgcn_readfirstlane(l1.tile_m[qtile]), GS);
      const bool tight = w8 && l1.q_l1c != nullptr;
      const int ktm = sgpr_opaque(l1.kt);
      const float md = __uint_as_float(sgpr_opaque(__float_as_uint(l1d)));
      const float mf = (float)(ktm + 4) * 0x1p-23f * (1.0f + 0x1p-8f);  // = l1f
      const float mc = __builtin_fmaf((float)ktm * 1.03f, md, 0x1p-120f);  // = l1c
      const uint32_t om2 = tight ? 2u * l1.hdr[3] : 0u;
      // thread t: row t % TQ, slots t / TQ + 2 u -- entry t + u NT. Three dependent rounds of
      // loads for all of them at once (the row's map entry and error sum; its members' ids; their
      // thresholds), not a chain per entry: the workgroup waits here once per row tile.
      static_assert(NT == 2 * TQ && GS % 2 == 0, "two slots' rows per pass");
      const int r = tid % TQ, s0 = tid / TQ;
      const int64_t row = (int64_t)qtile * TQ + r;
      const int cnt = l1.row_cnt[row];
      const int64_t off = l1.row_off[row];
      const float rc = tight ? l1.q_l1c[row] : 0.0f;
      int q[GS / 2];
      float th[GS / 2];
#pragma unroll
      for (int u = 0; u < GS / 2; ++u) {
        q[u] = -1;
        if (s0 + 2 * u < cnt) {
          const int qq = l1.grp_q[off + s0 + 2 * u];
          q[u] = (uint32_t)qq < (uint32_t)n_query ? qq : -1;
        }
      }
      if constexpr (w8) {
        // a routed member (k_heavy_rows counts it) becomes an empty slot. A round of its
        // own, before the thresholds': with the bytes in flight beside the thresholds the tile's
        // 64 accumulators no longer fit (8 VGPRs spilled); once per row tile.
        if (l1.routed != nullptr) {
#pragma unroll
          for (int u = 0; u < GS / 2; ++u)
            if (q[u] >= 0 && l1.routed[q[u]]) q[u] = -1;
        }
      }
#pragma unroll
      for (int u = 0; u < GS / 2; ++u) th[u] = q[u] >= 0 ? thr[q[u]] : -INFINITY;
#pragma unroll
      for (int u = 0; u < GS / 2; ++u) {
        const int sl = s0 + 2 * u;
        if (sl < m) {
          uint32_t t_sure, t_span;
          l1_int_thresholds(th[u], tight ? (q[u] >= 0 ? rc : 0.0f) + 0x1p-120f : mc, md, mf, om2, t_sure, t_span);
          sm.g_ts[GRP ? sl : 0][r] = t_sure;
          sm.g_tw[GRP ? sl : 0][r] = t_span;
          sm.g_mq[GRP ? sl : 0][r] = q[u];
        }
      }
    }
    return m;
  };

  const int srow = tid >> 5, sc4 = tid & 31;
  float4 rq0, re0, rq1, re1;  // plane 0 / plane 1 (RotatE) staging: scalars, kept in VGPRs
  // staging position (unit, kc) of the next load, advanced incrementally (no divisions)
  int ld_unit = u0, ld_kc = 0, ld_qt, ld_et;
  um.at(u0, ld_qt, ld_et);
  // type constraints: the staged unit's type words (row tid / 2, words (tid & 1) and 2 + (tid & 1)),
  // whether the pending stage carries them, and the unit parity they go to (the epilogue's
  // ep_par reads them back); the loader's parity starts at 1 so that unit u0 gets 0
  uint32_t rt0 = 0u, rt1 = 0u;
  bool st_new = false;
  int ld_tpar = 1, st_par = 0, ep_par = 0;
  auto gload = [&]() {
    if constexpr (TC) {
      st_new = ld_kc == 0;
      if (st_new) {  // the unit's first stage: its rows' type words ride along
        ld_tpar ^= 1;
        st_par = ld_tpar;
        const int tt = vgpr_opaque(threadIdx.x);
        const int rr = tt >> 1, jw = tt & 1;
        const int64_t q = (int64_t)ld_qt * TQ + rr;
        uint32_t w0 = 0u, w1 = 0u;
        if (q < n_query) {
          const uint32_t* tm = (qmode[q] == MMRE_HEAD_BATCH ? type_head : type_tail) + qr[q] * type_words;
          const int64_t wb = (e_base + (int64_t)ld_et * TE) >> 5;  // e_base and tiles: whole words
          if (wb + jw < type_words) w0 = tm[wb + jw];
          if (wb + 2 + jw < type_words) w1 = tm[wb + 2 + jw];
        }
        rt0 = w0;
        rt1 = w1;
      }
    }
    const int k = ld_kc * KC + srow;
    const int64_t q0 = (int64_t)ld_qt * TQ, e0 = (int64_t)ld_et * TE;
    const float* qp = q_km + (int64_t)k * q_pad + q0 + sc4 * 4;
    const float* ep = ent_km + (int64_t)k * e_pad + e0 + sc4 * 4;
    rq0 = *reinterpret_cast<const float4*>(qp);
    re0 = *reinterpret_cast<const float4*>(ep);
    if constexpr (NPL == 2) {
      rq1 = *reinterpret_cast<const float4*>(qp + (int64_t)kp * q_pad);
      re1 = *reinterpret_cast<const float4*>(ep + (int64_t)kp * e_pad);
    }
    if (++ld_kc == nkc) {
      ld_kc = 0;
      if (dyn) {
        // the next unit of the chunk, or the first of the claimed chunk (published >= 1 barrier ago)
        ld_unit = ((ld_unit + 1) & ch_mask) != 0 ? ld_unit + 1 : sm.s_unit;
        if (ld_unit < u1) um.at(ld_unit, ld_qt, ld_et);
      } else if (++ld_unit < u1) {
        um.at(ld_unit, ld_qt, ld_et);
      }
    }
  };
  auto swrite = [&](int buf) {
    if constexpr (TC) {
      if (st_new) {
        const int tt = vgpr_opaque(threadIdx.x);
        *reinterpret_cast<uint2*>(&sm.s_tb[st_par][tt >> 1][(tt & 1) * 2]) = make_uint2(rt0, rt1);
      }
    }
    sq[buf][0][srow][sc4] = rq0;
    se[buf][0][srow][sc4] = re0;
    if constexpr (NPL == 2) {
      sq[buf][NPL - 1][srow][sc4] = rq1;
      se[buf][NPL - 1][srow][sc4] = re1;
    }
  };

  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
  f32x2 accp[4][8];  // RotatE filter: the packed accumulators (pair layout at the inner loop)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) accp[i][j] = f32x2{0.0f, 0.0f};
  if constexpr (GRP) {
    for (int idx = tid; idx < GS * TQ; idx += NT) (&sm.g_acc[0][0])[idx] = 0u;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s_cnt[0][i][tid] = 0;
      if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] = 0;
    }
  }
  if (L1F && tid < NT / 64) sm.s_unc[tid] = 0u;
  // L1 filter: the wave's undecided pairs are appended to its LDS list (ballot order, no
  // atomics) and rescored 64 at a time, one pair per lane, whenever the list holds a full
  // batch -- the dependent row loads of the canonical chain are paid once per 64 pairs, not once
  // per lane-pair with the wave waiting on its busiest lane (which made the 8-bit codes' 0.4 %
  // of undecided pairs cost 0.8 ms at C2). Rescored pairs that beat their threshold go straight
  // to the raw count columns (the query tile's counts may have been flushed already).
  // (Type-constrained sweeps too, since round 6: 16-bit LDS counters make room for the list at
  // four workgroups per CU; their per-lane loop kept 232-240 B of scratch per lane.)
  constexpr bool LIST = L1F;
  int list_n = 0;         // wave-uniform
  uint32_t n_listed = 0;  // the wave's undecided pairs (the filter's counter; per lane without the list)
  // A batch of listed pairs, one per lane (active lanes): each rescored with the canonical chain;
  // the beating pairs' raw counts go out as ONE atomic per distinct query of the batch (a wave's
  // 64 pairs come from its 32 query rows, and the undecided pairs concentrate on few queries --
  // C2: half of the 1.09 M in 103 queries of ~7,000 beating pairs each -- whose count words were
  // a same-address chain of per-pair atomics, serialised at ~13 ns each).
  auto rescore = [&](int2 p, bool active) {
    const int64_t q = p.x;
    const int e = p.y;
    // a guard on the list's invariant: every entry is a (query row, slice column) pair of the
    // unit just swept, with q < n_query (padding query rows open no band) and 0 <= e < n_ent.
    // A pair outside is counted in hdr[4] (mmre_link_l1q_stats, asserted 0 by the filter tests)
    // and never reaches a row gather.
    bool ok = active;
    if (active && ((uint64_t)q >= (uint64_t)n_query || (uint32_t)e >= (uint32_t)n_ent)) {
      if (l1.guard) atomicAdd(l1.guard, 1u);
      ok = false;
    }
    if constexpr (GRP) {
      // grouped: a member's own truth is skipped here (the slot loop keeps no truth ids in LDS),
      // and the pairs are counted here, after the skip
      if (ok && e + e_base == qtrue[q]) ok = false;
      n_listed += (uint32_t)__builtin_popcountll(__ballot(ok));
    }
    bool beat = false;
    if (ok) {
      if (l1.und_q) atomicAdd(&l1.und_q[q], 1u);
      const float th = thr[q];
      const float sx = l1_exact_rows<GRP ? 3 : 5>(l1.q_rows + q * (int64_t)l1.kt,
                                                  l1.ent_rows + (int64_t)(e + e_base) * l1.kt, l1.kt);
      beat = pred(sx) < th;
      if constexpr (TC) {
        const uint32_t* tm = qmode[q] == MMRE_HEAD_BATCH ? type_head : type_tail;
        if (beat && type_bit(tm, type_words, qr[q], e + e_base)) atomicAdd(&counts[2 * n_query + q], 1);
      }
    }
    const int qi = (int)q;  // (int32 ids: check_link_args)
    uint64_t pend = __ballot(beat);
    while (pend) {  // uniform: one query of the batch per round
      const int leader = __builtin_ctzll(pend);
      const int ql = __builtin_amdgcn_readlane(qi, leader);
      const bool mine = beat && qi == ql;
      const uint64_t same = __ballot(mine);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&counts[ql], (int)__builtin_popcountll(same));
      if (mine) beat = false;
      pend &= ~same;
    }
  };

  int cur_qt, cur_et;
  um.at(u0, cur_qt, cur_et);
  int slot = 0;
  uint32_t lo = 0xFFFFFFFFu;  // RotatE: min of the sqrt inputs' bits over this unit (see rot_mag)
  // L1 filter: the code rows actually used in the last stage (the plane is padded to whole
  // stages; 100 of 104 rows at d = 200: the pad rows' zeros are not swept)
  // (OP 6: the words of the k values + the entity error-offset row, l1q_quant8)
  const int kk_last = L1F ? ((((l1.kt + (w8 ? 3 : 1)) >> (w8 ? 2 : 1)) + (w8 ? 2 : 1)) & ~1) - (nkc - 1) * KC
                          : KC;
  // the L1 filter's code-width word (L1Q_CODES8 / _CODES16 / _F32: which of the gated sweeps
  // counts), in flight with the stage
  const uint32_t fb_flag = L1F ? l1.hdr[1] : 0u;
  int cur_m = 0;  // grouped: the row tile's member slots (uniform)
  if constexpr (GRP) cur_m = load_meta_grp(cur_qt);
  else load_meta(cur_qt, 0);
  gload();
  swrite(0);
  __syncthreads();
  if (L1F && __builtin_amdgcn_readfirstlane(fb_flag) != (w8 ? L1Q_CODES8 : L1Q_CODES16)) return;  // uniform
  if (dyn && ch_mask == 0) {  // u0's successor (after the gate: a shut launch claims none); the
                              // loader reads it at compute stage nkc - 2 of u0, which may be stage 0
    if (tid == 0) {
      if constexpr (AFF) sm.s_unit = claim_affine(cur_qt);
      else sm.s_unit = per_grp + (int)atomicAdd(&l1.wq[grp * L1Q_WQ_STRIDE], 1u);
    }
    __syncthreads();
  }

  constexpr int KKU = 2;  // LDS rows of operands per inner-loop iteration
  int buf = 0;
  for (int unit = u0; unit < u1;) {
    int unit_next = unit + 1;
    for (int kc = 0; kc < nkc; ++kc) {
      const bool more = ld_unit < u1;
      if (more) gload();
      if constexpr (AFF) {
        // The affine claim of the unit after ld_unit, on ld_unit's row tile -- here, at the top of
        // the unit's last stage, with that stage's loads issued: the loader entered ld_unit in the
        // stage before (its read of s_unit is a barrier back) and leaves it >= 1 barrier on. (In
        // the epilogue, where the sequential claim sits, a claim whose address moves with the tile
        // cost the 8-bit instance 8 spilled VGPRs -- 20 B of scratch per lane -- even as one
        // atomicAdd; here both widths keep 0 B.)
        if (kc == nkc - 1 && more && threadIdx.x == 0) sm.s_unit = claim_affine(ld_qt);
      }
      const int kk_n = (L1F && kc == nkc - 1) ? kk_last : KC;
#pragma unroll KKU
      for (int kk = 0; kk < kk_n; ++kk) {
        float4 a0 = sq[buf][0][kk][tq], a1 = sq[buf][0][kk][16 + tq];
        float4 x0 = se[buf][0][kk][te], x1 = se[buf][0][kk][16 + te];
        const float qa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        if constexpr (OP == 2 && FAST) {
          // packed f32: every v_pk_* computes two pairs' IEEE-identical results (the scalar
          // chain's sub, sub, mul, fma, add per half), so one full-rate issue covers two
          // elements and only the two v_sqrt_f32 stay per-element. Pair (ip, jp) of query rows
          // (2ip, 2ip+1) and entity columns (2jp, 2jp+1): the straight product takes
          // (2ip, 2jp) | (2ip+1, 2jp+1), the swapped one (op_sel) (2ip, 2jp+1) | (2ip+1, 2jp).
          float4 b0 = sq[buf][NPL - 1][kk][tq], b1 = sq[buf][NPL - 1][kk][16 + tq];
          float4 y0 = se[buf][NPL - 1][kk][te], y1 = se[buf][NPL - 1][kk][16 + te];
          const f32x2 qa2[4] = {{a0.x, a0.y}, {a0.z, a0.w}, {a1.x, a1.y}, {a1.z, a1.w}};
          const f32x2 qb2[4] = {{b0.x, b0.y}, {b0.z, b0.w}, {b1.x, b1.y}, {b1.z, b1.w}};
          const f32x2 xv2[4] = {{x0.x, x0.y}, {x0.z, x0.w}, {x1.x, x1.y}, {x1.z, x1.w}};
          const f32x2 yv2[4] = {{y0.x, y0.y}, {y0.z, y0.w}, {y1.x, y1.y}, {y1.z, y1.w}};
#pragma unroll
          for (int ip = 0; ip < 4; ++ip)
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {  // the straight and swapped chains issued side by side
              const f32x2 dr0 = qa2[ip] - xv2[jp], dr1 = qa2[ip] - xv2[jp].yx;
              const f32x2 di0 = qb2[ip] - yv2[jp], di1 = qb2[ip] - yv2[jp].yx;
              const f32x2 p0 = dr0 * dr0, p1 = dr1 * dr1;
              const f32x2 v0 = __builtin_elementwise_fma(di0, di0, p0), v1 = __builtin_elementwise_fma(di1, di1, p1);
              const f32x2 m0 = {__builtin_amdgcn_sqrtf(v0.x), __builtin_amdgcn_sqrtf(v0.y)};
              const f32x2 m1 = {__builtin_amdgcn_sqrtf(v1.x), __builtin_amdgcn_sqrtf(v1.y)};
              accp[ip][2 * jp] = accp[ip][2 * jp] + m0;
              accp[ip][2 * jp + 1] = accp[ip][2 * jp + 1] + m1;
            }
        } else if constexpr (OP == 2) {
          float4 b0 = sq[buf][NPL - 1][kk][tq], b1 = sq[buf][NPL - 1][kk][16 + tq];
          float4 y0 = se[buf][NPL - 1][kk][te], y1 = se[buf][NPL - 1][kk][16 + te];
          const float qb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
          const float yv[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
          // software pipeline across rows: row i + 1's v and v_rsq_f32 are issued before row i's
          // uses, so every rsq result is consumed a whole row later (C4 83.6 -> 81.2 ms; the 16
          // extra VGPRs cost a few dwords of scratch at 168)
          float v[8], y[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float dr = qa[0] - xv[j], di = qb[0] - yv[j];
            v[j] = __builtin_fmaf(di, di, dr * dr);
            y[j] = __builtin_amdgcn_rsqf(v[j]);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            float vn[8], yn[8];
            if (i + 1 < 8) {
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const float dr = qa[i + 1] - xv[j], di = qb[i + 1] - yv[j];
                vn[j] = __builtin_fmaf(di, di, dr * dr);
                yn[j] = __builtin_amdgcn_rsqf(vn[j]);
              }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
              lo = min(min(lo, __float_as_uint(v[j])), __float_as_uint(v[j + 1]));  // v >= 0: bit order; one v_min3
              acc[i][j] = acc[i][j] + rot_mag(v[j], y[j]);
              acc[i][j + 1] = acc[i][j + 1] + rot_mag(v[j + 1], y[j + 1]);
            }
            if (i + 1 < 8) {
#pragma unroll
              for (int j = 0; j < 8; ++j) { v[j] = vn[j]; y[j] = yn[j]; }
            }
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = op_step<OP>(acc[i][j], qa[i], 0.0f, xv[j], 0.0f);
        }
      }
      if (kc == nkc - 1) {  // unit finished: rank epilogue
        const int64_t q0 = (int64_t)cur_qt * TQ;
        const int64_t ebase = (int64_t)cur_et * TE;
        // type constraints: this thread's 8 type bits of query row ql (bit j = column j), from the
        // unit's staged words
        auto tbits = [&](int ql) -> uint32_t {
          const uint2 w = *reinterpret_cast<const uint2*>(&sm.s_tb[TC ? ep_par : 0][TC ? ql : 0][(te >> 3) * 2]);
          const int sh = (te & 7) * 4;
          return ((w.x >> sh) & 15u) | (((w.y >> sh) & 15u) << 4);
        };
        if constexpr (GRP) {
          // Grouped: the tile's integer scores are ranked once per member slot -- the whole-tile
          // pass below (four VALU per pair) against that slot's thresholds; the last entity tile
          // adds its column test. No truth test in either: no pair below t_sure is a truth
          // (S_int < t_sure proves S < th), and the rescoring skips a member's own truth. Per slot
          // the thread's 8 row counts (<= 8 each) are packed four to a dword, summed over the 16
          // te lanes of the row (one DPP row: 16 x 8 <= 128 fits a byte; 8 cross-lane adds), and
          // lane te < 8 adds row te's sum into the slot's LDS accumulator -- one owner per (slot,
          // row) in the workgroup, so a plain read-modify-write (the flush to counts[], shared with
          // the other workgroups, is one global atomic per non-zero (slot, row) and row tile).
          const bool whole = ebase + TE <= n_ent;  // uniform
          int2* wl = sm.s_pairs[tid >> 6];
          const int lane = tid & 63;
          for (int s = 0; s < cur_m; ++s) {  // uniform bound
            uint32_t unc[2] = {0u, 0u}, pk[2] = {0u, 0u};
            if (whole) {
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
                const uint32_t t_sure = sm.g_ts[GRP ? s : 0][ql], t_span = sm.g_tw[GRP ? s : 0][ql];
                int c = 0;
                uint32_t u = unc[i >> 2];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  const uint32_t si = __float_as_uint(acc[i][j]);
                  const uint32_t d = si - t_sure;
                  c += si < t_sure;
                  u = u + u + (uint32_t)(d < t_span);
                }
                unc[i >> 2] = u;
                pk[i >> 2] |= (uint32_t)c << (8 * (i & 3));
              }
            } else {
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
                const uint32_t t_sure = sm.g_ts[GRP ? s : 0][ql], t_span = sm.g_tw[GRP ? s : 0][ql];
                int c = 0;
                uint32_t u = unc[i >> 2];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
                  const bool valid = e < n_ent;
                  const uint32_t si = __float_as_uint(acc[i][j]);
                  c += (si < t_sure) & valid;
                  u = u + u + (uint32_t)((si - t_sure < t_span) & valid);
                }
                unc[i >> 2] = u;
                pk[i >> 2] |= (uint32_t)c << (8 * (i & 3));
              }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // sum over the row's 16 lanes: xor 1, xor 2, half mirror, mirror
              uint32_t v = pk[h];
              v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
              v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
              v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);
              v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);
              pk[h] = v;
            }
            if (te < 8) {
              const uint32_t cnt = ((te < 4 ? pk[0] : pk[1]) >> (8 * (te & 3))) & 255u;
              const int ql = (te < 4) ? tq * 4 + te : 64 + tq * 4 + (te - 4);
              if (cnt) sm.g_acc[GRP ? s : 0][ql] += cnt;
            }
            for (;;) {  // uniform: one undecided pair per lane and round into the wave's list
              const bool has = (unc[0] | unc[1]) != 0u;
              const uint64_t bal = __ballot(has);
              if (bal == 0) break;
              if (has) {
                const int h = unc[0] ? 0 : 1;
                const int p = __builtin_clz(unc[h]);  // pair p = (i & 3) * 8 + j sits at bit 31 - p
                unc[h] &= ~(0x80000000u >> p);
                const int i = h * 4 + (p >> 3), j = p & 7;
                const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
                const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
                // list_n < 64 at the top of every round and a round appends <= 64: pos < 128
                const int pos = list_n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                wl[pos] = make_int2(sm.g_mq[GRP ? s : 0][ql], e);
              }
              list_n += __builtin_popcountll(bal);
              if (list_n >= 64) {  // a full batch
                list_n -= 64;
                rescore(wl[list_n + lane], true);
              }
            }
          }
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
        } else if constexpr (FAST) {
          if constexpr (OP == 2) {  // unpack the pair layout (register renames) and restart it
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const f32x2 p = accp[i >> 1][(j & ~1) + ((i ^ j) & 1)];
                acc[i][j] = (i & 1) ? p.y : p.x;
              }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 8; ++j) accp[i][j] = f32x2{0.0f, 0.0f};
          }
          // undecided pairs: pair (i, j) is bit 31 - ((i & 3) * 8 + j) of unc[i >> 2] (rows 0-3 /
          // 4-7; the whole-tile epilogue shifts the bits in, pair by pair)
          uint32_t unc[2] = {0u, 0u};
          bool whole = false;
          if constexpr (L1F && PK == 0 && !TC) {
            // L1 filter, a whole entity tile (every tile but the last, uniform), ONE pass: per
            // pair d = S_int - t_sure (its borrow, S_int < t_sure, carry-added to the count) and
            // the undecided band d < t_out - t_sure carry-shifted into the pair's bit: four VALU
            // per pair (v_sub_co, v_addc, v_cmp, v_addc). The count needs no truth test: the
            // truth's S is th itself, which no pair below t_sure reaches (S_int < t_sure proves
            // S < th). The truth's own pair is in the band; the rescoring list skips it. (A first
            // pass with a wave-wide "any" ballot and the per-pair bits rebuilt when it was set
            // paid ~420 more VALU per wave and unit: at C2 nearly every wave holds an undecided
            // pair in every unit -- a quarter of them hold a truth.)
            if (ebase + TE <= n_ent) {
              whole = true;
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
                const uint32_t t_sure = sm.s_ts[slot][ql], t_span = sm.s_tw[slot][ql];
                // type constraints: the row's 8 type bits (a pair below t_sure is never the truth)
                const uint32_t tb = TC ? tbits(ql) : 0u;
                int c = 0, cc = 0;
                uint32_t u = unc[i >> 2];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  const uint32_t si = __float_as_uint(acc[i][j]);
                  const uint32_t d = si - t_sure;
                  const bool sure = si < t_sure;
                  c += sure;
                  if constexpr (TC) cc += sure & ((tb >> j) & 1u);
                  u = u + u + (uint32_t)(d < t_span);
                }
                unc[i >> 2] = u;
                s_cnt[0][i][tid] += c;
                if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] += cc;
              }
            }
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            if (whole) break;
            const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
            const float th = s_thr[slot][ql];
            const int32_t tr = s_true[slot][ql];
            int c = 0, cc = 0;
            const uint32_t tb = TC ? tbits(ql) : 0u;
            if constexpr (L1F && PK == 0) {
              // prediction = the score: the integer thresholds of load_meta
              const uint32_t t_sure = sm.s_ts[slot][ql], t_span = sm.s_tw[slot][ql];
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
                const bool valid = (e + e_base != tr) & (e < n_ent);
                const uint32_t si = __float_as_uint(acc[i][j]);
                const bool sure = si < t_sure;
                const bool better = sure & valid;
                c += better;
                if constexpr (TC) cc += better & ((tb >> j) & 1u);
                unc[i >> 2] |= (uint32_t)((si - t_sure < t_span) & valid) << (31 - ((i & 3) * 8 + j));
              }
              s_cnt[0][i][tid] += c;
              if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] += cc;
              continue;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
              const bool valid = (e + e_base != tr) & (e < n_ent);
              float a, bnd;
              if constexpr (L1F) {
                a = (float)__float_as_uint(acc[i][j]) * l1d;
                bnd = __builtin_fmaf(a, l1f, l1c);
              } else {
                a = acc[i][j];
                bnd = rot_bound(a, kp);
              }
              const float p1 = pred(a - bnd), p2 = pred(a + bnd);
              const bool fin = a < INFINITY;  // false for inf and NaN: rescored
              const bool sure = fin & (fmaxf(p1, p2) < th);
              const bool out = (fin & (fminf(p1, p2) >= th)) | (th != th);
              const bool better = sure & valid;
              c += better;
              if constexpr (TC) cc += better & ((tb >> j) & 1u);
              unc[i >> 2] |= (uint32_t)(!sure & !out & valid) << (31 - ((i & 3) * 8 + j));
            }
            s_cnt[0][i][tid] += c;
            if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] += cc;
          }
          if constexpr (LIST) {
            int2* wl = sm.s_pairs[tid >> 6];
            const int lane = tid & 63;
            for (;;) {  // uniform: one undecided pair per lane and round into the list
              const bool has = (unc[0] | unc[1]) != 0u;
              if (__ballot(has) == 0) break;
              bool keep = false;
              int2 pr = make_int2(0, 0);
              if (has) {
                const int h = unc[0] ? 0 : 1;
                const int p = __builtin_clz(unc[h]);  // pair p = (i & 3) * 8 + j sits at bit 31 - p
                unc[h] &= ~(0x80000000u >> p);
                const int i = h * 4 + (p >> 3), j = p & 7;
                const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
                const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
                keep = (int)(e + e_base) != s_true[slot][ql];  // the truth's own pair is not rescored
                pr = make_int2((int)(q0 + ql), e);
              }
              const uint64_t bal = __ballot(keep);
              if (keep) {
                // list_n < 64 at the top of every round and a round appends <= 64: pos < 128
                const int pos = list_n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                wl[pos] = pr;
              }
              const int nb = __builtin_popcountll(bal);
              list_n += nb;
              n_listed += (uint32_t)nb;
              if (list_n >= 64) {  // a full batch (the list holds < 128: < 64 before this round)
                list_n -= 64;
                rescore(wl[list_n + lane], true);
              }
            }
          }
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            uint32_t m = LIST ? 0u : unc[h];  // (the L1 filter's pairs went to the wave's list)
            while (m) {  // rare: exact rescoring, one pair at a time
              const int p = __builtin_clz(m);
              m &= ~(0x80000000u >> p);
              const int i = h * 4 + (p >> 3), j = p & 7;
              const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
              const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
              float sx;
              if constexpr (L1F) {
                ++n_listed;
                sx = l1_exact_rows(l1.q_rows + (q0 + ql) * (int64_t)l1.kt, l1.ent_rows + (int64_t)(e + e_base) * l1.kt,
                                   l1.kt);
              } else {
                sx = rot_exact(q_km, q_pad, q0 + ql, ent_km, e_pad, e, kp);
              }
              const float v = pred(sx);
              if (v < s_thr[slot][ql]) {
                s_cnt[0][i][tid] += 1;
                if constexpr (TC) {
                  const uint32_t* tm = s_mode[slot][ql] == MMRE_HEAD_BATCH ? type_head : type_tail;
                  s_cnt[TC ? 1 : 0][i][tid] += type_bit(tm, type_words, s_rel[slot][ql], e + e_base) ? 1 : 0;
                }
              }
            }
          }
          // the accumulators restart here, after the rescoring: dead while it runs, so its row
          // loads have the registers
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
        } else {
        if constexpr (OP == 2) {
          bool bad = lo < __float_as_uint(kRotMin);  // v = 0 or v < 2^-96
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) bad |= acc[i][j] != acc[i][j];  // v = inf (or a NaN input)
          if (__ballot(bad)) {  // rare: redo this wave's tiles with the IEEE sqrtf
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
            for (int k = 0; k < kp; ++k) {
              float qa[8], qb[8], xv[8], yv[8];
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const int64_t ql = q0 + ((i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4));
                const int64_t ec = ebase + ((i < 4) ? te * 4 + i : 64 + te * 4 + (i - 4));
                qa[i] = q_km[(int64_t)k * q_pad + ql];
                qb[i] = q_km[(int64_t)(kp + k) * q_pad + ql];
                xv[i] = ent_km[(int64_t)k * e_pad + ec];
                yv[i] = ent_km[(int64_t)(kp + k) * e_pad + ec];
              }
#pragma unroll
              for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = op_step<2>(acc[i][j], qa[i], qb[i], xv[j], yv[j]);
            }
          }
          lo = 0xFFFFFFFFu;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
          const float th = s_thr[slot][ql];
          const int32_t tr = s_true[slot][ql];
          int c = 0, cc = 0;
          const uint32_t tb = TC ? tbits(ql) : 0u;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // 32-bit ids (int32 by check_link_args); bitwise &: no per-pair branch
            const int e = (int)ebase + ((j < 4) ? te * 4 + j : 64 + te * 4 + (j - 4));
            const float v = pred(op_final<OP>(acc[i][j]));
            const bool better = (v < th) & (e + e_base != tr) & (e < n_ent);
            c += better;
            if constexpr (TC) cc += better & ((tb >> j) & 1u);
            if constexpr (STORE) {
              if (q0 + ql < n_query && e < n_ent) scores[(q0 + ql) * n_ent + e] = v;
            }
            acc[i][j] = 0.0f;
          }
          s_cnt[0][i][tid] += c;
          if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] += cc;
        }
        }  // !FAST
        if (dyn) unit_next = ld_unit;  // the loader entered it at the top of the stage before
        const bool last = unit_next >= u1;
        int next_qt = cur_qt, next_et = cur_et;
        if (!last) um.at(unit_next, next_qt, next_et);
        // (TC: 16-bit counters, up to 8 per unit, so 8,191 units -- flush every unit where the units
        // of one query tile that an XCD group owns, all of which one workgroup may sweep back to
        // back, could exceed them: um.m = n_et / n_groups whole tiles and, when the leftover units
        // that follow start in that query tile, up to 7 more (UnitMap); n_groups is 1 for a grid
        // that is no multiple of 8)
        if constexpr (GRP) {
          if (last || next_qt != cur_qt) {  // uniform: flush this row tile's member counts
            __syncthreads();  // every wave's adds of this unit are in, and its threshold reads done
            const int tid = vgpr_opaque(threadIdx.x);
            for (int idx = tid; idx < cur_m * TQ; idx += NT) {
              const uint32_t c = (&sm.g_acc[0][0])[idx];
              if (c) {
                const int q = (&sm.g_mq[0][0])[idx];
                if (q >= 0) atomicAdd(&counts[q], (int)c);
                (&sm.g_acc[0][0])[idx] = 0u;
              }
            }
            if (!last) cur_m = load_meta_grp(next_qt);  // visible after the stage's barrier below
          }
        } else
        if (last || next_qt != cur_qt || (TC && um.m > 8184)) {  // uniform: flush this query tile's counts
          const int tid = vgpr_opaque(threadIdx.x);  // (see load_meta)
          const int tq = tid >> 4, te = tid & 15;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            int c = s_cnt[0][i][tid], cc = TC ? s_cnt[TC ? 1 : 0][i][tid] : 0;
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) {
              c += __shfl_xor(c, sh);
              if constexpr (TC) cc += __shfl_xor(cc, sh);
            }
            const int ql = (i < 4) ? tq * 4 + i : 64 + tq * 4 + (i - 4);
            const int64_t q = q0 + ql;
            const bool vq = q < n_query;
            if (te == 0 && vq) {  // raw columns only: k_counts_finalize adds them to the filtered ones
              if (c) atomicAdd(&counts[q], c);
              if constexpr (TC) {
                if (cc) atomicAdd(&counts[2 * n_query + q], cc);
              }
            }
            s_cnt[0][i][tid] = 0;
            if constexpr (TC) s_cnt[TC ? 1 : 0][i][tid] = 0;
          }
          if (!last) {
            slot ^= 1;
            load_meta(next_qt, slot);
          }
        }
        // the loader entered the last unit of its chunk one stage ago: the next chunk, claimed for
        // the loader's exit from it >= 1 barrier later (the previous claim was read long before);
        // here, after the accumulators were reset, where the claim costs no registers
        // (the affine claim: at the top of this stage)
        if (dyn && !AFF && !last && ((unit_next + 1) & ch_mask) == 0 && threadIdx.x == 0)
          sm.s_unit = (per_grp + (int)atomicAdd(&l1.wq[grp * L1Q_WQ_STRIDE], 1u)) << ch_log2;
        if constexpr (TC) ep_par ^= 1;  // the next unit's staged type words
        cur_qt = next_qt;
        cur_et = next_et;
      }
      if (more) swrite(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
    unit = unit_next;
  }
  if constexpr (L1F) {  // the filter's undecided pairs: one atomic per workgroup, 16 slots
    if constexpr (LIST) {
      if (list_n > 0) rescore(sm.s_pairs[tid >> 6][tid & 63], (tid & 63) < list_n);  // the last partial batch
      if ((tid & 63) == 0) sm.s_unc[tid >> 6] = n_listed;
    } else {
      if (n_listed) atomicAdd(&sm.s_unc[tid >> 6], n_listed);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) t += sm.s_unc[w];
      // 32-bit counter in the slot's low word (the stats kernel reads only that word)
      if (t) atomicAdd(reinterpret_cast<uint32_t*>(l1.undecided + (blockIdx.x & (L1Q_SLOTS - 1)) * L1Q_SLOT_STRIDE), t);
    }
  }
}

template <int OP, bool TC, bool STORE, int PK, int DYNC = 0, int GS = 0>
__global__ __launch_bounds__(NT, (OP == 2) ? 3 : 4) void k_sweep_valu(
    const float* __restrict__ ent_km, int64_t e_pad, int64_t n_ent, const float* __restrict__ q_km,
    int64_t q_pad, int64_t n_query, int kp, int n_et, int e_base, int n_groups, int pred_kind, float margin,
    const float* __restrict__ thr, const int32_t* __restrict__ qtrue, const int64_t* __restrict__ qr,
    const int8_t* __restrict__ qmode, const uint32_t* __restrict__ type_head,
    const uint32_t* __restrict__ type_tail, int64_t type_words, int32_t* __restrict__ counts,
    float* __restrict__ scores, L1Q l1) {
  constexpr int NPL = (OP == 2) ? 2 : 1;
  __shared__ ValuSmem<NPL, TC, (OP == 5 || OP == 6), GS> sm;
  // the L1 filter's fallback (k_l1q_quant decided that the codes are too coarse for these
  // planes -- one outlier value sets the code step for everything): the filter launch does
  // nothing (sweep_valu_body tests the flag once its first stage is loaded, so the flag's load
  // latency hides under the stage's) and the exact f32 sweep launched after it, gated on the
  // same flag, counts. A separate launch, not a branch here: inlining the f32 body beside the
  // filter's grew the kernel by half and its register spills (18 -> 23)
  if (l1.gate != nullptr) {
    const uint32_t want = OP == 6 ? L1Q_CODES8 : OP == 5 ? L1Q_CODES16 : L1Q_F32;
    if (__builtin_amdgcn_readfirstlane(*l1.gate) != want) {
      if (l1.fin_counts != nullptr) {  // shut (the codes counted): this workgroup's slice of the finalize
        for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < l1.fin_n; q += (int64_t)gridDim.x * NT) {
          l1.fin_counts[l1.fin_n + q] += l1.fin_counts[q];
          if constexpr (TC) l1.fin_counts[3 * l1.fin_n + q] += l1.fin_counts[2 * l1.fin_n + q];
        }
      }
      return;
    }
  }
  sweep_valu_body<OP, TC, STORE, PK, NPL, DYNC, GS>(sm, ent_km, e_pad, n_ent, q_km, q_pad, n_query, kp, n_et, e_base,
                                                    n_groups, pred_kind, margin, thr, qtrue, qr, qmode, type_head, type_tail,
                                                    type_words, counts, scores, l1);
  if (l1.gate != nullptr && l1.fin_counts != nullptr) {
    // open (the rare f32 fallback): the finalize after every workgroup's counts, by the last
    // workgroup (each wave's count atomics drained, then ONE ticket add per workgroup)
    __shared__ uint32_t s_last;
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
      s_last = __hip_atomic_fetch_add(l1.fin_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (s_last) {
      for (int64_t q = threadIdx.x; q < l1.fin_n; q += NT) {
        atomicAdd(&l1.fin_counts[l1.fin_n + q],
                  __hip_atomic_load(&l1.fin_counts[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if constexpr (TC)
          atomicAdd(&l1.fin_counts[3 * l1.fin_n + q],
                    __hip_atomic_load(&l1.fin_counts[2 * l1.fin_n + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      }
      if (threadIdx.x == 0) *l1.fin_ticket = 0u;
    }
  }
}

// ---------------------------------------------------------------- launch ---
// f(integral_constant<int, DYNC>) for the units per claim, among the instances the caller has
// (MASK: their sum)
template <int MASK, class F>
static void with_chunk(int chunk, F&& f) {
  if ((MASK & 8) && chunk == 8) f(std::integral_constant<int, MASK & 8>{});
  else if ((MASK & 4) && chunk == 4) f(std::integral_constant<int, MASK & 4>{});
  else if ((MASK & 2) && chunk == 2) f(std::integral_constant<int, MASK & 2>{});
  else if ((MASK & 1) && chunk == 1) f(std::integral_constant<int, MASK & 1>{});
  else f(std::integral_constant<int, 0>{});
}
// Units per claim of a dynamically scheduled sweep: 4 from 16 units per workgroup on, else 1
// (measurements: launch_valu_grp, sweep_valu_body). MMRE_SWEEP_CHUNK (A/B) forces 1, 4 or -- where
// the launcher has that instance (allow2) -- 2.
static int sweep_chunk(int64_t per_wg, bool allow2) {
  static const char* env = getenv("MMRE_SWEEP_CHUNK");
  if (!env) return per_wg >= 16 ? 4 : 1;
  const int v = atoi(env);
  return v >= 4 ? 4 : (allow2 && v >= 2) ? 2 : 1;
}

struct ValuGrid { int g, ng, chunk; };  // workgroups, XCD groups, units per claim (0: static ranges)
// (k_static / k_dyn: the instance with static ranges and the dynamically scheduled one, if any)
static ValuGrid valu_grid(const SweepCall& C, const L1Q& l1, const void* k_static, const void* k_dyn) {
  // 16 workgroups per resident slot: short per-workgroup ranges let the dispatcher balance
  // CUs that run at different speeds (C2 on MI355X: 1,024 groups 4.0 ms, 8,192 3.43 ms,
  // 16,384 3.30 ms, 30,528 (one unit each) 3.36 ms).
  int g = 16 * resident_groups(k_static, NT);
  // a gated launch (the L1 filter's f32 fallback, l1.gate) runs 4 workgroups per resident
  // slot: when the gate is shut -- every time but the rare fallback -- its workgroups only
  // read the flag and leave, and a 16x grid of such workgroups cost 77 us per evaluation at
  // C2; one per slot (1x) made the open-gate sweep 15% slower than the plain f32 sweep
  static const char* fbdiv = getenv("MMRE_L1_FB_DIV");
  if (l1.gate != nullptr) {
    const int div = fbdiv ? atoi(fbdiv) : 4;
    g /= div > 1 ? div : 1;
  }
  // Dynamic scheduling (l1.wq, the TransE L1 filter sweeps): one persistent workgroup per
  // resident slot, units from the XCD groups' work counters -- the shut gated launch too (its
  // workgroups only read the gate).
  const bool dyn = k_dyn != nullptr && l1.wq != nullptr && C.kp / KC >= 2;
  const int64_t q_tiles = C.q_tiles();
  int chunk = 0;
  if (dyn) {
    g = resident_groups(k_dyn, NT);
    chunk = sweep_chunk(q_tiles * C.n_et / (g > 0 ? g : 1), false);
  }
  // Small sweeps (a rank's share under relation sharding): no more workgroups than the
  // busiest XCD group has units, so every workgroup gets at most one unit and no empty
  // workgroups are dispatched (C2 at 8-way: 4,380 sweeps 0.52 -> 0.47 ms; 4-way 0.89 -> 0.85).
  const int64_t units = sweep_units(q_tiles, C.n_et);
  if (units < g) g = (int)(units > 0 ? units : 1);
  // Dynamic scheduling of a small share: as many workgroups per XCD group as make its units an
  // (almost) whole number of rounds -- the same rounds as the full grid, no nearly empty last
  // round (an 8-way C2 share: 527 units per group over 128 workgroups = 4.1 rounds, the fifth
  // run by 15 of them; over 106 workgroups, 5 rounds). Measured no faster on 8-way C2 shares
  // (ranks 1 / 3 / 7: 0.190 / 0.203 / 0.199 against 0.185 / 0.193 / 0.196 ms, profiles/r6): off
  // unless MMRE_SWEEP_BALANCE=1 (A/B).
  static const char* bal_env = getenv("MMRE_SWEEP_BALANCE");
  if (dyn && g % 8 == 0 && C.n_et >= 8 && bal_env && bal_env[0] == '1') {
    const int64_t per_group = (q_tiles * C.n_et + 7) / 8;  // UnitMap: every group within +-1 of this
    const int64_t slots = g / 8;
    const int64_t rounds = (per_group + slots - 1) / slots;
    if (rounds <= 16) g = 8 * (int)((per_group + rounds - 1) / rounds);
  }
  g = grid_override(g, 8 * (int)q_tiles);  // "tiles": one workgroup per (query tile, 1/8 of the entity tiles)
  return {g, xcd_groups(g, C.n_et), chunk};
}

// The VALU sweep of operator OP (0 - 2 the f32 sweeps, 5 / 6 the integer filter's count-only ones,
// the only ones with DYNC instances). The model's usual prediction kind is compiled into the
// epilogue (PK = fast) of the plain sweep (C2 3.27 -> 3.23 ms) and of the integer filter's sweeps,
// type masks or not (integer thresholds: prediction = the score); all else decodes it (PK = -1).
template <int OP>
int launch_valu(const SweepCall& C, const L1Q& l1, bool finalize) {
  constexpr int fast = (OP == 2) ? 3 : 0;  // RotatE -(m - s), TransE s
  constexpr bool COUNT_ONLY = OP == 5 || OP == 6;
  if (COUNT_ONLY && C.store()) return MMRE_ERR_ARG;
  const bool fast_pk = C.pred_kind == fast && (COUNT_ONLY || (!C.tc() && !C.store()));
  with_bools(C.tc(), C.store(), fast_pk, [&](auto tc_, auto st_, auto fast_) {
    constexpr bool TC = decltype(tc_)::value, ST = decltype(st_)::value;
    constexpr int PK = decltype(fast_)::value ? fast : -1;
    if constexpr (!(COUNT_ONLY && ST) && !(PK == fast && !COUNT_ONLY && (TC || ST))) {  // the instances there are
      const void* k_dyn = COUNT_ONLY ? (const void*)k_sweep_valu<OP, TC, ST, PK, COUNT_ONLY ? 4 : 0> : nullptr;
      const ValuGrid G = valu_grid(C, l1, (const void*)k_sweep_valu<OP, TC, ST, PK>, k_dyn);
      with_chunk<COUNT_ONLY ? 4 + 1 : 0>(G.chunk, [&](auto dync_) {
        hipLaunchKernelGGL((k_sweep_valu<OP, TC, ST, PK, decltype(dync_)::value>), dim3((unsigned)G.g), dim3(NT), 0,
                           C.st, C.ent, C.e_pad, C.n_slice, C.q, C.q_pad, C.n_query, C.kp, C.n_et, C.e_base, G.ng,
                           C.pred_kind, C.margin, C.truth, C.q_true, C.qr, C.qmode, C.type_head, C.type_tail, C.tw,
                           C.counts, C.scores, l1);
      });
    }
    return MMRE_OK;
  });
  MMRE_CHECK_LAUNCH();
  return finalize ? launch_finalize(C.st, C.counts, C.n_query, C.tc()) : MMRE_OK;
}

// The grouped integer-filter sweep of the fused evaluation (k_sweep_valu<.., GS = L1Q_GS>): work
// units are (row tile) x (entity tile), the row tiles known on the device only -- the host sizes
// the grid from rows_max, an upper bound (workgroups past the last unit leave at once).
// Units per claim, C2 N = 1 (103 row tiles x 111 entity tiles over 1,024 workgroups, ~11 units
// each, heavy tiles first), per evaluation: chunks of 1 / 2 / 4 units (MMRE_SWEEP_CHUNK) 0.705 /
// 0.733 / 0.969 ms -- with so few units per workgroup a 4-unit claim is a third of its share, and
// the last claims leave a long tail (the ungrouped sweep's ~30 units each favoured 4: see
// sweep_valu_body). The host picks 1 below 16 units per workgroup, as valu_grid does.
template <int OP>
int launch_valu_grp(const SweepCall& C, L1Q l1, int64_t rows_max) {
  const bool dyn = l1.wq != nullptr && C.kp / KC >= 2;
  if (!dyn) l1.wq = nullptr;
  int g = resident_groups((const void*)k_sweep_valu<OP, false, false, 0, 1, L1Q_GS>, NT);
  if (!dyn) g *= 16;  // static ranges: short ones (valu_grid)
  const int64_t q_tiles = (rows_max + TQ - 1) / TQ;
  const int64_t units = sweep_units(q_tiles, C.n_et);
  if (units < g) g = (int)(units > 0 ? units : 1);
  // MMRE_SWEEP_GRID (A/B, tests; read per call here, as MMRE_SWEEP_AFFINE is): that many workgroups
  const char* grid_env = getenv("MMRE_SWEEP_GRID");
  if (grid_env && grid_env[0] >= '1' && grid_env[0] <= '9') g = std::max(1, atoi(grid_env));
  // Row-tile-affine claims (l1.tq) are 1-unit claims at any share -- a claim keeps the workgroup's
  // row tile, which is what the longer chunks were for; a chunk forced by MMRE_SWEEP_CHUNK keeps
  // the sequential counter.
  int chunk = dyn ? sweep_chunk(q_tiles * C.n_et / (g > 0 ? g : 1), true) : 0;
  if (dyn && l1.tq != nullptr && getenv("MMRE_SWEEP_CHUNK") == nullptr) chunk = DYNC_AFFINE;
  if (chunk != DYNC_AFFINE) l1.tq = nullptr;
  const int ng = xcd_groups(g, C.n_et);
  with_chunk<DYNC_AFFINE + 4 + 2 + 1>(chunk, [&](auto dync_) {
    hipLaunchKernelGGL((k_sweep_valu<OP, false, false, 0, decltype(dync_)::value, L1Q_GS>), dim3((unsigned)g), dim3(NT),
                       0, C.st, C.ent, C.e_pad, C.n_slice, C.q, C.q_pad, C.n_query, C.kp, C.n_et, C.e_base, ng, 0, 0.0f,
                       C.truth, C.q_true, nullptr, nullptr, nullptr, nullptr, (int64_t)0, C.counts, nullptr, l1);
  });
  MMRE_CHECK_LAUNCH();
  return MMRE_OK;
}

// The fused evaluation's rule (mmre_link_evaluate_l1q: whether to group, whether to route): the
// rows' units give every resident workgroup of the grouped 8-bit sweep one.
bool valu_grp_fills_grid(int64_t rows, int n_et) {
  return (rows + TQ - 1) / TQ * n_et >= resident_groups((const void*)k_sweep_valu<6, false, false, 0, 1, L1Q_GS>, NT);
}

// Every operator link.hip asks for: the f32 sweeps (OP 0 also the integer filter's gated
// fallback) and the code sweeps
template int launch_valu<0>(const SweepCall&, const L1Q&, bool);
template int launch_valu<1>(const SweepCall&, const L1Q&, bool);
template int launch_valu<2>(const SweepCall&, const L1Q&, bool);
template int launch_valu<5>(const SweepCall&, const L1Q&, bool);
template int launch_valu<6>(const SweepCall&, const L1Q&, bool);
template int launch_valu_grp<5>(const SweepCall&, L1Q, int64_t);
template int launch_valu_grp<6>(const SweepCall&, L1Q, int64_t);

}  // namespace mmre
