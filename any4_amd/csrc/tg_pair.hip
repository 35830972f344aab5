// tg_pair.hip -- launch paths of w4_gemm_pair_kernel (Bint4 32x32x16 / Bint4 16x16x32 / Aint4) and its activation pre-pass;
// one object per 16-bit type (-DTG_TU_F16); see tg_common.cuh
#include "tg_common.cuh"
#ifdef TG_TU_F16
#define TG_TU_DT F16
#define TG_TU_SUF(n) n##_f16
#else
#define TG_TU_DT BF16
#define TG_TU_SUF(n) n##_bf16
#endif
namespace {
#include "w4_gemm_pair.cuh"
template <typename DT, int I, int GPS, int MR, bool QMX, int NSG, bool XG = false, int LA = 0, bool NORM = false, bool M1_MFMA = false>
int launch_pair_k(const GemmParams& p, PairParams& pp, unsigned lds) {
#ifdef TG_DEV_MIN  // developer builds: only the headline instantiation (fast A/B builds)
#ifndef TG_DEV_GPS
#define TG_DEV_GPS 1
#endif
#ifndef TG_DEV_QMX
#define TG_DEV_QMX false
#endif
#ifndef TG_DEV_MR
#define TG_DEV_MR TG_PAIR_MR1
#endif
#ifndef TG_DEV_LA
#define TG_DEV_LA 0
#endif
  if constexpr (!(std::is_same<DT, BF16>::value && I == 4 && GPS == TG_DEV_GPS && MR == TG_DEV_MR && QMX == TG_DEV_QMX && NSG == TG_DEV_MIN && LA == TG_DEV_LA && !NORM)) return TG_PAIR_NA;
  else {
#endif
  if constexpr (QMX && !std::is_same<DT, BF16>::value) return TG_E_DTYPE;  // mx4 is bf16-only (TinyGemm_int4.cu:758)
  else {
  // several groups per super-tile (group 32 / 64 with wide super-tiles): more per-slot state, one slot in flight fits the
  // 128-VGPR budget without spills (ring depth measured irrelevant between 2 and 4)
  // (mx4 on the 32x32x16 tiles converts its weights in registers and has no per-group state in the slots: the usual depth)
  constexpr int RING = (QMX && LA == 0) ? TG_PAIR_R : (MR == 1 && NSG == 4 && LA == 0) ? 4 : GPS > 1 ? (LA ? TG_PAIR_RA1 : 1) : LA == 1 ? TG_PAIR_RA : LA == 2 ? TG_PAIR_RB16 : TG_PAIR_R;
  if (p.dry) return TG_PLAN_PAIR;
  const unsigned wgs = (unsigned)(pp.items < TG_PAIR_WGS ? pp.items : TG_PAIR_WGS);
  return launch_lds_kernel<w4_gemm_pair_kernel<DT, I, GPS, MR, QMX, RING, NSG, M1_MFMA, XG, LA, NORM>>(dim3(wgs), dim3(512), lds, p.st, pp, false);
  }
#ifdef TG_DEV_MIN
  }
#endif
}

// The lean m = 1 kernel (w4_pair_m1_lean_kernel): a plain stacked call of one activation row -- staged activations, row-major operands,
// no bias / epilogue / fused norm, whole 64-row blocks, partial sums beside the table -- at innerKTiles 4 with a group of one ring round
// (g = 128), int4 / any4.  Every other call keeps the general template.
inline bool pair_lean_call(const GemmParams& p, const PairParams& pp, bool xg) {
  return TG_PAIR_M1_LEAN && TG_PAIR_MR1 == 1 && TG_PAIR_R == 2 && p.m == 1 && !xg && !p.norm_w && !p.bias && !p.epilogue && !p.x_tc && !p.y_tc &&
         p.wrows % 64 == 0 && p.ntiles * 8 == p.wrows && !pp.red_alias && pp.cblocks == 1 && pp.spw % 2 == 0 && p.ksuper % 2 == 0 &&
         p.numerics != TG_NUM_FAST_MFMA;
}
template <typename DT>
int launch_pair_lean(const GemmParams& p, const PairParams& pp, unsigned lds) {
#ifdef TG_DEV_MIN
  if constexpr (!(std::is_same<DT, BF16>::value && TG_DEV_MIN == 2)) return TG_PAIR_NA;
  else {
#endif
  if (p.dry) return p.dry_detail ? (int)TG_PLAN_PAIR_M1_LEAN : (int)TG_PLAN_PAIR;
  PairLeanParams lp;
  copy_call(lp, p);
  lp.spw = pp.spw; lp.lds_x = pp.lds_x; lp.lds_xs = pp.lds_xs; lp.lds_red = pp.lds_red; lp.rblocks = pp.rblocks; lp.items = pp.items;
  const unsigned wgs = (unsigned)(pp.items < TG_PAIR_WGS ? pp.items : TG_PAIR_WGS);
  return launch_lds_kernel<w4_pair_m1_lean_kernel<DT, TG_PAIR_M1_AHEAD != 0>>(dim3(wgs), dim3(512), lds, p.st, lp, false);
#ifdef TG_DEV_MIN
  }
#endif
}

// The activation block of one pass does not fit next to the table (m = 8 at k = 4096, m = 1 at k >= 8192): the XG variant
// takes the activations pre-arranged from a caller-provided workspace (w4_xprep_kernel, one small launch in front).
// Workspace = [batch][m k 2 bytes] arranged activations, then [batch][passes][groups][xs_rows] f32 sums.
template <typename DT>
int launch_xprep(const GemmParams& p, const PairParams& pp, int ma, int la = 0) {
  XPrepParams xq;
  xq.la = la;
  xq.x = pp.x; xq.xp = const_cast<char*>(pp.xp); xq.xsum = const_cast<char*>(pp.xsum);
  xq.x_tc = pp.x_tc;
  xq.m = pp.m; xq.k = pp.k; xq.ma = ma; xq.cps = p.inner / 2; xq.gshift = pp.gshift; xq.gch_mask = pp.gch_mask;
  xq.ngroups = pp.ngroups; xq.xs_rows = pp.xs_rows;
  xq.stride_x = pp.stride_x; xq.stride_xp = pp.stride_xp; xq.stride_xsum = pp.stride_xsum;
  const int64_t chunks = (int64_t)pp.m * (pp.k / 32);
  hipLaunchKernelGGL(w4_xprep_kernel<DT>, dim3((unsigned)cdiv(chunks, 256), (unsigned)p.batch), dim3(256), 0, p.st, xq);
  return launch_status();
}

// m = 1 has its own specialisation (one accumulator register finalised per group, taken as a running difference) -- except
// with several groups per super-tile, where the general kernel's zero-C group starts compile without spills; `norm`: the
// instantiations with LlamaRMSNorm fused into the activation staging (staged activations, m <= 8, not mx4)
template <typename DT, int I, int GPS, bool QMX, int NSG>
int launch_pair_m(const GemmParams& p, PairParams& pp, unsigned lds, bool xg, int mregs) {
  const bool norm = p.norm_w != nullptr;
  const bool m1 = p.m == 1 && TG_PAIR_MR1 == 1 && (QMX || GPS <= TG_PAIR_MR1_GPS);  // (mx4: no per-group state, the specialisation fits at any GPS)
  // Not instantiated (round 4: every one of them compiled with 70 ... 1100 bytes of scratch per lane, and a scratch reload drains
  // the weight ring behind vmcnt(0)): the 32-activation-row accumulator sets (m > 8 on staged activations), innerKTiles 8 beyond the
  // m = 1 kernel of int4 / any4, the fused norm with several groups per super-tile.  Those calls take the next kernel family
  // (16x16x32 tiles with workspace activations, w4_gemm_pair16_kernel, or the reference-numerics kernels).
  if (mregs != 4) return TG_PAIR_NA;
  if constexpr (I == 8) {
    if constexpr (QMX) return TG_PAIR_NA;
    else {
      if (!m1 || norm) return TG_PAIR_NA;
      return xg ? launch_pair_k<DT, I, GPS, 1, false, NSG, true>(p, pp, lds) : launch_pair_k<DT, I, GPS, 1, false, NSG>(p, pp, lds);
    }
  } else {
  if (xg) return m1 ? launch_pair_k<DT, I, GPS, 1, QMX, NSG, true>(p, pp, lds) : launch_pair_k<DT, I, GPS, 4, QMX, NSG, true>(p, pp, lds);
  if (norm) {
    if constexpr (QMX || GPS > 1) return TG_PAIR_NA;
    else {
      return m1 ? launch_pair_k<DT, I, GPS, 1, false, NSG, false, false, true>(p, pp, lds)
                : launch_pair_k<DT, I, GPS, 4, false, NSG, false, false, true>(p, pp, lds);
    }
  }
  if (m1) return launch_pair_k<DT, I, GPS, 1, QMX, NSG>(p, pp, lds);
  return launch_pair_k<DT, I, GPS, 4, QMX, NSG>(p, pp, lds);
  }
}

// ---- what the three launch paths below share: how PairParams is filled from a call ---------------------------------------------

// Group geometry.  A group covers nsg whole super-tiles (g >= 16 I k) or a super-tile holds gps groups; a wave's slice of k (spw
// super-tiles: an eighth of the units of nsg) never cuts a group.
struct PairGroups {
  int gps, nsg;
};
template <int I>
PairGroups pair_groups(const GemmParams& p, PairParams& pp) {
  const int g = 1 << p.gshift;
  const PairGroups r = {g >= 16 * I ? 1 : (16 * I) / g, g >= 16 * I ? g / (16 * I) : 1};
  const int units = p.ksuper / r.nsg;
  pp.spw = ((units + 7) / 8) * r.nsg;
  pp.nsg_shift = 0;
  while ((1 << pp.nsg_shift) < r.nsg) ++pp.nsg_shift;
  pp.gch_mask = g / 32 - 1;
  return r;
}

// mx4: exponent blocks of 16 bytes per row, read at 4-byte alignment (w4_gemm_pair.cuh, e_request)
// (a slice that starts off a 4-byte boundary loses up to 3 bytes of its one block)
inline bool mx4_blocks_fit(const GemmParams& p, const PairParams& pp, int gps) {
  return !(p.ngroups < 16 || p.ngroups % 4 != 0 || ((pp.spw * gps) % 4 != 0 && pp.spw * gps > 12));
}

// LDS plan, in this order: the pair table (64 KiB; mx4 converts its weights in registers, v_cvt_scalef32_pk_bf16_fp4: no table, the
// LDS starts with the activations) | x_bytes of activations and a zero piece of one super-tile | the activation sums per group (mx4:
// no zero point, no sums) | the waves' partial sums.  red_alias: the partial sums reuse the table's LDS instead (`alias`: always;
// `alias_if_large`: when the plan would not leave room for two workgroups per CU, 80 KiB).  Returns the dynamic LDS of the launch.
template <int I, bool QMX>
unsigned pair_lds_plan(const GemmParams& p, PairParams& pp, int x_bytes, bool alias, bool alias_if_large) {
  pp.lds_x = QMX ? 0 : 65536;
  pp.lds_xs = (pp.lds_x + x_bytes + 32 * I + 15) & ~15;
  pp.lds_red = (pp.lds_xs + (QMX ? 0 : p.ngroups * pp.xs_rows * 4) + 15) & ~15;
  unsigned lds = (unsigned)pp.lds_red + (unsigned)(8 * 2 * pp.rused * pp.red_lanes * 4);
  pp.red_alias = alias || (alias_if_large && lds > 80u * 1024u);
  if (pp.red_alias) {
    lds = (unsigned)pp.lds_red;
    pp.lds_red = 0;
  }
  return lds;
}

// Workspace = [batch][xrows k 2 bytes] arranged activations, then [batch][groups][xs_rows] f32 sums (w4_xprep_kernel writes both).
// Returns the bytes; 0: the caller did not bring them.
inline int64_t pair_workspace(const GemmParams& p, PairParams& pp, int xrows) {
  pp.stride_xp = (int64_t)xrows * p.k * 2;
  pp.stride_xsum = ((int64_t)p.ngroups * pp.xs_rows * 4 + 15) & ~(int64_t)15;
  const int64_t need = p.batch * (pp.stride_xp + pp.stride_xsum);
  if (!has_workspace(p, need)) return 0;
  pp.xp = p.ws;
  pp.xsum = p.ws + p.batch * pp.stride_xp;
  return need;
}

template <typename DT, int I, bool QMX>
int launch_pair(GemmParams& p) {
  constexpr int RW = 64;
  const int mregs = p.m <= 8 ? 4 : 16;  // accumulator registers of a row set (8 or 32 activation rows per pass)
  const int ma = 2 * mregs;
  PairParams pp;
  copy_call(pp, p);
  pp.y_tiles = (p.wrows + 15) / 16;
  const auto [gps, nsg] = pair_groups<I>(p, pp);
  const int mrows = p.m < ma ? p.m : ma;
  pp.rused = mrows < 4 ? mrows : mregs;
  pp.xs_rows = mrows <= 4 ? 4 : ma;
  pp.red_lanes = mrows <= 4 ? 32 : 64;
  pp.x_pitch = p.k * 2 + 16;
  // the staged rows; 16 KiB and more of partial sums (more than four rows) reuse the table's LDS
  unsigned lds = pair_lds_plan<I, QMX>(p, pp, mrows * pp.x_pitch, !QMX && mrows > 4, false);
  if (QMX && !mx4_blocks_fit(p, pp, gps)) return TG_PAIR_NA;
  // fused RMSNorm: done in the workgroup's own staging of the whole activation block (its partial sums borrow the activation-sum
  // area, which mx4 does not have); the workspace variant would need it in the pre-pass
  if (p.norm_w && (QMX || lds > 80u * 1024u || p.m > ma)) return TG_PAIR_NA;
  int64_t need = 0;  // XG: the workspace of the launch
  if (lds > 80u * 1024u) {  // two workgroups per CU
    // XG: every wave keeps one super-tile of the pass's activations (<= 8 rows) in a private buffer
    if (mregs != 4 || p.m > ma) return TG_PAIR_NA;
    pp.xw_pitch = 32 * I + 16;
    pp.xw_bytes = (I == 2 ? 16 : 8) * pp.xw_pitch;  // a row for every 2 I lanes of the wave's (unmasked) store
    lds = pair_lds_plan<I, QMX>(p, pp, 8 * pp.xw_bytes, pp.red_alias, true);  // 8 buffers
    if (QMX && pp.red_alias) return TG_PAIR_NA;  // (no table to put the partial sums over; cannot happen: 8 one-KiB buffers + 16 KiB)
    if (lds > 80u * 1024u) return TG_PAIR_NA;
    need = pair_workspace(p, pp, p.m);
    if (!need) return TG_PAIR_NA;
  }
  const bool xg = need != 0;
  pp.rblocks = (p.wrows + RW - 1) / RW;
  pp.cblocks = (p.m + ma - 1) / ma;
  const int64_t items = (int64_t)pp.rblocks * pp.cblocks * p.batch;
  if (items > INT32_MAX) return TG_PAIR_NA;
  // The kernel's unit of work is a 64-row block over the whole k (8 waves): a launch needs about one item per workgroup slot
  // (2 per CU) to fill the chip.  Smaller launches (one 4096-row layer = 64 items) are latency-bound and stay on the
  // split-K kernels, which spread one 16-row tile over up to 16 waves.
  if (items < TG_PAIR_MIN_ITEMS) return TG_PAIR_NA;
  pp.items = (int32_t)items;
  // XG item dealing: chunks of consecutive items once every workgroup still gets several chunks
  pp.chunk = items >= (int64_t)TG_PAIR_WGS * TG_XG_CHUNK * 4 ? TG_XG_CHUNK : 1;
  p.ws_need = need;  // (the call is this family's from here on, but for the gaps in the tables of instantiations below)
  if (xg && !p.dry) {
    const int rc = launch_xprep<DT>(p, pp, ma);
    if (rc != 0) return rc;
  }
  if (gps == 1) {
    // group boundaries at fixed places of the unrolled round when a group is one super-tile or one whole round
    // (the m = 1 specialisation too since its group update is spelled out instruction by instruction: before that, fixed
    //  boundaries made the compiler scatter its accumulator chain over several register tuples and spill)
    // (a group of ONE super-tile, g = 64 at I = 4, also keeps the run-time test: its fixed-boundary build spills 27 registers,
    //  m = 8 50 % against 59 %)
    const bool fixed = TG_PAIR_NSG2 && (TG_PAIR_NSG2_M1 || !(p.m == 1 && TG_PAIR_MR1 == 1));
    // TG_NUM_FAST_MFMA: the headline shape's m = 1 kernel with the 32x32x16 MFMA as its contraction (north_star: "dequantized
    // in-register and fed to bf16 MFMA") instead of the per-lane v_dot2 the default takes -- one instantiation, g = 128 at innerKTiles 4
    if constexpr (I == 4 && !QMX) {
      if (p.numerics == TG_NUM_FAST_MFMA && p.m == 1 && !xg && !p.norm_w && fixed && nsg == TG_PAIR_R)
        return launch_pair_k<DT, I, 1, 1, false, TG_PAIR_R, false, 0, false, true>(p, pp, lds);
    }
    if constexpr (I == 4 && !QMX) {
      if (fixed && nsg == TG_PAIR_R && pair_lean_call(p, pp, xg)) return launch_pair_lean<DT>(p, pp, lds);
    }
    if (fixed && nsg == TG_PAIR_R) return launch_pair_m<DT, I, 1, QMX, TG_PAIR_R>(p, pp, lds, xg, mregs);
    // m = 1, a group of ONE super-tile (g = 64 at innerKTiles 4): fixed boundaries too since the dot2 contraction freed the registers
    // (with the MFMA this build spilled 27; 77 -> 81 %), and a group of FOUR super-tiles (g = 256) as one round of a ring of four
    // (76.7 -> 84.0 %; a ring of four at g = 128 / 64 measured 1-1.5 points below the ring of two).  Only the m = 1 kernels are
    // instantiated for these (launch_pair_k directly: launch_pair_m would drag the general kernels in as well).
    if constexpr (!QMX) {
      if (fixed && p.m == 1 && TG_PAIR_MR1 == 1 && !p.norm_w && (nsg == 1 || nsg == 4)) {
        if (nsg == 1) return xg ? launch_pair_k<DT, I, 1, 1, false, 1, true>(p, pp, lds) : launch_pair_k<DT, I, 1, 1, false, 1>(p, pp, lds);
        if constexpr (I <= 4)  // (innerKTiles 8: four super-tiles would be g = 512)
          return xg ? launch_pair_k<DT, I, 1, 1, false, 4, true>(p, pp, lds) : launch_pair_k<DT, I, 1, 1, false, 4>(p, pp, lds);
      }
    }
    return launch_pair_m<DT, I, 1, QMX, 0>(p, pp, lds, xg, mregs);
  }
  if constexpr (I >= 4) {
    if (gps == 2) return launch_pair_m<DT, I, 2, QMX, 0>(p, pp, lds, xg, mregs);
  }
  if constexpr (I >= 8) {
    if (gps == 4) return launch_pair_m<DT, I, 4, QMX, 0>(p, pp, lds, xg, mregs);
  }
  return TG_PAIR_NA;
}

// The 16x16x32 structure: 32 weight rows per work item, v_mfma_f32_16x16x32, a duplicated table, the activations of ONE pass -- all
// m <= 16 rows -- always through the workspace and from there straight into the MFMA operand (LDS only holds a zero piece).
//   LA = 1  Aint4 weights (weightOnRight = false): row-major operands only.
//   LA = 2  Bint4 weights with 9 ... 16 activation rows: one packed word is one B operand, 4 vector ops per word.  (The 32x32x16
//           kernel holds 8 rows per pass; a second pass would stream the weights twice.)
template <typename DT, int I, bool QMX, int LA>
int launch_pair_la(GemmParams& p) {
  if constexpr (LA == 1 && I < 2) return TG_PAIR_NA;  // one 16-k tile per word set: no word pair for a 32-k MFMA step
  else {
  constexpr bool B = LA == 2;
  constexpr int RING = B ? TG_PAIR_RB16 : TG_PAIR_R;  // the group length with fixed boundaries in the unrolled round
  if (p.m > 16 || p.norm_w || p.epilogue || (!B && (p.x_tc || p.y_tc))) return TG_PAIR_NA;
  PairParams pp;
  copy_call(pp, p);
  pp.y_tiles = (p.wrows + 15) / 16;
  const auto [gps, nsg] = pair_groups<I>(p, pp);
  if (QMX && !mx4_blocks_fit(p, pp, gps)) return TG_PAIR_NA;
  const int mrows = p.m;
  pp.rused = mrows < 4 ? mrows : 4;
  pp.xs_rows = mrows <= 4 ? 4 : mrows <= 8 ? 8 : 16;
  pp.red_lanes = mrows <= 8 ? 32 : 64;  // lanes 0..31 hold activation rows 0..7
  pp.x_pitch = 0;
  pp.xw_pitch = 0;
  pp.xw_bytes = 0;
  const unsigned lds = pair_lds_plan<I, QMX>(p, pp, 0, false, true);
  if (lds > 80u * 1024u) return TG_PAIR_NA;
  pp.rblocks = (p.wrows + 31) / 32;
  pp.cblocks = 1;
  const int64_t items = (int64_t)pp.rblocks * p.batch;
  // (LA = 2: 32-row items, two per 64-row item of the 32x32x16 kernel that TG_PAIR_MIN_ITEMS was measured on)
  if (items > INT32_MAX || items < (B ? 2 : 1) * TG_PAIR_MIN_ITEMS) return TG_PAIR_NA;
  p.ws_need = pair_workspace(p, pp, p.m + 1);  // + a zero row
  if (!p.ws_need) return TG_PAIR_NA;
  pp.items = (int32_t)items;
  // Aint4: plain round-robin dealing (chunks of consecutive items measured slower for the 32-row items of this layout)
  pp.chunk = B && items >= (int64_t)TG_PAIR_WGS * TG_B16_CHUNK * 4 ? TG_B16_CHUNK : 1;
  if (!p.dry) {
    const int rc = launch_xprep<DT>(p, pp, 16, 1);
    if (rc != 0) return rc;
  }
  if (gps == 1) {
    if (TG_PAIR_NSG2 && nsg == 1) return launch_pair_k<DT, I, 1, 4, QMX, 1, true, LA>(p, pp, lds);
    if (TG_PAIR_NSG2 && nsg == RING) return launch_pair_k<DT, I, 1, 4, QMX, RING, true, LA>(p, pp, lds);
    return launch_pair_k<DT, I, 1, 4, QMX, 0, true, LA>(p, pp, lds);
  }
  if constexpr (I >= 4) {
    if (gps == 2) return launch_pair_k<DT, I, 2, 4, QMX, 0, true, LA>(p, pp, lds);
  }
  return TG_PAIR_NA;  // (four groups per super-tile are innerKTiles 8, which has no 16x16x32 instantiation: tgx::pair_b16)
  }
}

}  // namespace
namespace tgx {
int TG_TU_SUF(pair)(GemmParams& p) {  // (innerKTiles 2, 4, 8)
  return pick<2, 4, 8>(p.inner, [&](auto I_) {
    return pick<0, 1>(p.qmx, [&](auto QMX_) { return launch_pair<TG_TU_DT, decltype(I_)::value, (decltype(QMX_)::value != 0)>(p); });
  });
}
int TG_TU_SUF(pair_a)(GemmParams& p) {  // (innerKTiles 1, 2, 4)
  return pick<1, 2, 4>(p.inner, [&](auto I_) {
    return pick<0, 1>(p.qmx, [&](auto QMX_) { return launch_pair_la<TG_TU_DT, decltype(I_)::value, (decltype(QMX_)::value != 0), 1>(p); });
  });
}
int TG_TU_SUF(pair_b16)(GemmParams& p) {
  // (innerKTiles 8 on the 16x16x32 tiles compiled with > 100 bytes of scratch per lane: not instantiated)
  return pick<2, 4>(p.inner, [&](auto I_) {
    return pick<0, 1>(p.qmx, [&](auto QMX_) { return launch_pair_la<TG_TU_DT, decltype(I_)::value, (decltype(QMX_)::value != 0), 2>(p); });
  });
}
}  // namespace tgx
