// tg_pair16.hip -- launch path of w4_gemm_pair16_kernel (one layer per launch); see tg_common.cuh
#include "tg_common.cuh"
#if GEMV_TRACE
static TraceRing g_p16_trace;
extern "C" TG_API void tg_dev_p16_trace(unsigned long long* buf, int slots) { g_p16_trace.set(buf, slots); }
#endif
namespace {
#include "w4_helpers.cuh"
#include "w4_gemm_pair16.cuh"
#include "w4_gemm_pair16_loop.cuh"
#ifndef TG_P16_XREG_MIN_M
#define TG_P16_XREG_MIN_M 5  // activation rows from which the A operands are arranged in registers instead of staged through LDS
#endif
// Small launches of Bint4 weights (one layer per call): w4_gemm_pair16_kernel, 16 weight rows per workgroup, the whole k-slice
// of a wave requested up front.  Taken when the launch is too small for the persistent kernel (or its LDS plan does not fit)
// and the activations (m <= 16 rows) fit in LDS next to the table.
template <typename DT, int I, bool QMX>
int launch_pair16(const GemmParams& p) {
  const int64_t batch = p.batch;
  if constexpr (QMX && !std::is_same<DT, BF16>::value) return TG_E_DTYPE;  // mx4 is bf16-only (TinyGemm_int4.cu:758)
  else {
#ifdef TG_DEV_MIN
  if constexpr (!(std::is_same<DT, BF16>::value && I == 4 && !QMX)) return TG_PAIR_NA;
#endif
  if (p.m > 16 || batch > 65535) return TG_PAIR_NA;
  // m = 1 and more than one round of workgroups (one per CU): the streaming kernel's split-K launches are faster there
  // (per hipGraph node, 6144 x 4096: 8.6 us against 10.2 us; 14336 x 4096: 13.8 against 18.3)
  // (not when a fused stage is asked for: only the pair-table kernels have them)
  if (p.m == 1 && !p.x_tc && !p.y_tc && !p.norm_w && !p.epilogue && (int64_t)((p.wrows + 15) / 16) * batch > 256 && (1 << p.gshift) >= 128) return TG_PAIR_NA;
  if (p.norm_w && (QMX || (int64_t)p.m * p.k > 32768)) return TG_PAIR_NA;  // the norm pass: one 32-k chunk per thread
  const int g = 1 << p.gshift;
  const int nsg = g >= 16 * I ? g / (16 * I) : 1;
  Pair16Params pp;
  copy_call(pp, p);
  pp.gch_mask = g / 32 - 1;
  pp.lds_x = 65536;
  const int64_t wgs = (int64_t)((p.wrows + 15) / 16) * batch;
  // one workgroup per CU may take the whole LDS; a launch of more than two rounds of workgroups should fit two per CU
  const unsigned lds_limit = (wgs <= 512 ? 160u : 80u) * 1024u;
  // activation rows that do not fit next to the table are staged one part of k at a time (whole groups per part)
  unsigned lds = 0;
  int phases = 1;
  // XREG (w4_gemm_pair16.cuh): no LDS for activations, one pass whatever m x k is; one workgroup per CU (two rounds at most)
  bool xreg = p.m >= TG_P16_XREG_MIN_M && !p.norm_w && wgs <= 512 && p.ksuper % nsg == 0;
  if (xreg && g == 32 && I == 4 && ((p.ksuper / nsg + 15) / 16) * nsg > 4) xreg = false;  // (see the selection below: that instantiation spills)
  if (xreg) {
    pp.x_pitch = 0;
    pp.lds_xs = pp.lds_x;
    lds = 65536u;
  } else
  for (; phases <= (wgs <= 512 && !p.norm_w ? 8 : 1); phases *= 2) {  // (the fused norm needs a row's whole k in one part)
    if (p.ksuper % (phases * nsg) != 0 || p.ngroups % phases != 0) return TG_PAIR_NA;
    const int kp = p.k / phases;
    pp.x_pitch = kp * 2 + 16;
    pp.lds_xs = (pp.lds_x + p.m * pp.x_pitch + 16 + 15) & ~15;
    lds = (unsigned)pp.lds_xs + (QMX ? 0u : (unsigned)(p.ngroups / phases) * 64u);
    if (lds <= lds_limit) break;
  }
  if (lds > lds_limit) return TG_PAIR_NA;
  if (xreg) phases = 1;
  pp.phases = phases;
  pp.ksuper_p = p.ksuper / phases;
  pp.spw = ((pp.ksuper_p / nsg + 15) / 16) * nsg;
  pp.y_tiles = (p.wrows + 15) / 16;
  if (p.dry) return TG_PLAN_PAIR;
  const dim3 grid((unsigned)((p.wrows + 15) / 16), (unsigned)batch);
#if GEMV_TRACE
  pp.trace = grid.x <= 512 ? g_p16_trace.next() : nullptr;
#endif
  // the kernel: NORM (the fused norm), else XREG with the whole slice in one block (CH = 4) or in two register sets (CH = 2), else the LDS path
  // (xreg excludes the norm: see above)
  return pick<1, 2, 4, 8>(QMX ? 1 : g / 32, [&](auto CPG_) {  // (g = 32, 64, 128, 256; mx4: group = 32)
    return pick<0, 1>(p.norm_w != nullptr, [&](auto NORM_) {
      return pick<0, 1>(xreg, [&](auto XREG_) {
        return pick<2, 4>(xreg && pp.spw > 4 ? 2 : 4, [&](auto CH_) {
          return pick<0, 1>(xreg && p.x_tc, [&](auto XTC_) {
            constexpr int CPG = decltype(CPG_)::value, CH = decltype(CH_)::value;
            constexpr bool NORM = decltype(NORM_)::value, XREG = decltype(XREG_)::value, XTC = decltype(XTC_)::value;
            // (groups of 32 at innerKTiles 4 with slices longer than a block: 84 ... 128 bytes of scratch -- not instantiated, the LDS path)
            if constexpr ((QMX && (CPG != 1 || NORM)) || (NORM && XREG) || (!XREG && (CH != 4 || XTC)) || (XREG && CH == 2 && CPG == 1 && I == 4)) {
              return (int)TG_PAIR_NA;
            } else {
              return launch_lds_kernel<w4_gemm_pair16_kernel<DT, I, QMX, CPG, 1, NORM, XREG, CH, XTC>>(grid, dim3(1024), lds, p.st, pp, false);
            }
          });
        });
      });
    });
  });
  }
}

// ONE layer per launch with more 16-row tiles than compute units (w4_gemm_pair16_loop.cuh): 5 ... 16 activation rows, k = 4096, innerKTiles 4,
// row-major operands, no fused stage; a workgroup owns up to 32 tiles.
#ifndef TG_P16_LOOP_MAX_TILES
#define TG_P16_LOOP_MAX_TILES 8   // tiles per workgroup up to which this path takes the launch.  Per graph node at m = 16, rows 5120 / 8192 / 11008 / 12288 /
                                  // 14336 / 16384 / 20480 / 28672: 8.5 / 9.0 / 10.8 / 10.9 / 13.0 / 13.1 / 15.2 / 19.5 us here; w4_gemm_xr_kernel with one workgroup per
                                  // 64-row item: 12.3 / 12.4 / 12.6 / - / 13.2 / 13.7 / - / 19.4 (profiles/r05_ab_p16_loop.txt, r05_p16_loop_sweep.txt)
#endif
template <typename DT>
int launch_pair16_loop(const GemmParams& p) {
  if (p.batch != 1 || p.m < TG_P16_XREG_MIN_M || p.m > 16 || p.k != 4096 || p.ksuper != 64 || (p.epilogue && (p.epilogue != TG_EPI_SWIGLU || p.bias || p.wrows % 16 != 0)) || p.x_tc || p.y_tc ||
      p.qtype == TG_Q_MX4)
    return TG_PAIR_NA;
  if (p.norm_w && p.gshift == 5) return TG_PAIR_NA;  // (groups of 32 with the fused norm: not instantiated, see the kernel)
  const int tiles = (p.wrows + 15) / 16;
  const int cus = plan_cu_count(p);
  if (tiles <= cus) return TG_PAIR_NA;  // (one tile per workgroup: w4_gemm_pair16_kernel)
  const int per = (tiles + cus - 1) / cus;
  if (per > TG_P16_LOOP_MAX_TILES || per > 32) return TG_PAIR_NA;
  Pair16LoopParams pp;
  copy_call(pp, p);
  pp.tbase = tiles / cus; pp.trem = tiles % cus;
  pp.lds_red = 65536;
  pp.lds_lut = 65536 + 2 * 16384;
  pp.lds_nrm = pp.lds_lut + (p.qtype == TG_Q_ANY4_ROWWISE ? per * 544 : 0);
  const unsigned lds = (unsigned)pp.lds_nrm + 16u * 16u * 4u;
  if (p.dry) return TG_PLAN_PAIR;
  const int g = 1 << p.gshift;
  return pick<1, 2, 4, 8>(g / 32, [&](auto CPG_) {  // (g = 32, 64, 128, 256)
    return pick<0, 1>(p.norm_w != nullptr, [&](auto NORM_) {
      constexpr int CPG = decltype(CPG_)::value;
      constexpr bool NORM = decltype(NORM_)::value;
      if constexpr (NORM && CPG == 1) {  // (groups of 32 with the fused norm: not instantiated, see the kernel)
        return (int)TG_PAIR_NA;
      } else {
        return launch_lds_kernel<w4_gemm_pair16_loop_kernel<DT, CPG, NORM>>(dim3((unsigned)cus), dim3(1024), lds, p.st, pp, false);
      }
    });
  });
}

}  // namespace
int tgx::pair16_loop(const GemmParams& p) {
  if (p.inner != 4 || p.qmx) return TG_PAIR_NA;
  return pick_dt(p.dt, [&](auto DT_) { return launch_pair16_loop<decltype(DT_)>(p); });
}
int tgx::pair16(const GemmParams& p) {
  return pick_dt(p.dt, [&](auto DT_) {
    // (innerKTiles 8: every instantiation compiled with 76 ... 308 bytes of scratch per lane at the 128-VGPR budget of a 1024-thread
    //  workgroup -- not instantiated; those layers take the streaming kernels)
    return pick<2, 4>(p.inner, [&](auto I_) {
      return pick<0, 1>(p.qmx, [&](auto QMX_) { return launch_pair16<decltype(DT_), decltype(I_)::value, (decltype(QMX_)::value != 0)>(p); });
    });
  });
}
