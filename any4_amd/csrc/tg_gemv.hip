// tg_gemv.hip -- launch path of w4_gemv_kernel (one layer per launch, 1 ... 4 activation rows: the GEMMs of a batch-1 decode step
// and of Any4Linear.forward / Int4Linear.forward at batch 1); see tg_common.cuh and w4_gemv.cuh
#include "tg_common.cuh"
namespace {
#include "w4_helpers.cuh"
#include "w4_gemv.cuh"

#ifndef TG_GEMV_MF_MIN_M
#define TG_GEMV_MF_MIN_M 1  // activation rows from which the contraction runs on the matrix core where its conditions hold (k <= 4096, groups
                            // of 128 / 256).  Same box, per graph node, v_dot2 -> matrix core: m = 1: 4096^2 5.10 -> 4.92 us, 28672 x 4096
                            // 15.4 -> 14.85, the decode step 622 -> 630 tokens/s; m = 2: 5.8 -> 5.1, 19.3 -> 14.9, decode at batch 2
                            // 1054 -> 1173 tokens/s (the kernel's bound was vector-ALU issue; profiles/r04_ab_gemv_mf_min_m.txt)
#endif
#ifndef TG_GEMV_MAX_TILES
#define TG_GEMV_MAX_TILES 16384  // 8-row tiles per launch up to which this kernel takes single-problem launches (131072 rows)
#endif
}  // namespace

#if GEMV_TRACE
static TraceRing g_trace;
extern "C" TG_API void tg_dev_gemv_trace(unsigned long long* buf, int slots) { g_trace.set(buf, slots); }
#endif

int tgx::gemv(const GemmParams& p) {
  const int g0 = 1 << p.gshift;
  // matrix-core contraction: 16-row passes of two super-tiles per step inside ONE group, a piece per thread in the staging
#ifndef TG_GEMV_MF_MAX_M
#define TG_GEMV_MF_MAX_M 8  // (developer A/B against w4_gemm_pair16_kernel / the loop kernel at 5 ... 8 rows)
#endif
  const bool mf = p.m >= TG_GEMV_MF_MIN_M && p.m <= TG_GEMV_MF_MAX_M && (g0 == 128 || g0 == 256) && (p.k <= 4096 || p.m <= 4) && p.ksuper % 2 == 0;
  if (p.inner != 4 || p.qmx || (p.m > 4 && !mf) || p.x_tc || p.y_tc || p.batch != 1) return TG_PAIR_NA;
  if (p.ksuper * 64 != p.k || p.ntiles * 8 != p.wrows || p.ntiles > TG_GEMV_MAX_TILES) return TG_PAIR_NA;
  const int g = 1 << p.gshift;
  const int gps = g == 32 ? 2 : 1;
  GemvParams gp;
  copy_call(gp, p);
  gp.sg_shift = g <= 64 ? 0 : g == 128 ? 1 : 2;
  gp.trace = nullptr;
  // (per graph node, same box: 4096^2 m = 8 6.74 -> 6.50 us, 6144 rows 9.2 -> 8.7, m = 6 + 1.6 %, m = 5 - 2 %: from six rows on;
  //  profiles/r05_ab_gemv_chunk_staging.txt)
  gp.cm = (mf && p.m >= 6 && (p.k == 4096 || p.k == 2048)) ? 1 : 0;
  gp.unit = p.epilogue == TG_EPI_SWIGLU ? 2 : 1;
  if (p.ntiles % gp.unit != 0) return TG_PAIR_NA;
  const int units = p.ntiles / gp.unit;
  const int cus = plan_cu_count(p);
  // one workgroup per CU (two per CU were measured on gate_up of Llama-3-8B: the second workgroup of a CU trails the first by 3 us
  // through its prologue and the launch ends no earlier -- the CU's instruction issue, not latency, bounds the main loop)
  // ... except for the longest layers: a dependent graph node that streams 64 MiB takes 14.3 us from one workgroup per CU and 13.1 us
  // from two (tools/ubench/graph_chain.hip, round 5: 32 MiB equal, 8 MiB slower) -- more requests in flight per CU, and with the
  // contraction on the matrix core (MF) the vector ALU no longer bounds the main loop
#ifndef TG_GEMV_WG2_MIN_BYTES
#define TG_GEMV_WG2_MIN_BYTES (48ll << 20)
#endif
  // (both workgroups of a CU must fit its 160 KiB of LDS together: the formula of `lds` below for the halved ranges)
  auto lds_two_per_cu = [&]() -> int64_t {
    const int tpw2 = ((units + 2 * cus - 1) / (2 * cus)) * gp.unit;
    const int64_t xs = (int64_t)p.m * (p.k / 4), xsmf = mf ? (int64_t)(p.k / 128) * 64 : 0;
    return 65536 + (p.qtype == TG_Q_ANY4_ROWWISE ? tpw2 * 8 * 32 : 0) + (int64_t)p.m * (p.k * 2 + (p.m > 1 ? 16 : 0)) + (xsmf > xs ? xsmf : xs) +
           2 * 8 * p.m * 32 * 4 + 8 * p.m * 4;
  };
  // (... and the halved ranges must not pad more 16-row passes than the whole ones: 28672 rows as 7-tile ranges run 4 passes where
  //  14-tile ranges run 7 -- 15.3 -> 16.4 us; the same layer with SwiGLU tile pairs, 8- and 6-tile ranges: the decode step -2.2 %)
  auto padded_tiles = [&](int n_wgs) -> int64_t {
    const int ub = units / n_wgs, ur = units % n_wgs;
    auto pad2 = [&](int u) -> int64_t { return (int64_t)((u * gp.unit + 1) / 2) * 2; };
    return ur * pad2(ub + 1) + (int64_t)(n_wgs - ur) * pad2(ub);
  };
#ifndef TG_GEMV_WG2_MIN_UNITS_PER_CU
#define TG_GEMV_WG2_MIN_UNITS_PER_CU 4
#endif
  const bool two_per_cu = (int64_t)p.wrows * p.k / 2 >= TG_GEMV_WG2_MIN_BYTES && units >= TG_GEMV_WG2_MIN_UNITS_PER_CU * cus && lds_two_per_cu() <= 80 * 1024 &&
                          padded_tiles(2 * cus) <= padded_tiles(cus);
  const int wgs = units < cus ? units : (two_per_cu ? 2 * cus : cus);
  gp.ubase = units / wgs;
  gp.urem = units % wgs;
  gp.uextra = 1;
  // Two workgroups per CU: the workgroups 0 ... cus - 1 are the first on their CU and through their prologue ~2 us before the second
  // ones (dev/gemv_trace.py).  TG_GEMV_WG2_EXTRA = E (odd) deals them E units more than the second ones instead of one (units a
  // multiple of the CU count: Llama-3-8B's gate_up, 7 SwiGLU units per CU as 4 + 3)
  // Same box, the decode step: 4 + 3 (E = 1) 1.523-1.545 ms, 5 + 2 (E = 3) **1.490-1.498**, 6 + 1 (E = 5) 1.542-1.550
  // (profiles/r05_ab_gemv_wg2_extra.txt)
#ifndef TG_GEMV_WG2_EXTRA
#define TG_GEMV_WG2_EXTRA 3
#endif
  if (TG_GEMV_WG2_EXTRA > 1 && two_per_cu && wgs == 2 * cus && units % cus == 0 && (units / cus) % 2 == 1 && units / cus > TG_GEMV_WG2_EXTRA) {
    gp.ubase = (units / cus - TG_GEMV_WG2_EXTRA) / 2;
    gp.urem = cus;
    gp.uextra = TG_GEMV_WG2_EXTRA;
  }
  gp.uh = 0;  // (always: 64 / 128 / 192 of the CUs on 5 + 2 and the rest on 4 + 3 measured slower than 5 + 2 everywhere, the decode step 1.486-1.50 against 1.470-1.479 ms; profiles/r05_ab_gemv_wg2_half.txt)
  const int tpw = (gp.ubase + (gp.urem ? gp.uextra : 0)) * gp.unit;  // tiles of the largest range
  // Ranges of THREE tiles at one activation row (q/k/v of Llama-3-8B: 6144 rows over 256 CUs) keep the matrix-core contraction: two
  // 16-row passes carry a padding tile (4 tile slots for 3 tiles), but three 8-row passes of the v_dot2 contraction, which would stream
  // exactly the range, measured SLOWER (6144 x 4096 per graph node 6.8 -> 7.2 us, the decode step unchanged; profiles/r05_ab_gemv_odd_p8.txt)
  // rows per pass of ranges longer than two tiles: 16 (two super-tiles of k per ring step), not 32 -- a range is rarely a multiple of
  // four tiles (Llama-3-8B: gate_up 14, q/k/v 3) and the padding tiles of its last pass cost what real ones do.  Same box, per graph
  // node, 32 -> 16: 28672 x 4096 17.6 -> 16.2-16.6 us, 8192 rows 7.6 -> 6.4, 10240 11.2 -> 8.9, 12288 10.8 -> 8.4, 32768 (a multiple
  // of four tiles) 16.5 -> 16.7; 8-row passes 22.5 us at 28672 rows; the decode step 1.667 -> 1.600 ms (profiles/r04_ab_gemv_pass_rows.txt)
#ifndef TG_GEMV_P_BIG
#define TG_GEMV_P_BIG 16
#endif
  gp.P = mf ? 16 : tpw <= 1 ? 8 : tpw <= 2 ? 16 : TG_GEMV_P_BIG;
  // a step covers SS = 32 / P consecutive super-tiles: they must all lie inside the matrix (the kernel's addressing has no per-lane
  // clamp), so k = 64 x odd runs 32-row passes whatever the range, k = 128 x odd at least 16-row passes
  if (p.ksuper % 2 != 0) gp.P = 32;
  else if (p.ksuper % 4 != 0 && gp.P < 16) gp.P = 16;
  gp.p_shift = gp.P == 8 ? 3 : gp.P == 16 ? 4 : 5;
  const int tpp = gp.P / 8;
  const int passes = (tpw + tpp - 1) / tpp;
  const int SS = 32 / gp.P;
  gp.spw = ((p.ksuper + 7) / 8 + SS - 1) / SS * SS;  // a wave's slice: whole steps
  gp.spp = gp.spw / SS;
  const int d = gp.spp <= 4 ? 4 : 8;  // ring depth: a pass occupies whole rounds of D slots
  gp.rounds = (gp.spp + d - 1) / d;
  gp.xcd4 = (gp.urem == 0 && wgs % 32 == 0) ? 1 : 0;
  if (p.k > 16384) return TG_PAIR_NA;  // a thread keeps its pieces of the activation block in registers: four rounds of 512 per row
  gp.lds_lut = 65536;
  const bool stage_lut = p.qtype == TG_Q_ANY4_ROWWISE && passes > 1;
  gp.x_pitch = p.k * 2 + (p.m > 1 ? 16 : 0);
  gp.lds_x = gp.lds_lut + (stage_lut ? tpw * 8 * 32 : 0);
  gp.xs_pitch = p.k / 4;
  gp.lds_xs = gp.lds_x + p.m * gp.x_pitch;
  // (matrix-core contraction: the sums are [step of 128 k][16 rows] f32 instead -- more than one row's k / 4 bytes)
  gp.lds_red = gp.lds_xs + (mf && (p.k / 128) * 64 > p.m * gp.xs_pitch ? (p.k / 128) * 64 : p.m * gp.xs_pitch);
  gp.lds_nrm = gp.lds_red + 2 * 8 * p.m * 32 * 4;
  const unsigned lds = (unsigned)gp.lds_nrm + (unsigned)(8 * p.m * 4);
  if (lds > 160u * 1024u) return TG_PAIR_NA;
  if (p.dry) return TG_PLAN_GEMV;
  const dim3 grid((unsigned)wgs, (unsigned)p.batch);
#if GEMV_TRACE
  gp.trace = g_trace.next();
#endif
  return pick_dt(p.dt, [&](auto DT_) {
    using DT = decltype(DT_);
    // (p.m: 1 ... 4, the matrix-core contraction 1 ... 8; gps: 1, 2; d: 4, 8 -- the tests and the plan above)
    return pick<1, 2, 3, 4, 5, 6, 7, 8>(p.m, [&](auto M_) {
      return pick<1, 2>(gps, [&](auto GPS_) {
        return pick<4, 8>(d, [&](auto D_) {
          return pick<0, 1>(p.norm_w != nullptr, [&](auto NORM_) {
            return pick<0, 1>(mf, [&](auto MF_) {
              constexpr int M = decltype(M_)::value, GPS = decltype(GPS_)::value, D = decltype(D_)::value;
              constexpr bool NORM = decltype(NORM_)::value, MF = decltype(MF_)::value;
              // the matrix-core contraction (w4_gemv.cuh, MF): 3 ... 8 rows, one group per step, ring of four (k <= 4096: four steps per pass)
              // (k > 4096: slices of more than four steps; up to four rows -- the activation block has to fit next to the table)
              if constexpr (MF ? (M < TG_GEMV_MF_MIN_M || GPS != 1 || (D == 8 && M > 4)) : M > 4) {
                return (int)TG_PAIR_NA;
              } else {
                return launch_lds_kernel<w4_gemv_kernel<DT, M, GPS, D, NORM, MF>>(grid, dim3(512), lds, p.st, gp, true);  // (a part with less LDS: the older kernels take over)
              }
            });
          });
        });
      });
    });
  });
}
