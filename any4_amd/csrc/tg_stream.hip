// tg_stream.hip -- launch path of w4_gemm_stream_kernel (reference numerics); one object per 16-bit type (-DTG_TU_F16); see tg_common.cuh
#include "tg_common.cuh"
#ifdef TG_TU_F16
#define TG_TU_DT F16
#define TG_TU_FN stream_f16
#else
#define TG_TU_DT BF16
#define TG_TU_FN stream_bf16
#endif
namespace {
#include "w4_gemm_stream.cuh"
#ifndef STREAM_MINW
#define STREAM_MINW 4
#endif
// Bint4, TG_STREAM_LK_MIN <= m <= 15: the lookup block with the X fragment read under an EXEC mask (w4_gemm_stream.cuh, LK).  Same-box
// A/B at 4096^2, reference numerics: m = 8 46.9 -> 50.1 % of the roofline; m = 4 50.9 -> 49.8 and m = 1 55.6 -> 54.9 (the block's
// lgkmcnt(0) costs more than the few lanes' reads save); m = 16 reads with every lane either way.
#ifndef TG_STREAM_LK_MIN
#define TG_STREAM_LK_MIN 6
#endif
// ---- streaming kernel launch ---------------------------------------------------------------------
// LDS per workgroup: lookup tables (4 KiB per wave and row set) + two X slabs (+ split-K tiles).
template <bool LAYOUT_A>
inline unsigned stream_lds_bytes(int sw, int mrows, int sk, bool privx = false) {
  const unsigned nr = 1u;  // lookup tables per wave
  const unsigned unit = LAYOUT_A ? 64u : 128u;
  // shared slab: rows of all k-slices; private slabs: one per wave with the rows of its own slice; + the all-zero row
  const unsigned slab = (unsigned)(mrows * 4 * (privx ? 1 : sk) + 1) * (unit * 2u + 16u);
  return (unsigned)sw * nr * 4096u + 2u * slab * (privx ? (unsigned)sw : 1u) + (sk > 1 ? (unsigned)sw * nr * 1024u : 0u);
}

template <typename DT, bool LAYOUT_A, int WPL, bool QMX, int SW, bool privx = (SW == 1)>
int launch_stream_sw(const GemmParams& p, StreamParams& sp, int sk) {
  constexpr int UNIT = LAYOUT_A ? 64 : 128;
  constexpr unsigned NR = 1u;
  const int nunits = (sp.k + UNIT - 1) / UNIT;
  const int upg = (1 << sp.gshift) / UNIT;  // units per quantisation group (>= 1)
  const int mrows = sp.m < 16 ? sp.m : 16;
  int nu = (nunits + 4 * sk - 1) / (4 * sk);
  nu = (nu + upg - 1) / upg * upg;
  sp.splitk = sk;
  sp.sk_shift = 0;
  while ((1 << sp.sk_shift) < sk) ++sp.sk_shift;
  sp.units_per_lane = nu;
  sp.upg_mask = upg - 1;
  const int xrows = mrows * 4 * (privx ? 1 : sk);
  sp.xslab_bytes = (xrows + 1) * (UNIT * 2 + 16);
  sp.red_off = (int32_t)(SW * NR * 4096u + 2u * (unsigned)sp.xslab_bytes * (privx ? SW : 1));
  const int pieces = xrows * (UNIT * 2 / 16);
  // privx: every wave stages its own X slab (no barrier in the main loop)
  const int nstage = privx ? 64 : SW * 64;
  const int xl = pieces <= nstage ? 1 : (pieces <= 2 * nstage ? 2 : 4);
  const unsigned lds = stream_lds_bytes<LAYOUT_A>(SW, mrows, sk, privx);
  const int tpb = SW / sk;
  const dim3 grid((unsigned)((sp.rowtiles + tpb - 1) / tpb), (unsigned)coltiles(p), (unsigned)p.batch);
  if constexpr (privx && SW > 1) {
    if (xl != 1) return TG_E_SHAPE;  // private slabs with split-K are only instantiated for one piece per lane (m = 1)
  }
  if (p.dry) return TG_PLAN_STREAM;
  const bool lk = !LAYOUT_A && !privx && sp.m >= TG_STREAM_LK_MIN && sp.m <= 15;
  // (one wave, SW = 1: more than one piece per lane is XL = 2; private slabs with split-K: XL = 1, see above)
  return pick<1, 2, 4>(SW == 1 && xl == 4 ? 2 : xl, [&](auto XL_) {
    return pick<0, 1>(lk, [&](auto LK_) {
      constexpr int XL = decltype(XL_)::value, LK = decltype(LK_)::value;
      if constexpr ((privx && SW > 1 && XL != 1) || (SW == 1 && XL == 4) || (LK && (LAYOUT_A || privx))) {
        return (int)TG_PAIR_NA;
      } else {
        return launch_lds_kernel<w4_gemm_stream_kernel<DT, LAYOUT_A, WPL, QMX, SW, STREAM_MINW, XL, privx, false, LK>>(grid, dim3(SW * 64), lds, p.st, sp, false);
      }
    });
  });
}

// Resident-X launch: 16-wave workgroups, the whole [mrows][k] activation block staged once per workgroup.
template <typename DT, bool LAYOUT_A, int WPL, bool QMX>
int launch_stream_xres(const GemmParams& p, StreamParams& sp, unsigned lds) {
  // one workgroup walks up to 4 consecutive groups of 16 tiles of its layer (X staged once, tile-granularity tail
  // amortised) as long as that leaves at least two workgroups per CU
  int tpw = 4;
  while (tpw > 1 && ((sp.rowtiles + 16 * tpw - 1) / (16 * tpw)) * coltiles(p) * p.batch < 512) tpw >>= 1;
  sp.tiles_per_wave = tpw;
  if (p.dry) return TG_PLAN_STREAM;
  const dim3 grid((unsigned)((sp.rowtiles + 16 * tpw - 1) / (16 * tpw)), (unsigned)coltiles(p), (unsigned)p.batch);
  if constexpr (!LAYOUT_A) {
    if (sp.m >= TG_STREAM_LK_MIN && sp.m <= 15)
      return launch_lds_kernel<w4_gemm_stream_kernel<DT, LAYOUT_A, WPL, QMX, 16, STREAM_MINW, 1, false, true, 1>>(grid, dim3(16 * 64), lds, p.st, sp, false);
  }
  return launch_lds_kernel<w4_gemm_stream_kernel<DT, LAYOUT_A, WPL, QMX, 16, STREAM_MINW, 1, false, true, 0>>(grid, dim3(16 * 64), lds, p.st, sp, false);
}

template <typename DT, bool LAYOUT_A, int WPL, bool QMX>
int launch_stream(const GemmParams& p) {
  constexpr int UNIT = LAYOUT_A ? 64 : 128;
  constexpr int RPW = 16;  // weight rows per wave
  StreamParams sp;
  copy_call(sp, p);
  sp.rowtiles = (p.wrows + RPW - 1) / RPW;
  sp.tiles_per_wave = 1;
  const int mrows = p.m < 16 ? p.m : 16;
  const int nunits = (p.k + UNIT - 1) / UNIT;
  const int upg = (1 << p.gshift) / UNIT;
  // split-K: aim for at least two rounds of 16 waves on every CU; the X slab limits act rows * splitk to 16
  const int64_t wave_tiles = (int64_t)sp.rowtiles * coltiles(p) * p.batch;
  int sk = 1;
  // (m = 1, private slabs: one round of 16 waves per CU is enough -- measured on the Llama-3-8B shapes)
  const int64_t want = mrows == 1 ? 256 * 16 : 2 * 256 * 16;
  while (sk < 8 && wave_tiles * sk < want && nunits >= 8 * sk * upg && mrows * sk * 2 <= 16) sk *= 2;
  // m == 1: every wave stages its own X slab (no barrier in the main loop); a workgroup is the sk waves of one tile
  if (mrows == 1)  // (sk = 1, 2, 4, 8)
    return pick<1, 2, 4, 8>(sk, [&](auto SK_) { return launch_stream_sw<DT, LAYOUT_A, WPL, QMX, decltype(SK_)::value, true>(p, sp, decltype(SK_)::value); });
  // m >= 2, one tile per wave: keep the whole activation block resident in LDS when it fits next to 16 lookup
  // tables (m = 8 at k = 4096 does: 66 KiB + 64 KiB) -- one barrier per workgroup instead of one per unit
  // (measured: wins for m >= 8 at k = 4096 and for m >= 2 at k = 8192; the 16-wave workgroup costs ~15 % in tile-granularity
  //  tail against 4-wave workgroups, which the small slabs of m <= 4 at k = 4096 do not pay back)
  if (sk == 1 && (mrows * UNIT >= 1024 || sp.k >= 8192)) {
    const int nu = (int)(((nunits + 3) / 4 + upg - 1) / upg * upg);
    const unsigned xrow = (unsigned)(nu * UNIT * 2 + 16);
    const unsigned lds = 16u * 4096u + (unsigned)(mrows * 4) * xrow + (unsigned)(UNIT * 2 + 16);
    if (lds <= 160u * 1024u) {
      sp.splitk = 1; sp.sk_shift = 0; sp.units_per_lane = nu; sp.upg_mask = upg - 1;
      sp.xslab_bytes = (int32_t)xrow; sp.red_off = 0;
      return launch_stream_xres<DT, LAYOUT_A, WPL, QMX>(p, sp, lds);
    }
  }
  // otherwise 4-wave workgroups while their LDS footprint lets 16 waves live on a CU and the X slab is small;
  // X slabs of 8 KiB or more per unit (Bint4: m >= 8, Aint4: m = 16): 8-wave workgroups halve the staging work per wave
  const int sk4 = sk < 4 ? sk : 4;
  if (mrows * UNIT < 1024 && 160u * 1024u / stream_lds_bytes<LAYOUT_A>(4, mrows, sk4) >= 4)
    return launch_stream_sw<DT, LAYOUT_A, WPL, QMX, 4>(p, sp, sk4);
  return launch_stream_sw<DT, LAYOUT_A, WPL, QMX, 8>(p, sp, sk);
}

}  // namespace
int tgx::TG_TU_FN(const GemmParams& p) {
  using DT = TG_TU_DT;
  return pick<1, 0>(!p.on_right, [&](auto LAYOUT_A_) {
    return pick<1, 2, 4>(words_per_lane(p), [&](auto WPL_) {  // (innerKTiles 2, 4, 8 on the right; 1, 2, 4 on the left)
      return pick<0, 1>(p.qmx, [&](auto QMX_) {
        constexpr bool QMX = decltype(QMX_)::value != 0;
        if constexpr (QMX && !std::is_same<DT, BF16>::value) {
          return (int)TG_E_DTYPE;
        } else {
          return launch_stream<DT, (decltype(LAYOUT_A_)::value != 0), decltype(WPL_)::value, QMX>(p);
        }
      });
    });
  });
}
