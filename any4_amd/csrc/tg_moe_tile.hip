// tg_moe_tile.hip -- dg_moe_group and the launcher and planner of dg_moe_launch's kernel DG_MOE_GROUPED (include/decode_glue_hip.h):
// mixture-of-experts PREFILL -- the pairs sorted by expert on the device (moe_grouped.cuh), then the grouped flavour of the tile GEMM
// (w4_gemm_tile.cuh, GRP) over the tile list, each selected expert's weights read once per 128 of its rows.  dg_moe_launch / dg_moe_plan
// (tg_moe.hip) check the call and reach moe_grouped_launch / moe_grouped_plan from the other translation unit; see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "w4_helpers.cuh"
#include "moe.cuh"
#include "w4_gemm_tile.cuh"
#include "moe_call.cuh"
#include "moe_grouped.cuh"

// 128 x 64 tiles, the dense GEMM's choice below a full chip of 128 x 128 tiles; two super-tiles per step where k allows (k % 128 == 0)
template <typename DT, int GRP, int KS>
int go(const GroupedTileParams& tp, hipStream_t st) {
  constexpr int DX = KS == 2 ? 2 : 3;
  constexpr auto kern = w4_gemm_tile_kernel<DT, MG_BM, MG_BN, DX, 8, KS, 4, false, 0, GRP, GroupedTileParams>;
  return launch_lds_kernel<kern>(dim3((unsigned)(tp.tiles_m * tp.tiles_n)), dim3(1024), TileLds<MG_BM, MG_BN, DX, KS>::BYTES, st, tp, false);
}

// the tile kernel's parameter block of an accepted call
GroupedTileParams tile_params(const dg_moe& c) {
  const int64_t pairs = c.m * c.top_k;
  GroupedTileParams P = {};
  P.x = (const char*)c.x; P.w = (const char*)c.w; P.qinfo = (const char*)c.qinfo;
  P.lut = c.qtype == TG_Q_INT4 ? nullptr : (const char*)c.lut;
  P.y = (char*)c.y; P.bias = nullptr;
  P.m = (int32_t)c.m; P.wrows = (int32_t)c.wrows; P.k = (int32_t)c.k; P.ksuper = P.k / 64; P.gshift = group_shift(c.group); P.qtype = c.qtype;
  P.tiles_m = (int32_t)mg_bound(pairs, c.E, MG_BM);
  P.tiles_n = (int32_t)cdiv(c.wrows, MG_BN);
  P.splits = 0;
  P.part = c.stage == DG_MOE_DOWN ? c.f32_ws : nullptr;
  P.x_pitch = c.k;
  P.grp = c.group_ws;
  P.stride_w = c.stride_w; P.stride_qinfo = c.stride_qinfo; P.stride_lut = c.stride_lut;
  P.top_k = c.top_k;
  P.perm_off = MG_PERM;
  P.inv_off = MG_PERM + (int32_t)pairs;
  P.tiles_off = MG_PERM + 2 * (int32_t)pairs;
  return P;
}

}  // namespace

extern "C" int dg_moe_group(const int32_t* ids, int32_t* group_ws, int64_t group_ws_bytes, int64_t m, int64_t top_k, int64_t E, int64_t bm,
                            int device, tg_stream_t stream) {
  if (!ids || !group_ws) return TG_E_NULL;
  if (m < 1 || E < 1 || E > MOE_MAX_E || top_k < 1 || top_k > MOE_MAX_TOPK || top_k > E || bm != MG_BM) return TG_E_SHAPE;
  if (m > MG_MAX_PAIRS || m * top_k > MG_MAX_PAIRS || group_ws_bytes < 4 * mg_ints(m * top_k, E, bm)) return TG_E_SIZE;
  if (!aligned4(ids) || !aligned4(group_ws)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const unsigned lds = (unsigned)(((E + 1) * MG_THREADS + 3 * (E + 1)) * 4);   // (more than 64 KiB from E = 63 on: launch_lds_kernel raises the limit)
  const MoeGroupParams G = {ids, group_ws, (int32_t)(m * top_k), (int32_t)E, (int32_t)bm, (int32_t)mg_bound(m * top_k, E, bm)};
  return launch_lds_kernel<moe_group_kernel>(dim3(1), dim3(MG_THREADS), lds, (hipStream_t)stream, G, false);
}

int moe_grouped_launch(const dg_moe& c, int device, tg_stream_t stream) {
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const GroupedTileParams P = tile_params(c);
  const bool two = P.ksuper % 2 == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (c.stage == DG_MOE_GATE_UP)
    return pick_dt(c.dtype, [&](auto DT_) { return two ? go<decltype(DT_), 1, 2>(P, st) : go<decltype(DT_), 1, 1>(P, st); });
  const int rc = pick_dt(c.dtype, [&](auto DT_) { return two ? go<decltype(DT_), 2, 2>(P, st) : go<decltype(DT_), 2, 1>(P, st); });
  if (rc != 0) return rc;
  MoeCombineParams C;
  C.d = c.f32_ws; C.ids = c.ids; C.gates = c.gates; C.residual = (const char*)c.residual; C.y = (char*)c.y;
  C.m = P.m; C.top_k = P.top_k; C.E = c.E; C.wrows = P.wrows;
  const int64_t threads = (int64_t)P.m * (P.wrows / 4);
  return pick_dt(c.dtype, [&](auto DT_) {
    hipLaunchKernelGGL(moe_combine_kernel<decltype(DT_)>, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, st, C);
    return launch_status();
  });
}

void moe_grouped_plan(const dg_moe& c, int64_t* out) {
  const int64_t pairs = c.m * c.top_k;
  out[0] = MG_BM;                            // activation rows (pairs) per tile
  out[1] = MG_BN;                            // weight rows per tile
  out[2] = mg_bound(pairs, c.E, MG_BM);      // the grid's m-extent: the bound of the tile list's length
  out[3] = cdiv(c.wrows, MG_BN);             // n tiles
  out[4] = (c.k / 64) % 2 == 0 ? 2 : 1;      // 64-k super-tiles per step
  out[5] = 4 * mg_ints(pairs, c.E, MG_BM);   // bytes of the group workspace
  out[6] = c.stage == DG_MOE_DOWN ? pairs * c.wrows * 4 : 0;   // bytes of the f32 workspace
}
