// tg_moe_tile.hip -- dg_moe_group / dg_moe_grouped_launch / dg_moe_grouped_plan (include/decode_glue_hip.h): mixture-of-experts PREFILL --
// the pairs sorted by expert on the device (moe_grouped.cuh), then the grouped flavour of the tile GEMM (w4_gemm_tile.cuh, GRP) over the
// tile list, each selected expert's weights read once per 128 of its rows; see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "w4_helpers.cuh"
#include "moe.cuh"
#include "w4_gemm_tile.cuh"
#include "moe_grouped.cuh"

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// 128 x 64 tiles, the dense GEMM's choice below a full chip of 128 x 128 tiles; two super-tiles per step where k allows (k % 128 == 0)
template <typename DT, int GRP, int KS>
int go(const GroupedTileParams& tp, hipStream_t st) {
  constexpr int DX = KS == 2 ? 2 : 3;
  constexpr auto kern = w4_gemm_tile_kernel<DT, MG_BM, MG_BN, DX, 8, KS, 4, false, 0, GRP, GroupedTileParams>;
  return launch_lds_kernel<kern>(dim3((unsigned)(tp.tiles_m * tp.tiles_n)), dim3(1024), TileLds<MG_BM, MG_BN, DX, KS>::BYTES, st, tp, false);
}

// everything of a call that needs no device, in dg_moe_w4's order; fills P.  plan: the workspaces are not looked at (the plan tells their sizes)
int check_grouped(const dg_moe_grouped* c, GroupedTileParams& P, bool plan) {
  if (!c) return TG_E_NULL;
  if (c->struct_bytes != sizeof(dg_moe_grouped)) return TG_E_STRUCT;
  if (c->stage != DG_MOE_GATE_UP && c->stage != DG_MOE_DOWN) return TG_E_LAYOUT;
  const bool any4 = c->qtype == TG_Q_ANY4_GLOBAL || c->qtype == TG_Q_ANY4_ROWWISE;
  const bool down = c->stage == DG_MOE_DOWN;
  if (!c->x || !c->w || !c->qinfo || !c->y || !c->ids || (any4 && !c->lut) || (down && !c->gates) ||
      (!plan && (!c->group_ws || (down && !c->f32_ws))))
    return TG_E_NULL;
  if (c->dtype != TG_BF16 && c->dtype != TG_F16) return TG_E_DTYPE;
  if (c->qtype != TG_Q_INT4 && !any4) return TG_E_QTYPE;
  if (c->m < 1 || c->E < 1 || c->E > MOE_MAX_E || c->top_k < 1 || c->top_k > MOE_MAX_TOPK || c->top_k > c->E) return TG_E_SHAPE;
  if (c->k < 64 || (c->k % 64) != 0 || c->wrows < 16 || (c->wrows % 16) != 0) return TG_E_SHAPE;
  if (c->m > MG_MAX_PAIRS || c->m * c->top_k > MG_MAX_PAIRS || c->wrows > (1 << 24) || c->wrows * c->k / 2 > INT32_MAX) return TG_E_SIZE;
  const int64_t pairs = c->m * c->top_k;
  if (!plan && (c->group_ws_bytes < 4 * mg_ints(pairs, c->E, MG_BM) || (down && c->f32_ws_bytes < pairs * c->wrows * 4))) return TG_E_SIZE;
  if (c->inner_k_tiles != 4) return TG_E_INNER_K;
  if ((c->group != 64 && c->group != 128 && c->group != 256) || (c->k % c->group) != 0) return TG_E_GROUP;
  if (!aligned16(c->x) || !aligned16(c->w) || !aligned16(c->qinfo) || !aligned16(c->lut) || !aligned16(c->y) || !aligned16(c->residual) ||
      !aligned4(c->ids) || !aligned4(c->gates) || (!plan && (!aligned4(c->group_ws) || !aligned16(c->f32_ws))) || (c->stride_w % 16) != 0 ||
      (c->stride_qinfo % 16) != 0 || (c->stride_lut % 16) != 0)
    return TG_E_ALIGN;
  P.x = (const char*)c->x; P.w = (const char*)c->w; P.qinfo = (const char*)c->qinfo; P.lut = any4 ? (const char*)c->lut : nullptr;
  P.y = (char*)c->y; P.bias = nullptr;
  P.m = (int32_t)c->m; P.wrows = (int32_t)c->wrows; P.k = (int32_t)c->k; P.ksuper = P.k / 64; P.gshift = group_shift(c->group); P.qtype = c->qtype;
  P.tiles_m = (int32_t)mg_bound(pairs, c->E, MG_BM);
  P.tiles_n = (int32_t)cdiv(c->wrows, MG_BN);
  P.splits = 0;
  P.part = c->f32_ws;
  P.x_pitch = c->k;
  P.grp = c->group_ws;
  P.stride_w = c->stride_w; P.stride_qinfo = c->stride_qinfo; P.stride_lut = c->stride_lut;
  P.top_k = c->top_k;
  P.perm_off = MG_PERM;
  P.inv_off = MG_PERM + (int32_t)pairs;
  P.tiles_off = MG_PERM + 2 * (int32_t)pairs;
  return 0;
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

extern "C" int dg_moe_grouped_launch(const dg_moe_grouped* call, int device, tg_stream_t stream) {
  GroupedTileParams P = {};
  int rc = check_grouped(call, P, false);
  if (rc != 0) return rc;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const bool two = P.ksuper % 2 == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (call->stage == DG_MOE_GATE_UP)
    return pick_dt(call->dtype, [&](auto DT_) { return two ? go<decltype(DT_), 1, 2>(P, st) : go<decltype(DT_), 1, 1>(P, st); });
  rc = pick_dt(call->dtype, [&](auto DT_) { return two ? go<decltype(DT_), 2, 2>(P, st) : go<decltype(DT_), 2, 1>(P, st); });
  if (rc != 0) return rc;
  MoeCombineParams C;
  C.d = call->f32_ws; C.ids = call->ids; C.gates = call->gates; C.residual = (const char*)call->residual; C.y = (char*)call->y;
  C.m = P.m; C.top_k = P.top_k; C.E = call->E; C.wrows = P.wrows;
  const int64_t threads = (int64_t)P.m * (P.wrows / 4);
  return pick_dt(call->dtype, [&](auto DT_) {
    hipLaunchKernelGGL(moe_combine_kernel<decltype(DT_)>, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, st, C);
    return launch_status();
  });
}

extern "C" int dg_moe_grouped_plan(const dg_moe_grouped* call, int device, int64_t* out) {
  if (!out) return TG_E_NULL;
  GroupedTileParams P = {};
  const int rc = check_grouped(call, P, true);
  if (rc != 0) return rc;
  if (device >= 0) {  // (the plan does not depend on the device's compute units; a device is only checked)
    DeviceScope ds(device);
    if (!ds.ok) return TG_E_DEVICE;
  }
  const int64_t pairs = call->m * call->top_k;
  out[0] = MG_BM;                               // activation rows (pairs) per tile
  out[1] = MG_BN;                               // weight rows per tile
  out[2] = P.tiles_m;                           // the grid's m-extent: the bound of the tile list's length
  out[3] = P.tiles_n;                           // n tiles
  out[4] = P.ksuper % 2 == 0 ? 2 : 1;           // 64-k super-tiles per step
  out[5] = 4 * mg_ints(pairs, call->E, MG_BM);  // bytes of the group workspace
  out[6] = call->stage == DG_MOE_DOWN ? pairs * call->wrows * 4 : 0;   // bytes of the f32 workspace
  return 0;
}
