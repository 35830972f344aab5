// tg_moe.hip -- dg_moe_route / dg_moe_w4_launch (include/decode_glue_hip.h): mixture-of-experts decode -- the top-k router and the 4-bit GEMV
// whose weights are picked by expert ids on the device (moe.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "w4_helpers.cuh"
#include "moe.cuh"

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The plan of one launch of up to 8 activation rows: workgroups, 16-row units per workgroup, pairs per sweep, LDS layout.
// One workgroup per CU streams from the first cycle; more than MW_MAX_UPW units per workgroup are not planned (the DOWN accumulators).
int plan_moe(MoeW4Params& P, int cus) {
  P.units = P.wrows / 16;
  P.upw = (int)cdiv(P.units, cus < P.units ? cus : P.units);
  if (P.upw > MW_MAX_UPW) P.upw = MW_MAX_UPW;
  P.ksuper = P.k / 64;
  P.spw = (int)cdiv(P.ksuper, MW_WAVES);
  P.x_pitch = P.k * 2;
  P.xs_pitch = P.ksuper * 2 * 4;
  const int red = MW_WAVES * MW_NP * 16 * 4;
  const int acc = P.stage == DG_MOE_DOWN ? P.m * P.upw * 16 * 4 : 0;
  const int avail = 160 * 1024 - MW_TABLE_BYTES - red - acc;
  const int np = avail / (P.x_pitch + P.xs_pitch);
  if (np < 1) return TG_E_SIZE;
  P.np = np < MW_NP ? np : MW_NP;
  P.lds_x = MW_TABLE_BYTES;
  P.lds_xs = P.lds_x + P.np * P.x_pitch;
  P.lds_red = P.lds_xs + P.np * P.xs_pitch;
  P.lds_acc = P.lds_red + red;
  return 0;
}

// everything of a call that needs no device; fills the sizes of P
int check_moe(const dg_moe_w4* c, MoeW4Params& P) {
  if (!c) return TG_E_NULL;
  if (c->struct_bytes != sizeof(dg_moe_w4)) return TG_E_STRUCT;
  if (c->stage != DG_MOE_GATE_UP && c->stage != DG_MOE_DOWN) return TG_E_LAYOUT;
  const bool any4 = c->qtype == TG_Q_ANY4_GLOBAL || c->qtype == TG_Q_ANY4_ROWWISE;
  if (!c->x || !c->w || !c->qinfo || !c->y || !c->ids || (any4 && !c->lut) || (c->stage == DG_MOE_DOWN && !c->gates)) return TG_E_NULL;
  if (c->dtype != TG_BF16 && c->dtype != TG_F16) return TG_E_DTYPE;
  if (c->qtype != TG_Q_INT4 && !any4) return TG_E_QTYPE;
  if (c->m < 1 || c->E < 1 || c->E > MOE_MAX_E || c->top_k < 1 || c->top_k > MOE_MAX_TOPK || c->top_k > c->E) return TG_E_SHAPE;
  if (c->k < 64 || (c->k % 64) != 0 || c->wrows < 16 || (c->wrows % 16) != 0) return TG_E_SHAPE;
  if (c->m * c->top_k > INT32_MAX / 2 || c->wrows > (1 << 24) || c->wrows * c->k / 2 > INT32_MAX) return TG_E_SIZE;
  if (c->inner_k_tiles != 4) return TG_E_INNER_K;
  if ((c->group != 64 && c->group != 128 && c->group != 256) || (c->k % c->group) != 0) return TG_E_GROUP;
  if (!aligned16(c->x) || !aligned16(c->w) || !aligned16(c->qinfo) || !aligned16(c->lut) || !aligned16(c->y) || !aligned16(c->residual) ||
      !aligned4(c->ids) || !aligned4(c->gates) || (c->stride_w % 16) != 0 || (c->stride_qinfo % 16) != 0 || (c->stride_lut % 16) != 0)
    return TG_E_ALIGN;
  P.w = (const char*)c->w; P.qinfo = (const char*)c->qinfo; P.lut = any4 ? (const char*)c->lut : nullptr;
  P.stride_w = c->stride_w; P.stride_qinfo = c->stride_qinfo; P.stride_lut = c->stride_lut;
  P.top_k = c->top_k; P.E = c->E; P.wrows = (int32_t)c->wrows; P.k = (int32_t)c->k; P.qtype = c->qtype;
  P.sg_shift = group_shift(c->group) - 6;
  P.stage = c->stage;
  return 0;
}

}  // namespace

extern "C" int dg_moe_route(const void* x, const void* router_w, int32_t* ids, float* gates, int64_t m, int64_t k, int64_t E, int64_t top_k,
                            int dtype, int device, tg_stream_t stream) {
  if (!x || !router_w || !ids || !gates) return TG_E_NULL;
  if (dtype != TG_BF16 && dtype != TG_F16) return TG_E_DTYPE;
  if (m < 1 || E < 1 || E > MOE_MAX_E || top_k < 1 || top_k > MOE_MAX_TOPK || top_k > E || k < 8) return TG_E_SHAPE;
  if ((k % 8) != 0) return TG_E_K_DIV;
  if (m > INT32_MAX || k > (1 << 20)) return TG_E_SIZE;
  if (!aligned16(x) || !aligned16(router_w) || !aligned4(ids) || !aligned4(gates)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  MoeRouteParams P;
  P.x = (const uint16_t*)x; P.rw = (const uint16_t*)router_w; P.ids = ids; P.gates = gates;
  P.k = (int32_t)k; P.E = (int32_t)E; P.top_k = (int32_t)top_k;
  return pick_dt(dtype, [&](auto DT_) {
    hipLaunchKernelGGL(moe_route_kernel<decltype(DT_)>, dim3((unsigned)m), dim3(MR_THREADS), 0, (hipStream_t)stream, P);
    return launch_status();
  });
}

extern "C" int dg_moe_w4_launch(const dg_moe_w4* call, int device, tg_stream_t stream) {
  MoeW4Params P = {};
  int rc = check_moe(call, P);
  if (rc != 0) return rc;
  P.m = (int32_t)(call->m < 8 ? call->m : 8);
  rc = plan_moe(P, 256);  // (the sizes alone decide whether a plan exists)
  if (rc != 0) return rc;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t xrow = P.stage == DG_MOE_DOWN ? (int64_t)P.top_k * P.k * 2 : (int64_t)P.k * 2;           // bytes of x per activation row
  const int64_t yrow = P.stage == DG_MOE_DOWN ? (int64_t)P.wrows * 2 : (int64_t)P.top_k * (P.wrows / 2) * 2;  // ... of y
  for (int64_t r0 = 0; r0 < call->m; r0 += 8) {  // larger m: blocks of 8 rows on the caller's stream, as tg_gemm_w4's row blocks
    P.m = (int32_t)(call->m - r0 < 8 ? call->m - r0 : 8);
    rc = plan_moe(P, cu_count());
    if (rc != 0) return rc;
    P.x = (const char*)call->x + r0 * xrow;
    P.y = (char*)call->y + r0 * yrow;
    P.ids = call->ids + r0 * P.top_k;
    P.gates = call->gates ? call->gates + r0 * P.top_k : nullptr;
    P.residual = call->residual ? (const char*)call->residual + r0 * P.wrows * 2 : nullptr;
    const dim3 grid((unsigned)cdiv(P.units, P.upw));
    const unsigned lds = (unsigned)P.lds_acc + (unsigned)(P.stage == DG_MOE_DOWN ? P.m * P.upw * 16 * 4 : 0);
    rc = pick_dt(call->dtype, [&](auto DT_) {
      return launch_lds_kernel<moe_w4_kernel<decltype(DT_)>>(grid, dim3(MW_THREADS), lds, (hipStream_t)stream, P, false);
    });
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int dg_moe_w4_plan(const dg_moe_w4* call, int device, int32_t* out) {
  if (!out) return TG_E_NULL;
  MoeW4Params P = {};
  int rc = check_moe(call, P);
  if (rc != 0) return rc;
  P.m = (int32_t)(call->m < 8 ? call->m : 8);
  int cus = 256;
  if (device >= 0) {
    DeviceScope ds(device);
    if (!ds.ok) return TG_E_DEVICE;
    cus = cu_count();
  }
  rc = plan_moe(P, cus);
  if (rc != 0) return rc;
  out[0] = (int32_t)cdiv(P.units, P.upw);  // workgroups
  out[1] = P.upw;                          // 16-row units per workgroup (the last one may own fewer)
  out[2] = P.np;                           // pairs per sweep
  out[3] = (int32_t)cdiv(P.ksuper, P.spw); // waves that own some k
  return 0;
}
