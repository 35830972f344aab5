// tg_moe.hip -- dg_moe_route / dg_moe_launch / dg_moe_plan (include/decode_glue_hip.h): mixture-of-experts decode -- the top-k router and
// the 4-bit GEMV whose weights are picked by expert ids on the device (moe.cuh) --, and the one front of both MoE kernels: a call is
// checked here (moe_call.cuh), DG_MOE_GROUPED then goes to its launcher in tg_moe_tile.hip; see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"

// DG_MOE_GROUPED's launcher and planner, for a call that check_moe accepted: defined in tg_moe_tile.hip, where the tile kernel is compiled; not exported
__attribute__((visibility("hidden"))) int moe_grouped_launch(const dg_moe& c, int device, tg_stream_t stream);
__attribute__((visibility("hidden"))) void moe_grouped_plan(const dg_moe& c, int64_t* out);

namespace {
#include "w4_helpers.cuh"
#include "moe.cuh"
#include "moe_call.cuh"

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

// call == NULL, struct_bytes, then everything else of a call that needs no device
int check_call(const dg_moe* c, bool plan) {
  if (!c) return TG_E_NULL;
  if (c->struct_bytes != sizeof(dg_moe)) return TG_E_STRUCT;
  return check_moe(*c, plan);
}

// The GEMV's parameter block of an accepted call: everything but a row block's operands (x, y, ids, gates, residual) and plan; m is the first block's
MoeW4Params gemv_params(const dg_moe& c) {
  MoeW4Params P = {};
  P.w = (const char*)c.w; P.qinfo = (const char*)c.qinfo;
  P.lut = c.qtype == TG_Q_INT4 ? nullptr : (const char*)c.lut;
  P.stride_w = c.stride_w; P.stride_qinfo = c.stride_qinfo; P.stride_lut = c.stride_lut;
  P.top_k = c.top_k; P.E = c.E; P.wrows = (int32_t)c.wrows; P.k = (int32_t)c.k; P.qtype = c.qtype;
  P.sg_shift = group_shift(c.group) - 6;
  P.stage = c.stage;
  P.m = (int32_t)(c.m < 8 ? c.m : 8);
  return P;
}

int gemv_launch(const dg_moe& c, int device, tg_stream_t stream) {
  MoeW4Params P = gemv_params(c);
  int rc = plan_moe(P, 256);  // (the sizes alone decide whether a plan exists)
  if (rc != 0) return rc;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const bool down = P.stage == DG_MOE_DOWN;
  const int64_t xrow = down ? (int64_t)P.top_k * P.k * 2 : (int64_t)P.k * 2;                   // bytes of x per activation row
  const int64_t yrow = down ? (int64_t)P.wrows * 2 : (int64_t)P.top_k * (P.wrows / 2) * 2;  // ... of y
  for (int64_t r0 = 0; r0 < c.m; r0 += 8) {  // larger m: blocks of 8 rows on the caller's stream, as tg_gemm_w4's row blocks
    P.m = (int32_t)(c.m - r0 < 8 ? c.m - r0 : 8);
    rc = plan_moe(P, cu_count());
    if (rc != 0) return rc;
    P.x = (const char*)c.x + r0 * xrow;
    P.y = (char*)c.y + r0 * yrow;
    P.ids = c.ids + r0 * P.top_k;
    P.gates = down ? c.gates + r0 * P.top_k : nullptr;
    P.residual = down && c.residual ? (const char*)c.residual + r0 * P.wrows * 2 : nullptr;
    const dim3 grid((unsigned)cdiv(P.units, P.upw));
    const unsigned lds = (unsigned)P.lds_acc + (unsigned)(down ? P.m * P.upw * 16 * 4 : 0);
    rc = pick_dt(c.dtype, [&](auto DT_) {
      return launch_lds_kernel<moe_w4_kernel<decltype(DT_)>>(grid, dim3(MW_THREADS), lds, (hipStream_t)stream, P, false);
    });
    if (rc != 0) return rc;
  }
  return 0;
}

// the launch plan of the call's first row block; device < 0: planned for 256 compute units
int gemv_plan(const dg_moe& c, int device, int64_t* out) {
  MoeW4Params P = gemv_params(c);
  int cus = 256;
  if (device >= 0) {
    DeviceScope ds(device);
    if (!ds.ok) return TG_E_DEVICE;
    cus = cu_count();
  }
  const int rc = plan_moe(P, cus);
  if (rc != 0) return rc;
  out[0] = cdiv(P.units, P.upw);   // workgroups
  out[1] = P.upw;                  // 16-row units per workgroup (the last one may own fewer)
  out[2] = P.np;                   // pairs per sweep
  out[3] = cdiv(P.ksuper, P.spw);  // waves that own some k
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

extern "C" int dg_moe_launch(const dg_moe* call, int device, tg_stream_t stream) {
  const int rc = check_call(call, false);
  if (rc != 0) return rc;
  return call->kernel == DG_MOE_GROUPED ? moe_grouped_launch(*call, device, stream) : gemv_launch(*call, device, stream);
}

extern "C" int dg_moe_plan(const dg_moe* call, int device, int64_t* out) {
  if (!out) return TG_E_NULL;
  const int rc = check_call(call, true);
  if (rc != 0) return rc;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (call->kernel == DG_MOE_GEMV) return gemv_plan(*call, device, out);
  if (device >= 0) {  // (the grouped plan does not depend on the device's compute units; a device is only checked)
    DeviceScope ds(device);
    if (!ds.ok) return TG_E_DEVICE;
  }
  moe_grouped_plan(*call, out);
  return 0;
}
