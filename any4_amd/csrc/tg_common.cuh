// tg_common.cuh -- what every translation unit of libtinygemm_hip.so shares: type traits, host helpers, the description of one validated
// call (GemmParams: host-only, no kernel receives it), the pieces of the planning protocol every launch path repeats (has_workspace,
// plan_cu_count, launch_lds_kernel) and the entry points of the kernel families' launch paths (namespace tgx).
//
// The library is built from one translation unit per kernel family (any4_amd/build.py compiles them in parallel):
//   tinygemm_hip.hip   the C ABI, validation (check_gemm), GemmParams (make_params), dispatch (launch_w4, launch_w8); its kernels:
//                        w8_gemm_kernel (w8_gemm.cuh), f16_gemm_kernel (f16_gemm.cuh), packers / converters / dequantisers (tg_convert.cuh),
//                        decode glue (decode_glue.cuh), peer gather (peer_gather.cuh)
//   tg_splitk.hip      w4_gemm_kernel            (w4_gemm.cuh)
//   tg_stream.hip      w4_gemm_stream_kernel     (w4_gemm_stream.cuh)      compiled once per 16-bit type (-DTG_TU_F16)
//   tg_pair.hip        w4_gemm_pair_kernel       (w4_gemm_pair.cuh)        compiled once per 16-bit type
//   tg_pair16.hip      w4_gemm_pair16_kernel     (w4_gemm_pair16.cuh)
//   tg_xr.hip          w4_gemm_xr_kernel         (w4_gemm_xr.cuh)
//   tg_gemv.hip        w4_gemv_kernel            (w4_gemv.cuh)
//   tg_tile.hip        w4_gemm_tile_kernel       (w4_gemm_tile.cuh)
//   tg_dx.hip          w4_gemm_dx_kernel         (w4_gemm_dx.cuh)          the input gradient dX = dY . W (tg_gemm_w4_dx)
//   tg_dq.hip          w4_gemm_dq_kernel         (w4_gemm_dq.cuh)          the gradients of scales, zeros and LUT (tg_gemm_w4_dq)
//   tg_prefill.hip     prefill_attn_kernel       (attn_prefill.cuh)        prompt prefill: rope + cache append + causal flash attention (DG_ATTN_PREFILL)
//   tg_sample.hip      sample_kernel             (sample.cuh)              temperature / top-k / top-p sampling of the logits (dg_sample)
//   tg_lora.hip        lora_shrink_kernel, lora_expand_kernel (lora.cuh)   per-sequence LoRA adapters on a linear's output (dg_lora_shrink / dg_lora_expand)
//   tg_moe.hip         moe_route_kernel, moe_w4_kernel (moe.cuh)               mixture-of-experts decode: the top-k router and the expert-indexed 4-bit GEMV (dg_moe_route / dg_moe_launch / dg_moe_plan: the one front of both MoE kernels)
//   tg_moe_tile.hip    w4_gemm_tile_kernel<GRP>, moe_group_kernel, moe_combine_kernel (w4_gemm_tile.cuh, moe_grouped.cuh)  mixture-of-experts prefill: pairs sorted by expert, grouped tile GEMM (dg_moe_group / DG_MOE_GROUPED's launcher)
//   tg_kmeans.hip      kmeans_rows_kernel        (kmeans.cuh)              the any4 quantizer's per-row weighted 1-D k-means (tg_kmeans_rows); compiled with -ffp-contract=off
// Shared by several units' kernels, included inside the unit's anonymous namespace: w4_helpers.cuh (fragment-order addressing, mx4 converters,
// MFMA / v_dot2 wrappers, the stages fused into a GEMM), stage_math.cuh (the arithmetic of rope, RMSNorm and SwiGLU: one definition each), kv8.cuh (the mx8 KV-cache format: decode_glue.cuh, attn_prefill.cuh);
// tg_trace.cuh is the developer trace (-DGEMV_TRACE=1), included here.
// attn_call.cuh is the attention side's GemmParams: what the library does with one attention call of the decode stack (dg_attn, the public struct): the accepted
// (kernel, flags) pairs, its validation for all five kinds of kernel (check_attn) and the split kernels' scratch layout (split_scratch); included by decode_glue.cuh and tg_prefill.hip.
// moe_call.cuh is the same for one mixture-of-experts call (dg_moe, the public struct): its validation for both kernels (check_moe) and the group workspace's layout; included by tg_moe.hip and tg_moe_tile.hip.
// Kernels and their helpers stay in each unit's anonymous namespace (one device code object per unit, no symbol shared between
// them); only GemmParams and the tgx:: functions cross unit boundaries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <type_traits>
#include <utility>

#include "../../include/tinygemm_hip.h"
#include "tg_trace.cuh"

// One validated call, complete: everything a launch path needs to plan and launch it (make_params fills it once).  Host-only -- every
// kernel has an argument block of its own (copy_call).
struct GemmParams {
  const char* x;
  const char* w;
  const char* qinfo;
  const char* lut;
  char* y;
  int32_t m, wrows, k;
  int32_t ntiles;    // packed.size(0): 8-row (Bint4) or 16-row (Aint4) tiles
  int32_t ksuper;    // packed.size(1)
  int32_t gshift;    // log2(group)
  int32_t ngroups;   // k / group
  int32_t qtype;
  int32_t rowtiles;  // ceil(wrows / 16)
  int32_t dt;        // TG_BF16 / TG_F16
  int32_t on_right;  // the side and ...
  int32_t inner;     // ... innerKTiles the packed words actually hold (make_params)
  int32_t qmx;       // qtype == TG_Q_MX4
  int32_t batch;     // problems of the call (>= 1)
  hipStream_t st;
  int32_t numerics;  // TG_NUM_* (dispatch)
  int32_t dot2;      // TG_NUM_FAST_DOT2 was asked for (never promote a stacked m = 1 launch to the matrix-core contraction)
  int32_t dry;       // report the kernel family instead of launching (tg_gemm_w4_plan)
  int32_t dry_detail;  // ... and, within the pair-table family, the lean m = 1 kernel as TG_PLAN_PAIR_M1_LEAN (tg_gemm_w4_plan_detail)
  int64_t stride_x, stride_w, stride_qinfo, stride_lut, stride_y;
  const char* bias;   // optional [wrows] 16-bit, added after the first rounding (see store_rows4)
  int64_t stride_bias;
  int64_t bias_row_stride;  // elements between the bias rows of consecutive activation rows (0: one row for all; wrows: a residual)
  const char* norm_w;       // fused RMSNorm of the activations (pair-table kernels only)
  float norm_eps;
  int32_t epilogue;         // TG_EPI_* (pair-table kernels only)
  // The caller's workspace and the planner's answer to "how much would help".  ws_need: the dispatcher zeroes it when it offers the call
  // to a family, a family assigns it only where it accepts the call.
  char* ws;
  int64_t ws_bytes, ws_need;
  int32_t ws_query;    // tg_gemm_*_workspace_bytes: plan as if the caller had brought whatever is asked for
  int32_t x_tc, y_tc;  // fragment-order activations / output (pair-table kernels only)
};

// Argument block of w4_gemm_kernel (w4_gemm.cuh) and w8_gemm_kernel (w8_gemm.cuh): splitk_params.
struct SplitKParams {
  const char* x;
  const char* w;
  const char* qinfo;
  const char* lut;
  char* y;
  int32_t m, wrows, k;
  int32_t ntiles, ksuper, gshift, ngroups, qtype;  // as in GemmParams
  int32_t splitk;    // waves per tile (power of two, <= WAVES)
  int32_t sk_shift;  // log2(splitk)
  int32_t rowtiles;  // ceil(wrows / 16)
  int64_t stride_x, stride_w, stride_qinfo, stride_lut, stride_y;
  const char* bias;
  int64_t stride_bias;
  int64_t bias_row_stride;
};

// Lane exchanges WITHOUT the LDS crossbar.  hipcc turns every `__shfl_xor` into ds_bpermute_b32 -- an LDS-pipeline round trip (address
// register, lgkmcnt wait, ~100 cycles) -- and a butterfly is four to six of them back to back, usually on a launch's critical path in
// front of its first barrier (dev/gemv_trace.py: the 16-lane step sums were 0.6 us of a 5.8 us launch).  gfx950 has the data paths in
// the vector ALU: DPP operands (quad permutes, rotations within a 16-lane row) and v_permlane16_swap / v_permlane32_swap across rows.
namespace tgl {
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// the two halves of a pair of 16-lane rows / of the wave, side by side: [0] = (r0, r0, r2, r2) / (lo, lo), [1] = (r1, r1, r3, r3) / (hi, hi)
__device__ __forceinline__ void rows16(float v, float& even, float& odd) {
  const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
  even = __builtin_bit_cast(float, (unsigned)sw[0]);
  odd = __builtin_bit_cast(float, (unsigned)sw[1]);
}
__device__ __forceinline__ void halves32(float v, float& lo, float& hi) {
  const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
  lo = __builtin_bit_cast(float, (unsigned)sw[0]);
  hi = __builtin_bit_cast(float, (unsigned)sw[1]);
}
// the value lane ^ O holds (O = 1, 2, 8: one DPP move; 16, 32: one row swap and a select on this lane's side; `lane` = lane id)
template <int O>
__device__ __forceinline__ float lane_xor(float v, int lane) {
  static_assert(O == 1 || O == 2 || O == 8 || O == 16 || O == 32, "xor by 4 has no DPP form on gfx9: rotate (row_sum) or shuffle");
  if constexpr (O == 1) return dpp<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (O == 2) return dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (O == 8) return dpp<0x128>(v);  // row_ror:8
  else if constexpr (O == 16) { float a, b; rows16(v, a, b); return (lane & 16) ? a : b; }
  else { float a, b; halves32(v, a, b); return (lane & 32) ? a : b; }
}
// every lane of a 16-lane row gets the row's sum (rotations by 8, 4, 2, 1: the same bits in all 16 lanes)
__device__ __forceinline__ float row_sum(float v) {
  v += dpp<0x128>(v);
  v += dpp<0x124>(v);
  v += dpp<0x122>(v);
  v += dpp<0x121>(v);
  return v;
}
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp<0x128>(v));
  v = fmaxf(v, dpp<0x124>(v));
  v = fmaxf(v, dpp<0x122>(v));
  v = fmaxf(v, dpp<0x121>(v));
  return v;
}
// ... of the rows 2 j, 2 j + 1 / of the whole wave (every lane the same bits)
__device__ __forceinline__ float rows16_sum(float v) {
  float a, b; rows16(v, a, b); return a + b;
}
__device__ __forceinline__ float halves32_sum(float v) {
  float a, b; halves32(v, a, b); return a + b;
}
__device__ __forceinline__ float wave_sum(float v) { return halves32_sum(rows16_sum(row_sum(v))); }
__device__ __forceinline__ float wave_max(float v) {
  v = row_max(v);
  float a, b;
  rows16(v, a, b); v = fmaxf(a, b);
  halves32(v, a, b); return fmaxf(a, b);
}
}  // namespace tgl

enum { CANON_NONE = 0, CANON_PAIR = 1, CANON_QUAD = 2 };

// Returned by a family's launch path when the shape does not fit its plan (the caller then takes another kernel).
enum { TG_PAIR_NA = -100 };

// Launch paths of the kernel families: each takes the call and answers a TG_PLAN_* code (p.dry), 0 / an error code (launched), or
// TG_PAIR_NA.  The two largest families are compiled once per 16-bit type.
namespace tgx {
int pair_bf16(GemmParams& p);
int pair_f16(GemmParams& p);
int pair_a_bf16(GemmParams& p);
int pair_a_f16(GemmParams& p);
int pair_b16_bf16(GemmParams& p);
int pair_b16_f16(GemmParams& p);
int stream_bf16(const GemmParams& p);
int stream_f16(const GemmParams& p);
int pair_xr(GemmParams& p);
int pair16(const GemmParams& p);
int pair16_loop(const GemmParams& p);  // w4_gemm_pair16_loop.cuh: one layer, more 16-row tiles than CUs
int splitk(const GemmParams& p, int waves, int splitk);  // (the dispatcher routes on pick_geometry's answer, and passes it on)
int gemv(const GemmParams& p);
int tile(GemmParams& p);     // w4_gemm_tile.cuh: many activation rows
int tile_w8(GemmParams& p);  // ... int8 weights (tg_gemm_w8)
int gemm_dx(GemmParams& p);  // w4_gemm_dx.cuh: dX = dY . W (tg_gemm_w4_dx)
int gemm_dq(GemmParams& p, const char* dy, float* d_qinfo, float* d_lut);  // w4_gemm_dq.cuh: d(scales, zeros), dLUT (tg_gemm_w4_dq)
inline int pair(GemmParams& p) { return p.dt == TG_BF16 ? pair_bf16(p) : pair_f16(p); }
inline int pair_a(GemmParams& p) { return p.dt == TG_BF16 ? pair_a_bf16(p) : pair_a_f16(p); }
inline int pair_b16(GemmParams& p) { return p.dt == TG_BF16 ? pair_b16_bf16(p) : pair_b16_f16(p); }
inline int stream(const GemmParams& p) { return p.dt == TG_BF16 ? stream_bf16(p) : stream_f16(p); }
}  // namespace tgx

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

// LDS pointers (address space 3: ds_* instructions with constant offsets)
typedef const __attribute__((address_space(3))) float* lds_cfptr;
typedef __attribute__((address_space(3))) float* lds_fptr;
typedef const __attribute__((address_space(3))) uint16_t* lds_cu16ptr;
typedef const __attribute__((address_space(3))) uint32_t* lds_cu32ptr;
typedef __attribute__((address_space(3))) uint32_t* lds_u32ptr;
typedef const __attribute__((address_space(3))) u32x4* lds_cu32x4ptr;
typedef __attribute__((address_space(3))) u32x4* lds_u32x4ptr;
typedef const __attribute__((address_space(3))) f32x4* lds_cf32x4ptr;
typedef __attribute__((address_space(3))) f32x4* lds_f32x4ptr;

__device__ __forceinline__ float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }

// ---- 16-bit float traits ---------------------------------------------------------------------
struct BF16 {
  static __device__ __forceinline__ float to_f32(uint16_t h) { return u2f(((uint32_t)h) << 16); }
  static __device__ __forceinline__ float lo_f32(uint32_t pair) { return u2f(pair << 16); }
  static __device__ __forceinline__ float hi_f32(uint32_t pair) { return u2f(pair & 0xffff0000u); }
  // round-to-nearest-even pack; lowers to v_cvt_pk_bf16_f32 on gfx950
  static __device__ __forceinline__ uint32_t pack2(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
  }
  static __device__ __forceinline__ uint16_t from_f32(float a) { return (uint16_t)(pack2(a, 0.f) & 0xffffu); }
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
struct F16 {
  static __device__ __forceinline__ float to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
  static __device__ __forceinline__ float lo_f32(uint32_t pair) { return to_f32((uint16_t)(pair & 0xffffu)); }
  static __device__ __forceinline__ float hi_f32(uint32_t pair) { return to_f32((uint16_t)(pair >> 16)); }
  static __device__ __forceinline__ uint32_t pack2(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  }
  static __device__ __forceinline__ uint16_t from_f32(float a) { return (uint16_t)(pack2(a, 0.f) & 0xffffu); }
  static __device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// Kernel selection, the one idiom of the launch paths: a run-time value picks a template argument, the generic lambda `f` names the kernel.
// pick<V0, V1, ...>(v, f) calls f(std::integral_constant<int, Vi>{}) for the Vi that equals v and answers TG_PAIR_NA when none does;
// pick_dt(dt, f) calls f(BF16{}) or f(F16{}).  A combination that is not instantiated is an `if constexpr` in the lambda.
template <int... VS, typename F>
int pick(int v, F&& f) {
  int rc = TG_PAIR_NA;
  (void)((v == VS && ((rc = f(std::integral_constant<int, VS>{})), true)) || ...);
  return rc;
}
template <typename F>
int pick_dt(int dt, F&& f) {
  return dt == TG_BF16 ? f(BF16{}) : f(F16{});
}

// fp4-e2m1 values in code order (reference FloatDefs.cuh:18-34)
__device__ const float kMX4Values[16] = {0.0f,  0.5f,  1.0f,  1.5f,  2.0f,  3.0f,  4.0f,  6.0f,
                                         -0.0f, -0.5f, -1.0f, -1.5f, -2.0f, -3.0f, -4.0f, -6.0f};

// Output store of four consecutive weight rows of one activation row.  With a bias the sum is first rounded to 16 bits and
// the bias added in a second rounded step: bit-identical to the reference module's separate `y + bias` (modules.py:221-222).
template <typename DT>
__device__ __forceinline__ void store_rows4(char* yb, const char* bias, int64_t elem, int rowg, f32x4 acc) {
  u32x2 o = {DT::pack2(acc[0], acc[1]), DT::pack2(acc[2], acc[3])};
  if (bias) {
    const u32x2 bv = *reinterpret_cast<const u32x2*>(bias + (int64_t)rowg * 2);
    o[0] = DT::pack2(DT::lo_f32(o[0]) + DT::lo_f32(bv[0]), DT::hi_f32(o[0]) + DT::hi_f32(bv[0]));
    o[1] = DT::pack2(DT::lo_f32(o[1]) + DT::lo_f32(bv[1]), DT::hi_f32(o[1]) + DT::hi_f32(bv[1]));
  }
  *reinterpret_cast<u32x2*>(yb + elem * 2) = o;
}


// 4 x 4 transpose across the four 16-lane rows of a wave: out[e] in row Q = in[Q] of row e (lane = i + 16 row).  Two v_permlane16_swap
// (odd rows of the first operand <-> even rows of the second) and two v_permlane32_swap (upper half of the first <-> lower half of the second).
// Use: the MFMA 16x16x32 fragment of lane (i, Q) is the dwords Q, Q + 4, Q + 8, Q + 12 of a 64-byte block of row i -- one 16-byte load per
// lane of dwords 4Q ... 4Q + 3 and this transpose instead of four 4-byte loads (a quarter of the requests in the vector-memory path).
__device__ __forceinline__ u32x4 transpose_rows4(u32x4 v) {
  const auto s01 = __builtin_amdgcn_permlane16_swap(v[0], v[1], false, false);
  const auto s23 = __builtin_amdgcn_permlane16_swap(v[2], v[3], false, false);
  const auto t02 = __builtin_amdgcn_permlane32_swap(s01[0], s23[0], false, false);
  const auto t13 = __builtin_amdgcn_permlane32_swap(s01[1], s23[1], false, false);
  return u32x4{t02[0], t13[0], t02[1], t13[1]};
}

struct DeviceScope {
  int prev = -1;
  bool ok = true;
  explicit DeviceScope(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
    if (prev != device && hipSetDevice(device) != hipSuccess) ok = false;
    if (prev == device) prev = -1;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int group_shift(int g) { return g == 32 ? 5 : g == 64 ? 6 : g == 128 ? 7 : 8; }  // log2 of a validated qGroupSize
inline int64_t coltiles(const GemmParams& p) { return cdiv(p.m, 16); }                    // 16-row tiles of activations
// packed words per (k super-tile, lane-row) entry of the layout (1 / 2 / 4 = CANON_NONE / _PAIR / _QUAD: the in-register transpose)
inline int words_per_lane(const GemmParams& p) { return p.on_right ? p.inner / 2 : p.inner; }

// Every kernel has a parameter block of its own (its layout is that kernel's ABI), and each repeats part of GemmParams under the
// same names.  copy_call assigns, of the fields listed, those the destination has: the operands, the problem's sizes and group geometry,
// the batch strides, the bias, the fused stages, the fragment-order flags and `dry`.  What a family derives or overrides it sets afterwards.
template <typename D, typename F>
auto assign_if_member(D& d, F f, int) -> decltype(f(d)) { f(d); }
template <typename D, typename F>
void assign_if_member(D&, F, long) {}
template <typename D>
void copy_call(D& d, const GemmParams& p) {
#define TG_COPY(f) assign_if_member(d, [&](auto& t) -> decltype((void)(t.f = p.f)) { t.f = p.f; }, 0)
  TG_COPY(x); TG_COPY(w); TG_COPY(qinfo); TG_COPY(lut); TG_COPY(y);
  TG_COPY(m); TG_COPY(wrows); TG_COPY(k); TG_COPY(ntiles); TG_COPY(ksuper); TG_COPY(gshift); TG_COPY(ngroups); TG_COPY(qtype);
  TG_COPY(stride_x); TG_COPY(stride_w); TG_COPY(stride_qinfo); TG_COPY(stride_lut); TG_COPY(stride_y);
  TG_COPY(bias); TG_COPY(stride_bias); TG_COPY(bias_row_stride);
  TG_COPY(norm_w); TG_COPY(norm_eps); TG_COPY(epilogue); TG_COPY(x_tc); TG_COPY(y_tc); TG_COPY(dry);
#undef TG_COPY
}
inline SplitKParams splitk_params(const GemmParams& p, int splitk) {
  SplitKParams kp;
  copy_call(kp, p);
  kp.rowtiles = p.rowtiles;
  kp.splitk = splitk;
  kp.sk_shift = 0;
  while ((1 << kp.sk_shift) < splitk) ++kp.sk_shift;
  return kp;
}

// The workspace half of the planning protocol: does the caller have `need` bytes -- or is this the workspace query, which plans as if?
inline bool has_workspace(const GemmParams& p, int64_t need) { return p.ws_query || (p.ws != nullptr && p.ws_bytes >= need); }

// Kernels that address LDS from offset 0 (lookup tables at the start of the dynamic region) and / or need more than 64 KiB
// of dynamic LDS: once per device, check that the kernel has no static LDS (the dynamic region then starts at 0) and raise
// its dynamic-LDS limit.  State = one write-once bit per device and kernel; racing threads repeat the same idempotent calls.
template <auto KERN>
int prepare_lds_kernel() {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TG_E_DEVICE;
  if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_relaxed) >> dev) & 1u)) return 0;
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(KERN));
  if (e != hipSuccess) return (int)e;
  if (fa.sharedSizeBytes != 0) return TG_E_INTERNAL;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return (int)e;
  if (dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_relaxed);
  return 0;
}
// ... and launch it.  A failed preparation is either passed on, or (decline_on_failure: a part with less LDS) answered with TG_PAIR_NA --
// the older kernels take over -- unless it is TG_E_INTERNAL.
template <auto KERN, typename P>
int launch_lds_kernel(dim3 grid, dim3 block, unsigned lds, hipStream_t st, const P& params, bool decline_on_failure) {
  const int prc = prepare_lds_kernel<KERN>();
  if (prc != 0) return decline_on_failure && prc != TG_E_INTERNAL ? (int)TG_PAIR_NA : prc;
  hipLaunchKernelGGL(KERN, grid, block, lds, st, params);
  return launch_status();
}

// compute units of the current device (write-once cache per device index; racing threads store the same value)
inline int cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cache[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
  cache[dev].store(v, std::memory_order_relaxed);
  return v;
}
// ... a plan is made without a device: for 256
inline int plan_cu_count(const GemmParams& p) { return p.dry ? 256 : cu_count(); }


// Tuning constants of the pair-table launches, each with the measurement that set it.  The shipped library
// always uses these values; only developer builds (-DTG_DEV / -DTG_DEV_MIN, dev/build_variant.sh) may override one with -D<NAME>=<v>.
#if !defined(TG_DEV) && !defined(TG_DEV_MIN)
#if defined(TG_PAIR_R) || defined(TG_PAIR_MR1) || defined(TG_PAIR_NSG2) || defined(TG_PAIR_MR1_GPS) || defined(TG_PAIR_RA) ||   \
    defined(TG_PAIR_RA1) || defined(TG_PAIR_RB16) || defined(TG_B16_CHUNK) || defined(TG_PAIR_MIN_ITEMS) || defined(TG_XG_CHUNK) || defined(TG_PAIR_WGS) || \
    defined(TG_PAIR_NSG2_M1) || defined(TG_XR_MIN_M) || defined(TG_XR_R) || defined(TG_XR_R8K) || defined(TG_XR_RMX) || defined(TG_PAIR_M1_LEAN) || \
    defined(TG_PAIR_M1_AHEAD)
#error "the TG_PAIR_* / TG_XG_* / TG_B16_* tuning constants can only be overridden in developer builds (-DTG_DEV or -DTG_DEV_MIN)"
#endif
#endif
#ifndef TG_PAIR_R
#define TG_PAIR_R 2            // super-tiles a wave keeps in flight (2, 3, 4 measured equal; 5 spills)
#endif
#ifndef TG_PAIR_MR1
#define TG_PAIR_MR1 1          // 1: m = 1 runs the one-register specialisation (+2-3 %), 4: the general m <= 8 kernel
#endif
#ifndef TG_PAIR_NSG2
#define TG_PAIR_NSG2 1         // group boundaries at fixed places of the unrolled round when a group is one round of the ring
#endif
#ifndef TG_PAIR_NSG2_M1
#define TG_PAIR_NSG2_M1 1      // ... also in the m = 1 specialisation (74.8 -> 75.8 % once its group update was spelled out)
#endif
#ifndef TG_PAIR_MR1_GPS
#define TG_PAIR_MR1_GPS 1      // the m = 1 specialisation is used up to this many groups per super-tile (it spills beyond)
#endif
#ifndef TG_PAIR_RA
#define TG_PAIR_RA 2           // ring depth of the A-side kernels (4 / 6 / 8 measured 8.2 / 21 / 40 us against 6.8)
#endif
#ifndef TG_PAIR_RA1
#define TG_PAIR_RA1 1          // ... with several groups per super-tile
#endif
#ifndef TG_PAIR_RB16
#define TG_PAIR_RB16 2         // ring depth of the 16x16x32 kernels for Bint4 weights, m = 9 ... 16 (3 / 4: 41 % against 44 %)
#endif
#ifndef TG_B16_CHUNK
#define TG_B16_CHUNK 4         // consecutive 32-row work items per workgroup visit of those kernels (1 / 4 / 8 within 1 %)
#endif
#ifndef TG_TILE_W8_MIN_M
#define TG_TILE_W8_MIN_M 17  // int8 weights: activation rows from which tg_gemm_w8 takes the tile GEMM (tg_tile.hip): 14.3 us per 4096^2 layer; the 16-row kernel: 8.6 us up to 6 rows
#endif
#ifndef TG_TILE_MIN_M_SPLIT
#define TG_TILE_MIN_M_SPLIT 17  // ... and with a split-K launch of ONE layer (caller's workspace; tg_tile.hip): 12.6-14.8 us at 17 ... 64 rows against 7.5 us per 16-row pass
#endif
#ifndef TG_TILE_MIN_M
#define TG_TILE_MIN_M 65  // activation rows from which a call takes the LDS-tiled MFMA GEMM (w4_gemm_tile.cuh): beyond the 64 rows the row blocks of the group-scaled kernels cover
#endif
#ifndef TG_M1_DEFAULT_MFMA
#define TG_M1_DEFAULT_MFMA 0  // which contraction a STACKED m = 1 launch takes under TG_NUM_FAST: 0 = per-lane v_dot2, 1 = the matrix core (tg_m1_default_contraction())
#endif
#ifndef TG_PAIR_MIN_ITEMS
#define TG_PAIR_MIN_ITEMS 192  // fewer work items: the launch is latency-bound, w4_gemm_pair16_kernel / the reference kernels take
                               // it (measured per hipGraph node, one layer, m = 1: 14336 x 4096 = 224 items 12.3 us here against
                               // 18.3 us on pair16 and 13.8 us on the stream kernel; 6144 x 4096 = 96 items 10.7 against 9.9 / 8.2)
#endif
#ifndef TG_XG_CHUNK
#define TG_XG_CHUNK 4          // consecutive work items per workgroup visit in the workspace variant of Bint4 weights (1: plain
                               // round-robin): m = 8: 4096^2 66.1 -> 66.5 %, 8192^2 67.3 -> 68.6 %; Aint4 weights keep 1
#endif
#ifndef TG_XR_MIN_M
#define TG_XR_MIN_M 2          // activation rows from which the register-resident-activation kernel (w4_gemm_xr.cuh) takes stacked launches
                               // (same-box A/B against the kernels it replaces, 4096^2: m = 2 71.9 vs 69.7 %, 4: 68.9 vs 66.9, 8: 66.2 vs 62.7,
                               //  16: 65.2 vs 46.0; m = 1 stays on the 32x32x16 kernel, 77 %)
#endif
#ifndef TG_XR_RMX
#define TG_XR_RMX 8            // ... for mx4 (no lookups: latency-bound; the whole slice in flight: m = 16 75.4 -> 79.0 %, m = 2 81.7 -> 85.3 %)
#endif
#ifndef TG_XR_R8K
#define TG_XR_R8K 2            // ... at k = 8192 (128 registers of activations per lane: 4 in flight spill 25)
#endif
#ifndef TG_XR_R
#define TG_XR_R 4              // super-tiles a wave of that kernel keeps in flight
#endif
#ifndef TG_PAIR_M1_LEAN
#define TG_PAIR_M1_LEAN 1      // plain stacked m = 1 calls (g = 128, innerKTiles 4, int4 / any4) run w4_pair_m1_lean_kernel; 0: the general template
#endif
#ifndef TG_PAIR_M1_AHEAD
#define TG_PAIR_M1_AHEAD 1     // ... whose lookups run one step ahead of the products (+ 0.9 % over lookups in step, profiles/m1_lean_ab.txt)
#endif
#ifndef TG_PAIR_WGS
#define TG_PAIR_WGS 512        // persistent workgroups: two per CU (768 / 1024: +4 % / +1 % time)
#endif

}  // namespace
