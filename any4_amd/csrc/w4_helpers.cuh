// w4_helpers.cuh -- device helpers the W4A16 GEMM kernels share (w4_gemm_pair.cuh, w4_gemm_pair16.cuh, w4_gemm_pair16_loop.cuh,
// w4_gemm_xr.cuh, w4_gemv.cuh): fragment-order addressing, the mx4 converters, MFMA / v_dot2 / v_bfi wrappers and the stages fused into
// a GEMM's staging and output store.  Included inside the unit's anonymous namespace, after tg_common.cuh.
#pragma once
#include "stage_math.cuh"

// Element (r, c) of a matrix kept in the reference's m16n8k16 A-fragment order [ceil(rows/16)][ctiles = ceil(cols/16)][32][8]
// (TinyGemmConvertA.cu:19-141: lane t = 4 (r & 7) + (c & 7) / 2 holds (r, c0) (r, c0+1) (r+8, c0) (r+8, c0+1) and the same at
// c0 + 8): the "TC" activations / outputs of tinygemm_y_f16TC_x_f16TC_w_*TC with the weights on the right.
__device__ __forceinline__ int64_t tc_a_index(int r, int c, int ctiles) {
  const int t = (r & 7) * 4 + ((c & 7) >> 1);
  const int j = (c & 1) + 2 * ((r >> 3) & 1) + 4 * ((c >> 3) & 1);
  return (((int64_t)(r >> 4) * ctiles + (c >> 4)) * 32 + t) * 8 + j;
}
// the 32 k of chunk ch of row a (16 dwords in k order) from A-fragment-order activations
__device__ __forceinline__ void tc_a_load_chunk(const char* xb, int a, int ch, int ktiles, uint32_t (&d)[16]) {
#pragma unroll
  for (int dw = 0; dw < 16; ++dw) d[dw] = *reinterpret_cast<const uint32_t*>(xb + tc_a_index(a, ch * 32 + 2 * dw, ktiles) * 2);
}

// mx4 on gfx950 without a table: v_cvt_scalef32_pk_bf16_fp4 converts the two fp4-e2m1 codes of one byte of a packed word into a pair
// of bf16 values times an f32 scale -- the dequantised weights (fp4[code] * 2^(e - 127), exact) in ONE vector instruction per two
// weights, no LDS lookup, and with the group's scale already inside the operand no per-group accumulator update either.  Checked
// against the e2m1 table for every byte value, every byte position and scales from 2^-127 (denormal) to 2^127 and NaN (e = 255):
// tools/ubench/mx4_cvt_probe.hip.
__device__ __forceinline__ u32x4 mx4_cvt_word(uint32_t w, float scale) {
  u32x4 r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return r;
}

// ... one byte (sel = 0 ... 3, a constant after unrolling: the switch folds)
__device__ __forceinline__ uint32_t mx4_cvt_byte(uint32_t w, float scale, int sel) {
  switch (sel) {
    case 0: return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
    case 1: return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
    case 2: return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
    default: return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  }
}

typedef __attribute__((ext_vector_type(16))) float f32x16;

template <typename DT>
__device__ __forceinline__ f32x16 mfma32(u32x4 a, u32x4 b, f32x16 c) {
  if constexpr (std::is_same<DT, BF16>::value)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) {  // (mask & a) | (~mask & b)
  uint32_t d;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "s"(mask), "v"(a), "v"(b));
  return d;
}

template <typename DT>
__device__ __forceinline__ float dot2_ones(uint32_t pair, float acc) {
  if constexpr (std::is_same<DT, BF16>::value)
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, pair), __builtin_bit_cast(bf16x2, 0x3f803f80u), acc, false);
  else
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, pair), __builtin_bit_cast(f16x2, 0x3c003c00u), acc, false);
}

// sum of squares of the 32 values of a staged chunk (16 packed pairs), f32
template <typename DT>
__device__ __forceinline__ float chunk_sumsq(const uint32_t (&d)[16]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if constexpr (std::is_same<DT, BF16>::value)
      s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, d[j]), __builtin_bit_cast(bf16x2, d[j]), s, false);
    else
      s = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, d[j]), __builtin_bit_cast(f16x2, d[j]), s, false);
  }
  return s;
}
// LlamaRMSNorm of a staged chunk: x' = RNE16(RNE16(x rs) g), g = the chunk's 32 norm weights (64 bytes at gsrc): the formula
// and rounding points of rmsnorm_elem (stage_math.cuh; dg_add_rmsnorm calls it).  Written out here: through the call the norm weight is
// unpacked before the first product instead of after it, and the bf16 kernels with the fused norm come out in another schedule.
template <typename DT>
__device__ __forceinline__ void chunk_rmsnorm(uint32_t (&d)[16], float rs, const u32x4 (&gw)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u32x4 g = gw[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = d[4 * j + e];
      const float lo = round16<DT>(DT::lo_f32(v) * rs) * DT::lo_f32(g[e]);
      const float hi = round16<DT>(DT::hi_f32(v) * rs) * DT::hi_f32(g[e]);
      d[4 * j + e] = DT::pack2(lo, hi);
    }
  }
}
// SwiGLU of two 16-bit GEMM outputs (swiglu_elem, as dg_swiglu): RNE16(RNE16(silu(g)) u)
template <typename DT>
__device__ __forceinline__ uint16_t swiglu16(float gsum, float usum) {
  return DT::from_f32(swiglu_elem<DT>(round16<DT>(gsum), round16<DT>(usum)));
}
