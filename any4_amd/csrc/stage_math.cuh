// stage_math.cuh -- the arithmetic of the decode stages that more than one kernel computes, one definition each: the fused and the unfused
// path of a stage must agree bit for bit (decode_glue.cuh, attn_prefill.cuh, and w4_helpers.cuh for the stages fused into the GEMMs).
#pragma once

// a value as the 16-bit tensor of the torch formulation holds it
template <typename DT>
__device__ __forceinline__ float round16(float a) { return DT::to_f32(DT::from_f32(a)); }

// packed 16-bit pairs: acc + a.lo * b.lo + a.hi * b.hi in f32 (v_dot2)
template <typename DT>
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc) {
  if constexpr (std::is_same<DT, BF16>::value)
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
  else
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), acc, false);
}

// One output element of x * cos + rotate_half(x) * sin: a * c + b * s with each product and the sum rounded separately, as the torch
// ops do (decode._rope); the caller passes b = -x2 for the lower half.  Contraction is switched off here: the compiler otherwise fuses
// one product of the sum into an FMA (also through __fmul_rn / __fadd_rn), which differs from the torch bits in about one element of
// 1e5 after the rounding to 16 bit.
__device__ __forceinline__ float rope_mul_add(float a, float c, float b, float s) {
#pragma clang fp contract(off)
  const float ac = a * c;
  const float bs = b * s;
  return ac + bs;
}

// One element of LlamaRMSNorm, before its rounding to 16 bits: RNE16(x rs) g (rs = rsqrt(mean(x^2) + eps), g = the norm weight)
template <typename DT>
__device__ __forceinline__ float rmsnorm_elem(float x, float rs, float g) { return round16<DT>(x * rs) * g; }

// One element of SwiGLU, before its rounding to 16 bits: RNE16(silu(g)) u.  g and u are 16-bit values: a caller that holds f32 sums
// rounds them first (swiglu16, w4_helpers.cuh).
template <typename DT>
__device__ __forceinline__ float swiglu_elem(float g, float u) { return round16<DT>(g / (1.f + __expf(-g))) * u; }
