// rope_math.cuh -- the arithmetic of the rotary embedding, shared by every kernel that ropes (decode_glue.cuh, attn_prefill.cuh).
#pragma once

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
