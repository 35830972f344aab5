// kv8.cuh -- the mx8 KV-cache format on the device (any4_amd/kvcache.py is its definition: E4M3 codes, one E8M0 exponent byte per 32
// consecutive elements of a row), shared by decode_glue.cuh and attn_prefill.cuh.  Readers convert with gfx950's scaled conversion
// (v_cvt_scalef32_pk_{bf16,f16}_fp8: two codes times an f32 scale in one instruction, exact); the writers encode in plain arithmetic
// (exponent from the block maximum's f32 bits, an exact power-of-two scale, clamp, round to nearest even) because the host encoder's
// bytes are the contract and a writer handles two rows per token.
#pragma once

// What only the mx8 kernels read: their LAST argument, and an empty one for the 16-bit flavour (which keeps its argument offsets and its code)
struct Kv8Exps {
  uint8_t* k_exp;  // [bs][kvl][max_seq][d / 32]
  uint8_t* v_exp;
};
template <bool KV8> struct Kv8Arg {};
template <> struct Kv8Arg<true> : Kv8Exps {};

// eight codes (two dwords, element order) with exponent byte E -> eight values of the 16-bit type; E = 255: NaN in every place
template <typename DT>
__device__ __forceinline__ u32x4 mx8_to16(const u32x2& c, uint32_t E) {
  const float s = u2f(E == 0u ? 0x00400000u : (E << 23));  // 2^(E - 127); E = 0: 2^-127, a denormal
  u32x4 r;
  if constexpr (std::is_same<DT, BF16>::value) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], s, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], s, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], s, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], s, true));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], s, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], s, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], s, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], s, true));
  }
  if (E == 255u) {  // (selected, not left to what the conversion makes of an infinite scale)
    const uint32_t nan2 = std::is_same<DT, BF16>::value ? 0x7fc07fc0u : 0x7e007e00u;
    r = u32x4{nan2, nan2, nan2, nan2};
  }
  return r;
}

// E4M3 code of y, |y| <= 448 and finite, round to nearest even (subnormals are multiples of 2^-9; 8 is the smallest normal, 2^-6)
__device__ __forceinline__ uint32_t mx8_e4m3_rne(float y) {
  const uint32_t sign = (f2u(y) >> 24) & 0x80u;
  const float a = fabsf(y);
  uint32_t c;
  if (a < 0.015625f) {
    c = (uint32_t)__builtin_rintf(a * 512.f);
  } else {
    uint32_t v = f2u(a);
    v += 0x7ffffu + ((v >> 20) & 1u);
    c = (v >> 20) - (120u << 3);
  }
  return sign | c;
}

// One element per lane, a 32-element block = 32 ALIGNED lanes of a wave; every lane of the wave must be here (lanes without an element
// pass 0).  Returns the lane's code and the block's exponent byte.
__device__ __forceinline__ void mx8_encode_lane(float x, uint32_t& code, uint32_t& E) {
  float a = fabsf(x);
  a = a < INFINITY ? a : INFINITY;  // (a NaN too: the block is marked, fmaxf would drop it)
  float m = tgl::row_max(a), p, q;
  tgl::rows16(m, p, q);
  const uint32_t u = f2u(fmaxf(p, q));
  // amax = m 2^ex, m in [0.5, 1): ex = biased - 126; the byte is ex - 9 + 127, one more when m > 0.875 (mantissa above 1.75), clamped at 0
  int e = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < 0 ? 0 : e;
  const bool bad = u >= 0x7f800000u;
  const float y = fminf(fmaxf(x * u2f((uint32_t)(254 - e) << 23), -448.f), 448.f);
  code = bad ? 0x7fu : mx8_e4m3_rne(y);
  E = bad ? 255u : (uint32_t)e;
}
// ... and the value the cache row now holds in this place (f32 of the 16-bit type)
template <typename DT>
__device__ __forceinline__ float mx8_encode_lane(float x, uint32_t& code, uint32_t& E) {
  mx8_encode_lane(x, code, E);
  return DT::lo_f32(mx8_to16<DT>(u32x2{code, 0u}, E)[0]);
}

// (a kernel that takes the exponent pointers as an optional last parameter, `PG... pack`: the one element of the pack, and whether the pack is that)
__device__ __forceinline__ const Kv8Exps& kv8_exps_arg(const Kv8Exps& x) { return x; }
template <typename... PG> struct Kv8Pack : std::false_type {};
template <> struct Kv8Pack<Kv8Exps> : std::true_type {};
// (the paged mx8 flavour: the pack is `KvPages, Kv8Exps`, in that order -- kv_paged.cuh; the exponent pointers are then those of the pools)
template <typename PAGES> __device__ __forceinline__ const Kv8Exps& kv8_exps_arg(const PAGES&, const Kv8Exps& x) { return x; }
template <typename PAGES> struct Kv8Pack<PAGES, Kv8Exps> : std::true_type {};

// EIGHT elements per lane (a row lies across d / 8 lanes, as in rope_attn_online_kernel), a 32-element block = an ALIGNED QUAD of lanes;
// every lane of the quad must be here.  `v`: the lane's eight 16-bit values.  The block maximum is the lane's own maximum and two
// quad_perm exchanges; exponent rule, clamp, RNE and the non-finite block are mx8_encode_lane's, so the bytes are the host encoder's.
// Returns the lane's eight codes (element order), the block's exponent byte, and the eight values the cache row now holds.
template <typename DT>
__device__ __forceinline__ u32x4 mx8_encode_piece(const u32x4& v, u32x2& codes, uint32_t& E) {
  float x[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[2 * q] = DT::lo_f32(v[q]);
    x[2 * q + 1] = DT::hi_f32(v[q]);
  }
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float a = fabsf(x[e]);
    a = a < INFINITY ? a : INFINITY;  // (a NaN too: the block is marked, fmaxf would drop it)
    m = fmaxf(m, a);
  }
  m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, m), 0xB1, 0xf, 0xf, true)));  // quad_perm [1,0,3,2]
  m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, m), 0x4E, 0xf, 0xf, true)));  // quad_perm [2,3,0,1]
  const uint32_t u = f2u(m);
  int e = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < 0 ? 0 : e;
  const bool bad = u >= 0x7f800000u;
  const float s = u2f((uint32_t)(254 - e) << 23);
  uint32_t c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = bad ? 0x7fu : mx8_e4m3_rne(fminf(fmaxf(x[j] * s, -448.f), 448.f));
  codes = u32x2{c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24)};
  E = bad ? 255u : (uint32_t)e;
  return mx8_to16<DT>(codes, E);
}
