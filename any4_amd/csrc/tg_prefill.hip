// tg_prefill.hip -- dg_prefill_attn (include/decode_glue_hip.h): rope + KV-cache append + causal flash attention for a chunk of
// tokens per sequence (attn_prefill.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "attn_prefill.cuh"

template <typename DT, int D, int RG, bool SEQ, bool KV8>
int go(PrefillParams& P, const PrefillSeq& S, const Kv8Exps& E, hipStream_t st) {
  constexpr auto kern = prefill_attn_kernel<DT, D, RG, SEQ, KV8>;
  const int prc = prepare_lds_kernel<kern>();
  if (prc != 0) return prc;
  constexpr int BQ = 16 * 4 * PF_NU / RG;
  const int rep = P.hl / P.kvl;
  P.nqb = (int32_t)cdiv(P.T, BQ);
  P.hgroups = (int32_t)cdiv(rep, RG);
  const int64_t blocks = (int64_t)P.nqb * P.bs * P.kvl * P.hgroups;
  if (blocks > INT32_MAX) return TG_E_SIZE;
  PrefillSeqArg<SEQ> Q;
  if constexpr (SEQ) static_cast<PrefillSeq&>(Q) = S;
  Kv8Arg<KV8> X;
  if constexpr (KV8) static_cast<Kv8Exps&>(X) = E;
  hipLaunchKernelGGL((prefill_rope_kv_kernel<DT, SEQ, KV8>), dim3((unsigned)P.T, (unsigned)P.bs), dim3(256), 0, st, P, D, Q, X);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 2 * (64 * D * 2 + D * 128), st, P, Q, X);
  return launch_status();
}
template <typename DT, int D, bool SEQ, bool KV8>
int go_rg(PrefillParams& P, const PrefillSeq& S, const Kv8Exps& E, hipStream_t st) {
  const int rep = P.hl / P.kvl;  // query heads per kv head: 4 of them share a workgroup's K / V tiles (2 / 1 when there are no more)
  if (rep == 1) return go<DT, D, 1, SEQ, KV8>(P, S, E, st);
  if (rep == 2) return go<DT, D, 2, SEQ, KV8>(P, S, E, st);
  return go<DT, D, 4, SEQ, KV8>(P, S, E, st);
}

// dg_prefill_attn (SEQ = false: `len`, `slot` null, cache_bs = bs) and dg_prefill_attn_seq behind one validation; KV8: their _mx8 forms
// (mx8 caches, `k_exp` / `v_exp` their exponent bytes)
template <bool SEQ, bool KV8 = false>
int prefill_launch(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len, const int64_t* slot,
                   void* k_cache, void* v_cache, void* out, int64_t bs, int64_t T, int64_t cache_bs, int hl, int kvl, int d, int64_t max_seq,
                   float scale, int dtype, int device, tg_stream_t stream, void* k_exp = nullptr, void* v_exp = nullptr) {
  if (!qkv || !cos || !sin || !pos || !k_cache || !v_cache || !out || (KV8 && (!k_exp || !v_exp))) return TG_E_NULL;
  if (!(dtype == TG_BF16 || dtype == TG_F16)) return TG_E_DTYPE;
  if (bs <= 0 || bs > 65535 || T <= 0 || hl <= 0 || kvl <= 0 || hl % kvl != 0 || !(d == 64 || d == 128) || max_seq <= 0 || max_seq > 8192 ||
      bs * T > INT32_MAX / 2)
    return TG_E_SHAPE;
  if (SEQ && (cache_bs <= 0 || cache_bs > INT32_MAX || (!slot && bs != cache_bs))) return TG_E_SHAPE;
  if (!aligned16(qkv) || !aligned16(cos) || !aligned16(sin) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) ||
      !aligned16(k_exp) || !aligned16(v_exp))
    return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  PrefillParams P;
  P.qkv = (const uint16_t*)qkv; P.cos = cos; P.sin = sin; P.pos = pos;
  P.k_cache = (uint16_t*)k_cache; P.v_cache = (uint16_t*)v_cache; P.out = (uint16_t*)out;
  P.bs = (int32_t)bs; P.T = (int32_t)T; P.hl = hl; P.kvl = kvl; P.max_seq = (int32_t)max_seq; P.scale = scale;
  const PrefillSeq S{len, slot, (int32_t)cache_bs};
  hipStream_t st = (hipStream_t)stream;
  const Kv8Exps E{(uint8_t*)k_exp, (uint8_t*)v_exp};
  return pick_dt(dtype, [&](auto DT_) { return d == 128 ? go_rg<decltype(DT_), 128, SEQ, KV8>(P, S, E, st) : go_rg<decltype(DT_), 64, SEQ, KV8>(P, S, E, st); });
}
}  // namespace

extern "C" int dg_prefill_attn(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache,
                               void* out, int64_t bs, int64_t T, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype,
                               int device, tg_stream_t stream) {
  return prefill_launch<false>(qkv, cos, sin, pos, nullptr, nullptr, k_cache, v_cache, out, bs, T, bs, hl, kvl, d, max_seq, scale, dtype, device,
                               stream);
}

extern "C" int dg_prefill_attn_seq(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                   const int64_t* slot, void* k_cache, void* v_cache, void* out, int64_t n, int64_t T, int64_t cache_bs,
                                   int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device, tg_stream_t stream) {
  return prefill_launch<true>(qkv, cos, sin, pos, len, slot, k_cache, v_cache, out, n, T, cache_bs, hl, kvl, d, max_seq, scale, dtype, device,
                              stream);
}

extern "C" int dg_prefill_attn_mx8(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache,
                                   void* k_exp, void* v_exp, void* out, int64_t bs, int64_t T, int hl, int kvl, int d, int64_t max_seq, float scale,
                                   int dtype, int device, tg_stream_t stream) {
  return prefill_launch<false, true>(qkv, cos, sin, pos, nullptr, nullptr, k_cache, v_cache, out, bs, T, bs, hl, kvl, d, max_seq, scale, dtype,
                                     device, stream, k_exp, v_exp);
}

extern "C" int dg_prefill_attn_mx8_seq(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                       const int64_t* slot, void* k_cache, void* v_cache, void* k_exp, void* v_exp, void* out, int64_t n, int64_t T,
                                       int64_t cache_bs, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device,
                                       tg_stream_t stream) {
  return prefill_launch<true, true>(qkv, cos, sin, pos, len, slot, k_cache, v_cache, out, n, T, cache_bs, hl, kvl, d, max_seq, scale, dtype, device,
                                    stream, k_exp, v_exp);
}
