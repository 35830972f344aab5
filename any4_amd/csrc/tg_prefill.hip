// tg_prefill.hip -- dg_prefill_attn (include/decode_glue_hip.h): rope + KV-cache append + causal flash attention for a chunk of
// tokens per sequence (attn_prefill.cuh); see tg_common.cuh
#include "attn_call.cuh"
namespace {
#include "attn_prefill.cuh"

template <typename DT, int D, int RG, bool SEQ, bool KV8, bool PAGED = false>
int go(PrefillParams& P, const PrefillSeq& S, const Kv8Exps& E, const KvPages& pages, hipStream_t st) {
  constexpr auto kern = prefill_attn_kernel<DT, D, RG, SEQ, KV8, PAGED>;
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
  PagedArg<PAGED> G;
  if constexpr (PAGED) static_cast<KvPages&>(G) = pages;
  hipLaunchKernelGGL((prefill_rope_kv_kernel<DT, SEQ, KV8, PAGED>), dim3((unsigned)P.T, (unsigned)P.bs), dim3(256), 0, st, P, D, Q, X, G);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 2 * (64 * D * 2 + D * 128), st, P, Q, X, G);
  return launch_status();
}
template <typename DT, int D, bool SEQ, bool KV8, bool PAGED = false>
int go_rg(PrefillParams& P, const PrefillSeq& S, const Kv8Exps& E, const KvPages& pages, hipStream_t st) {
  const int rep = P.hl / P.kvl;  // query heads per kv head: 4 of them share a workgroup's K / V tiles (2 / 1 when there are no more)
  if (rep == 1) return go<DT, D, 1, SEQ, KV8, PAGED>(P, S, E, pages, st);
  if (rep == 2) return go<DT, D, 2, SEQ, KV8, PAGED>(P, S, E, pages, st);
  return go<DT, D, 4, SEQ, KV8, PAGED>(P, S, E, pages, st);
}

// The six entry points behind one validation (check_attn).  c.seq: `len` / `slot` / cache_bs per sequence (otherwise null, null, bs);
// c.kv8: mx8 caches, `k_exp` / `v_exp` their exponent bytes; c.paging: pools behind a block table (per sequence; with c.kv8 four pools, codes and exponents).
int prefill_launch(const AttnCall& c) {
  if (const int rc = check_attn(ATTN_PREFILL, c)) return rc;
  DeviceScope ds(c.device);
  if (!ds.ok) return TG_E_DEVICE;
  PrefillParams P;
  P.qkv = (const uint16_t*)c.qkv; P.cos = c.cos; P.sin = c.sin; P.pos = c.pos;
  P.k_cache = (uint16_t*)c.k_cache; P.v_cache = (uint16_t*)c.v_cache; P.out = (uint16_t*)c.out;
  P.bs = (int32_t)c.bs; P.T = (int32_t)c.T; P.hl = c.hl; P.kvl = c.kvl; P.max_seq = (int32_t)c.max_seq; P.scale = c.scale;
  const PrefillSeq S{c.len, c.slot, (int32_t)c.cache_bs};
  const Kv8Exps E{(uint8_t*)c.k_exp, (uint8_t*)c.v_exp};
  const KvPages pages = c.paging ? kv_pages(c) : KvPages{};
  hipStream_t st = (hipStream_t)c.stream;
  return pick_dt(c.dtype, [&](auto DT_) {
    return pick<128, 64>(c.d, [&](auto D_) {
      if (c.paging && c.kv8) return go_rg<decltype(DT_), decltype(D_)::value, true, true, true>(P, S, E, pages, st);
      if (c.paging) return go_rg<decltype(DT_), decltype(D_)::value, true, false, true>(P, S, E, pages, st);
      return pick<0, 1>(c.seq, [&](auto SEQ_) {
        return pick<0, 1>(c.kv8, [&](auto KV8_) {
          return go_rg<decltype(DT_), decltype(D_)::value, (bool)decltype(SEQ_)::value, (bool)decltype(KV8_)::value>(P, S, E, pages, st);
        });
      });
    });
  });
}

}  // namespace

extern "C" int dg_prefill_attn(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache,
                               void* out, int64_t bs, int64_t T, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype,
                               int device, tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_cache, v_cache, out, bs, hl, kvl, d, max_seq, scale, dtype, device, stream).chunk(T));
}

extern "C" int dg_prefill_attn_seq(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                   const int64_t* slot, void* k_cache, void* v_cache, void* out, int64_t n, int64_t T, int64_t cache_bs,
                                   int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device, tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_cache, v_cache, out, n, hl, kvl, d, max_seq, scale, dtype, device, stream)
                            .chunk(T).slots(len, slot, cache_bs));
}

extern "C" int dg_prefill_attn_mx8(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache,
                                   void* k_exp, void* v_exp, void* out, int64_t bs, int64_t T, int hl, int kvl, int d, int64_t max_seq, float scale,
                                   int dtype, int device, tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_cache, v_cache, out, bs, hl, kvl, d, max_seq, scale, dtype, device, stream)
                            .chunk(T).mx8(k_exp, v_exp));
}

extern "C" int dg_prefill_attn_mx8_seq(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                       const int64_t* slot, void* k_cache, void* v_cache, void* k_exp, void* v_exp, void* out, int64_t n, int64_t T,
                                       int64_t cache_bs, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device,
                                       tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_cache, v_cache, out, n, hl, kvl, d, max_seq, scale, dtype, device, stream)
                            .chunk(T).slots(len, slot, cache_bs).mx8(k_exp, v_exp));
}

extern "C" int dg_prefill_attn_paged(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                     const int64_t* slot, const int32_t* table, void* k_pool, void* v_pool, void* out, int64_t n, int64_t T,
                                     int64_t cache_bs, int hl, int kvl, int d, int64_t max_seq, int64_t page_size, int64_t num_pages, float scale,
                                     int dtype, int device, tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_pool, v_pool, out, n, hl, kvl, d, max_seq, scale, dtype, device, stream)
                            .chunk(T).slots(len, slot, cache_bs).paged(table, page_size, num_pages));
}

extern "C" int dg_prefill_attn_mx8_paged(const void* qkv, const float* cos, const float* sin, const int64_t* pos, const int64_t* len,
                                         const int64_t* slot, const int32_t* table, void* k_pool, void* v_pool, void* k_exp, void* v_exp,
                                         void* out, int64_t n, int64_t T, int64_t cache_bs, int hl, int kvl, int d, int64_t max_seq,
                                         int64_t page_size, int64_t num_pages, float scale, int dtype, int device, tg_stream_t stream) {
  return prefill_launch(attn_call(qkv, cos, sin, pos, k_pool, v_pool, out, n, hl, kvl, d, max_seq, scale, dtype, device, stream)
                            .chunk(T).slots(len, slot, cache_bs).mx8(k_exp, v_exp).paged(table, page_size, num_pages));
}
