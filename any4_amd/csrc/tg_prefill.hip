// tg_prefill.hip -- DG_ATTN_PREFILL of dg_attn_launch (include/decode_glue_hip.h): rope + KV-cache append + causal flash attention for a chunk of
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

}  // namespace

// The six DG_ATTN_PREFILL flavours behind one validation (check_attn).  f.seq: `len` / `slot` / cache_bs per sequence (otherwise null, null, bs);
// f.kv8: mx8 caches, `k_exp` / `v_exp` their exponent bytes; f.paging: pools behind a block table (per sequence; with f.kv8 four pools, codes and exponents).
int prefill_launch(const dg_attn& c, int device, tg_stream_t stream) {
  if (const int rc = check_attn(DG_ATTN_PREFILL, c)) return rc;
  const AttnFlags f(c);
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  PrefillParams P;
  P.qkv = (const uint16_t*)c.qkv; P.cos = c.cos; P.sin = c.sin; P.pos = c.pos;
  P.k_cache = (uint16_t*)c.k_cache; P.v_cache = (uint16_t*)c.v_cache; P.out = (uint16_t*)c.out;
  P.bs = (int32_t)c.bs; P.T = (int32_t)c.T; P.hl = c.hl; P.kvl = c.kvl; P.max_seq = (int32_t)c.max_seq; P.scale = c.scale;
  const PrefillSeq S{c.len, c.slot, (int32_t)c.cache_bs};
  const Kv8Exps E{(uint8_t*)c.k_exp, (uint8_t*)c.v_exp};
  const KvPages pages = f.paging ? kv_pages(c) : KvPages{};
  hipStream_t st = (hipStream_t)stream;
  return pick_dt(c.dtype, [&](auto DT_) {
    return pick<128, 64>(c.d, [&](auto D_) {
      if (f.paging && f.kv8) return go_rg<decltype(DT_), decltype(D_)::value, true, true, true>(P, S, E, pages, st);
      if (f.paging) return go_rg<decltype(DT_), decltype(D_)::value, true, false, true>(P, S, E, pages, st);
      return pick<0, 1>(f.seq, [&](auto SEQ_) {
        return pick<0, 1>(f.kv8, [&](auto KV8_) {
          return go_rg<decltype(DT_), decltype(D_)::value, (bool)decltype(SEQ_)::value, (bool)decltype(KV8_)::value>(P, S, E, pages, st);
        });
      });
    });
  });
}
