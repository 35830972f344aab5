// tg_prefill.hip -- dg_prefill_attn (include/decode_glue_hip.h): rope + KV-cache append + causal flash attention for a chunk of
// tokens per sequence (attn_prefill.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "attn_prefill.cuh"

template <typename DT, int D, int RG>
int go(PrefillParams& P, hipStream_t st) {
  constexpr auto kern = prefill_attn_kernel<DT, D, RG>;
  const int prc = prepare_lds_kernel<kern>();
  if (prc != 0) return prc;
  constexpr int BQ = 16 * 4 * PF_NU / RG;
  const int rep = P.hl / P.kvl;
  P.nqb = (int32_t)cdiv(P.T, BQ);
  P.hgroups = (int32_t)cdiv(rep, RG);
  const int64_t blocks = (int64_t)P.nqb * P.bs * P.kvl * P.hgroups;
  if (blocks > INT32_MAX) return TG_E_SIZE;
  hipLaunchKernelGGL(prefill_rope_kv_kernel<DT>, dim3((unsigned)P.T, (unsigned)P.bs), dim3(256), 0, st, P, D);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 2 * (64 * D * 2 + D * 128), st, P);
  return launch_status();
}
template <typename DT, int D>
int go_rg(PrefillParams& P, hipStream_t st) {
  const int rep = P.hl / P.kvl;  // query heads per kv head: 4 of them share a workgroup's K / V tiles (2 / 1 when there are no more)
  if (rep == 1) return go<DT, D, 1>(P, st);
  if (rep == 2) return go<DT, D, 2>(P, st);
  return go<DT, D, 4>(P, st);
}
}  // namespace

extern "C" int dg_prefill_attn(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache,
                               void* out, int64_t bs, int64_t T, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype,
                               int device, tg_stream_t stream) {
  if (!qkv || !cos || !sin || !pos || !k_cache || !v_cache || !out) return TG_E_NULL;
  if (!(dtype == TG_BF16 || dtype == TG_F16)) return TG_E_DTYPE;
  if (bs <= 0 || bs > 65535 || T <= 0 || hl <= 0 || kvl <= 0 || hl % kvl != 0 || !(d == 64 || d == 128) || max_seq <= 0 || max_seq > 8192 ||
      bs * T > INT32_MAX / 2)
    return TG_E_SHAPE;
  if (!aligned16(qkv) || !aligned16(cos) || !aligned16(sin) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  PrefillParams P;
  P.qkv = (const uint16_t*)qkv; P.cos = cos; P.sin = sin; P.pos = pos;
  P.k_cache = (uint16_t*)k_cache; P.v_cache = (uint16_t*)v_cache; P.out = (uint16_t*)out;
  P.bs = (int32_t)bs; P.T = (int32_t)T; P.hl = hl; P.kvl = kvl; P.max_seq = (int32_t)max_seq; P.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  return pick_dt(dtype, [&](auto DT_) { return d == 128 ? go_rg<decltype(DT_), 128>(P, st) : go_rg<decltype(DT_), 64>(P, st); });
}
