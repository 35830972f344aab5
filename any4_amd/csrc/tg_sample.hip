// tg_sample.hip -- dg_sample / dg_sample_scratch_bytes (include/decode_glue_hip.h): temperature / top-k / top-p sampling of the decode
// stack's logits in one launch (sample.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "sample.cuh"

template <typename DT>
int go(const SampleParams& P, int64_t bs, hipStream_t st) {
  constexpr auto kern = sample_kernel<DT>;
  const int prc = prepare_lds_kernel<kern>();
  if (prc != 0) return prc;
  hipLaunchKernelGGL(kern, dim3((unsigned)bs), dim3(SMP_THREADS), sizeof(SampleShared), st, P);
  return launch_status();
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t dg_sample_scratch_bytes(int64_t bs, int64_t vocab) {
  (void)bs; (void)vocab;
  return 0;  // the count tables of a row fit the LDS of the workgroup that owns the row
}

extern "C" int dg_sample(const void* logits, const int64_t* ctr, const float* temperature, const int32_t* top_k, const float* top_p,
                         const int64_t* seed, const float* u_in, int64_t* token_out, float* u_out, void* scratch, int64_t scratch_bytes,
                         int64_t bs, int64_t vocab, int64_t ld, int per_sequence, int64_t ctr_add, int dtype, int device, tg_stream_t stream) {
  (void)scratch; (void)scratch_bytes;
  if (!logits || !ctr || !temperature || !top_k || !top_p || !token_out || (!seed && !u_in)) return TG_E_NULL;
  if (dtype != TG_BF16 && dtype != TG_F16) return TG_E_DTYPE;
  if (bs < 1 || vocab < 1 || ld < vocab) return TG_E_SHAPE;
  if (bs > INT32_MAX || vocab > (1 << 30)) return TG_E_SIZE;
  if (!aligned_to(logits, 2) || !aligned_to(ctr, 8) || !aligned_to(seed, 8) || !aligned_to(token_out, 8) || !aligned_to(temperature, 4) ||
      !aligned_to(top_k, 4) || !aligned_to(top_p, 4) || !aligned_to(u_in, 4) || !aligned_to(u_out, 4))
    return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  SampleParams P;
  P.logits = (const uint16_t*)logits; P.ld = ld; P.ctr = ctr; P.temperature = temperature; P.top_k = top_k; P.top_p = top_p; P.seed = seed;
  P.u_in = u_in; P.token_out = token_out; P.u_out = u_out; P.ctr_add = ctr_add; P.vocab = (int32_t)vocab; P.per_sequence = per_sequence != 0;
  int bits = 0;  // vocab < 2^bits: masses are multiples of 2^-shift with vocab x 2^shift < 2^62
  while ((vocab >> bits) != 0) ++bits;
  P.shift = 62 - bits;
  return pick_dt(dtype, [&](auto DT_) { return go<decltype(DT_)>(P, bs, (hipStream_t)stream); });
}
