// tg_verify.hip -- dg_verify_attn / dg_verify_attn_scratch_bytes (include/decode_glue_hip.h): split-KV attention for the 1 ... 8 draft tokens
// per sequence of a speculative-decoding verify pass (attn_verify.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "attn_verify.cuh"

// The scratch of a call with nsplit > 1: one int counter per (sequence, kv head, head group) -- at most n * hl of them, rounded up to 16
// bytes --, then [(sequence, token, head)][split][max, sum, d outputs] floats.
struct VerifyScratch {
  int64_t part_offset, bytes;
};
inline VerifyScratch verify_scratch(int64_t n, int hl, int d, int T, int nsplit) {
  const int64_t counters = ((n * hl * 4 + 15) / 16) * 16;
  return {counters, counters + n * T * hl * (int64_t)nsplit * (d + 2) * 4};
}

// everything of a call that needs no device, in the order it is refused: null, dtype, shape, alignment, the scratch's size
int check_verify(const dg_verify& c) {
  const bool split = c.nsplit > 1;
  if (!c.qkv || !c.cos || !c.sin || !c.pos || !c.k_cache || !c.v_cache || !c.out || (split && !c.scratch)) return TG_E_NULL;
  if (!(c.dtype == TG_BF16 || c.dtype == TG_F16)) return TG_E_DTYPE;
  if (!(c.d == 64 || c.d == 128) || c.T < 1 || c.T > 8 || c.nsplit < 1 || c.nsplit > 64) return TG_E_SHAPE;
  if (c.bs <= 0 || c.bs > 65535 || c.hl <= 0 || c.kvl <= 0 || c.hl % c.kvl != 0 || c.hl > 65535 || c.max_seq <= 0 || c.max_seq > 65536)
    return TG_E_SHAPE;
  // slots are int32, and without `slot` sequence i lives in slot i
  if (c.cache_bs <= 0 || c.cache_bs > INT32_MAX || (!c.slot && c.bs != c.cache_bs)) return TG_E_SHAPE;
  if (!aligned16(c.qkv) || !aligned16(c.cos) || !aligned16(c.sin) || !aligned16(c.k_cache) || !aligned16(c.v_cache) || !aligned16(c.out) ||
      (split && !aligned16(c.scratch)))
    return TG_E_ALIGN;
  if (split && c.scratch_bytes < verify_scratch(c.bs, c.hl, c.d, c.T, c.nsplit).bytes) return TG_E_SHAPE;
  return 0;
}

template <typename DT, int D, int NU>
int go(const VerifyParams& P, int64_t n, hipStream_t st) {
  return launch_lds_kernel<verify_attn_kernel<DT, D, NU>>(dim3((unsigned)P.nsplit, (unsigned)(P.kvl * P.hgroups), (unsigned)n), dim3(256),
                                                          verify_lds_bytes<D, NU>(), st, P, false);
}

}  // namespace

extern "C" int64_t dg_verify_attn_scratch_bytes(int64_t n, int hl, int d, int T, int nsplit) {
  if (n <= 0 || hl <= 0 || d <= 0 || T <= 0 || nsplit <= 1) return 0;
  return verify_scratch(n, hl, d, T, nsplit).bytes;
}

extern "C" int dg_verify_attn(const dg_verify* call, int device, tg_stream_t stream) {
  if (!call) return TG_E_NULL;
  if (call->struct_bytes != sizeof(dg_verify)) return TG_E_STRUCT;
  const dg_verify& c = *call;
  if (const int rc = check_verify(c)) return rc;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int rep = c.hl / c.kvl;
  VerifyParams P;
  P.qkv = (const uint16_t*)c.qkv; P.cos = c.cos; P.sin = c.sin; P.pos = c.pos; P.len = c.len; P.slot = c.slot;
  P.k_cache = (uint16_t*)c.k_cache; P.v_cache = (uint16_t*)c.v_cache; P.out = (uint16_t*)c.out;
  P.counters = nullptr; P.part = nullptr;
  if (c.nsplit > 1) {
    P.counters = (int*)c.scratch;
    P.part = (float*)((char*)c.scratch + verify_scratch(c.bs, c.hl, c.d, c.T, c.nsplit).part_offset);
  }
  P.T = c.T; P.hl = c.hl; P.kvl = c.kvl; P.max_seq = (int32_t)c.max_seq; P.cache_bs = (int32_t)c.cache_bs;
  P.RG = rep < 4 ? rep : 4;  // query heads of a kv head that share a workgroup's K / V tiles
  P.hgroups = (int32_t)cdiv(rep, P.RG);
  P.nsplit = c.nsplit; P.scale = c.scale;
  const int64_t n = c.bs;
  hipStream_t st = (hipStream_t)stream;
  return pick_dt(c.dtype, [&](auto DT_) {
    return pick<128, 64>(c.d, [&](auto D_) {
      // one 16-row MFMA unit holds T x RG <= 16 query rows (hl / kvl = 4 and T = 4: exactly), two hold the 32 there can be
      if (P.RG * P.T <= 16) return go<decltype(DT_), decltype(D_)::value, 1>(P, n, st);
      return go<decltype(DT_), decltype(D_)::value, 2>(P, n, st);
    });
  });
}
