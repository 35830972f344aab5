// tg_lora.hip -- dg_lora_shrink / dg_lora_expand (include/decode_glue_hip.h): per-sequence LoRA adapters on a linear's output, picked on
// the device by an index per sequence (lora.cuh); see tg_common.cuh
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
namespace {
#include "lora.cuh"

// what both entries share: dtype, the rank, the row and adapter counts
int check_common(int dtype, int64_t m, int64_t r, int64_t n_adapters, int64_t rows_per_id) {
  if (dtype != TG_BF16 && dtype != TG_F16) return TG_E_DTYPE;
  if (m < 1 || n_adapters < 1 || rows_per_id < 1 || r < 8 || r > LORA_MAX_R || (r % 8) != 0) return TG_E_SHAPE;
  if (m > INT32_MAX || n_adapters > INT32_MAX) return TG_E_SIZE;
  return 0;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int dg_lora_shrink(const void* x, const void* norm_weight, const void* A, const int32_t* idx, float* t, int64_t m, int64_t k,
                              int64_t r, int64_t n_adapters, int64_t rows_per_id, float eps, int dtype, int device, tg_stream_t stream) {
  if (!x || !A || !idx || !t) return TG_E_NULL;
  const int rc = check_common(dtype, m, r, n_adapters, rows_per_id);
  if (rc != 0) return rc;
  if (k < 8) return TG_E_SHAPE;
  if ((k % 8) != 0) return TG_E_K_DIV;
  if (k > (1 << 17)) return TG_E_SIZE;  // (the f32 sum of squares of the norm flavour is derived for up to 32 passes)
  if (!aligned16(x) || !aligned16(A) || !aligned16(t) || !aligned16(norm_weight) || !aligned4(idx)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  LoraShrinkParams P;
  P.x = (const uint16_t*)x; P.g = (const uint16_t*)norm_weight; P.A = (const uint16_t*)A; P.idx = idx; P.t = t;
  P.m = m; P.k = (int32_t)k; P.r = (int32_t)r; P.n_adapters = (int32_t)n_adapters; P.rows_per_id = rows_per_id;
  P.eps = eps; P.inv_k = 1.0f / (float)k;
  return pick_dt(dtype, [&](auto DT_) {
    hipLaunchKernelGGL(lora_shrink_kernel<decltype(DT_)>, dim3((unsigned)m, (unsigned)(r / LSH_J)), dim3(LSH_THREADS), 0, (hipStream_t)stream, P);
    return launch_status();
  });
}

extern "C" int dg_lora_expand(const float* t, const void* B, const float* scale, const int32_t* idx, void* y, int64_t m, int64_t n, int64_t r,
                              int64_t ldy, int64_t n_adapters, int64_t rows_per_id, int dtype, int device, tg_stream_t stream) {
  if (!t || !B || !scale || !idx || !y) return TG_E_NULL;
  const int rc = check_common(dtype, m, r, n_adapters, rows_per_id);
  if (rc != 0) return rc;
  if (n < 8 || (n % 8) != 0 || ldy < n || (ldy % 8) != 0) return TG_E_SHAPE;
  if (n > (int64_t)65535 * LEX_COLS) return TG_E_SIZE;
  if (!aligned16(t) || !aligned16(B) || !aligned16(y) || !aligned4(scale) || !aligned4(idx)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  LoraExpandParams P;
  P.t = t; P.B = (const uint16_t*)B; P.scale = scale; P.idx = idx; P.y = (uint16_t*)y;
  P.m = m; P.ldy = ldy; P.n = (int32_t)n; P.r = (int32_t)r; P.n_adapters = (int32_t)n_adapters; P.rows_per_id = rows_per_id;
  return pick_dt(dtype, [&](auto DT_) {
    return pick<1, LEX_ROWS>(m == 1 ? 1 : LEX_ROWS, [&](auto NR_) {
      constexpr int NR = decltype(NR_)::value;
      hipLaunchKernelGGL((lora_expand_kernel<decltype(DT_), NR>), dim3((unsigned)cdiv(m, NR), (unsigned)cdiv(n, LEX_COLS)), dim3(LEX_THREADS), 0,
                         (hipStream_t)stream, P);
      return launch_status();
    });
  });
}
