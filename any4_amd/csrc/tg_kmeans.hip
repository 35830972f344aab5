// tg_kmeans.hip -- tg_kmeans_rows / tg_kmeans_rows_plan (include/tinygemm_hip.h): the any4 quantizer's per-row weighted 1-D k-means in
// one launch, one workgroup per row (kmeans.cuh); see tg_common.cuh
#include "tg_common.cuh"
namespace {
#include "kmeans.cuh"

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// everything of a call that needs neither a device nor a pointer: the refusals, the padded row length, the LDS of one workgroup
int plan_kmeans(int64_t rows, int64_t k, int C, int S, int max_iter, double tol, bool weighted, int32_t& n2, int64_t& lds) {
  if (rows < 0 || k < 1 || C < 1 || C > KM_MAX_C || S < 1 || S > KM_MAX_S) return TG_E_SHAPE;
  if (max_iter < 1 || max_iter > KM_MAX_ITER || !(tol >= 0.0) || !(tol < 1e300)) return TG_E_SHAPE;
  if (k > KM_MAX_K || rows > INT32_MAX) return TG_E_SIZE;
  n2 = 1;
  while (n2 < k) n2 <<= 1;
  lds = km_lds_bytes(n2, weighted);
  return lds <= 160 * 1024 ? 0 : (int)TG_E_SIZE;
}

template <bool W>
int go(const KmParams& P, int64_t lds, hipStream_t st) {
  constexpr auto kern = kmeans_rows_kernel<W>;
  const int prc = prepare_lds_kernel<kern>();
  if (prc != 0) return prc;
  hipLaunchKernelGGL(kern, dim3((unsigned)P.rows), dim3(KM_THREADS), (unsigned)lds, st, P);
  return launch_status();
}

}  // namespace

extern "C" int tg_kmeans_rows_plan(int64_t rows, int64_t k, int C, int S, int max_iter, double tol, int weighted, int64_t* out) {
  int32_t n2 = 0;
  int64_t lds = 0;
  const int rc = plan_kmeans(rows, k, C, S, max_iter, tol, weighted != 0, n2, lds);
  if (rc != 0) return rc;
  if (!out) return TG_E_NULL;
  out[0] = rows;  // workgroups: one per row
  out[1] = lds;   // dynamic LDS bytes of each
  return 0;
}

extern "C" int tg_kmeans_rows(const float* x, const float* w, int64_t w_row_stride, const float* c0, int32_t* assign, float* centers,
                              double* sse, int32_t* iters, int64_t rows, int64_t k, int C, int S, int max_iter, double tol, int device,
                              tg_stream_t stream) {
  int32_t n2 = 0;
  int64_t lds = 0;
  const int rc = plan_kmeans(rows, k, C, S, max_iter, tol, w != nullptr, n2, lds);
  if (rc != 0) return rc;
  if (w && w_row_stride != 0 && w_row_stride != k) return TG_E_SHAPE;
  if (rows == 0) return 0;
  if (!x || !c0 || !assign || !centers) return TG_E_NULL;
  if (!aligned_to(x, 4) || !aligned_to(w, 4) || !aligned_to(c0, 4) || !aligned_to(assign, 4) || !aligned_to(centers, 4) ||
      !aligned_to(sse, 8) || !aligned_to(iters, 4))
    return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  KmParams P;
  P.x = x; P.w = w; P.c0 = c0; P.assign = assign; P.centers = centers; P.sse = sse; P.iters = iters;
  P.w_stride = w_row_stride; P.rows = rows; P.tol = tol;
  P.k = (int32_t)k; P.n2 = n2; P.C = C; P.S = S; P.max_iter = max_iter;
  return w ? go<true>(P, lds, (hipStream_t)stream) : go<false>(P, lds, (hipStream_t)stream);
}
