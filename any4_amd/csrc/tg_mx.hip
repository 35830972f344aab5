// tg_mx.hip -- tg_quant_mx8_rows / tg_gemm_mx4a8 (include/tinygemm_hip.h): the MXFP8 activation quantiser and the MX4 x MXFP8 GEMM on the
// block-scaled MFMA (w4a8_gemm_mx.cuh); see tg_common.cuh
#include <stddef.h>
#include "tg_common.cuh"
namespace {
#include "w4a8_gemm_mx.cuh"

constexpr int64_t kLim = (int64_t)1 << 31;   // operands are addressed with 32-bit byte offsets inside a row tile; refused beyond

// everything of a GEMM call that needs no device, in the order it is refused
int check_mx(const tg_mx_gemm* c, tg_mx_gemm& a) {
  if (!c) return TG_E_NULL;
  if (c->struct_bytes != sizeof(tg_mx_gemm)) return TG_E_STRUCT;
  a = *c;
  if (a.struct_reserved != 0 || a.reserved != 0) return TG_E_STRUCT;
  if (!a.x_codes || !a.x_exps || !a.w || !a.w_exps || !a.y) return TG_E_NULL;
  if (!aligned16(a.x_codes) || !aligned16(a.w) || ((uintptr_t)a.x_exps & 3) || ((uintptr_t)a.w_exps & 3) || ((uintptr_t)a.y & 7) ||
      ((uintptr_t)a.bias & 7))
    return TG_E_ALIGN;
  if (a.m <= 0 || a.wrows <= 0 || a.k <= 0 || a.m > INT32_MAX || a.wrows > INT32_MAX || a.k > INT32_MAX) return TG_E_SHAPE;
  if (a.k % 128 != 0) return TG_E_K_DIV;
  if (a.inner_k_tiles != 4) return TG_E_INNER_K;
  if (!(a.w_format == TG_WFMT_M16N8K16 || a.w_format == TG_WFMT_ROWS) || (a.w_on_right && a.w_format)) return TG_E_SHAPE;
  if (!a.w_on_right && a.w_format != TG_WFMT_ROWS) return TG_E_LAYOUT;   // the reference's Aint4 words: repack to the native format
  if (a.wrows % (a.w_on_right ? 8 : 16) != 0) return TG_E_SHAPE;         // whole tiles of the packed tensor
  if (a.m * a.k >= kLim || a.wrows * a.k / 2 >= kLim || a.m * a.wrows * 2 >= kLim) return TG_E_SIZE;
  return 0;
}
}  // namespace

extern "C" int tg_quant_mx8_rows(const void* x, int64_t m, int64_t k, void* codes, void* exps, int device, tg_stream_t stream) {
  if (!x || !codes || !exps) return TG_E_NULL;
  if (!aligned16(x) || !aligned16(codes)) return TG_E_ALIGN;
  if (m <= 0 || k <= 0 || m > INT32_MAX || k > INT32_MAX) return TG_E_SHAPE;
  if (k % 32 != 0) return TG_E_K_DIV;
  if (m * k * 2 >= kLim) return TG_E_SIZE;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  hipLaunchKernelGGL(mx8_rows_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (uint8_t*)codes, (uint8_t*)exps,
                     (int)m, (int)k);
  return launch_status();
}

extern "C" int tg_gemm_mx4a8(const tg_mx_gemm* args, int device, tg_stream_t stream) {
  tg_mx_gemm a;
  const int rc = check_mx(args, a);
  if (rc != 0) return rc;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  MxGemmParams p;
  p.xc = (const char*)a.x_codes; p.xe = (const char*)a.x_exps; p.w = (const char*)a.w; p.we = (const char*)a.w_exps;
  p.bias = (const char*)a.bias; p.y = (char*)a.y;
  p.m = (int32_t)a.m; p.wrows = (int32_t)a.wrows; p.k = (int32_t)a.k;
  p.tiles_m = (int32_t)cdiv(a.m, MX_BM); p.tiles_n = (int32_t)cdiv(a.wrows, MX_BN);
  return launch_lds_kernel<mx4a8_gemm_kernel>(dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(384), MX_LDS, (hipStream_t)stream, p, false);
}
