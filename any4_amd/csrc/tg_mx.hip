// tg_mx.hip -- tg_quant_mx8_rows / tg_gemm_mx4a8 / tg_gemm_mx4a8_rows (include/tinygemm_hip.h): the MXFP8 activation quantiser and the two
// MX4 x MXFP8 GEMMs on the block-scaled MFMA (w4a8_gemm_mx.cuh: 64 x 256 tiles; w4a8_rows_mx.cuh: 1 ... 64 activation rows); see tg_common.cuh
#include <stddef.h>
#include "tg_common.cuh"
namespace {
#include "w4a8_gemm_mx.cuh"
#include "w4a8_rows_mx.cuh"

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

// The rows kernel's grid and workspace: a function of the shape alone (no device).
struct RowsPlan {
  int64_t tiles, mblocks, nwin, gx, counter_bytes, ws_bytes;
};
int plan_rows(int64_t m, int64_t wrows, int64_t k, RowsPlan& r) {
  if (m <= 0 || wrows <= 0 || k <= 0 || m > INT32_MAX || wrows > INT32_MAX || k > INT32_MAX) return TG_E_SHAPE;
  if (k % 128 != 0) return TG_E_K_DIV;
  if (m > 64 || wrows % 8 != 0) return TG_E_SHAPE;   // 65 rows and more: the tile kernel (tg_gemm_mx4a8)
  r.tiles = cdiv(wrows, 16); r.mblocks = cdiv(m, 16); r.nwin = cdiv(k, RW_WIN);
  if (r.nwin > 65535) return TG_E_SIZE;              // (the windows are grid z)
  r.gx = cdiv(r.tiles, cdiv(r.tiles, RW_GRID));   // every workgroup walks ceil(tiles / RW_GRID) row tiles (the last ones one fewer)
  r.counter_bytes = r.nwin > 1 ? cdiv(r.mblocks * r.tiles * 4, 256) * 256 : 0;
  r.ws_bytes = r.nwin > 1 ? r.counter_bytes + r.mblocks * r.tiles * r.nwin * RW_UNIT * 4 : 0;
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

extern "C" int tg_gemm_mx4a8_rows_plan(int64_t m, int64_t wrows, int64_t k, int64_t* out) {
  if (!out) return TG_E_NULL;
  RowsPlan r;
  const int rc = plan_rows(m, wrows, k, r);
  if (rc != 0) return rc;
  out[0] = r.gx; out[1] = r.mblocks; out[2] = r.nwin; out[3] = RW_WIN;
  return 0;
}

extern "C" int64_t tg_gemm_mx4a8_rows_workspace_bytes(int64_t m, int64_t wrows, int64_t k) {
  RowsPlan r;
  const int rc = plan_rows(m, wrows, k, r);
  return rc != 0 ? rc : r.ws_bytes;
}

extern "C" int tg_gemm_mx4a8_rows(const tg_mx_gemm* args, void* workspace, int64_t workspace_bytes, int device, tg_stream_t stream) {
  tg_mx_gemm a;
  int rc = check_mx(args, a);
  if (rc != 0) return rc;
  RowsPlan r;
  rc = plan_rows(a.m, a.wrows, a.k, r);
  if (rc != 0) return rc;
  if (r.ws_bytes > 0) {
    if (!workspace) return TG_E_NULL;
    if (!aligned16(workspace) || workspace_bytes < 0) return TG_E_ALIGN;
    if (workspace_bytes < r.ws_bytes) return TG_E_SHAPE;
  }
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  MxRowsParams p;
  p.xc = (const char*)a.x_codes; p.xe = (const char*)a.x_exps; p.w = (const char*)a.w; p.we = (const char*)a.w_exps;
  p.bias = (const char*)a.bias; p.y = (char*)a.y;
  p.counters = r.ws_bytes > 0 ? (int*)workspace : nullptr;
  p.part = r.ws_bytes > 0 ? (float*)((char*)workspace + r.counter_bytes) : nullptr;
  p.m = (int32_t)a.m; p.wrows = (int32_t)a.wrows; p.k = (int32_t)a.k;
  p.tiles = (int32_t)r.tiles; p.nwin = (int32_t)r.nwin; p.mblocks = (int32_t)r.mblocks; p.gx = (int32_t)r.gx;
  hipLaunchKernelGGL(mx4a8_rows_kernel, dim3((unsigned)(cdiv(r.gx, 8) * 8 * r.mblocks), 1, (unsigned)r.nwin), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status();
}
