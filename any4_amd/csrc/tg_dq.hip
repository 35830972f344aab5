// tg_dq.hip -- launch path of w4_gemm_dq_kernel and dq_finish_kernel (the gradients of scales, zeros and LUT of a 4-bit linear;
// w4_gemm_dq.cuh); see tg_common.cuh
#include "tg_common.cuh"
namespace {
#include "w4_gemm_dq.cuh"
}  // namespace

namespace tgx {
// Bint4 words (innerKTiles 2 / 4 / 8; also the native weights-on-the-left words), row-major x / dY, one problem, int4 / any4.  The caller
// (tinygemm_hip.hip, gemm_dq_impl) has validated everything, the size of the workspace included.  p.dry: report the workspace in p.ws_need,
// launch nothing.  Workspace: H (or its halves per group of 256) [k / min(g, 128)][wrows][16] f32, then -- global LUT -- the per-row
// table gradients [wrows][16] f32 that dq_rowsum_kernel folds.
// No split over m: a launch has ceil(wrows / 128) * ceil(k / 128) workgroups (4096^2: 1024), so a small layer leaves compute units idle.
int gemm_dq(GemmParams& p, const char* dy, float* d_qinfo, float* d_lut) {
  const int ushift = p.gshift < 7 ? p.gshift : 7;
  const int64_t hp_bytes = (int64_t)(p.k >> ushift) * p.wrows * 16 * 4;
  const int64_t rows_bytes = p.qtype == TG_Q_ANY4_GLOBAL ? (int64_t)p.wrows * 16 * 4 : 0;
  p.ws_need = hp_bytes + rows_bytes;
  if (p.dry) return 0;
  DqParams dp;
  dp.x = p.x; dp.dy = dy; dp.w = p.w; dp.hp = reinterpret_cast<float*>(p.ws);
  dp.m = p.m; dp.wrows = p.wrows; dp.k = p.k; dp.ksuper = p.ksuper; dp.inner = p.inner; dp.ushift = ushift;
  dp.tiles_r = (int32_t)cdiv(p.wrows, DQ_BR);
  dp.tiles_k = (int32_t)cdiv(p.k, DQ_BK);
  const dim3 grid((unsigned)((int64_t)dp.tiles_r * dp.tiles_k));
  int rc = pick_dt(p.dt, [&](auto DT_) { return launch_lds_kernel<w4_gemm_dq_kernel<decltype(DT_)>>(grid, dim3(256), DqLds::BYTES, p.st, dp, false); });
  if (rc != 0) return rc;
  const bool global = p.qtype == TG_Q_ANY4_GLOBAL, want_lut = d_lut && p.qtype != TG_Q_INT4;
  DqFinishParams fp;
  fp.hp = dp.hp; fp.qinfo = p.qinfo; fp.lut = p.lut; fp.d_qinfo = d_qinfo;
  fp.d_lut_rows = !want_lut ? nullptr : global ? reinterpret_cast<float*>(p.ws + hp_bytes) : d_lut;
  fp.wrows = p.wrows; fp.ngroups = p.ngroups; fp.upg = p.gshift > 7 ? 2 : 1; fp.qtype = p.qtype;
  rc = pick_dt(p.dt, [&](auto DT_) {
    hipLaunchKernelGGL(dq_finish_kernel<decltype(DT_)>, dim3((unsigned)cdiv((int64_t)p.wrows * 4, 256)), dim3(256), 0, p.st, fp);
    return launch_status();
  });
  if (rc != 0 || !(want_lut && global)) return rc;
  hipLaunchKernelGGL(dq_rowsum_kernel, dim3(1), dim3(256), 0, p.st, fp.d_lut_rows, (int)p.wrows, d_lut);
  return launch_status();
}
}  // namespace tgx
