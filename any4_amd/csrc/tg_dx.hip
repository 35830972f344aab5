// tg_dx.hip -- launch path of w4_gemm_dx_kernel (the input gradient dX = dY . W of a 4-bit linear; w4_gemm_dx.cuh); see tg_common.cuh
#include "tg_common.cuh"
namespace {
#include "w4_gemm_dx.cuh"

// CUs the split is sized for.  A constant, not the device's count: tg_gemm_w4_dx_workspace_bytes needs no GPU, and the split (so the
// summation order, so the bits) of a problem is the same on every device.
constexpr int kDxCUs = 256;

template <typename DT, int BM, bool QMX>
int go(const DxParams& dp, hipStream_t st) {
  const int ns = dp.splits > 1 ? dp.splits : 1;
  const int rc = launch_lds_kernel<w4_gemm_dx_kernel<DT, BM, QMX>>(dim3((unsigned)((int64_t)dp.tiles_m * dp.tiles_k * ns)), dim3(256), DxLds<BM>::BYTES, st, dp, false);
  if (rc != 0 || ns == 1) return rc;
  const int64_t quads = (int64_t)dp.m * dp.k / 4;
  hipLaunchKernelGGL(dx_split_sum_kernel<DT>, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, dp.part, ns, (int64_t)dp.m * dp.k, dp.dx, quads);
  return launch_status();
}
template <typename DT, bool QMX>
int go_bm(const DxParams& dp, int bm, hipStream_t st) {
  if (bm == 32) return go<DT, 32, QMX>(dp, st);
  if (bm == 64) return go<DT, 64, QMX>(dp, st);
  return go<DT, 128, QMX>(dp, st);
}
}  // namespace

namespace tgx {
// Bint4 words (innerKTiles 2 / 4 / 8; also the native weights-on-the-left words), row-major dY / dX, one problem.  The caller
// (tinygemm_hip.hip, gemm_dx_impl) has validated everything.  p.dry: report the workspace of the split in p.ws_need, launch nothing.
//
// Split over the weight rows: a tile's steps are a chain of dependent LDS round trips, so a launch with fewer tiles than CUs leaves the
// chip idle for as long as a full one takes.  With the caller's workspace the row steps are cut into 2 ... 16 splits (as many as keep
// tiles x splits <= 256 and at least four 64-row steps per split); without one the launch runs unsplit (slower, same contract as tg_gemm_w8).
int gemm_dx(GemmParams& p) {
  const int bm = p.m <= 32 ? 32 : p.m <= 64 ? 64 : 128;
  DxParams dp;
  dp.dy = p.x; dp.w = p.w; dp.qinfo = p.qinfo; dp.lut = p.lut; dp.dx = p.y;
  dp.m = p.m; dp.wrows = p.wrows; dp.k = p.k; dp.ksuper = p.ksuper; dp.inner = p.inner; dp.gshift = p.gshift; dp.qtype = p.qtype;
  dp.tiles_m = (int32_t)cdiv(p.m, bm);
  dp.tiles_k = (int32_t)cdiv(p.k, DX_BK);
  const int nsteps = (int)cdiv(p.wrows, DX_BR);
  const int64_t tiles = (int64_t)dp.tiles_m * dp.tiles_k;
  int splits = 1;
  while (splits < 16 && tiles * splits * 2 <= kDxCUs && nsteps >= splits * 2 * 4) splits *= 2;
  const int64_t need = splits > 1 ? (int64_t)splits * p.m * p.k * 4 : 0;
  if (!has_workspace(p, need)) splits = 1;
  p.ws_need = splits > 1 ? need : 0;
  if (p.dry) return 0;
  dp.splits = splits;
  dp.sps = (nsteps + splits - 1) / splits;
  dp.part = splits > 1 ? reinterpret_cast<float*>(p.ws) : nullptr;
  if (p.qmx) return go_bm<BF16, true>(dp, bm, p.st);
  return pick_dt(p.dt, [&](auto DT_) { return go_bm<decltype(DT_), false>(dp, bm, p.st); });
}
}  // namespace tgx
