// tg_splitk.hip -- launch path of w4_gemm_kernel (reference numerics, small launches); see tg_common.cuh
#include "tg_common.cuh"
namespace {
#include "w4_gemm.cuh"
template <typename DT, bool LAYOUT_A, int CANON, bool QMX>
int go(const GemmParams& p, int waves, int splitk) {
  const int tpb = waves / splitk;
  const dim3 grid((unsigned)((p.rowtiles + tpb - 1) / tpb), (unsigned)coltiles(p), (unsigned)p.batch);
  const SplitKParams kp = splitk_params(p, splitk);
  if (waves == 16) hipLaunchKernelGGL((w4_gemm_kernel<DT, LAYOUT_A, CANON, QMX, 16, 2, 4>), grid, dim3(16 * 64), 0, p.st, kp);
  else hipLaunchKernelGGL((w4_gemm_kernel<DT, LAYOUT_A, CANON, QMX, 8, 2, 4>), grid, dim3(8 * 64), 0, p.st, kp);
  return launch_status();
}
template <typename DT, bool LAYOUT_A, int CANON>
int go_q(const GemmParams& p, int waves, int splitk) {
  if constexpr (!std::is_same<DT, BF16>::value) {
    if (p.qmx) return TG_E_DTYPE;
    return go<DT, LAYOUT_A, CANON, false>(p, waves, splitk);
  } else {
    return p.qmx ? go<DT, LAYOUT_A, CANON, true>(p, waves, splitk) : go<DT, LAYOUT_A, CANON, false>(p, waves, splitk);
  }
}
template <typename DT, bool LAYOUT_A>
int go_c(const GemmParams& p, int waves, int splitk) {
  switch (words_per_lane(p)) {  // (the in-register transpose of the packed words)
    case 1: return go_q<DT, LAYOUT_A, CANON_NONE>(p, waves, splitk);
    case 2: return go_q<DT, LAYOUT_A, CANON_PAIR>(p, waves, splitk);
    default: return go_q<DT, LAYOUT_A, CANON_QUAD>(p, waves, splitk);
  }
}
}  // namespace
int tgx::splitk(const GemmParams& p, int waves, int splitk) {
  return pick_dt(p.dt, [&](auto DT_) {
    return !p.on_right ? go_c<decltype(DT_), true>(p, waves, splitk) : go_c<decltype(DT_), false>(p, waves, splitk);
  });
}
