// w4a8_rows_mx.cuh -- MX4 weights x MXFP8 activations at 1 ... 64 activation rows: a weight-streaming kernel on the block-scaled matrix
// instruction.  Operands, definition and contract are w4a8_gemm_mx.cuh's (same x codes in PI order, same packed words, same exponents,
// same RNE16(sum) [then RNE16(. + bias)], same NaN rule); what differs is the split of the work, for launches in which one 64 x 256 tile
// per workgroup leaves most of the chip idle (a 4096^2 layer is 16 such tiles).
//
//   unit      one 16-weight-row tile (the MFMA's A operand, cbsz = 4) x one block of up to 16 activation rows (B, fp8) x one WINDOW of
//             k: RW_WIN = 4096 = 4 waves x 2 steps of MX_KS = 512.  A workgroup is four waves, wave w takes the steps w and w + 4 of the
//             window; lane group g the k 128 g ... 128 g + 127 of a step (its four blocks are the four bytes of one exponent dword: op_sel
//             names the byte for all lanes alike, as in the tile kernel).  A wave without a step (k = 128: three of them) issues nothing.
//   x         RESIDENT IN REGISTERS: a wave's two steps of its activation block are loaded once, straight from global (x is small and
//             L2-resident): per step and MFMA two 16-byte halves (the fp8 operand's k order, w4a8_gemm_mx.cuh "x tile"), plus one exponent
//             dword per step: 2 x (4 x 8 + 1) = 66 registers, kept across every row tile the workgroup walks.  No LDS staging, no barrier
//             for x.  Rows j >= m of the block read row m - 1 again and are never stored; lane groups beyond k read unit 0 of their row and
//             are replaced by ZEROS with exponent 127: no address outside x is formed, and no load sits behind a branch of its own.
//   weights   global -> VGPR -> MFMA in the word order the tile kernel documents; a wave requests all 2 x (4 x 16 bytes + 1 exponent
//             dword) of a row tile before the tile's first product, and, where the workgroup walks several tiles, the NEXT tile's loads
//             before the current tile's products (a register ring of two: 2 x 34 registers).
//   sums      a wave's two steps go to two accumulators (two chains of four MFMAs, not one of eight) added once: step w + (step w + 4).
//             The four waves meet through LDS behind ONE barrier per tile (two LDS slots, by tile parity: a slot is rewritten two barriers
//             after it was read) and wave 0 sums ((w0 + w1) + w2) + w3.  k <= RW_WIN: that sum is rounded and stored.  Longer k: the
//             windows are separate workgroups (grid z); wave 0 writes the f32 partial of its window to the caller's workspace with
//             agent-scope stores, drains them (vmcnt(0)), counts the unit in; the last window to arrive adds the partials IN WINDOW ORDER,
//             rounds once, stores, and leaves the counter at zero: a captured launch replays (rope_attn_split_kernel's arrangement,
//             decode_glue.cuh, which says why there is no device-scope fence).  No float atomics.  How k is cut (steps, waves, windows) is a
//             function of k alone: a row's bits depend neither on m, nor on wrows, nor on the device.
//   grid      (gx rounded up to 8 x activation blocks, 1, windows).  Row tiles are dealt evenly: T = ceil(tiles / RW_GRID) tiles per workgroup,
//             gx = ceil(tiles / T) workgroups per activation block, workgroup `first` walks the tiles first, first + gx, ...: two each at
//             wrows = 14336, one at 4096.  Walking is what pays for x: a workgroup's slice of x (16 rows x 4096 bytes) is TWICE a tile's weights,
//             and at one tile per workgroup x, not the weights, is most of what the launch reads from L2.  Activation blocks 2 ... 4
//             (m = 17 ... 64) re-read the weights, as the 16-row W4A16 kernels do at those rows; the blocks of one tile are consecutive
//             workgroups of one XCD (see the kernel), so the re-reads are L2 hits.  m > 64 is the tile kernel's ground (refused by the launcher).
//   workspace [activation block][row tile] int32 counters (zero between launches), padded to 256 bytes, then
//             [activation block][row tile][window][64 lanes][4] f32 partials.  None when k <= RW_WIN.
#pragma once
#include "w4a8_gemm_mx.cuh"

struct MxRowsParams {
  const char* xc;    // as MxGemmParams
  const char* xe;
  const char* w;
  const char* we;
  const char* bias;
  char* y;
  float* part;       // nwin > 1: the partials ...
  int* counters;     // ... and the counters of the workspace
  int32_t m, wrows, k;
  int32_t tiles;     // ceil(wrows / 16)
  int32_t nwin;      // ceil(k / RW_WIN)
  int32_t mblocks;   // ceil(m / 16)
  int32_t gx;        // workgroups that share the row tiles of one activation block: ceil(tiles / ceil(tiles / RW_GRID))
};

constexpr int RW_WAVES = 4, RW_SLOTS = 2;                 // waves of a workgroup; steps of a window per wave
constexpr int RW_WIN = RW_WAVES * RW_SLOTS * MX_KS;       // k of a window
constexpr int RW_GRID = 512;                              // workgroups per activation block of a full grid: what a 256-CU part holds at once (two per CU at 182 registers)
constexpr int RW_UNIT = 64 * 4;                           // f32 of a unit's partial

struct RwWeights {             // a lane's weights of one row tile: row i, k 128 g ... 128 g + 127 of both steps of its wave
  u32x4 q[RW_SLOTS][2][2];     // [step][64-k chunk][half of its 32 bytes]
  uint32_t e[RW_SLOTS];        // [step]: the four exponent bytes
};

// wave 0, after the workgroup's sum: lane (activation row fi of block mb, weight rows 4 g ... 4 g + 3 of the tile)
__device__ __forceinline__ void rows_finish(const MxRowsParams& p, int mb, int tile, f32x4 acc) {
  const int lane = threadIdx.x & 63, fi = lane & 15, g = lane >> 4;
  const int win = blockIdx.z;
  const int mr = mb * 16 + fi, nr = tile * 16 + 4 * g;
  const bool live = mr < p.m && nr < p.wrows;             // (wrows is a multiple of 8: a group of four rows is inside or outside)
  const int64_t elem = (int64_t)mr * p.wrows + nr;
  if (p.nwin == 1) {                                      // (uniform over the launch)
    if (live) store_rows4<BF16>(p.y, p.bias, elem, nr, acc);
    return;
  }
  const int64_t unit = (int64_t)mb * p.tiles + tile;
  float* mine = p.part + unit * p.nwin * RW_UNIT + lane * 4;
  if (live) {
#pragma unroll
    for (int e = 0; e < 4; ++e) __hip_atomic_store(mine + win * RW_UNIT + e, acc[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  mx_wait_vm<0>();                                        // this wave's partial is complete before lane 0 counts the window in
  int last = 0;
  if (lane == 0) last = __hip_atomic_fetch_add(p.counters + unit, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.nwin - 1;
  if (!__builtin_amdgcn_readfirstlane(last)) return;
  if (live) {
    f32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = __hip_atomic_load(mine + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int w = 1; w < p.nwin; ++w)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += __hip_atomic_load(mine + w * RW_UNIT + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    store_rows4<BF16>(p.y, p.bias, elem, nr, s);
  }
  if (lane == 0) __hip_atomic_store(p.counters + unit, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch / graph replay
}

// A wave with NS of its two steps inside k (wave-uniform; a wave's live steps are a prefix).  One copy of the body per NS and a peeled
// last tile, so that NO load sits behind a branch: the compiler's vmcnt waits then count the loads in flight exactly, and a tile's products
// wait for that tile's weights with the next tile's still on their way.
template <int NS>
__device__ __forceinline__ void rows_body(const MxRowsParams& p, int mb, int first, f32x4 (*red)[RW_WAVES - 1][64]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fi = lane & 15, g = lane >> 4;
  const int nb = p.k >> 5;
  const int ks0 = blockIdx.z * RW_WIN + wave * MX_KS;     // this wave's steps begin at ks0 and ks0 + RW_WAVES MX_KS
  bool wl[RW_SLOTS];                                      // this lane group's 128 k of step j are inside k
#pragma unroll
  for (int j = 0; j < RW_SLOTS; ++j) wl[j] = ks0 + j * (RW_WAVES * MX_KS) + 128 * g < p.k;

  // a row tile's weights, as they are.  A lane group beyond k reads the words of k = 0; its exponent becomes 127 at the product and its
  // activations are zeros, so are its products.
  auto load_w = [&](int tile, RwWeights& d) {
    int r = tile * 16 + fi;
    r = r < p.wrows ? r : p.wrows - 1;                    // (rows beyond wrows: a valid row, never stored)
    const char* ws = p.w + ((int64_t)(r >> 3) * (p.k >> 6)) * 256 + (r & 7) * 32;
    const char* es = p.we + (int64_t)r * nb;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int kk = wl[j] ? ks0 + j * (RW_WAVES * MX_KS) + 128 * g : 0;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int v = 0; v < 2; ++v) d.q[j][h][v] = *reinterpret_cast<const u32x4*>(ws + (int64_t)((kk >> 6) + h) * 256 + v * 16);
      d.e[j] = *reinterpret_cast<const uint32_t*>(es + (kk >> 5));
    }
  };

  const int stride = p.gx;
  RwWeights ring[2];
  load_w(first, ring[0]);                            // (the long way, from HBM: requested first)

  // ---- the activation block's slice of this wave: loaded once.  Every load is on an address inside x (a row beyond m: row m - 1 again; a
  // unit beyond k: unit 0); what must not count becomes zeros / exponent 127 once all are requested. ----
  const int mr = mb * 16 + fi;
  const char* xrp = p.xc + (int64_t)(mr < p.m ? mr : p.m - 1) * p.k;
  const char* xep = p.xe + (int64_t)(mr < p.m ? mr : p.m - 1) * nb;
  u32x4 xr[RW_SLOTS][4][2];
  i32x8 xf[RW_SLOTS][4];
  uint32_t xe[RW_SLOTS];
  // the fp8 operand of lane group g: half g & 1 of the hardware blocks g >> 1 and 2 + (g >> 1) = the step's blocks 4 (g >> 1) + c and 8 + 4 (g >> 1) + c
  auto x_off = [&](int j, int c, int h) { return ks0 + j * (RW_WAVES * MX_KS) + 16 * (8 * (g >> 1) + 2 * c + (g & 1)) + 256 * h; };
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    xe[j] = *reinterpret_cast<const uint32_t*>(xep + ((wl[j] ? ks0 + j * (RW_WAVES * MX_KS) + 128 * g : 0) >> 5));
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) xr[j][c][h] = *reinterpret_cast<const u32x4*>(xrp + (x_off(j, c, h) < p.k ? x_off(j, c, h) : 0));
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    xe[j] = wl[j] ? xe[j] : 0x7f7f7f7fu;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const u32x4 x0 = x_off(j, c, 0) < p.k ? xr[j][c][0] : u32x4{0u, 0u, 0u, 0u}, x1 = x_off(j, c, 1) < p.k ? xr[j][c][1] : u32x4{0u, 0u, 0u, 0u};
      xf[j][c] = i32x8{(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
    }
  }

  // one row tile: the products of this wave's steps (a chain of four MFMAs each), the workgroup's sum behind one barrier, wave 0 stores
  auto tile_sum = [&](int t, const RwWeights& wq, int u) {
    f32x4 a[RW_SLOTS] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    auto block = [&](auto J_, auto C_) {   // MFMA c of step j: block 4 g + c of the step, byte c of the exponent words; c = 2 h + v: the words v, 2 + v of both halves of chunk h
      constexpr int j = decltype(J_)::value, c = decltype(C_)::value;
      if constexpr (j < NS) {
        const u32x4 &lo = wq.q[j][c >> 1][0], &hi = wq.q[j][c >> 1][1];
        const i32x8 wf = {(int)lo[c & 1], (int)lo[2 + (c & 1)], (int)hi[c & 1], (int)hi[2 + (c & 1)], 0, 0, 0, 0};
        a[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, xf[j][c], a[j], 4 /* A: fp4 */, 0 /* B: fp8 e4m3 */, c,
                                                                (int)(wl[j] ? wq.e[j] : 0x7f7f7f7fu), c, (int)xe[j]);
      }
    };
    auto both = [&](auto C_) { block(std::integral_constant<int, 0>{}, C_); block(std::integral_constant<int, 1>{}, C_); };
    both(std::integral_constant<int, 0>{});
    both(std::integral_constant<int, 1>{});
    both(std::integral_constant<int, 2>{});
    both(std::integral_constant<int, 3>{});
    f32x4 acc = a[0] + a[1];
    if (wave) red[u][wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0) {
      acc = ((acc + red[u][0][lane]) + red[u][1][lane]) + red[u][2][lane];
      rows_finish(p, mb, t, acc);
    }
  };

  int t = first;
  for (; t + 2 * stride < p.tiles; t += 2 * stride) {     // both tiles of a round have a successor
    load_w(t + stride, ring[1]);
    tile_sum(t, ring[0], 0);
    load_w(t + 2 * stride, ring[0]);
    tile_sum(t + stride, ring[1], 1);
  }
  if (t + stride < p.tiles) {                             // two tiles left, or one
    load_w(t + stride, ring[1]);
    tile_sum(t, ring[0], 0);
    tile_sum(t + stride, ring[1], 1);
  } else {
    tile_sum(t, ring[0], 0);
  }
}

__global__ void __launch_bounds__(256) mx4a8_rows_kernel(const MxRowsParams p) {
  __shared__ f32x4 red[2][RW_WAVES - 1][64];
  // workgroup b runs on XCD b % 8: the activation blocks of one row tile are CONSECUTIVE workgroups of ONE XCD (b, b + 8, ...), so that blocks
  // 2 ... 4 find the tile's weights in that XCD's L2
  const int b = blockIdx.x, mb = (b >> 3) % p.mblocks, first = (b / (8 * p.mblocks)) * 8 + (b & 7);
  if (first >= p.gx) return;                              // (the whole workgroup: gx is rounded up to 8 in the grid)
  // The waves of a workgroup may take DIFFERENT copies of the body and meet at barriers that sit at different program points: s_barrier counts
  // arrivals, and every copy makes the same number of tile_sum calls (one per tile walked, whatever NS).  A copy whose tile count depended
  // on NS would hang the workgroup.
  const int ks0 = blockIdx.z * RW_WIN + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * MX_KS;
  if (ks0 + RW_WAVES * MX_KS < p.k) rows_body<2>(p, mb, first, red);
  else if (ks0 < p.k) rows_body<1>(p, mb, first, red);
  else rows_body<0>(p, mb, first, red);                   // (a wave beyond k: zeros into the sum, the barriers)
}
