// w4a8_gemm_mx.cuh -- MX4 weights x MXFP8 activations on gfx950's block-scaled matrix instruction, and the activation quantiser in front of it.
//
//   Y[a][r] = RNE16( sum over 32-k blocks b of 2^(Ea[a][b] + Ew[r][b] - 254) * sum_{j < 32} fp8(xc[a][b][j]) * fp4(wc[r][b][j])  [+ bias] )
//
// v_mfma_scale_f32_16x16x128_f8f6f4 contracts 128 k per issue: lane (i = lane & 15, g = lane >> 4) brings 32 k of row i of each operand and ONE
// E8M0 byte per operand (a byte of a VGPR, picked by op_sel), which scales the 32 consecutive k 32 g ... 32 g + 31 -- one MX block.  The fp4
// operand's 32 k are that block; the fp8 operand's are two halves of two blocks (see "x tile").
//
//   weights    stay where an MX4Linear keeps them: Bint4 words of innerKTiles 4, [wrows / 8][k / 64][32][2] (tg_convert.cuh, pack_Bint4_kernel;
//              TG_WFMT_ROWS holds the same words), exponents [wrows][k / 32].  The 64 k of one weight row in a 64-k chunk are the eight words
//              of lanes 4 (r % 8) + q, q = 0 ... 3, two words each: 32 contiguous bytes (q0j0 q0j1 q1j0 q1j1 | q2j0 q2j1 q3j0 q3j1).  Word (q, j)
//              holds k = 32 j + 2 q + {0, 8, 16, 24, 1, 9, 17, 25} in nibbles 0 ... 7, so the even words are the hardware block of k 0 ... 31 and
//              the odd words that of k 32 ... 63 -- in a fixed order of their own: operand position p = 8 q + n holds k offset
//                  PI(p) = 2 (p / 8) + 8 (p % 4) + (p % 8) / 4.
//              A contraction does not care as long as the activation bytes sit in the same order, so mx8_rows_kernel WRITES its codes in that
//              order (any4_amd.utils.mx8_rows_ref is the layout's definition).  Picking the even / odd words is register selection: the inner
//              loop has no per-byte or per-nibble operation on either operand.  Global -> VGPR -> MFMA, no weight byte goes through LDS; the
//              loads of step s + 1 are issued before the products of step s (a register ring of two).
//   k step     MX_KS = 512, and lane group g owns k 128 g ... 128 g + 127 of it: its four blocks 4 g + c, c = 0 ... 3, are the four bytes of ONE
//              dword of the exponent row, and MFMA c of the step names byte c in op_sel for every lane alike.  (With a 128- or 256-k step the
//              byte would depend on the lane: a shift per exponent word.)  k % 128 == 0: in the last step whole lane groups may lie beyond k;
//              they contract zero weights with exponent 127 against bytes of a valid address (finite, or NaN in a row that is NaN anyway).
//   operands   the WEIGHTS are the A operand (cbsz = 4: fp4), the activations B (blgp = 0: fp8 e4m3): D[i = weight row][j = activation row]
//              puts four consecutive weight rows of one activation row into a lane's accumulator: one 8-byte store into y[m][wrows].
//   x tile     codes and exponent bytes global -> LDS by LDS-DMA (global_load_lds_dwordx4 / _dword, the tile GEMM's machinery) from two loader
//              waves, three stages (requested two steps ahead), shared by the four MFMA waves, which hold different weight rows.  A stage is
//              64 rows x 512 bytes.  The instruction's fp8 operand orders k differently from its fp4 operand (measured with one-hot weights: lane
//              group g holds k 16 g ... 16 g + 15 and 64 + 16 g ... 64 + 16 g + 15 of the 128, where the fp4 operand holds 32 g ... 32 g + 31; the
//              exponent of hardware block j is lane group j's for both), so a lane reads two 16-byte halves of two blocks of its row, one
//              ds_read_b128 each.  Bank arithmetic: a row is 32 16-byte units, and unit u of row r is stored at u ^ (r & 15) (on the DMA's source
//              address: the DMA writes lane-linear).  The 16 lanes of one g read rows i = 0 ... 15 at unit U ^ i for one U: sixteen different units
//              mod 16 = all 64 banks once per 16-lane group; unswizzled they would all start in the same bank.  Exponents: [g][row] dwords,
//              lane-linear, conflict-free.
//   tile       BM = 64 activation rows x BN = 256 weight rows, one workgroup per (m tile, n tile), k never split: a token's bits do not depend on
//              its batch.  Wave w of 0 ... 3 owns weight rows 64 w ... 64 w + 63 (four 16-row tiles) x the 64 activation rows: 16 accumulators =
//              64 VGPRs; the weight ring 2 x (4 tiles x 16 + 4 exponent words) = 136; fragments and addresses ~40: 1 wave per SIMD at <= 256.
//              LDS: 3 x (32 KiB + 1 KiB) = 99 KiB.  Per step a wave issues 64 MFMAs and reads 16 fragments x 2 KiB = 32 KiB of LDS: 2 MFMAs
//              (2 x 32768 products) per KiB read; the tile GEMM's bf16 MFMAs get 1 (of 8192 products) per KiB.
//   ragged     rows beyond m / wrows load a valid row again and are never stored.  Any m >= 1; tuned for m >= 64.  This kernel never splits k:
//              a 4096^2 layer at m = 512 is 128 workgroups, at m <= 64 it is 16.  Launches of 1 ... 64 rows have a kernel of their own,
//              mx4a8_rows_kernel (w4a8_rows_mx.cuh, tg_gemm_mx4a8_rows): 16-row tiles, k in windows, the partials summed in a fixed order.
//   NaN        an exponent byte of 255 is E8M0's NaN: the instruction's product is NaN for exactly that (weight row, activation row) pair's block,
//              so the row / column of the output is NaN and nothing else (tests/test_gpu_mx4a8.py holds it to that).
#pragma once
#include "kv8.cuh"

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct MxGemmParams {
  const char* xc;    // [m][k] E4M3 codes, each 32-block in PI order
  const char* xe;    // [m][k / 32] E8M0
  const char* w;     // Bint4 words, innerKTiles 4
  const char* we;    // [wrows][k / 32] E8M0
  const char* bias;  // optional [wrows] bf16
  char* y;           // [m][wrows] bf16
  int32_t m, wrows, k;
  int32_t tiles_m, tiles_n;
};

constexpr int MX_BM = 64, MX_BN = 256, MX_KS = 512;
constexpr int MX_DX = 2;                          // x of step u is requested MX_DX steps ahead
constexpr int MX_NST = MX_DX + 1;
constexpr int MX_CODES = MX_BM * MX_KS;           // bytes of a stage's codes
constexpr int MX_STAGE = MX_CODES + MX_BM * 16;   // ... and its exponent dwords [4][MX_BM]
constexpr int MX_LDS = MX_NST * MX_STAGE;
constexpr int MX_DMA = (MX_BM / 2 + 4) / 2;       // DMA instructions per loader wave and step: 16 of codes (two rows each), 2 of exponents
static_assert(MX_LDS <= 160 * 1024 && MX_DX * MX_DMA < 64, "LDS / vmcnt");

template <int N>
__device__ __forceinline__ void mx_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void mx_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// k offset inside its block of the element at operand position p (see above)
__host__ __device__ constexpr int mx_pi(int p) { return 2 * (p / 8) + 8 * (p % 4) + (p % 8) / 4; }

// ---- the activation quantiser: bf16 x [m][k] -> E4M3 codes [m][k] (PI order inside a block) and E8M0 exponents [m][k / 32] ----
// kvcache.mx8_encode's bytes (kv8.cuh's exponent rule and rounding).  One wave per row, a lane per 32-block (64 bytes in, the maximum in
// registers, 32 bytes out as two 16-byte stores); no LDS, no atomics.
__global__ void __launch_bounds__(256) mx8_rows_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ codes, uint8_t* __restrict__ exps,
                                                       int m, int k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const int nb = k >> 5;
  for (int b = lane; b < nb; b += 64) {
    const u32x4* src = reinterpret_cast<const u32x4*>(x + row * k + b * 32);
    float v[32];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32x4 t = src[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[8 * q + 2 * e] = BF16::lo_f32(t[e]);
        v[8 * q + 2 * e + 1] = BF16::hi_f32(t[e]);
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      float a = fabsf(v[j]);
      a = a < INFINITY ? a : INFINITY;  // (a NaN too: the block is marked, fmaxf would drop it)
      amax = fmaxf(amax, a);
    }
    uint32_t E;
    bool bad;
    const float s = mx8_block_scale(f2u(amax), E, bad);
    uint32_t c[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) c[j] = bad ? 0x7fu : mx8_e4m3_rne(fminf(fmaxf(v[j] * s, -448.f), 448.f));
    u32x4 o[2];
#pragma unroll
    for (int d = 0; d < 8; ++d)
      o[d >> 2][d & 3] = c[mx_pi(4 * d)] | (c[mx_pi(4 * d + 1)] << 8) | (c[mx_pi(4 * d + 2)] << 16) | (c[mx_pi(4 * d + 3)] << 24);
    u32x4* dst = reinterpret_cast<u32x4*>(codes + row * k + b * 32);
    dst[0] = o[0];
    dst[1] = o[1];
    exps[row * nb + b] = (uint8_t)E;
  }
}

// ---- the GEMM ----
struct MxWeights {      // a lane's weights of one k step: row i of each of its wave's four 16-row tiles, k 128 g ... 128 g + 127
  u32x4 q[4][2][2];     // [tile][64-k chunk][half of its 32 bytes]
  uint32_t e[4];        // [tile]: the four exponent bytes
};

__global__ void __launch_bounds__(384) mx4a8_gemm_kernel(const MxGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int tile;
  {  // consecutive tiles on ONE XCD (block b runs on XCD b % 8): the m tiles of a weight tile share its L2
    const int ntot = p.tiles_m * p.tiles_n, b = blockIdx.x, q = ntot >> 3, r = ntot & 7, xcd = b & 7, idx = b >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int tn = tile / p.tiles_m, tm = tile - tn * p.tiles_m;
  const int m0 = tm * MX_BM, n0 = tn * MX_BN;
  const int ksteps = (p.k + MX_KS - 1) / MX_KS, last = ksteps - 1;
  const int nb = p.k >> 5;

  if (wave >= 4) {
    // =================================== loader waves: LDS-DMA only ===================================
    const int lw = wave - 4;
    const int er = m0 + lane < p.m ? m0 + lane : p.m - 1;   // (rows beyond m: a valid row, never stored)
    auto dma = [&](int step) {                              // (past the end: the last step again, into a stage nobody reads)
      const int c = step < last ? step : last;
      char* st = lds + (step % MX_NST) * MX_STAGE;
#pragma unroll
      for (int n = 0; n < MX_BM / 4; ++n) {                 // instruction = rows 2 j, 2 j + 1 of the stage: 64 units of 16 bytes, lane-linear
        const int j = lw * (MX_BM / 4) + n;
        const int row = 2 * j + (lane >> 5);
        const int mr = m0 + row < p.m ? m0 + row : p.m - 1;
        int koff = c * MX_KS + (((lane & 31) ^ (row & 15)) << 4);
        koff = koff < p.k ? koff : 0;                       // (units beyond k: a valid address; their lane group contracts zero weights)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.xc + (int64_t)mr * p.k + koff),
                                         (__attribute__((address_space(3))) void*)(st + j * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int n = 0; n < 2; ++n) {                         // instruction = exponent dword g of the 64 rows
        const int g = lw * 2 + n;
        int boff = c * (MX_KS / 32) + 4 * g;
        boff = boff < nb ? boff : 0;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.xe + (int64_t)er * nb + boff),
                                         (__attribute__((address_space(3))) void*)(st + MX_CODES + g * 256), 4, 0, 0);
      }
    };
#pragma unroll
    for (int t = 0; t < MX_DX; ++t) dma(t);
    mx_wait_vm<0>();
    mx_barrier();
    for (int s = 0; s < ksteps; ++s) {
      dma(s + MX_DX);
      mx_wait_vm<(MX_DX - 1) * MX_DMA>();
      mx_barrier();
    }
    mx_wait_vm<0>();
    return;
  }

  // =================================== MFMA waves ===================================
  const int fi = lane & 15, g = lane >> 4;
  const char* wsrc[4];
  const char* esrc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int r = n0 + wave * 64 + t * 16 + fi;
    r = r < p.wrows ? r : p.wrows - 1;                      // (rows beyond wrows: a valid row, never stored)
    wsrc[t] = p.w + ((int64_t)(r >> 3) * (p.k >> 6)) * 256 + (r & 7) * 32;
    esrc[t] = p.we + (int64_t)r * nb;
  }
  auto load_w = [&](int step, MxWeights& d) {
    const int c = step < last ? step : last;
    const int k0 = c * MX_KS + 128 * g;
    const bool live = k0 < p.k;
    const int ks = live ? k0 >> 6 : 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const u32x4 q = *reinterpret_cast<const u32x4*>(wsrc[t] + (int64_t)(ks + h) * 256 + v * 16);
          d.q[t][h][v] = live ? q : u32x4{0u, 0u, 0u, 0u};
        }
      const uint32_t e = *reinterpret_cast<const uint32_t*>(esrc[t] + (live ? k0 >> 5 : 0));
      d.e[t] = live ? e : 0x7f7f7f7fu;
    }
  };
  // this lane's fragment addresses in a stage: row 16 a + fi, units (8 g + 2 c + h) ^ fi; exponent dword [g][16 a + fi]
  const uint32_t x_row = (uint32_t)(fi * MX_KS), e_off = (uint32_t)(MX_CODES + g * 256 + fi * 4);
  f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mma = [&](int step, const MxWeights& wq) {
    const char* st = lds + (step % MX_NST) * MX_STAGE;
    uint32_t xe[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xe[a] = *reinterpret_cast<const uint32_t*>(st + e_off + a * 64);
    auto block = [&](auto C_) {   // MFMA c of the step: block 4 g + c of every row, byte c of the exponent words (op_sel is an immediate)
      constexpr int c = decltype(C_)::value;
      // the fp8 operand's k order is not the fp4 one's: lane group g brings k 16 g ... 16 g + 15 (registers 0-3) and 64 + 16 g ... (registers 4-7) of
      // the MFMA's 128, i.e. half g & 1 of the hardware blocks g >> 1 and 2 + (g >> 1) = of this step's blocks 4 (g >> 1) + c and 8 + 4 (g >> 1) + c
      const uint32_t u0 = x_row + ((uint32_t)((8 * (g >> 1) + 2 * c + (g & 1)) ^ fi) << 4), u1 = x_row + ((uint32_t)((16 + 8 * (g >> 1) + 2 * c + (g & 1)) ^ fi) << 4);
      i32x8 wf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {   // c = 2 h + j: the words j, 2 + j of both halves of chunk h
        const u32x4 &lo = wq.q[t][c >> 1][0], &hi = wq.q[t][c >> 1][1];
        wf[t] = i32x8{(int)lo[c & 1], (int)lo[2 + (c & 1)], (int)hi[c & 1], (int)hi[2 + (c & 1)], 0, 0, 0, 0};
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const u32x4 x0 = *reinterpret_cast<const u32x4*>(st + u0 + a * (16 * MX_KS)), x1 = *reinterpret_cast<const u32x4*>(st + u1 + a * (16 * MX_KS));
        const i32x8 xf = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[t][a] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[t], xf, acc[t][a], 4 /* A: fp4 */, 0 /* B: fp8 e4m3 */, c, (int)wq.e[t], c, (int)xe[a]);
      }
    };
    block(std::integral_constant<int, 0>{});
    block(std::integral_constant<int, 1>{});
    block(std::integral_constant<int, 2>{});
    block(std::integral_constant<int, 3>{});
  };

  MxWeights ring[2];
  load_w(0, ring[0]);
  mx_barrier();
  for (int s = 0; s < ksteps; s += 2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (s + j >= ksteps) break;
      load_w(s + j + 1, ring[(j + 1) & 1]);
      mma(s + j, ring[j]);
      mx_barrier();
    }
  }

  // ---- store: lane (activation row fi of tile a, weight rows 4 g ... 4 g + 3 of tile t) ----
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int mr = m0 + a * 16 + fi;
    if (mr >= p.m) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int nr = n0 + wave * 64 + t * 16 + 4 * g;
      if (nr >= p.wrows) continue;   // (wrows is a multiple of 8: a group of four rows is inside or outside)
      store_rows4<BF16>(p.y, p.bias, (int64_t)mr * p.wrows + nr, nr, acc[t][a]);
    }
  }
}
