// w4_gemm_dx.cuh -- the INPUT GRADIENT of a 4-bit linear (the backward of y = x . W^T with respect to x):
//
//   dX[a][j] = RNE16( sum_r dY[a][r] * w[r][j] ),   w[r][j] = RNE16(fma(lut[r][code], scale[g][r], zero[g][r]))   (int4: lut = code - 8;
//   mx4: fp4[code] * 2^(e - 127), e = 255: NaN)
//
// w is the reference's dequantised weight exactly as w4_gemm_tile_kernel and tg_dequant_w4 compute it (MatrixLayoutB.cuh:1042-1046), the
// products are summed in f32 by v_mfma_f32_16x16x32_{bf16,f16} and the result is rounded once.  The contraction runs over the WEIGHT ROWS,
// so none of the forward kernels can compute it: their packed words are walked along k.  Weights are Bint4 words (innerKTiles 2 / 4 / 8),
// which is also the native weights-on-the-left format (TG_WFMT_ROWS: the same words for the rows padded to 16).
//
//   tile       BM = 32 / 64 / 128 rows of dY x BK = 128 columns of dX per workgroup; it walks the weight rows BR = 64 per step.
//              4 waves, 2 (m) x 2 (k), every wave does every role: a wave owns BM/2 x 64 outputs.
//   operands   the WEIGHTS are the MFMA's A operand, read from a [k column][weight row] image of the step's w tile (lane (i, kq): column i,
//              rows 8 kq ... 8 kq + 7: one 16-byte read), dY its B operand ([dY row][weight row], rows of dY as they lie in memory), so
//              D[i = column][j = dY row] puts FOUR CONSECUTIVE columns of one dY row into a lane's accumulators: 8-byte stores.
//              Both images have 128-byte rows whose 16-byte chunks are XOR-swizzled with (row >> 1) & 7 (the forward's scheme).
//   w tile     a lane owns TWO ADJACENT weight rows (r, r + 1) and a packed word of each (the same position in the Bint4 block: lanes
//              t and t + 4 of the layout, 8 codes each at k = 2 i + {0, 1} + 8 h of a 32-k run): for each of its 8 columns it writes
//              the pair (w[r][c], w[r + 1][c]) as ONE 4-byte piece of the [column][row] image -- the transpose costs nothing extra.
//              The weights are computed directly, w = RNE16(fma(lut[code], scale, zero)): the LUT entries (f32) come from a small
//              per-wave LDS table (row-wise any4: the wave's 16 rows, staged every step; otherwise one 16-entry table for all rows),
//              scale / zero are one word per (row, group).  Unlike the forward, the rows -- and with them the per-(row, group) tables
//              of final 16-bit values the forward builds -- change every step, so a table would serve at most BK / g weights of a row
//              per build; the direct fma costs one lookup and one fma per weight whatever g is.
//   pipeline   register staging, two LDS stages, ONE barrier per step: the global loads of step s + 1 are issued before the MFMAs of
//              step s, and written (dY chunks, the dequantised w image) into the other stage after them.
//   padding    weight rows at or past wrows (the step's 64 rows overhang a multiple of 8) are zero in BOTH images, columns at or past
//              k are zero in the w image and never stored, dY rows at or past m load row m - 1 and are never stored: a zero dY column
//              never meets garbage, and a NaN weight of a real row spreads exactly as in the dense product.
//   split      DxParams::splits > 1 (few tiles: m <= 256 at k = 4096): workgroup z walks the steps z * sps ... of the weight rows and
//              stores f32 partial tiles to part[z][m][k]; dx_split_sum_kernel adds the splits in split order and rounds once, so a
//              result is the same bits call to call (and the same as unsplit only up to f32 summation order).
//   numerics   one setting: the reference weights are exact here and cheap, so TG_NUM_FAST and TG_NUM_REFERENCE give the same bits.
#pragma once

struct DxParams {
  const char* dy;      // [m][wrows] 16-bit, row-major
  const char* w;       // Bint4 words [wrows / 8][k / (16 I)][32][I / 2] uint32
  const char* qinfo;   // [k / g][wrows][2] 16-bit (scale, zero); mx4: [wrows][k / g] uint8 exponents
  const char* lut;     // [wrows][16] (row-wise) / [16] (global) 16-bit, nullptr for int4 / mx4
  char* dx;            // [m][k] 16-bit
  float* part;         // splits > 1: [splits][m][k] f32 partial tiles
  int32_t m, wrows, k, ksuper, inner, gshift, qtype;
  int32_t tiles_m, tiles_k, splits, sps;   // sps: 64-row steps per split
};

constexpr int DX_BK = 128;   // columns of dX per workgroup
constexpr int DX_BR = 64;    // weight rows per step

template <int BM>
struct DxLds {
  static constexpr int Y_STAGE = BM * 128;        // [BM dY rows][64 weight rows] 16-bit
  static constexpr int W_STAGE = DX_BK * 128;     // [128 columns][64 weight rows] 16-bit
  static constexpr int Y_OFF = 0;
  static constexpr int W_OFF = 2 * Y_STAGE;
  static constexpr int L_OFF = W_OFF + 2 * W_STAGE;
  static constexpr int L_WAVE = 16 * 16 * 4;      // a wave's LUT: 16 rows x 16 f32
  static constexpr int BYTES = L_OFF + 4 * L_WAVE;
  static_assert(BYTES <= 160 * 1024, "LDS");
};

__device__ __forceinline__ void dx_barrier() { __syncthreads(); }

template <typename DT, int BM, bool QMX>
__global__ void __launch_bounds__(256) w4_gemm_dx_kernel(const DxParams p) {
  constexpr int MT = BM / 32;           // 16-row tiles of dY per wave
  constexpr int NT = 4;                 // 16-column tiles of dX per wave (64 columns)
  constexpr int YCH = BM * 8 / 256;     // 16-byte chunks of the dY tile per thread and step
  using L = DxLds<BM>;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const int tm = b % p.tiles_m, rest = b / p.tiles_m;
  const int tk = rest % p.tiles_k, z = rest / p.tiles_k;
  const int m0 = tm * BM, k0 = tk * DX_BK;
  const int nsteps = (p.wrows + DX_BR - 1) / DX_BR;
  const int s0 = z * p.sps;
  const int s1 = s0 + p.sps < nsteps ? s0 + p.sps : nsteps;
  const bool rowwise = p.qtype == TG_Q_ANY4_ROWWISE;
  const int W = p.inner >> 1;           // words per lane of the packed layout
  const int kg = p.k >> p.gshift;       // groups along k

  // ---- the LUT of this wave (f32): row-wise any4 re-stages it every step; otherwise one table of 16 entries, written once here ----
  char* lutw = lds + L::L_OFF + wv * L::L_WAVE;
  if (!rowwise && lane < 16) {
    float v;
    if (QMX) {
      const int mag = lane & 7;
      v = (lane & 8 ? -1.f : 1.f) * (mag < 5 ? 0.5f * mag : (mag == 5 ? 3.f : mag == 6 ? 4.f : 6.f));   // fp4-e2m1 (FloatDefs.cuh:18-34)
    } else if (p.qtype == TG_Q_INT4) {
      v = (float)(lane - 8);
    } else {
      v = DT::to_f32(reinterpret_cast<const uint16_t*>(p.lut)[lane]);
    }
    *reinterpret_cast<float*>(lutw + lane * 4) = v;
  }

  // ---- the dequantising part of this lane: rows rl, rl + 1 of a step (rl = 16 wv + 2 pr), two (32-k run, word) units ----
  const int pr = lane & 7, rl = wv * 16 + 2 * pr;
  int run[2], di[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int combo = (lane >> 3) + 8 * u;   // 16 (run, word) units of the 128 columns
    run[u] = combo >> 2;
    di[u] = combo & 3;
  }
  // dY tile: chunk c = tid + 256 q -> row c >> 3, 16-byte chunk c & 7 (8 weight rows)
  struct Regs {
    u32x4 y[YCH];
    uint32_t wd[2][2];   // [unit][row of the pair]
    uint32_t sz[2][2];   // scale | zero (mx4: the exponent byte)
    u32x2 lt;            // row-wise LUT: 4 entries of row lane >> 2
  };
  auto load = [&](int step, Regs& R) {
    const int r0 = step * DX_BR;
#pragma unroll
    for (int q = 0; q < YCH; ++q) {
      const int c = tid + 256 * q, row = c >> 3, ch = c & 7;
      int a = m0 + row;
      a = a < p.m ? a : p.m - 1;
      const int rr = r0 + ch * 8;
      if (rr < p.wrows) R.y[q] = *reinterpret_cast<const u32x4*>(p.dy + ((int64_t)a * p.wrows + rr) * 2);
      else R.y[q] = u32x4{0u, 0u, 0u, 0u};
    }
    const int r = r0 + rl;
    const bool rv = r < p.wrows;         // (wrows % 8 == 0: r + 1 too)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kc = k0 + 32 * run[u];
      if (rv && kc < p.k) {
        const int s = kc / (16 * p.inner), jw = (kc - s * 16 * p.inner) >> 5;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.w) + (((int64_t)(r >> 3) * p.ksuper + s) * 32 + 4 * (r & 7) + di[u]) * W + jw;
        R.wd[u][0] = src[0];
        R.wd[u][1] = src[4 * W];
        const int g = kc >> p.gshift;
        if (QMX) {
          R.sz[u][0] = reinterpret_cast<const uint8_t*>(p.qinfo)[(int64_t)r * kg + g];
          R.sz[u][1] = reinterpret_cast<const uint8_t*>(p.qinfo)[(int64_t)(r + 1) * kg + g];
        } else {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(p.qinfo) + (int64_t)g * p.wrows + r;
          R.sz[u][0] = q[0];
          R.sz[u][1] = q[1];
        }
      } else {
        R.wd[u][0] = R.wd[u][1] = 0u;
        R.sz[u][0] = R.sz[u][1] = 0u;   // (scale = zero = 0: every weight of the unit is 0)
      }
    }
    if (rowwise) {
      const int lr = r0 + wv * 16 + (lane >> 2);
      R.lt = lr < p.wrows ? *reinterpret_cast<const u32x2*>(p.lut + ((int64_t)lr * 16 + 4 * (lane & 3)) * 2) : u32x2{0u, 0u};
    }
  };
  auto commit = [&](int step, const Regs& R) {
    char* yst = lds + L::Y_OFF + (step & 1) * L::Y_STAGE;
    char* wst = lds + L::W_OFF + (step & 1) * L::W_STAGE;
#pragma unroll
    for (int q = 0; q < YCH; ++q) {
      const int c = tid + 256 * q, row = c >> 3, ch = c & 7;
      *reinterpret_cast<u32x4*>(yst + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = R.y[q];
    }
    if (rowwise) {
      const f32x4 v = {DT::lo_f32(R.lt[0]), DT::hi_f32(R.lt[0]), DT::lo_f32(R.lt[1]), DT::hi_f32(R.lt[1])};
      *reinterpret_cast<f32x4*>(lutw + (lane >> 2) * 64 + (lane & 3) * 16) = v;
      // (the wave's own region, read below by other lanes of the same wave: a wave's LDS operations execute in order; this only
      // keeps the compiler from moving the lookups above the write)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const char* lt0 = lutw + (rowwise ? (2 * pr) * 64 : 0);
    const char* lt1 = lutw + (rowwise ? (2 * pr + 1) * 64 : 0);
    const int rch = rl >> 3, rbyte = (rl & 7) * 2;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float sc0, z0, sc1, z1;
      if (QMX) {
        // scale = 2^(e - 127) as bf16 bits (Dequantization.cuh:331-346: 255 -> NaN, 0 -> 2^-127), zero = -0.0: fma(v, s, -0) = v * s
        auto e8 = [](uint32_t q) { return u2f((q == 255u ? 0x7fc0u : (q == 0u ? 0x0040u : (q << 7))) << 16); };
        sc0 = e8(R.sz[u][0]); sc1 = e8(R.sz[u][1]);
        z0 = z1 = -0.f;
        if (!(p.wrows > step * DX_BR + rl && k0 + 32 * run[u] < p.k)) sc0 = sc1 = 0.f;   // (padding: zero weights, not 2^-127 * 0)
      } else {
        sc0 = DT::lo_f32(R.sz[u][0]); z0 = DT::hi_f32(R.sz[u][0]);
        sc1 = DT::lo_f32(R.sz[u][1]); z1 = DT::hi_f32(R.sz[u][1]);
      }
      const uint32_t w0 = R.wd[u][0], w1 = R.wd[u][1];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint32_t c0 = (w0 >> (16 * e + 4 * h)) & 15u, c1 = (w1 >> (16 * e + 4 * h)) & 15u;
          const float v0 = __builtin_fmaf(*reinterpret_cast<const float*>(lt0 + c0 * 4), sc0, z0);
          const float v1 = __builtin_fmaf(*reinterpret_cast<const float*>(lt1 + c1 * 4), sc1, z1);
          const int col = 32 * run[u] + 8 * h + 2 * di[u] + e;
          *reinterpret_cast<uint32_t*>(wst + col * 128 + ((rch ^ ((col >> 1) & 7)) << 4) + rbyte) = DT::pack2(v0, v1);
        }
      }
    }
  };

  // ---- MFMAs: wave (wm, wn) owns dY rows wm * BM/2 ... and columns wn * 64 ... of the tile ----
  const int wm = wv >> 1, wn = wv & 1, fi = lane & 15, kq = lane >> 4;
  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int c = 0; c < MT; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](int step) {
    const char* yst = lds + L::Y_OFF + (step & 1) * L::Y_STAGE;
    const char* wst = lds + L::W_OFF + (step & 1) * L::W_STAGE;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      u32x4 wf[NT], yf[MT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = wn * 64 + t * 16 + fi;
        wf[t] = *reinterpret_cast<const u32x4*>(wst + col * 128 + (((4 * kb + kq) ^ ((col >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int row = wm * (BM / 2) + t * 16 + fi;
        yf[t] = *reinterpret_cast<const u32x4*>(yst + row * 128 + (((4 * kb + kq) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int c = 0; c < MT; ++c) acc[a][c] = DT::mfma(wf[a], yf[c], acc[a][c]);
    }
  };

  if (s0 < s1) {   // (workgroup-uniform: a split past the last step stores zeros)
    Regs R;
    load(s0, R);
    commit(s0, R);
    dx_barrier();
    for (int s = s0; s < s1; ++s) {
      const bool more = s + 1 < s1;
      if (more) load(s + 1, R);
      mma(s);
      if (more) commit(s + 1, R);
      dx_barrier();
    }
  }

  // ---- store: lane (dY row fi of tile c, columns 4 kq ... 4 kq + 3 of tile a) ----
#pragma unroll
  for (int c = 0; c < MT; ++c) {
    const int a = m0 + wm * (BM / 2) + c * 16 + fi;
    if (a >= p.m) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = k0 + wn * 64 + t * 16 + 4 * kq;
      if (col >= p.k) continue;   // (k % 32 == 0: a group of four columns is inside or outside)
      if (p.splits > 1) *reinterpret_cast<f32x4*>(p.part + ((int64_t)z * p.m + a) * p.k + col) = acc[t][c];
      else store_rows4<DT>(p.dx, nullptr, (int64_t)a * p.k + col, col, acc[t][c]);
    }
  }
}

// dX[a][j ... j + 3] = RNE16(sum of the splits' f32 partial tiles, in split order)
template <typename DT>
__global__ void __launch_bounds__(256) dx_split_sum_kernel(const float* __restrict__ part, int splits, int64_t part_stride, char* __restrict__ dx,
                                                           int64_t quads) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  f32x4 acc = *reinterpret_cast<const f32x4*>(part + i * 4);
  for (int s = 1; s < splits; ++s) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + s * part_stride + i * 4);
    acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
  }
  store_rows4<DT>(dx, nullptr, i * 4, 0, acc);
}
