// w4_gemm_dq.cuh -- the gradients of the QUANTISATION PARAMETERS of a 4-bit linear (scales, zeros, LUT), straight through the 16-bit rounding
// of w[r][j] = RNE16(fma(lut[r][c(r,j)], s[g(j)][r], z[g(j)][r])).  With the weight gradient G[r][j] = sum_a dY[a][r] * x[a][j] one primitive
// carries all three:
//
//   H[g][r][c] = sum over the columns j of group g whose code c(r, j) is c of G[r][j]          (f32, [k / g][wrows][16])
//   dz[g][r]   = sum_c H[g][r][c]      ds[g][r] = sum_c lut[r][c] * H[g][r][c]      dlut[r][c] = sum_g s[g][r] * H[g][r][c]  (global LUT: and sum_r)
//
// w4_gemm_dq_kernel computes H -- a TN GEMM whose epilogue bins the accumulators by code and group, so the [wrows][k] f32 matrix G is never
// written -- from x, dY and the packed codes alone; dq_finish_kernel applies the parameters in a small second pass.
//
//   tile       128 weight rows x 128 columns of k per workgroup; it walks the m activation rows 64 per step.  4 waves, 2 (rows) x 2
//              (columns), a wave owns 64 x 64 outputs = 64 f32 accumulators per lane.
//   operands   both have the contraction index on the slow memory axis (dY[a][r], x[a][j]).  A thread loads the same 16-byte chunk (8 rows /
//              columns) of TWO ADJACENT activation rows and writes the eight (a, a + 1) pairs as 4-byte pieces of a [row or column][activation
//              row] image: the transpose costs the packing only.  Images have 128-byte rows whose 16-byte chunks are XOR-swizzled with
//              (row >> 1) & 7 (the forward's and dx's scheme: the 16-byte fragment reads are conflict-free; the 4-byte writes of a wave reach
//              32 of the 64 banks, two lanes each).  x is the MFMA's A operand, dY its B operand: D[i = column][j = weight row] puts FOUR
//              CONSECUTIVE columns of one weight row into a lane's accumulators, so a lane bins its own values with no lane exchange.
//   pipeline   register staging, two LDS stages, ONE barrier per step (as w4_gemm_dx.cuh).  No load sits under a lane mask: addresses are
//              clamped (activation rows to m - 1, chunks to the last one of the matrix) and the rows at or past m are zeroed on the way to LDS.
//   padding    weight rows at or past wrows and columns at or past k accumulate clamped (finite or not) data and are never stored.
//   epilogue   once per tile: the tile's packed words (loaded before the loop) become a byte-per-code image in LDS; a lane select-accumulates
//              its 8 values of a (row, 32-column segment) into 16 bins, the four lanes of the row are summed by two row swaps, the segments
//              of a unit (= min(group, 128) columns) are folded in segment order and stored to hp[k / unit][wrows][16].  Every sum has a fixed
//              order and there is no atomic: a result is the same bits call to call.
//   words      Bint4 (innerKTiles 2 / 4 / 8), which is also the native weights-on-the-left format: the set of w4_gemm_dx.cuh.
#pragma once

struct DqParams {
  const char* x;       // [m][k] 16-bit, row-major
  const char* dy;      // [m][wrows] 16-bit, row-major
  const char* w;       // Bint4 words [wrows / 8][k / (16 I)][32][I / 2] uint32
  float* hp;           // [k / unit][wrows][16] f32: H, or its two halves per group when the group (256) is wider than the tile
  int32_t m, wrows, k, ksuper, inner, ushift;   // ushift: log2(unit), unit = min(group, 128)
  int32_t tiles_r, tiles_k;
};

constexpr int DQ_BR = 128;   // weight rows per workgroup
constexpr int DQ_BK = 128;   // columns of k per workgroup
constexpr int DQ_BA = 64;    // activation rows per step

struct DqLds {
  static constexpr int IMG = 128 * 128;          // one operand image: [128 rows / columns][64 activation rows] 16-bit
  static constexpr int STAGE = 2 * IMG;          // dY image, x image
  static constexpr int BYTES = 2 * STAGE;
  // the epilogue's (the images are dead by then)
  static constexpr int C_ROW = 132;              // code image: a byte per (row, column); rows padded by one word
  static constexpr int C_OFF = 0;
  static constexpr int P_OFF = 128 * C_ROW;      // partial bins [128 rows][4 segments][16] f32
  static_assert(P_OFF % 16 == 0 && P_OFF + 128 * 4 * 16 * 4 <= BYTES && BYTES <= 160 * 1024, "LDS");
};

template <typename DT>
__global__ void __launch_bounds__(256) w4_gemm_dq_kernel(const DqParams p) {
  using L = DqLds;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tr = blockIdx.x % p.tiles_r, tk = blockIdx.x / p.tiles_r;
  const int r0 = tr * DQ_BR, k0 = tk * DQ_BK;
  const int nsteps = (p.m + DQ_BA - 1) / DQ_BA;

  // ---- the tile's packed words: thread -> two (row, 32-k run) owners, the four words (8 codes each at k = 8 h + 2 di + {0, 1}) of each ----
  uint32_t cw[2][4];
  {
    const int W = p.inner >> 1;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = tid + 256 * u, r = r0 + (o >> 2), kc = k0 + 32 * (o & 3);
      if (r < p.wrows && kc < p.k) {
        const int s = kc / (16 * p.inner), jw = (kc - s * 16 * p.inner) >> 5;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.w) + (((int64_t)(r >> 3) * p.ksuper + s) * 32 + 4 * (r & 7)) * W + jw;
#pragma unroll
        for (int di = 0; di < 4; ++di) cw[u][di] = src[di * W];
      } else {
#pragma unroll
        for (int di = 0; di < 4; ++di) cw[u][di] = 0u;
      }
    }
  }

  // ---- loader: 16-byte chunk rc (8 rows / columns) of the activation rows 2 P, 2 P + 1 of a step, P = pp + 16 q ----
  const int rc = (tid & 3) | (wv << 2), pp = (tid >> 2) & 15;
  int rr = r0 + 8 * rc, jj = k0 + 8 * rc;
  rr = rr < p.wrows ? rr : p.wrows - 8;   // (wrows % 8 == 0, k % 32 == 0: a chunk is inside or outside)
  jj = jj < p.k ? jj : p.k - 8;
  struct Regs {
    u32x4 y[2][2], x[2][2];   // [q][row of the pair]
  };
  auto load = [&](int step, Regs& R) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int a = step * DQ_BA + 2 * (pp + 16 * q) + h;
        a = a < p.m ? a : p.m - 1;
        R.y[q][h] = *reinterpret_cast<const u32x4*>(p.dy + ((int64_t)a * p.wrows + rr) * 2);
        R.x[q][h] = *reinterpret_cast<const u32x4*>(p.x + ((int64_t)a * p.k + jj) * 2);
      }
    }
  };
  // the pairs (v[a][i], v[a + 1][i]) of the chunk's eight rows / columns i, one 4-byte piece each
  auto put = [&](char* img, u32x4 lo, u32x4 hi, int P) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int row = 8 * rc + e, d = e >> 1;
      const uint32_t v = (e & 1) ? (lo[d] >> 16) | (hi[d] & 0xffff0000u) : (lo[d] & 0xffffu) | (hi[d] << 16);
      *reinterpret_cast<uint32_t*>(img + row * 128 + (((P >> 2) ^ ((row >> 1) & 7)) << 4) + (P & 3) * 4) = v;
    }
  };
  auto commit = [&](int step, const Regs& R) {
    char* yst = lds + (step & 1) * L::STAGE;
    char* xst = yst + L::IMG;
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int P = pp + 16 * q, a = step * DQ_BA + 2 * P;
      const bool v0 = a < p.m, v1 = a + 1 < p.m;   // rows past m contribute zero
      put(yst, v0 ? R.y[q][0] : zero, v1 ? R.y[q][1] : zero, P);
      put(xst, v0 ? R.x[q][0] : zero, v1 ? R.x[q][1] : zero, P);
    }
  };

  // ---- MFMAs: wave (wr, wj) owns weight rows wr * 64 ... and columns wj * 64 ... of the tile ----
  const int wr = wv >> 1, wj = wv & 1, fi = lane & 15, kq = lane >> 4;
  f32x4 acc[4][4];   // [column tile][row tile]: G[wr * 64 + 16 tr + fi][wj * 64 + 16 tc + 4 kq + e]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](int step) {
    const char* yst = lds + (step & 1) * L::STAGE;
    const char* xst = yst + L::IMG;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      u32x4 xf[4], yf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int col = wj * 64 + t * 16 + fi;
        xf[t] = *reinterpret_cast<const u32x4*>(xst + col * 128 + (((4 * kb + kq) ^ ((col >> 1) & 7)) << 4));
        const int row = wr * 64 + t * 16 + fi;
        yf[t] = *reinterpret_cast<const u32x4*>(yst + row * 128 + (((4 * kb + kq) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = DT::mfma(xf[a], yf[c], acc[a][c]);
    }
  };

  {
    Regs R;
    load(0, R);
    commit(0, R);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const bool more = s + 1 < nsteps;
      if (more) load(s + 1, R);
      mma(s);
      if (more) commit(s + 1, R);
      __syncthreads();
    }
  }

  // ---- epilogue 1: the code image, a byte per (row, column) ----
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int o = tid + 256 * u;
    char* dst = lds + L::C_OFF + (o >> 2) * L::C_ROW + 32 * (o & 3);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      uint32_t v = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) v |= ((cw[u][2 * (t & 1) + (b >> 1)] >> (16 * (b & 1) + 4 * (t >> 1))) & 15u) << (8 * b);
      *reinterpret_cast<uint32_t*>(dst + 4 * t) = v;   // columns 4 t ... 4 t + 3 of the run
    }
  }
  __syncthreads();

  // ---- epilogue 2: bins of a (row, 32-column segment): 8 values per lane, then the row's four lanes (fi + 16 kq) ----
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = wr * 64 + t * 16 + fi;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float bins[16];
#pragma unroll
      for (int b = 0; b < 16; ++b) bins[b] = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tc = 2 * s + h;
        const uint32_t cd = *reinterpret_cast<const uint32_t*>(lds + L::C_OFF + row * L::C_ROW + wj * 64 + tc * 16 + 4 * kq);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t c = (cd >> (8 * e)) & 15u;
          const float v = acc[tc][t][e];
#pragma unroll
          for (int b = 0; b < 16; ++b) bins[b] += c == (uint32_t)b ? v : 0.f;
        }
      }
#pragma unroll
      for (int b = 0; b < 16; ++b) bins[b] = tgl::halves32_sum(tgl::rows16_sum(bins[b]));
      if (kq == 0) {
        float* dst = reinterpret_cast<float*>(lds + L::P_OFF) + (row * 4 + wj * 2 + s) * 16;
#pragma unroll
        for (int b = 0; b < 4; ++b) *reinterpret_cast<f32x4*>(dst + 4 * b) = f32x4{bins[4 * b], bins[4 * b + 1], bins[4 * b + 2], bins[4 * b + 3]};
      }
    }
  }
  __syncthreads();

  // ---- epilogue 3: the segments of a unit in segment order; rows past wrows and units past k are not stored ----
  const int spu = 1 << (p.ushift - 5), nu = 4 / spu, units = p.k >> p.ushift;
  const float* part = reinterpret_cast<const float*>(lds + L::P_OFF);
  for (int it = tid; it < 128 * 4 * nu; it += 256) {
    const int c4 = it & 3, row = (it >> 2) & 127, u = it >> 9;
    f32x4 sum = *reinterpret_cast<const f32x4*>(part + (row * 4 + u * spu) * 16 + 4 * c4);
    for (int s = 1; s < spu; ++s) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(part + (row * 4 + u * spu + s) * 16 + 4 * c4);
      sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
    }
    const int r = r0 + row, gu = (k0 >> p.ushift) + u;
    if (r < p.wrows && gu < units) *reinterpret_cast<f32x4*>(p.hp + ((int64_t)gu * p.wrows + r) * 16 + 4 * c4) = sum;
  }
}

// H -> d_qinfo [k / g][wrows][2] = (ds, dz) and the per-row dlut [wrows][16], all f32.  Thread (row, quarter of the 16 codes): the groups in
// group order, the codes of a row in a fixed tree (quarter sums, then the quad's lanes by two DPP moves).
struct DqFinishParams {
  const float* hp;     // [ngroups * upg][wrows][16]
  const char* qinfo;   // [ngroups][wrows][2] 16-bit
  const char* lut;     // [wrows][16] / [16] 16-bit; int4: unused
  float* d_qinfo;      // nullptr: skipped
  float* d_lut_rows;   // [wrows][16] (row-wise: the output; global: the workspace dq_rowsum_kernel reads); nullptr: skipped
  int32_t wrows, ngroups, upg, qtype;   // upg: units per group (2 for groups of 256)
};

template <typename DT>
__global__ void __launch_bounds__(256) dq_finish_kernel(const DqFinishParams p) {
  const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int c4 = t & 3;
  const bool valid = (t >> 2) < p.wrows;
  const int r = valid ? (t >> 2) : p.wrows - 1;   // (every lane of a quad stays in the DPP sums)
  f32x4 lt;
  if (p.qtype == TG_Q_INT4) {
    lt = f32x4{(float)(4 * c4 - 8), (float)(4 * c4 - 7), (float)(4 * c4 - 6), (float)(4 * c4 - 5)};
  } else {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p.lut + ((p.qtype == TG_Q_ANY4_ROWWISE ? (int64_t)r * 16 : 0) + 4 * c4) * 2);
    lt = f32x4{DT::lo_f32(v[0]), DT::hi_f32(v[0]), DT::lo_f32(v[1]), DT::hi_f32(v[1])};
  }
  f32x4 dl = {0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < p.ngroups; ++g) {
    f32x4 h = *reinterpret_cast<const f32x4*>(p.hp + ((int64_t)g * p.upg * p.wrows + r) * 16 + 4 * c4);
    if (p.upg == 2) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.hp + ((int64_t)(g * 2 + 1) * p.wrows + r) * 16 + 4 * c4);
      h[0] += v[0]; h[1] += v[1]; h[2] += v[2]; h[3] += v[3];
    }
    const float s = DT::lo_f32(reinterpret_cast<const uint32_t*>(p.qinfo)[(int64_t)g * p.wrows + r]);
    float dz = (h[0] + h[1]) + (h[2] + h[3]);
    float ds = (lt[0] * h[0] + lt[1] * h[1]) + (lt[2] * h[2] + lt[3] * h[3]);
    dz += tgl::lane_xor<1>(dz, lane); dz += tgl::lane_xor<2>(dz, lane);
    ds += tgl::lane_xor<1>(ds, lane); ds += tgl::lane_xor<2>(ds, lane);
    if (valid && c4 == 0 && p.d_qinfo) *reinterpret_cast<f32x2*>(p.d_qinfo + ((int64_t)g * p.wrows + r) * 2) = f32x2{ds, dz};
    dl[0] += s * h[0]; dl[1] += s * h[1]; dl[2] += s * h[2]; dl[3] += s * h[3];
  }
  if (valid && p.d_lut_rows) *reinterpret_cast<f32x4*>(p.d_lut_rows + (int64_t)r * 16 + 4 * c4) = dl;
}

// the global table: out[c] = sum over the rows of rows[r][c].  One workgroup; lane group j adds the rows j, j + 16, ... in row order, the 16
// groups are folded in a fixed tree.
__global__ void __launch_bounds__(256) dq_rowsum_kernel(const float* __restrict__ rows, int wrows, float* __restrict__ out) {
  __shared__ float part[256];
  const int tid = threadIdx.x, c = tid & 15, j = tid >> 4;
  float acc = 0.f;
  for (int r = j; r < wrows; r += 16) acc += rows[(int64_t)r * 16 + c];
  part[tid] = acc;
  __syncthreads();
  for (int st = 8; st >= 1; st >>= 1) {
    if (j < st) part[tid] += part[tid + 16 * st];
    __syncthreads();
  }
  if (j == 0) out[c] = part[c];
}
