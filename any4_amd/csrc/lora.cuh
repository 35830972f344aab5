// lora.cuh -- per-sequence LoRA adapters on a linear's output (dg_lora_shrink / dg_lora_expand, include/decode_glue_hip.h): the "BGMV" pair.
// Included inside tg_lora.hip's anonymous namespace.
//
// Adapter weights of one linear: A [n_adapters][r][k] and B [n_adapters][n][r], 16-bit, scale [n_adapters] f32.  The adapter of activation
// row i is idx[i / rows_per_id]; a value outside [0, n_adapters) means "no adapter" and neither kernel forms an address from it.
//
//   lora_shrink_kernel   t[i][j] = sum_c A[a][j][c] x~[i][c]                (x~ = x, or with a norm weight g: x~ = RNE16(x g) and the sum
//                                                                            times rs = rsqrt(mean(x^2) + eps): the "sum" convention of the
//                                                                            GEMV's fused RMSNorm, so the adapter contracts the 16-bit
//                                                                            activations the base GEMM contracts)
//   lora_expand_kernel   y[i][c] = RNE16(f32(y[i][c]) + scale[a] sum_j B[a][c][j] t[i][j])     in place; j ascending
//
// Both sum in f32 in a fixed order and use no atomics: the same inputs give the same bits on every launch.
//
// Shrink: a workgroup owns one activation row and LSH_J of its r dot products.  Its LSH_THREADS lanes walk k together, 8 elements
// (16 bytes) per lane and pass, LSH_PASS = 8 LSH_THREADS elements per pass: at k = 4096 one pass, at k = 14336 three and a ragged fourth,
// so no wave walks more than k / LSH_THREADS x 64 elements.  A lane chains its products per j; the wave sums them in the vector ALU
// (tgl::wave_sum, every lane the same bits), the LSH_WAVES partials meet in LDS and are added in wave order.
// Expand: a workgroup owns LEX_ROWS activation rows and LEX_COLS = 2 LEX_THREADS output columns, two per lane.  It stages t of its rows in
// LDS once; a lane then reads its two rows of B (r 16-bit values each, 16 bytes per load) per activation row and updates one dword of y.
// The loads of all its rows are issued together (the rows are independent; one after the other they cost the memory latency per row).

constexpr int LSH_THREADS = 512;
constexpr int LSH_WAVES = LSH_THREADS / 64;
constexpr int LSH_J = 4;                      // dot products per workgroup (r % 8 == 0: r / 4 workgroups per row)
constexpr int LSH_PASS = 8 * LSH_THREADS;     // elements of k per pass
constexpr int LEX_THREADS = 256;
constexpr int LEX_COLS = 2 * LEX_THREADS;     // output columns per workgroup
constexpr int LEX_ROWS = 8;                   // activation rows per workgroup
constexpr int LORA_MAX_R = 64;

struct LoraShrinkParams {
  const uint16_t* x;       // [m][k]
  const uint16_t* g;       // [k] or null
  const uint16_t* A;       // [n_adapters][r][k]
  const int32_t* idx;      // [ceil(m / rows_per_id)]
  float* t;                // [m][r]
  int64_t m;
  int32_t k, r, n_adapters;
  int64_t rows_per_id;
  float eps, inv_k;
};

struct LoraExpandParams {
  const float* t;          // [m][r]
  const uint16_t* B;       // [n_adapters][n][r]
  const float* scale;      // [n_adapters]
  const int32_t* idx;
  uint16_t* y;             // [m][ldy], the first n columns
  int64_t m, ldy;
  int32_t n, r, n_adapters;
  int64_t rows_per_id;
};

template <typename DT>
__global__ __launch_bounds__(LSH_THREADS) void lora_shrink_kernel(const LoraShrinkParams P) {
  __shared__ float part[LSH_WAVES][LSH_J + 1];
  const int64_t row = blockIdx.x;
  const int j0 = blockIdx.y * LSH_J;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t a = P.idx[row / P.rows_per_id];
  if (a < 0 || a >= P.n_adapters) {  // (uniform over the workgroup) no adapter: zeros, and A is not addressed
    if (tid < LSH_J) P.t[row * P.r + j0 + tid] = 0.f;
    return;
  }
  const uint16_t* xr = P.x + row * P.k;
  const uint16_t* Ar = P.A + ((int64_t)a * P.r + j0) * P.k;
  const bool norm = P.g != nullptr;
  float acc[LSH_J] = {};
  float ss = 0.f;
  for (int c = tid * 8; c < P.k; c += LSH_PASS) {  // (k % 8 == 0: a lane's 8 elements are inside or outside as a whole)
    u32x4 xv = *reinterpret_cast<const u32x4*>(xr + c);
    u32x4 av[LSH_J];
#pragma unroll
    for (int j = 0; j < LSH_J; ++j) av[j] = *reinterpret_cast<const u32x4*>(Ar + (int64_t)j * P.k + c);
    if (norm) {
      const u32x4 gv = *reinterpret_cast<const u32x4*>(P.g + c);
      float q[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = DT::lo_f32(xv[e]), hi = DT::hi_f32(xv[e]);
        q[e] = fmaf(hi, hi, lo * lo);
        xv[e] = DT::pack2(lo * DT::lo_f32(gv[e]), hi * DT::hi_f32(gv[e]));  // x~ = RNE16(x g): the product is exact in f32
      }
      ss += (q[0] + q[1]) + (q[2] + q[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = DT::lo_f32(xv[e]), hi = DT::hi_f32(xv[e]);
#pragma unroll
      for (int j = 0; j < LSH_J; ++j) {
        acc[j] = fmaf(DT::lo_f32(av[j][e]), lo, acc[j]);
        acc[j] = fmaf(DT::hi_f32(av[j][e]), hi, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < LSH_J; ++j) acc[j] = tgl::wave_sum(acc[j]);
  if (norm) ss = tgl::wave_sum(ss);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < LSH_J; ++j) part[wave][j] = acc[j];
    part[wave][LSH_J] = ss;
  }
  __syncthreads();
  if (tid < LSH_J) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int w = 0; w < LSH_WAVES; ++w) {
      s += part[w][tid];
      q += part[w][LSH_J];
    }
    if (norm) s *= rsqrtf(q * P.inv_k + P.eps);
    P.t[row * P.r + j0 + tid] = s;
  }
}

// NR: activation rows per workgroup -- LEX_ROWS, or 1 for a launch of one row (which then issues no load twice)
template <typename DT, int NR>
__global__ __launch_bounds__(LEX_THREADS) void lora_expand_kernel(const LoraExpandParams P) {
  __shared__ __attribute__((aligned(16))) float ts[NR][LORA_MAX_R];
  __shared__ int32_t as[NR];
  const int64_t row0 = (int64_t)blockIdx.x * NR;
  const int rows = (int)(P.m - row0 < NR ? P.m - row0 : NR);
  const int tid = threadIdx.x;
  // t of the block's rows, once: every row below m is read, with or without an adapter (the shrink wrote zeros for a row without one;
  // its sums are dropped below).  Rows of the block past m are not staged: their part of `ts` is uninitialised LDS, which is summed
  // like the rest and dropped as well -- nothing of it reaches memory.
  if (tid < NR) {
    int32_t a = -1;
    if (tid < rows) {
      a = P.idx[(row0 + tid) / P.rows_per_id];
      if (a < 0 || a >= P.n_adapters) a = -1;
    }
    as[tid] = a;
  }
  for (int e = tid; e < rows * P.r; e += LEX_THREADS) ts[e / P.r][e % P.r] = P.t[row0 * P.r + e];
  __syncthreads();
  const int c = blockIdx.y * LEX_COLS + 2 * tid;  // this lane's two columns (n % 8 == 0: both inside or both outside)
  if (c >= P.n) return;
  // Every row's loads are issued before any row's sums: the rows of a block are independent, and a loop that finished one row before it
  // touched the next would pay the memory latency once per row.  A row without an adapter borrows the address of a row of the block that
  // has one (its sums are dropped); a block without any adapted row has nothing to do.
  int32_t a[NR], any = -1;
#pragma unroll
  for (int i = NR - 1; i >= 0; --i) {
    a[i] = as[i];
    if (a[i] >= 0) any = a[i];
  }
  if (any < 0) return;
  const uint16_t* bp[NR];
  float s0[NR], s1[NR], sc[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int32_t ai = a[i] >= 0 ? a[i] : any;
    bp[i] = P.B + ((int64_t)ai * P.n + c) * P.r;
    sc[i] = P.scale[ai];
    s0[i] = s1[i] = 0.f;
  }
  for (int j = 0; j < P.r; j += 8) {
    u32x4 v0[NR], v1[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      v0[i] = *reinterpret_cast<const u32x4*>(bp[i] + j);
      v1[i] = *reinterpret_cast<const u32x4*>(bp[i] + P.r + j);
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const f32x4 ta = *reinterpret_cast<const f32x4*>(&ts[i][j]);
      const f32x4 tb = *reinterpret_cast<const f32x4*>(&ts[i][j + 4]);
      const float tv[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // j ascending
        s0[i] = fmaf(DT::lo_f32(v0[i][e]), tv[2 * e], s0[i]);
        s0[i] = fmaf(DT::hi_f32(v0[i][e]), tv[2 * e + 1], s0[i]);
        s1[i] = fmaf(DT::lo_f32(v1[i][e]), tv[2 * e], s1[i]);
        s1[i] = fmaf(DT::hi_f32(v1[i][e]), tv[2 * e + 1], s1[i]);
      }
    }
  }
  uint32_t yv[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i)
    if (a[i] >= 0) yv[i] = *reinterpret_cast<const uint32_t*>(P.y + (row0 + i) * P.ldy + c);
#pragma unroll
  for (int i = 0; i < NR; ++i)
    if (a[i] >= 0)  // (a row without an adapter keeps its bits: it is not rewritten; scale x sum enters through one fused multiply-add)
      *reinterpret_cast<uint32_t*>(P.y + (row0 + i) * P.ldy + c) = DT::pack2(fmaf(sc[i], s0[i], DT::lo_f32(yv[i])), fmaf(sc[i], s1[i], DT::hi_f32(yv[i])));
}
