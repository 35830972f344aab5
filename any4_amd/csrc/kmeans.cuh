// kmeans.cuh -- kmeans_rows_kernel: the any4 quantizer's weighted 1-D k-means (any4_amd/quantize.py: lloyd_rows_ref is its definition),
// one workgroup per row, the row resident in LDS.  Included inside tg_kmeans.hip's anonymous namespace.
//
// A row is sorted once (bitonic network over (x, w) pairs, padded to a power of two with +inf / 0), then f64 prefix sums of w and x w
// are kept PER BLOCK OF 32 sorted elements (the full arrays do not fit beside a 16384-element row): the prefix at a boundary b is
// block_prefix[b / 32] plus at most 31 elements added one by one in ascending position.  A Lloyd iteration is then, for cluster j on
// lane j of wave 0: one binary search for the midpoint, one prefix, two differences and one division -- O(C log k), no pass over the row.
// The only O(k) work inside the loop is the re-seeding of empty clusters (at most C - 1 workgroup-wide arg-max rounds).
//
// Numerics: IEEE f64, one operation per rounding of the reference, contraction off (the unit is also compiled with -ffp-contract=off).
// Safety: every loop bound is fixed before the launch (k, n2, C, S, max_iter, 15 search steps, 32 tail elements); every LDS index that
// comes from data (search results, re-seed positions) is clamped to [0, k]; nothing read from memory becomes a global address; outputs
// go to positions fixed by (row, column).
#pragma once
#pragma clang fp contract(off)

constexpr int KM_THREADS = 256;
constexpr int KM_MAX_C = 16;
constexpr int KM_MAX_S = 4;
constexpr int KM_MAX_K = 16384;
constexpr int KM_MAX_ITER = 10000;
constexpr int KM_SEARCH_STEPS = 15;  // 2^14 = KM_MAX_K: a search over [0, k] halves to one position in at most 15 steps

struct KmParams {
  const float* x;      // [rows][k]
  const float* w;      // [rows][k] (w_stride = k), [k] (w_stride = 0) or unused
  const float* c0;     // [S][rows][C]
  int32_t* assign;     // [rows][k]
  float* centers;      // [rows][C]
  double* sse;         // [rows] or null
  int32_t* iters;      // [rows] or null
  int64_t w_stride;
  int64_t rows;
  double tol;
  int32_t k, n2, C, S, max_iter;
};

// LDS, all of it dynamic (prepare_lds_kernel: the kernel has no static LDS): this header, then the block prefixes, then the row
struct alignas(16) KmShared {
  double cs[KM_MAX_C];     // the iteration's centres, ascending
  double cn[KM_MAX_C];     // the centres it produces
  double best[KM_MAX_C];   // ascending centres of the best seeding so far
  double mid[KM_MAX_C];    // midpoints of `best` for the assignment pass
  double pw[KM_MAX_C + 1], px[KM_MAX_C + 1];  // prefix of w / x w at the clusters' boundaries
  double red_d[KM_THREADS];
  int32_t red_i[KM_THREADS];
  int32_t b[KM_MAX_C + 1];  // b[j] = first sorted position of cluster j; b[C] = k
  uint32_t flag_empty, flag_moved;
};
static_assert(sizeof(KmShared) % 16 == 0, "the arrays behind the header stay 16-byte aligned");

__host__ __device__ inline int km_bp_entries(int n2) { return (n2 + 31) / 32 + 1; }
inline int64_t km_lds_bytes(int n2, bool weighted) {
  return (int64_t)sizeof(KmShared) + (weighted ? 2 : 1) * ((int64_t)km_bp_entries(n2) * 8 + (int64_t)n2 * 4);
}

// largest t in [0, C - 1] with t == 0 or b[t] <= i (b ascending): the cluster of sorted position i
__device__ __forceinline__ int km_cluster_of_pos(const int32_t* b, int C, int i) {
  int cl = 0;
#pragma unroll
  for (int step = 8; step > 0; step >>= 1) {
    const int t = cl + step;
    if (t <= C - 1 && b[t] <= i) cl = t;
  }
  return cl;
}
// largest t in [0, C - 1] with t == 0 or mid[t - 1] < x (mid ascending): searchsorted(mid, x)
__device__ __forceinline__ int km_cluster_of_value(const double* mid, int C, double x) {
  int cl = 0;
#pragma unroll
  for (int step = 8; step > 0; step >>= 1) {
    const int t = cl + step;
    if (t <= C - 1 && mid[t - 1] < x) cl = t;
  }
  return cl;
}

template <bool W>
__global__ void __launch_bounds__(KM_THREADS) kmeans_rows_kernel(KmParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
  KmShared& S = *reinterpret_cast<KmShared*>(km_lds);
  const int tid = threadIdx.x;
  const int k = P.k, n2 = P.n2, C = P.C;
  const int nbp = km_bp_entries(n2);
  double* const bpx = reinterpret_cast<double*>(km_lds + sizeof(KmShared));  // [nbp] prefix of x w in front of block i
  double* const bpw = bpx + nbp;                                             // [nbp] ... of w (W only)
  float* const xs = reinterpret_cast<float*>(bpx + (W ? 2 : 1) * nbp);       // [n2] the sorted row
  float* const ws = xs + n2;                                                 // [n2] its weights (W only)
  const int64_t row = blockIdx.x;
  const float* const xrow = P.x + row * (int64_t)k;

  // ---- the row into LDS, padded with (+inf, 0) ----
  for (int i = tid; i < n2; i += KM_THREADS) {
    xs[i] = i < k ? xrow[i] : __builtin_inff();
    if (W) ws[i] = i < k ? P.w[row * P.w_stride + i] : 0.f;
  }
  __syncthreads();
  // ---- bitonic sort, ascending by x, carrying w ----
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += KM_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const float a = xs[i], b = xs[j];
        if ((a > b) == up && a != b) {
          xs[i] = b; xs[j] = a;
          if (W) { const float wa = ws[i]; ws[i] = ws[j]; ws[j] = wa; }
        }
      }
      __syncthreads();
    }
  }
  // ---- block totals (sequential within a block), then their exclusive prefix (sequential over the blocks) ----
  const int nblk = (k + 31) >> 5;
  for (int blk = tid; blk < nblk; blk += KM_THREADS) {
    double tw = 0.0, tx = 0.0;
    for (int t = 0; t < 32; ++t) {
      const int i = blk * 32 + t;
      if (i < k) {
        const double wv = W ? (double)ws[i] : 1.0;
        tw += wv;
        tx += (double)xs[i] * wv;
      }
    }
    bpx[blk + 1] = tx;
    if (W) bpw[blk + 1] = tw;
  }
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    bpx[0] = 0.0;
    for (int blk = 1; blk <= nblk; ++blk) { acc += bpx[blk]; bpx[blk] = acc; }
  }
  if (W && tid == 64) {  // (another wave: the two scans run side by side)
    double acc = 0.0;
    bpw[0] = 0.0;
    for (int blk = 1; blk <= nblk; ++blk) { acc += bpw[blk]; bpw[blk] = acc; }
  }
  if (tid == 0) { S.b[0] = 0; S.pw[0] = 0.0; S.px[0] = 0.0; }
  __syncthreads();

  double span = (double)xs[k - 1] - (double)xs[0];
  span = span > 1e-12 ? span : 1e-12;
  const double thr = P.tol * span;

  // number of sorted points <= v, in [0, k]
  auto upper_bound = [&](double v) {
    int lo = 0, hi = k;
    for (int s = 0; s < KM_SEARCH_STEPS; ++s) {
      if (lo < hi) {
        const int m = (lo + hi) >> 1;
        if ((double)xs[m] <= v) lo = m + 1; else hi = m;
      }
    }
    return min(max(lo, 0), k);
  };
  // cn -> cs, ascending (lane j of wave 0 places centre j by its rank; equal values are interchangeable)
  auto sort_centres = [&]() {
    if (tid < C) {
      const double v = S.cn[tid];
      int rank = 0;
      for (int i = 0; i < C; ++i) {
        const double u = S.cn[i];
        rank += (u < v || (u == v && i < tid)) ? 1 : 0;
      }
      S.cs[min(rank, C - 1)] = v;
    }
    __syncthreads();
  };

  double best_sse = 0.0;
  int total_iters = 0;
  for (int s = 0; s < P.S; ++s) {
    if (tid < C) S.cn[tid] = (double)P.c0[((int64_t)s * P.rows + row) * C + tid];
    __syncthreads();
    for (int it = 0; it < P.max_iter; ++it) {
      sort_centres();
      // boundaries and the prefixes there
      if (tid < C) {
        const int b = tid < C - 1 ? upper_bound((S.cs[tid + 1] + S.cs[tid]) * 0.5) : k;
        const int blk = b >> 5;
        double px = bpx[blk], pw = W ? bpw[blk] : (double)(blk * 32);
        for (int t = 0; t < 32; ++t) {
          const int i = blk * 32 + t;
          if (i < b) {
            const double wv = W ? (double)ws[i] : 1.0;
            pw += wv;
            px += (double)xs[i] * wv;
          }
        }
        S.b[tid + 1] = b; S.pw[tid + 1] = pw; S.px[tid + 1] = px;
      }
      __syncthreads();
      // the update; a cluster without points keeps its centre
      bool is_empty = false;
      if (tid < C) {
        const int n = S.b[tid + 1] - S.b[tid];
        const double cnt = S.pw[tid + 1] - S.pw[tid], tot = S.px[tid + 1] - S.px[tid];
        is_empty = n <= 0;
        S.cn[tid] = (n > 0 && cnt > 0.0) ? tot / cnt : S.cs[tid];
      }
      {
        const unsigned long long bal = __ballot(is_empty);
        if (tid == 0) S.flag_empty = (uint32_t)bal & 0xffffu;
      }
      __syncthreads();
      const uint32_t empties = S.flag_empty;
      if (empties != 0) {
        // the j-th empty cluster goes to the point with the j-th largest |x - centre| w (ties: the lower sorted position), while that is > 0
        double prev_e = __builtin_inf();
        int prev_p = -1;
        for (int j = 0; j < C; ++j) {
          if (!((empties >> j) & 1u)) continue;
          double be = -1.0;
          int bp = 0x7fffffff;
          for (int i = tid; i < k; i += KM_THREADS) {
            const int cl = km_cluster_of_pos(S.b, C, i);
            const double d = (double)xs[i] - S.cn[cl];
            const double e = __builtin_fabs(d) * (W ? (double)ws[i] : 1.0);
            const bool after = e < prev_e || (e == prev_e && i > prev_p);
            if (after && (e > be || (e == be && i < bp))) { be = e; bp = i; }
          }
          S.red_d[tid] = be; S.red_i[tid] = bp;
          __syncthreads();
          for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) {
              const double e2 = S.red_d[tid + h];
              const int p2 = S.red_i[tid + h];
              if (e2 > S.red_d[tid] || (e2 == S.red_d[tid] && p2 < S.red_i[tid])) { S.red_d[tid] = e2; S.red_i[tid] = p2; }
            }
            __syncthreads();
          }
          const double re = S.red_d[0];
          const int rp = S.red_i[0];
          __syncthreads();  // (red_* and cn[j] are free to be written again)
          if (!(re > 0.0)) break;  // uniform; the later ones are no larger
          if (tid == 0) S.cn[j] = (double)xs[min(max(rp, 0), k - 1)];
          prev_e = re; prev_p = rp;
        }
        __syncthreads();
      }
      bool mv = false;
      if (tid < C) mv = __builtin_fabs(S.cn[tid] - S.cs[tid]) > thr;
      {
        const unsigned long long bal = __ballot(mv);
        if (tid == 0) S.flag_moved = (uint32_t)bal & 0xffffu;
      }
      __syncthreads();
      ++total_iters;
      if (S.flag_moved == 0) break;  // uniform
    }
    // ---- this seeding's result: ascending centres, boundaries, weighted SSE over the sorted row ----
    sort_centres();
    if (tid < C) S.b[tid + 1] = tid < C - 1 ? upper_bound((S.cs[tid + 1] + S.cs[tid]) * 0.5) : k;
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < k; i += KM_THREADS) {
      const int cl = km_cluster_of_pos(S.b, C, i);
      const double d = (double)xs[i] - S.cs[cl];
      const double dd = d * d;
      const double t = dd * (W ? (double)ws[i] : 1.0);
      acc += t;
    }
    S.red_d[tid] = acc;
    __syncthreads();
    for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) S.red_d[tid] += S.red_d[tid + h];
      __syncthreads();
    }
    const double sse = S.red_d[0];
    if (s == 0 || sse < best_sse) {  // uniform; strictly smaller, in order
      best_sse = sse;
      if (tid < C) S.best[tid] = S.cs[tid];
    }
    __syncthreads();
  }

  // ---- outputs: one pass over the row in its original order ----
  if (tid < C - 1) S.mid[tid] = (S.best[tid + 1] + S.best[tid]) * 0.5;
  if (tid < C) P.centers[row * C + tid] = (float)S.best[tid];
  if (tid == 0) {
    if (P.sse) P.sse[row] = best_sse;
    if (P.iters) P.iters[row] = total_iters;
  }
  __syncthreads();
  int32_t* const arow = P.assign + row * (int64_t)k;
  for (int i = tid; i < k; i += KM_THREADS) arow[i] = km_cluster_of_value(S.mid, C, (double)xrow[i]);
}
