// moe_grouped.cuh -- mixture-of-experts PREFILL (dg_moe_group / dg_moe_launch's DG_MOE_GROUPED, include/decode_glue_hip.h): what the grouped
// flavour of w4_gemm_tile_kernel (w4_gemm_tile.cuh, template parameter GRP) needs around it.  Included inside tg_moe_tile.hip's anonymous
// namespace, behind moe_call.cuh (the group workspace's layout: MG_*).  The definition is any4_amd/moe.py: moe_grouped_ref; the group
// workspace's is group_ref.
//
//   GroupedTileParams    the tile kernel's parameter block for GRP != 0: TileParams' fields under their names, the experts' strides, the
//                        group workspace and where perm / invalid / tiles start in it.
//   moe_group_kernel     ONE workgroup: a stable counting sort of the pairs p = i top_k + s by expert, without atomics.  Thread t owns the
//                        pairs [t chunk, (t + 1) chunk) and counts them per expert into its own column of hist[E + 1][T] in LDS (bucket E =
//                        ids outside [0, E): never an address); thread b then turns row b into the exclusive prefix over threads, thread 0
//                        the totals into offsets and tile starts; every thread walks its chunk again and writes pair p at
//                        offset[e] + hist[e][t]++.  Order within an expert = (thread, position in the chunk) = pair index: stable.  The
//                        unused tails of perm / invalid are -1 and those of the tile list 0, so the same ids give the same bytes.
//   moe_combine_kernel   y[i] = RNE16(sum_s gates[i][s] d[i top_k + s] (+ residual[i])) from the f32 rows the DOWN tiles stored: a thread
//                        owns four columns of one row, picks its row's valid slots in (expert id, slot) order and chains fused
//                        multiply-adds from 0, the residual last (moe_w4_kernel's DOWN order).  The row of a pair without a valid id is
//                        never read (the workspace is not cleared).  y may be residual: a thread reads its four elements, then writes them.

struct GroupedTileParams {
  const char* x;       // GRP 1: [m][k]; GRP 2: [m top_k][k] 16-bit
  const char* w;       // [E] x stride_w
  const char* qinfo;
  const char* lut;
  char* y;             // GRP 1: [m top_k][wrows / 2] 16-bit
  const char* bias;    // (unused)
  int32_t m, wrows, k, ksuper, gshift, qtype;
  int32_t tiles_m, tiles_n;   // tiles_m = the BOUND of the tile list's length (the grid's m-extent); the list's length is grp[0]
  int32_t splits;      // 0
  float* part;         // GRP 2: d [m top_k][wrows] f32
  int64_t x_pitch;
  const int32_t* grp;  // the group workspace
  int64_t stride_w, stride_qinfo, stride_lut;
  int32_t top_k, perm_off, inv_off, tiles_off;   // offsets in int32 units
};

struct MoeGroupParams {
  const int32_t* ids;  // [P]
  int32_t* ws;         // the group workspace
  int32_t P, E, BM, bound;
};

__global__ void __launch_bounds__(MG_THREADS) moe_group_kernel(const MoeGroupParams prm) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int T = MG_THREADS;
  const int32_t* __restrict__ ids = prm.ids;
  int32_t* __restrict__ ws = prm.ws;
  const int P = prm.P, E = prm.E, BM = prm.BM, bound = prm.bound;
  int32_t* hist = reinterpret_cast<int32_t*>(lds);   // [E + 1][T]
  int32_t* tot = hist + (E + 1) * T;                 // [E + 1]
  int32_t* off = tot + (E + 1);                      // [E + 1]
  int32_t* tstart = off + (E + 1);                   // [E + 1]
  const int tid = threadIdx.x;
  const int chunk = (P + T - 1) / T;
  const int p0 = min(tid * chunk, P), p1 = min(p0 + chunk, P);
  auto bucket = [&](int id) { return id >= 0 && id < E ? id : E; };   // the only use of an id
  for (int b = 0; b <= E; ++b) hist[b * T + tid] = 0;
  for (int p = p0; p < p1; ++p) hist[bucket(ids[p]) * T + tid] += 1;   // (own column)
  __syncthreads();
  if (tid <= E) {
    int s = 0;
    for (int t = 0; t < T; ++t) {
      const int v = hist[tid * T + t];
      hist[tid * T + t] = s;
      s += v;
    }
    tot[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0, ts = 0;
    for (int e = 0; e < E; ++e) {
      off[e] = o;
      tstart[e] = ts;
      o += tot[e];
      ts += (tot[e] + BM - 1) / BM;
    }
    off[E] = o;
    tstart[E] = ts;
  }
  __syncthreads();
  const int n_valid = off[E], n_inv = tot[E], n_tiles = tstart[E];
  if (tid == 0) {
    ws[MG_HDR + 0] = n_tiles;
    ws[MG_HDR + 1] = n_inv;
    ws[MG_HDR + 2] = n_valid;
    ws[MG_HDR + 3] = BM;
  }
  if (tid < 64) ws[MG_COUNT + tid] = tid < E ? tot[tid] : 0;
  if (tid < 68) ws[MG_OFFSET + tid] = tid <= E ? off[tid] : 0;
  int32_t* perm = ws + MG_PERM;
  int32_t* inv = perm + P;
  int32_t* tiles = inv + P;
  for (int p = p0; p < p1; ++p) {
    const int b = bucket(ids[p]);
    const int r = hist[b * T + tid]++;
    if (b < E) perm[off[b] + r] = p;
    else inv[r] = p;
  }
  for (int j = n_valid + tid; j < P; j += T) perm[j] = -1;
  for (int j = n_inv + tid; j < P; j += T) inv[j] = -1;
  for (int e = tid; e < E; e += T) {
    const int c = tot[e];
    for (int t = 0; t * BM < c; ++t) {
      int32_t* te = tiles + 3 * (tstart[e] + t);
      te[0] = e;
      te[1] = off[e] + t * BM;
      te[2] = min(BM, c - t * BM);
    }
  }
  for (int j = 3 * n_tiles + tid; j < 3 * bound; j += T) tiles[j] = 0;
}

struct MoeCombineParams {
  const float* d;        // [m top_k][wrows]
  const int32_t* ids;    // [m][top_k]
  const float* gates;    // [m][top_k]
  const char* residual;  // [m][wrows] 16-bit or nullptr
  char* y;               // [m][wrows] 16-bit
  int32_t m, top_k, E, wrows;
};

template <typename DT>
__global__ void __launch_bounds__(256) moe_combine_kernel(const MoeCombineParams P) {
  const int quads = P.wrows >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)P.m * quads) return;
  const int i = (int)(t / quads), c = (int)(t - (int64_t)i * quads) * 4;
  int key[MOE_MAX_TOPK];
#pragma unroll
  for (int s = 0; s < MOE_MAX_TOPK; ++s) {
    key[s] = INT32_MAX;
    if (s < P.top_k) {
      const int id = P.ids[(int64_t)i * P.top_k + s];
      if (id >= 0 && id < P.E) key[s] = id * MOE_MAX_TOPK + s;   // (expert ascending, then slot ascending)
    }
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int lastk = -1;
  for (int r = 0; r < P.top_k; ++r) {
    int best = INT32_MAX;
#pragma unroll
    for (int s = 0; s < MOE_MAX_TOPK; ++s) best = key[s] > lastk && key[s] < best ? key[s] : best;
    if (best == INT32_MAX) break;
    lastk = best;
    const int64_t pr = (int64_t)i * P.top_k + (best & (MOE_MAX_TOPK - 1));
    const float g = P.gates[pr];
    const f32x4 dv = *reinterpret_cast<const f32x4*>(P.d + pr * P.wrows + c);
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] = __builtin_fmaf(g, dv[v], acc[v]);
  }
  const int64_t o = (int64_t)i * P.wrows + c;
  if (P.residual) {
    const u32x2 rv = *reinterpret_cast<const u32x2*>(P.residual + o * 2);
    acc[0] += DT::lo_f32(rv[0]); acc[1] += DT::hi_f32(rv[0]); acc[2] += DT::lo_f32(rv[1]); acc[3] += DT::hi_f32(rv[1]);
  }
  const u32x2 out = {DT::pack2(acc[0], acc[1]), DT::pack2(acc[2], acc[3])};
  *reinterpret_cast<u32x2*>(P.y + o * 2) = out;
}
