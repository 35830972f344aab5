// attn_verify.cuh -- the verify pass of speculative decoding (include/decode_glue_hip.h, dg_verify_attn): 1 ... 8 draft tokens per sequence
// are roped, appended to the contiguous 16-bit KV cache [cache_bs][kvl][max_seq][D] and attended causally over cache + chunk, in ONE
// launch whose grid splits the cached context.  The call is dg_prefill_attn_seq's (position, length and slot per sequence) and so are
// the rounding points (attn_prefill.cuh); the partition of the work is this kernel's own, made for a few query rows over a long cache.
//
// Rows       a workgroup (4 waves) serves one (sequence, kv head, group of RG = min(hl / kvl, 4) query heads): its query rows are
//            row j = t RG + hu (token t, head hu of the group), at most 8 x 4 = 32 = NU 16-row MFMA units.  EVERY wave holds all of them,
//            roped and rounded to 16 bit, as the B operand of v_mfma_f32_16x16x32 -- so no K / V tile is shared between waves.
// Split      grid (nsplit, kvl ceil((hl / kvl) / RG), n).  The cached range [0, pos_i) is cut into 64-position tiles; block x takes the
//            contiguous tiles [x tps, (x + 1) tps), tps = ceil(tiles / nsplit), and wave w of it the tiles w, w + 4, ... of that slice with a
//            (max, sum, O) state of its own.  No workgroup barrier in the loop.  A slice (or a wave's share) may be empty: max = -inf,
//            sum = 0, O = 0, which the combines weigh with 0.
// Tile       S^T = K . Q^T: the A operand is K, global -> VGPR in fragment order: lane (r, g) reads the 16 bytes [32 kd + 8 g, + 8) of
//            row 16 sb + r, every fetched byte is used.  The score of position 16 sb + 4 g + e and query row r lands in register e of
//            lane (r, g): softmax row reductions are register-local plus two row swaps (lane ^ 16, lane ^ 32).  O^T += V^T . P^T: B is
//            the probabilities straight from the score registers (rounded to 16 bit), A is V^T, which the wave stages through a
//            wave-private LDS region in exactly the position order those registers have (attn_prefill.cuh's V^T image: 8-byte writes of
//            four consecutive positions of one column, XOR-swizzled, one b128 read per fragment).  The next tile's K and V loads are
//            issued before the current tile's MFMAs.  Rows of a tile at or above pos_i are zero-filled, not read.
// Chunk      the chunk's own K / V rows come from qkv (K roped here: rope_mul_add, decode._rope's bits) as one 16-position pseudo-tile
//            under the causal and the length mask; wave 3 of block x = nsplit - 1 processes it, and where the head group is 0 -- exactly one
//            workgroup per (sequence, kv head) -- stores the rows to the cache.  Nothing the launch writes to the cache is read by it.
// Combine    the four waves meet through LDS behind one barrier (thread = 1 row x D / 8 columns, waves in order).  nsplit = 1: normalise
//            once, round once, store; the scratch is not touched.  nsplit > 1: the block's (max, sum, D values) per row goes to the
//            scratch with agent-scope stores, a counter per (sequence, kv head, head group) names the last block to arrive, and that block
//            sums the partials IN SPLIT ORDER and leaves the counter at zero (rope_attn_split_kernel's arrangement, decode_glue.cuh):
//            the same call gives the same bits, and a captured launch replays.
// Guards     pos / len / slot as in pf_seq (attn_prefill.cuh): token t exists iff t < min(len_i, T) and 0 <= pos_i + t < max_seq; a token
//            that does not exist writes no cache row and no output row, and is seen by nobody.  len_i <= 0, a slot outside [0, cache_bs)
//            or no existing token: every block of the sequence returns at once (the counters stay untouched).  Whatever the three hold,
//            nothing outside the caches is indexed.
#pragma once
#include "stage_math.cuh"  // rope_mul_add: two rounded products, a rounded sum (contraction off)

struct VerifyParams {
  const uint16_t* qkv;
  const float* cos;
  const float* sin;
  const int64_t* pos;
  const int64_t* len;   // [n] or null: every length is T
  const int64_t* slot;  // [n] or null: sequence i lives in cache slot i
  uint16_t* k_cache;
  uint16_t* v_cache;
  uint16_t* out;
  int* counters;        // nsplit > 1: one per (sequence, kv head, head group), zero between launches
  float* part;          // nsplit > 1: [(i T + t) hl + head][nsplit][max, sum, D values]
  int32_t T, hl, kvl, max_seq, cache_bs;
  int32_t RG;           // query heads of a kv head per workgroup: min(hl / kvl, 4)
  int32_t hgroups;      // ceil((hl / kvl) / RG)
  int32_t nsplit;
  float scale;
};

// 16-byte slot of (column d, 8-position chunk) in the V^T image (128-byte rows: 8 chunks)
__device__ __forceinline__ int vf_swz_v(int d, int chunk) { return chunk ^ (((d >> 1) ^ (d >> 3)) & 7); }

// One 16-bit row of D elements at `src`, roped at position p and rounded to 16 bit, as the fragments of lane group g: f[kd] holds columns
// 32 kd + 8 g ... + 7 (a rotation pair j, j + D / 2 lies in the fragments kd and kd + D / 64 of the same lane)
template <typename DT, int D>
__device__ __forceinline__ void vf_rope_row(const uint16_t* src, const float* cos, const float* sin, int p, int g, u32x4 (&f)[D / 32]) {
  constexpr int KD = D / 32;
#pragma unroll
  for (int kd = 0; kd < KD / 2; ++kd) {
    const int dl = 32 * kd + 8 * g;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(src + dl);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(src + dl + D / 2);
    float x1[8], x2[8], o1[8], o2[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x1[2 * e] = DT::lo_f32(lo[e]); x1[2 * e + 1] = DT::hi_f32(lo[e]);
      x2[2 * e] = DT::lo_f32(hi[e]); x2[2 * e + 1] = DT::hi_f32(hi[e]);
    }
    const float* cp = cos + (int64_t)p * D + dl;
    const float* sp = sin + (int64_t)p * D + dl;
#pragma unroll
    for (int e = 0; e < 8; e += 4) {
      const f32x4 c1 = *reinterpret_cast<const f32x4*>(cp + e), c2 = *reinterpret_cast<const f32x4*>(cp + D / 2 + e);
      const f32x4 s1 = *reinterpret_cast<const f32x4*>(sp + e), s2 = *reinterpret_cast<const f32x4*>(sp + D / 2 + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // the cache rows' arithmetic: each product and the sum rounded separately
        o1[e + i] = rope_mul_add(x1[e + i], c1[i], -x2[e + i], s1[i]);
        o2[e + i] = rope_mul_add(x2[e + i], c2[i], x1[e + i], s2[i]);
      }
    }
    f[kd] = u32x4{DT::pack2(o1[0], o1[1]), DT::pack2(o1[2], o1[3]), DT::pack2(o1[4], o1[5]), DT::pack2(o1[6], o1[7])};
    f[kd + KD / 2] = u32x4{DT::pack2(o2[0], o2[1]), DT::pack2(o2[2], o2[3]), DT::pack2(o2[4], o2[5]), DT::pack2(o2[6], o2[7])};
  }
}

// dynamic LDS of a launch: the four V^T images, the four waves' states [4][16 NU][D + 4] floats, the "last block" word
template <int D, int NU>
constexpr int verify_lds_bytes() { return 4 * D * 128 + 4 * 16 * NU * (D + 4) * 4 + 16; }

template <typename DT, int D, int NU>
__global__ void __launch_bounds__(256) verify_attn_kernel(VerifyParams P) {
  constexpr int KD = D / 32;           // k-steps of the score product
  constexpr int DB = D / 16;           // 16-column blocks of the output
  constexpr int CPR = D / 8;           // 16-byte chunks per K / V row
  constexpr int NVP = 16 * CPR / 64;   // passes of a wave over the (4-row group, chunk) items of a V tile
  constexpr int VBYTES = D * 128;      // a V^T image: D columns x 64 positions
  constexpr int NR = 16 * NU;          // query rows of the workgroup
  constexpr int OST = D + 4;           // floats per row of a wave's state in LDS: D of O, max, sum (rows stay 16-byte aligned)
  constexpr int CT = D / 8;            // columns per thread in the combine
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int x = blockIdx.x, i = blockIdx.z;
  const int hgi = blockIdx.y % P.hgroups, kv = blockIdx.y / P.hgroups;
  const int rep = P.hl / P.kvl, RG = P.RG;
  const int64_t W = (int64_t)(P.hl + 2 * P.kvl) * D;  // elements of a qkv row

  // ---- the sequence: every block of it takes the same decision here
  const int64_t p0l = P.pos[i];
  const int64_t li = P.len ? P.len[i] : (int64_t)P.T, sl = P.slot ? P.slot[i] : (int64_t)i;
  const int Tv = (int)(li < P.T ? li : P.T);
  if (li <= 0 || sl < 0 || sl >= P.cache_bs || p0l <= -(int64_t)Tv || p0l >= P.max_seq) return;
  const int p0 = (int)p0l;
  const int Pc = p0 > 0 ? p0 : 0;                                    // the cached range is [0, Pc), Pc < max_seq
  const int c_lo = p0 < 0 ? -p0 : 0;                                 // chunk tokens [c_lo, c_hi) exist (c_lo < c_hi <= 8)
  const int c_hi = Tv < P.max_seq - p0 ? Tv : P.max_seq - p0;
  const int64_t head0 = ((int64_t)sl * P.kvl + kv) * P.max_seq;      // first row of (slot, kv head) among the rows of a cache
  const char* Kg = reinterpret_cast<const char*>(P.k_cache) + head0 * (D * 2);
  const char* Vg = reinterpret_cast<const char*>(P.v_cache) + head0 * (D * 2);

  // row j of the workgroup -> (token, query head); false: no such row, nothing of it is stored
  auto row_of = [&](int j, int& t, int& head) -> bool {
    t = j / RG;
    const int hu = hgi * RG + j % RG;
    head = kv * rep + hu;
    return hu < rep && t >= c_lo && t < c_hi;
  };

  // ---- q: roped on load, rounded to 16 bit, kept as B fragments: lane (r, g) holds q[row 16 u + r][32 kd + 8 g + 0..7]
  u32x4 qf[NU][KD];
  int tq[NU];  // token of this lane's query row per unit (-1: no such row: it sees nothing of the chunk)
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    int t, head;
    const bool ok = row_of(16 * u + r, t, head);
    tq[u] = ok ? t : -1;
#pragma unroll
    for (int kd = 0; kd < KD; ++kd) qf[u][kd] = u32x4{0u, 0u, 0u, 0u};
    if (ok) vf_rope_row<DT, D>(P.qkv + ((int64_t)i * P.T + t) * W + (int64_t)head * D, P.cos, P.sin, p0 + t, g, qf[u]);
  }

  // ---- this block's slice of the cached tiles, this wave's tiles of it
  const int ntiles = (Pc + 63) >> 6;
  const int tps = (ntiles + P.nsplit - 1) / P.nsplit;
  const int tlo = x * tps, thi = tlo + tps < ntiles ? tlo + tps : ntiles;

  char* vb = smem + w * VBYTES;  // wave-private
  auto load_k = [&](int s0, u32x4 (&kf)[4][KD]) {
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const int row = s0 + 16 * sb + r;
#pragma unroll
      for (int kd = 0; kd < KD; ++kd) {
        kf[sb][kd] = u32x4{0u, 0u, 0u, 0u};
        if (row < Pc) kf[sb][kd] = *reinterpret_cast<const u32x4*>(Kg + (int64_t)row * (D * 2) + (32 * kd + 8 * g) * 2);
      }
    }
  };
  // V: item q = lane + 64 pass is (chunk vc = q % CPR, rows 4 vsg ... 4 vsg + 3 with vsg = q / CPR < 16)
  auto load_v = [&](int s0, u32x4 (&vr)[NVP][4]) {
#pragma unroll
    for (int ps = 0; ps < NVP; ++ps) {
      const int q = lane + 64 * ps, vc = q % CPR, vsg = q / CPR;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = s0 + 4 * vsg + e;
        vr[ps][e] = u32x4{0u, 0u, 0u, 0u};
        if (row < Pc) vr[ps][e] = *reinterpret_cast<const u32x4*>(Vg + (int64_t)row * (D * 2) + vc * 16);
      }
    }
  };
  // positions 4 vsg ... 4 vsg + 3 = 32 ks + 16 h + 4 gg + (0..3) sit at element 32 ks + 8 gg + 4 h of a V^T row (the order the P fragment has)
  auto write_v = [&](const u32x4 (&vr)[NVP][4]) {
#pragma unroll
    for (int ps = 0; ps < NVP; ++ps) {
      const int q = lane + 64 * ps, vc = q % CPR, vsg = q / CPR;
      const int ks = vsg >> 3, h = (vsg >> 2) & 1, gg = vsg & 3;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int dcol = 8 * vc + e, sh = 16 * (e & 1);
        const uint32_t e0 = (vr[ps][0][e >> 1] >> sh) & 0xffffu, e1 = (vr[ps][1][e >> 1] >> sh) & 0xffffu;
        const uint32_t e2 = (vr[ps][2][e >> 1] >> sh) & 0xffffu, e3 = (vr[ps][3][e >> 1] >> sh) & 0xffffu;
        *reinterpret_cast<u32x2*>(vb + dcol * 128 + vf_swz_v(dcol, 4 * ks + gg) * 16 + 8 * h) = u32x2{e0 | (e1 << 16), e2 | (e3 << 16)};
      }
    }
  };
  // the lanes of a wave exchange V through LDS: its writes are ordered in front of its reads, and its reads in front of the next tile's writes
  auto wave_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };

  f32x4 O[DB][NU];
  float m[NU], l[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    m[u] = -INFINITY;
    l[u] = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db) O[db][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // One tile in two halves -- scores: kf its K fragments, pf the probabilities as B fragments; values: its V^T image in `vb`.  chunk: the 16-position pseudo-tile of the chunk's own tokens (column c of
  // score block 0 is token c, visible to a row of token t iff c_lo <= c <= t); else the cached tile at s0 (visible iff s0 + c < Pc)
  auto scores = [&](const u32x4 (&kf)[4][KD], bool chunk, int s0, u32x4 (&pf)[NU][2]) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      f32x4 S[4];
#pragma unroll
      for (int sb = 0; sb < 4; ++sb) S[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kd = 0; kd < KD; ++kd)
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) S[sb] = DT::mfma(kf[sb][kd], qf[u][kd], S[sb]);
#pragma unroll
      for (int sb = 0; sb < 4; ++sb) S[sb] *= P.scale;
      if (chunk || s0 + 64 > Pc) {  // (wave-uniform)
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = 16 * sb + 4 * g + e;
            const bool vis = chunk ? (c >= c_lo && c <= tq[u]) : (s0 + c < Pc);
            if (!vis) S[sb][e] = -INFINITY;
          }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, S[sb][e]);
      mx = fmaxf(mx, tgl::lane_xor<16>(mx, lane));
      mx = fmaxf(mx, tgl::lane_xor<32>(mx, lane));
      const float mn = fmaxf(m[u], mx);
      const float ms = mn == -INFINITY ? 0.f : mn;  // (a row that has seen nothing yet: keep exp's arguments away from inf - inf)
      const float alpha = __expf(m[u] - ms);
      float sum = 0.f;
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pe = __expf(S[sb][e] - ms);
          S[sb][e] = pe;
          sum += pe;
        }
      sum += tgl::lane_xor<16>(sum, lane);
      sum += tgl::lane_xor<32>(sum, lane);
      l[u] = l[u] * alpha + sum;
      m[u] = mn;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        pf[u][ks] = u32x4{DT::pack2(S[2 * ks][0], S[2 * ks][1]), DT::pack2(S[2 * ks][2], S[2 * ks][3]),
                          DT::pack2(S[2 * ks + 1][0], S[2 * ks + 1][1]), DT::pack2(S[2 * ks + 1][2], S[2 * ks + 1][3])};
#pragma unroll
      for (int db = 0; db < DB; ++db) O[db][u] *= alpha;
    }
  };
  // O^T += V^T . P^T
  auto values = [&](const u32x4 (&pf)[NU][2]) {
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int dcol = 16 * db + r;
        const u32x4 vf = *reinterpret_cast<const u32x4*>(vb + dcol * 128 + vf_swz_v(dcol, 4 * ks + g) * 16);
#pragma unroll
        for (int u = 0; u < NU; ++u) O[db][u] = DT::mfma(vf, pf[u][ks], O[db][u]);
      }
      __builtin_amdgcn_sched_barrier(0);  // (keeps the scheduler from hoisting every fragment read of the tile to the top: it spills)
    }
  };

  // ---- the cached tiles of this wave: the next tile's loads are in flight under the current tile's MFMAs
  {
    u32x4 kc[4][KD], vc[NVP][4];
    int j = tlo + w;
    if (j < thi) {
      load_k(64 * j, kc);
      load_v(64 * j, vc);
    }
    for (; j < thi; j += 4) {
      write_v(vc);
      const bool more = j + 4 < thi;  // (wave-uniform)
      u32x4 kn[4][KD], pf[NU][2];
      if (more) load_k(64 * (j + 4), kn);
      wave_sync();
      scores(kc, false, 64 * j, pf);
      __builtin_amdgcn_sched_barrier(0);  // (the next V is requested once the current K fragments are dead: its registers are theirs)
      if (more) load_v(64 * (j + 4), vc);
      values(pf);
      wave_sync();
      if (more) {
#pragma unroll
        for (int sb = 0; sb < 4; ++sb)
#pragma unroll
          for (int kd = 0; kd < KD; ++kd) kc[sb][kd] = kn[sb][kd];
      }
    }
  }

  // ---- the chunk's own tokens: K roped from qkv (lane (r, g): token r), V raw; head group 0 appends both to the cache
  if (x == P.nsplit - 1 && w == 3) {
    u32x4 kq[4][KD], vq[NVP][4];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int kd = 0; kd < KD; ++kd) kq[sb][kd] = u32x4{0u, 0u, 0u, 0u};
    const bool mine = r >= c_lo && r < c_hi;
    if (mine) vf_rope_row<DT, D>(P.qkv + ((int64_t)i * P.T + r) * W + (int64_t)(P.hl + kv) * D, P.cos, P.sin, p0 + r, g, kq[0]);
#pragma unroll
    for (int ps = 0; ps < NVP; ++ps) {
      const int q = lane + 64 * ps, vc = q % CPR, vsg = q / CPR;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * vsg + e;
        vq[ps][e] = u32x4{0u, 0u, 0u, 0u};
        if (c >= c_lo && c < c_hi)
          vq[ps][e] = *reinterpret_cast<const u32x4*>(P.qkv + ((int64_t)i * P.T + c) * W + (int64_t)(P.hl + P.kvl + kv) * D + vc * 8);
      }
    }
    if (hgi == 0) {  // rows p0 + c with c_lo <= c < c_hi: inside [0, max_seq) of the slot's head
      char* Kw = reinterpret_cast<char*>(P.k_cache) + head0 * (D * 2);
      char* Vw = reinterpret_cast<char*>(P.v_cache) + head0 * (D * 2);
      if (mine) {
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) *reinterpret_cast<u32x4*>(Kw + (int64_t)(p0 + r) * (D * 2) + (32 * kd + 8 * g) * 2) = kq[0][kd];
      }
#pragma unroll
      for (int ps = 0; ps < NVP; ++ps) {
        const int q = lane + 64 * ps, vc = q % CPR, vsg = q / CPR;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * vsg + e;
          if (c >= c_lo && c < c_hi) *reinterpret_cast<u32x4*>(Vw + (int64_t)(p0 + c) * (D * 2) + vc * 16) = vq[ps][e];
        }
      }
    }
    u32x4 pf[NU][2];
    write_v(vq);
    wave_sync();
    scores(kq, true, 0, pf);
    values(pf);
  }

  // ---- the four waves meet: lane (r, g) holds columns 16 db + 4 g + 0..3 of row 16 u + r
  float* so = reinterpret_cast<float*>(smem + 4 * VBYTES);
  int* s_last = reinterpret_cast<int*>(smem + 4 * VBYTES + 4 * NR * OST * 4);
  {
    float* mine = so + w * NR * OST;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      float* row = mine + (16 * u + r) * OST;
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(row + 16 * db + 4 * g) = O[db][u];
      if (g == 0) {
        row[D] = m[u];
        row[D + 1] = l[u];
      }
    }
  }
  __syncthreads();
  const int row = tid >> 3, c0 = (tid & 7) * CT;  // this thread's row and first column
  int t = 0, head = 0;
  const bool ok = row < NR && row_of(row, t, head);
  float M = -INFINITY, L = 0.f, o[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) o[c] = 0.f;
  if (row < NR) {
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) M = fmaxf(M, so[(wv * NR + row) * OST + D]);
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      const float* sr = so + (wv * NR + row) * OST;
      const float wt = sr[D] == -INFINITY ? 0.f : __expf(sr[D] - M);  // (a wave without a tile, a row that saw nothing)
      L += wt * sr[D + 1];
#pragma unroll
      for (int c = 0; c < CT; ++c) o[c] += wt * sr[c0 + c];
    }
  }
  // normalise once, one rounding, store
  auto store_row = [&](float den) {
    const float inv = 1.f / den;
    uint16_t* dst = P.out + ((int64_t)i * P.T + t) * (int64_t)P.hl * D + (int64_t)head * D + c0;
#pragma unroll
    for (int c = 0; c < CT; c += 8)
      *reinterpret_cast<u32x4*>(dst + c) = u32x4{DT::pack2(o[c] * inv, o[c + 1] * inv), DT::pack2(o[c + 2] * inv, o[c + 3] * inv),
                                                 DT::pack2(o[c + 4] * inv, o[c + 5] * inv), DT::pack2(o[c + 6] * inv, o[c + 7] * inv)};
  };
  if (P.nsplit == 1) {  // (uniform over the launch)
    if (ok) store_row(L);
    return;
  }
  // ---- across blocks: what crosses goes through agent-scope atomics (no device-scope fence: rope_attn_split_kernel says why); a thread's
  // stores are complete before thread 0 counts the block in, and the last block to arrive reads every partial
  const int NS = P.nsplit;
  const int grp = (i * P.kvl + kv) * P.hgroups + hgi;
  float* base = P.part + (((int64_t)i * P.T + t) * P.hl + head) * (int64_t)NS * (D + 2);
  if (ok) {
    float* mp = base + (int64_t)x * (D + 2);
#pragma unroll
    for (int c = 0; c < CT; ++c) __hip_atomic_store(mp + 2 + c0 + c, o[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((tid & 7) == 0) {
      __hip_atomic_store(mp, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mp + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (tid == 0) *s_last = __hip_atomic_fetch_add(&P.counters[grp], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == NS - 1;
  __syncthreads();
  if (*s_last) {
    if (ok) {
      float M2 = -INFINITY;
      for (int s = 0; s < NS; ++s) M2 = fmaxf(M2, __hip_atomic_load(base + s * (D + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      float L2 = 0.f;
#pragma unroll
      for (int c = 0; c < CT; ++c) o[c] = 0.f;
      for (int s = 0; s < NS; ++s) {
        const float* sp = base + s * (D + 2);
        const float mi = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float wt = mi == -INFINITY ? 0.f : __expf(mi - M2);
        L2 += wt * __hip_atomic_load(sp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int c = 0; c < CT; ++c) o[c] += wt * __hip_atomic_load(sp + 2 + c0 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      store_row(L2);
    }
    if (tid == 0) __hip_atomic_store(&P.counters[grp], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch / graph replay
  }
}
