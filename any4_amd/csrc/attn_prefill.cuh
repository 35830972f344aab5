// attn_prefill.cuh -- prompt prefill for the decode stack (include/decode_glue_hip.h, DG_ATTN_PREFILL): a chunk of T new tokens per
// sequence is roped, appended to the static KV cache [bs][kvl][max_seq][D] and attended causally over cache + chunk.
//
// Two launches:
//   prefill_rope_kv_kernel   k_cache[b][kv][p0 + t] = rope(k), v_cache[...] = v in the arithmetic dg_rope_kv documents (two rounded
//                            products, a rounded sum, one rounding to 16 bit: decode._rope's bits; contraction into an FMA is switched off).
//   prefill_attn_kernel      flash attention over the cache.  A workgroup (4 waves, one per SIMD) owns BQ = 128 / RG query tokens of
//                            one (sequence, kv head) for RG of the hl / kvl query heads of that kv head, so a K / V tile is fetched once
//                            per group.  A wave holds two 16-row units (unit i of the workgroup: head i % RG, token sub-block i / RG); their q is roped on load
//                            and stays in registers as the B operand of v_mfma_f32_16x16x32.
//
// Per 64-position KV tile (double-buffered in LDS, one barrier per tile, the next tile's global loads in flight under the MFMAs):
//   S^T = K . Q^T        A = K rows from the XOR-swizzled row-major K image (b128 reads, conflict-free), B = q.  The result has the query
//                        row on the lane (col = lane & 15) and 4 of a 16-position block's scores in its registers (row = 4 (lane >> 4) + r),
//                        so the softmax row reductions are register-local plus two row swaps (lane ^ 16, lane ^ 32), no LDS.
//   online softmax       f32 scores and statistics; the running max / sum live once per lane per unit.
//   O^T += V^T . P^T     B = the probabilities straight from the score registers, rounded to 16 bit: k-slot j of lane group g is position
//                        32 ks + 16 (j >> 2) + 4 g + (j & 3), i.e. the registers of two score blocks side by side, no lane movement.
//                        A = V^T, which the staging pass writes transposed into LDS in exactly that position order (8-byte writes of four
//                        consecutive positions of one column, XOR-swizzled), so a fragment is one b128 read.
// KV tiles above a workgroup's last query position are never visited; inside the visited range a wave skips the tiles above the diagonal
// of all its units, and a unit masks only the tiles that straddle its diagonal.  Blocks are numbered so that the longest (last) query blocks are dispatched first.
//
// Positions: *pos = p0 is read on the device.  A token whose position p0 + t is outside [0, max_seq) writes no cache row, is read by
// nobody (every token only reads rows <= its own position) and leaves its output row unwritten; rows of a tile beyond the workgroup's
// last valid position are zero-filled in LDS instead of being read, so NaN-filled or unallocated tails are never touched.
//
// SEQ (DG_ATTN_SEQ): position, length and cache slot are per sequence, read by every workgroup: p0 = pos[i], T_i = min(len[i], T)
// decides which tokens exist (the padded T stays in the row addressing and sizes the grid), the cache base is slot[i]'s.  A sequence
// with T_i <= 0 or a slot outside [0, cache_bs) does nothing.  The SEQ = false instantiations read none of the three.
//
// PAGED (DG_ATTN_PAGED, with or without DG_ATTN_MX8; goes with SEQ): the caches are pools [num_pages][kvl][page_size][D] behind a block table
// (kv_paged.cuh) whose row is slot[i]'s.  A 64-position tile lies in one page (page_size >= 64), so the staging pass takes the tile's
// first row from its page (kv_unit_row) -- one scalar table read per tile, made when the tile's loads are issued, i.e. one tile ahead of
// its use -- and the rows stay tile-relative; the append drops a row whose own table entry is outside the pool.  Everything else is the
// SEQ flavour's.  With KV8 the four pools (codes [num_pages][kvl][page_size][D] bytes, exponents [...][D / 32] bytes) sit behind the one
// table: the same row, times D for the codes and times D / 32 for the exponents.
#pragma once
#include "stage_math.cuh"  // rope_mul_add: two rounded products, a rounded sum (contraction off)
#include "kv8.cuh"         // the mx8 cache format (KV8 flavours)
#include "kv_paged.cuh"    // the paged cache (PAGED flavours)

struct PrefillParams {
  const uint16_t* qkv;
  const float* cos;
  const float* sin;
  const int64_t* pos;
  uint16_t* k_cache;
  uint16_t* v_cache;
  uint16_t* out;
  int32_t bs, T, hl, kvl, max_seq;
  int32_t nqb;     // query blocks per (sequence, kv head, head group)
  int32_t hgroups; // ceil((hl / kvl) / RG)
  float scale;
};

// What only the SEQ kernels read: their LAST argument, and an empty one for SEQ = false, so that the scalar kernels keep the argument
// offsets (and with them the code) they had before there was a SEQ flavour.
struct PrefillSeq {
  const int64_t* len;   // [bs] or null: every length is T
  const int64_t* slot;  // [bs] or null: sequence i lives in cache slot i
  int32_t cache_bs;
};
template <bool SEQ> struct PrefillSeqArg {};
template <> struct PrefillSeqArg<true> : PrefillSeq {};

// (developer builds: -D'DG_SEQ_INDEX(i)=0', -D'DG_SEQ_LEN(p)=nullptr', -D'DG_SEQ_SLOT(p)=nullptr' give three wrong-on-purpose
// libraries -- every sequence at pos[0], len ignored, slot ignored -- to see tests/test_gpu_ragged.py fail; each still indexes only
// what the right one may index)
#ifndef DG_SEQ_INDEX
#define DG_SEQ_INDEX(i) (i)
#endif
#ifndef DG_SEQ_LEN
#define DG_SEQ_LEN(p) (p)
#endif
#ifndef DG_SEQ_SLOT
#define DG_SEQ_SLOT(p) (p)
#endif

// (p0, T_i, slot) of sequence i; false: the sequence does nothing
__device__ __forceinline__ bool pf_seq(const PrefillParams& P, const PrefillSeq& Q, int i, int64_t& p0, int& Ti, int& slot) {
  p0 = P.pos[DG_SEQ_INDEX(i)];
  const int64_t* lenp = DG_SEQ_LEN(Q.len);
  const int64_t* slotp = DG_SEQ_SLOT(Q.slot);
  const int64_t li = lenp ? lenp[i] : (int64_t)P.T, sl = slotp ? slotp[i] : (int64_t)i;
  Ti = (int)(li < P.T ? li : P.T);
  slot = (int)sl;
  return li > 0 && sl >= 0 && sl < Q.cache_bs;
}

// ---- rope + cache append: block = one token of one sequence; a thread walks (kv head, rotation pair) items, k first, then v ----
template <typename DT, bool SEQ = false, bool KV8 = false, bool PAGED = false>
__global__ void __launch_bounds__(256) prefill_rope_kv_kernel(PrefillParams P, int d, PrefillSeqArg<SEQ> Q, Kv8Arg<KV8> X, PagedArg<PAGED> G) {
  static_assert(!PAGED || SEQ, "a paged cache has a position per sequence");
  const int t = blockIdx.x, b = blockIdx.y, d2 = d >> 1;
  int cb = b;  // the sequence's cache slot
  int64_t pos;
  if constexpr (SEQ) {
    int64_t p0;
    int Ti;
    if (!pf_seq(P, Q, b, p0, Ti, cb) || t >= Ti || p0 < -(int64_t)P.T || p0 >= P.max_seq) return;
    pos = p0 + t;
  } else {
    pos = *P.pos + t;
  }
  if (pos < 0 || pos >= P.max_seq) return;  // never index the cache (or the tables) outside [0, max_seq)
  const uint16_t* row = P.qkv + ((int64_t)b * P.T + t) * (int64_t)(P.hl + 2 * P.kvl) * d;
  const int per = P.kvl * d2;
  // The destination row of kv head `kv` among the rows of the cache (PAGED: of the pool).  PAGED: (block-uniform) the row's own page is
  // looked up once; an entry outside the pool: nothing is written, neither rows, nor codes, nor exponents
  [[maybe_unused]] int page = 0;
  if constexpr (PAGED) {
    page = kv_page_write(G, cb, (int)pos);
    if (page < 0) return;
  }
  auto dst_row = [&](int kv) -> int64_t {
    if constexpr (PAGED) return kv_page_row(G, page, P.kvl, kv, (int)pos);
    else return kv_head_row(cb, P.kvl, kv, P.max_seq) + pos;
  };
  if constexpr (KV8) {
    // d / 2 is a multiple of 32 and 2 * per of 64: the waves of the loop are whole, and 32 aligned lanes hold the elements j of ONE 32-element
    // block and their rotation partners j + d / 2 of another -- a block maximum is a reduction over those lanes
    for (int i = threadIdx.x; i < 2 * per; i += 256) {
      const bool isv = i >= per;
      const int kv = (isv ? i - per : i) / d2, j = (isv ? i - per : i) % d2;
      const uint16_t* src = row + (int64_t)(P.hl + (isv ? P.kvl : 0) + kv) * d;
      float x1 = DT::to_f32(src[j]), x2 = DT::to_f32(src[j + d2]);
      if (!isv) {
        const float c1 = P.cos[pos * d + j], c2 = P.cos[pos * d + j + d2], s1 = P.sin[pos * d + j], s2 = P.sin[pos * d + j + d2];
        const float o1 = round16<DT>(rope_mul_add(x1, c1, -x2, s1)), o2 = round16<DT>(rope_mul_add(x2, c2, x1, s2));
        x1 = o1;
        x2 = o2;
      }
      uint32_t c1, e1, c2, e2;
      mx8_encode_lane(x1, c1, e1);
      mx8_encode_lane(x2, c2, e2);
      const int64_t r = dst_row(kv);
      uint8_t* dst = reinterpret_cast<uint8_t*>(isv ? P.v_cache : P.k_cache) + r * d;
      dst[j] = (uint8_t)c1;
      dst[j + d2] = (uint8_t)c2;
      if ((j & 31) == 0) {
        uint8_t* ed = (isv ? X.v_exp : X.k_exp) + r * (d >> 5);
        ed[j >> 5] = (uint8_t)e1;
        ed[(j + d2) >> 5] = (uint8_t)e2;
      }
    }
    return;
  }
  // (16-bit caches from here on)
  for (int i = threadIdx.x; i < 2 * per; i += 256) {
    const bool isv = i >= per;
    const int kv = (isv ? i - per : i) / d2, j = (isv ? i - per : i) % d2;
    const uint16_t* src = row + (int64_t)(P.hl + (isv ? P.kvl : 0) + kv) * d;
    uint16_t* dst = (isv ? P.v_cache : P.k_cache) + dst_row(kv) * d;
    if (isv) {
      dst[j] = src[j];
      dst[j + d2] = src[j + d2];
    } else {
      const float x1 = DT::to_f32(src[j]), x2 = DT::to_f32(src[j + d2]);
      const float c1 = P.cos[pos * d + j], c2 = P.cos[pos * d + j + d2], s1 = P.sin[pos * d + j], s2 = P.sin[pos * d + j + d2];
      dst[j] = DT::from_f32(rope_mul_add(x1, c1, -x2, s1));
      dst[j + d2] = DT::from_f32(rope_mul_add(x2, c2, x1, s2));
    }
  }
}

// 16-byte slot of (row, chunk) in the K image: the 16 lanes of a b128 read take 16 rows at one chunk -> 16 distinct slots of a 256-B window
template <int D>
__device__ __forceinline__ int pf_swz_k(int row, int chunk) {
  return D == 128 ? (chunk ^ (row & 15)) : (chunk ^ ((row >> 1) & 7));
}
// ... of (column d, 8-position chunk) in the V^T image (128-B rows: 8 chunks)
__device__ __forceinline__ int pf_swz_v(int d, int chunk) { return chunk ^ (((d >> 1) ^ (d >> 3)) & 7); }

constexpr int PF_NU = 2;  // 16-row units per wave: 2 x (O 4 D/16 + q D/8 + S 16) registers leave room for two workgroups per CU; 4 spill at D = 128

template <typename DT, int D, int RG, bool SEQ = false, bool KV8 = false, bool PAGED = false>
__global__ void __launch_bounds__(256) prefill_attn_kernel(PrefillParams P, PrefillSeqArg<SEQ> Q, Kv8Arg<KV8> X, PagedArg<PAGED> G) {
  static_assert(!PAGED || SEQ, "a paged cache has a position per sequence");
  constexpr int KD = D / 32;        // k-steps of the score product
  constexpr int DB = D / 16;        // 16-column blocks of the output
  constexpr int NU = PF_NU;         // 16-row units per wave
  constexpr int BQ = 16 * 4 * NU / RG;  // query tokens per workgroup (4 waves x NU units over RG heads)
  constexpr int CPR = D / 8;        // 16-byte chunks per K / V row
  constexpr int NCK = 64 * CPR / 256;  // K chunks staged per thread
  constexpr int KBYTES = 64 * D * 2, VBYTES = D * 128, BUF = KBYTES + VBYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  int64_t p0l;
  if constexpr (!SEQ) {
    p0l = *P.pos;
    if (p0l <= -(int64_t)P.T || p0l >= P.max_seq) return;  // no token of the chunk is inside the cache
  }
  int idx = blockIdx.x;
  const int per = P.bs * P.kvl * P.hgroups;
  const int qb = P.nqb - 1 - idx / per;  // longest blocks first
  idx %= per;
  const int hgi = idx % P.hgroups, kv = (idx / P.hgroups) % P.kvl, b = idx / (P.hgroups * P.kvl);
  const int rep = P.hl / P.kvl;
  const int tq0 = qb * BQ;
  int Tv = P.T, cb = b;  // tokens of this sequence that exist (T_i); its cache slot
  if constexpr (SEQ) {
    if (!pf_seq(P, Q, b, p0l, Tv, cb) || p0l <= -(int64_t)Tv || p0l >= P.max_seq || tq0 >= Tv) return;
  }
  const int p0 = (int)p0l;
  const int tend = tq0 + BQ < Tv ? tq0 + BQ : Tv;               // (tq0 < T by construction of the grid)
  const int p_hi = p0 + tend - 1 < P.max_seq - 1 ? p0 + tend - 1 : P.max_seq - 1;  // last valid position any row of this block may see
  if (p_hi < 0 || p0 + tq0 >= P.max_seq) return;
  const int ntiles = p_hi / 64 + 1;

  // ---- q: roped on load, rounded to 16 bit, kept as B fragments: lane (r, g) holds q[row r][32 kd + 8 g + 0..7]
  u32x4 qf[NU][KD];
  int pq[NU];        // position of this lane's query row per unit (INT32_MAX: no valid row, nothing is masked, nothing is stored)
  int tu0[NU];      // first token of the unit
  int64_t orow[NU];  // element offset of this lane's output row
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int hu = hgi * RG + (NU * w + u) % RG, tb = (NU * w + u) / RG;
    tu0[u] = tq0 + 16 * tb;
    const int t = tu0[u] + r, p = p0 + t;
    const bool ok = hu < rep && t < Tv && p >= 0 && p < P.max_seq;
    pq[u] = ok ? p : INT32_MAX;
    const int head = kv * rep + hu;
    orow[u] = ((int64_t)b * P.T + t) * (int64_t)P.hl * D + (int64_t)head * D;
    if (hu >= rep) tu0[u] = INT32_MAX / 2;  // a head beyond the group: the unit is never active
#pragma unroll
    for (int kd = 0; kd < KD; ++kd) qf[u][kd] = u32x4{0u, 0u, 0u, 0u};
    if (ok) {
      const uint16_t* src = P.qkv + ((int64_t)b * P.T + t) * (int64_t)(P.hl + 2 * P.kvl) * D + (int64_t)head * D;
#pragma unroll
      for (int kd = 0; kd < KD / 2; ++kd) {
        const int dl = 32 * kd + 8 * g;  // columns dl ... dl + 7 and their rotation partners dl + D / 2 ...
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src + dl);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src + dl + D / 2);
        float x1[8], x2[8], o1[8], o2[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x1[2 * e] = DT::lo_f32(lo[e]); x1[2 * e + 1] = DT::hi_f32(lo[e]);
          x2[2 * e] = DT::lo_f32(hi[e]); x2[2 * e + 1] = DT::hi_f32(hi[e]);
        }
        const float* cp = P.cos + (int64_t)p * D + dl;
        const float* sp = P.sin + (int64_t)p * D + dl;
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
        qf[u][kd] = u32x4{DT::pack2(o1[0], o1[1]), DT::pack2(o1[2], o1[3]), DT::pack2(o1[4], o1[5]), DT::pack2(o1[6], o1[7])};
        qf[u][kd + KD / 2] = u32x4{DT::pack2(o2[0], o2[1]), DT::pack2(o2[2], o2[3]), DT::pack2(o2[4], o2[5]), DT::pack2(o2[6], o2[7])};
      }
    }
  }

  // one base per cache or pool: the first byte of this (slot, kv head)'s rows; PAGED: the pool's, and stage_load adds the tile's
  constexpr int RB = KV8 ? D : D * 2;  // bytes of a row
  const int64_t head0 = PAGED ? (int64_t)0 : kv_head_row(cb, P.kvl, kv, P.max_seq);
  const char* Kg = reinterpret_cast<const char*>(P.k_cache) + head0 * RB;
  const char* Vg = reinterpret_cast<const char*>(P.v_cache) + head0 * RB;

  // ---- staging: K as 16-byte chunks (row, chunk); V as four consecutive positions 4 sg ... 4 sg + 3 of one 8-column chunk c
  // (KV8: a chunk is 8 bytes of codes in the first two dwords of its register slot, and its block's exponent byte is byte i of kexp / vexp)
  u32x4 kreg[NCK], vreg[4];
  u32x2 kreg8[NCK], vreg8[4];
  uint32_t kexp = 0u, vexp = 0u;
  const int vc = tid % CPR, vsg = tid / CPR;  // (D = 64: the threads with vsg >= 16 stage no V)
  auto stage_load = [&](int j) {
    const int s0 = 64 * j;
    // The tile's rows are rows r0, r0 + 1, ... of a unit of rows whose first row is row u behind the bases: the head's rows from s0 on;
    // PAGED: the tile itself, u its first row among the rows of the pool (s0 <= p_hi < max_seq; workgroup-uniform, one table read per
    // tile, made one tile ahead of its use) -- a 64-bit scalar, so that the rows stay 32-bit offsets
    int64_t u = 0;
    int r0 = s0;
    if constexpr (PAGED) {
      u = kv_unit_row(G, cb, P.kvl, kv, s0);
      r0 = 0;
    }
    const int64_t ub = u * RB;  // (added LAST: what stands in front of it does not change from tile to tile)
    using Off = std::conditional_t<PAGED, int, int64_t>;  // (the head's rows need 64-bit offsets, a tile's own rows do not)
    if constexpr (KV8) {
      const uint8_t *Ke = X.k_exp + (head0 + u) * (D / 32), *Ve = X.v_exp + (head0 + u) * (D / 32);
      kexp = vexp = 0u;  // (rows beyond p_hi: codes 0 with any exponent below 255 are the zero bits of the 16-bit flavour)
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int q = tid + 256 * i, row = q / CPR, ch = q % CPR;
        kreg8[i] = u32x2{0u, 0u};
        if (s0 + row <= p_hi) {
          kreg8[i] = *reinterpret_cast<const u32x2*>(Kg + (Off)(r0 + row) * D + ch * 8 + ub);
          kexp |= (uint32_t)Ke[(Off)(r0 + row) * (D / 32) + (ch >> 2)] << (8 * i);
        }
      }
      if (vsg < 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = 4 * vsg + i;
          vreg8[i] = u32x2{0u, 0u};
          if (s0 + row <= p_hi) {
            vreg8[i] = *reinterpret_cast<const u32x2*>(Vg + (Off)(r0 + row) * D + vc * 8 + ub);
            vexp |= (uint32_t)Ve[(Off)(r0 + row) * (D / 32) + (vc >> 2)] << (8 * i);
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int q = tid + 256 * i, row = q / CPR, ch = q % CPR;
        kreg[i] = u32x4{0u, 0u, 0u, 0u};
        if (s0 + row <= p_hi) kreg[i] = *reinterpret_cast<const u32x4*>(Kg + (Off)(r0 + row) * (D * 2) + ch * 16 + ub);
      }
      if (vsg < 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = 4 * vsg + i;
          vreg[i] = u32x4{0u, 0u, 0u, 0u};
          if (s0 + row <= p_hi) vreg[i] = *reinterpret_cast<const u32x4*>(Vg + (Off)(r0 + row) * (D * 2) + vc * 16 + ub);
        }
      }
    }
  };
  auto stage_write = [&](int buf) {
    char* kb = smem + buf * BUF;
    char* vb = kb + KBYTES;
    if constexpr (KV8) {  // the chunks become what the 16-bit flavour staged
#pragma unroll
      for (int i = 0; i < NCK; ++i) kreg[i] = mx8_to16<DT>(kreg8[i], (kexp >> (8 * i)) & 255u);
      if (vsg < 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) vreg[i] = mx8_to16<DT>(vreg8[i], (vexp >> (8 * i)) & 255u);
      }
    }
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int q = tid + 256 * i, row = q / CPR, ch = q % CPR;
      *reinterpret_cast<u32x4*>(kb + row * (D * 2) + pf_swz_k<D>(row, ch) * 16) = kreg[i];
    }
    if (vsg < 16) {
      // positions 4 vsg ... 4 vsg + 3 = 32 ks + 16 h + 4 gg + (0..3) sit at element 32 ks + 8 gg + 4 h of a V^T row (the order the P fragment has)
      const int ks = vsg >> 3, h = (vsg >> 2) & 1, gg = vsg & 3;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int dcol = 8 * vc + i, sh = 16 * (i & 1);
        const uint32_t e0 = (vreg[0][i >> 1] >> sh) & 0xffffu, e1 = (vreg[1][i >> 1] >> sh) & 0xffffu;
        const uint32_t e2 = (vreg[2][i >> 1] >> sh) & 0xffffu, e3 = (vreg[3][i >> 1] >> sh) & 0xffffu;
        *reinterpret_cast<u32x2*>(vb + dcol * 128 + pf_swz_v(dcol, 4 * ks + gg) * 16 + 8 * h) = u32x2{e0 | (e1 << 16), e2 | (e3 << 16)};
      }
    }
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

  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int j = 0; j < ntiles; ++j) {
    if (j + 1 < ntiles) stage_load(j + 1);
    const char* kb = smem + (j & 1) * BUF;
    const char* vb = kb + KBYTES;
    const int s0 = 64 * j;
    bool any = false;
#pragma unroll
    for (int u = 0; u < NU; ++u) any = any || (tu0[u] < Tv && s0 <= p0 + tu0[u] + 15);
    // (wave-uniform) the tile is not entirely above the diagonal of every unit of this wave; a unit it is above masks all of it
    if (any) {
      // ---- S^T = K . Q^T and the online softmax (two units share the K fragments); the probabilities become the B fragments of the
      // value product
      u32x4 pf[NU][2];
#pragma unroll
      for (int up = 0; up < NU; up += 2) {
        f32x4 S[2][4];
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int sb = 0; sb < 4; ++sb) S[v][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) {
          u32x4 kf[4];
#pragma unroll
          for (int sb = 0; sb < 4; ++sb) {
            const int row = 16 * sb + r;
            kf[sb] = *reinterpret_cast<const u32x4*>(kb + row * (D * 2) + pf_swz_k<D>(row, 4 * kd + g) * 16);
          }
#pragma unroll
          for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int sb = 0; sb < 4; ++sb) S[v][sb] = DT::mfma(kf[sb], qf[up + v][kd], S[v][sb]);
          __builtin_amdgcn_sched_barrier(0);  // (keeps the scheduler from hoisting every fragment read of the tile to the top: it spills)
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int u = up + v;
#pragma unroll
          for (int sb = 0; sb < 4; ++sb) S[v][sb] *= P.scale;
          if (s0 + 63 > p0 + tu0[u]) {  // (wave-uniform) some position of the tile is above some row of the unit: mask
#pragma unroll
            for (int sb = 0; sb < 4; ++sb)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (s0 + 16 * sb + 4 * g + i > pq[u]) S[v][sb][i] = -INFINITY;
          }
          float mx = -INFINITY;
#pragma unroll
          for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, S[v][sb][i]);
          mx = fmaxf(mx, tgl::lane_xor<16>(mx, lane));
          mx = fmaxf(mx, tgl::lane_xor<32>(mx, lane));
          const float mn = fmaxf(m[u], mx);
          const float ms = mn == -INFINITY ? 0.f : mn;  // (a row that has seen nothing yet: keep exp's arguments away from inf - inf)
          const float alpha = __expf(m[u] - ms);
          float sum = 0.f;
#pragma unroll
          for (int sb = 0; sb < 4; ++sb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float e = __expf(S[v][sb][i] - ms);
              S[v][sb][i] = e;
              sum += e;
            }
          sum += tgl::lane_xor<16>(sum, lane);
          sum += tgl::lane_xor<32>(sum, lane);
          l[u] = l[u] * alpha + sum;
          m[u] = mn;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            pf[u][ks] = u32x4{DT::pack2(S[v][2 * ks][0], S[v][2 * ks][1]), DT::pack2(S[v][2 * ks][2], S[v][2 * ks][3]),
                              DT::pack2(S[v][2 * ks + 1][0], S[v][2 * ks + 1][1]), DT::pack2(S[v][2 * ks + 1][2], S[v][2 * ks + 1][3])};
#pragma unroll
          for (int db = 0; db < DB; ++db) O[db][u] *= alpha;
        }
      }
      // ---- O^T += V^T . P^T
#pragma unroll
      for (int db = 0; db < DB; ++db) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int dcol = 16 * db + r;
          const u32x4 vf = *reinterpret_cast<const u32x4*>(vb + dcol * 128 + pf_swz_v(dcol, 4 * ks + g) * 16);
#pragma unroll
          for (int u = 0; u < NU; ++u) O[db][u] = DT::mfma(vf, pf[u][ks], O[db][u]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (j + 1 < ntiles) stage_write((j + 1) & 1);
    __syncthreads();
  }

  // ---- normalise once, one rounding, store: lane (r, g) holds columns 16 db + 4 g + 0..3 of its row
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if (pq[u] != INT32_MAX) {
      const float inv = 1.f / l[u];
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const f32x4 o = O[db][u] * inv;
        *reinterpret_cast<u32x2*>(P.out + orow[u] + 16 * db + 4 * g) = u32x2{DT::pack2(o[0], o[1]), DT::pack2(o[2], o[3])};
      }
    }
  }
}
