// tg_convert.cuh -- the layout kernels behind the tg_convert_* / tg_unpack_int4 / tg_dequant_* entry points: int4 and int8 packers, the
// unpacker, the 16-bit fragment-order converters and the dequantisers (reference TinyGemmConvert{A,B}.cu, TinyGemmDequantize.cu;
// included by tinygemm_hip.hip).
#pragma once

// ---- packing kernels (integer only, bit-exact) -----------------------------------------------
// One workgroup stages a [ROWS x KB] tile of codes as bytes in LDS with fully coalesced 16-byte
// reads of the int32 input, then every thread assembles output words from four 2-byte LDS reads
// and writes them contiguously (the packed tile is contiguous in the output tensor).

// Bint4: tile = 8 rows (one n-tile) x KB k.   ref TinyGemmConvertB.cu:252-308
template <int I>
__global__ void __launch_bounds__(256) pack_Bint4_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        int64_t n, int64_t k, int64_t ksuper) {
  constexpr int KB = 512;  // k per workgroup; multiple of 16*I for I <= 8
  // codes are staged as full 32-bit values: the reference ORs the shifted UNMASKED inputs (TinyGemmConvertB.cu:302-303),
  // so out-of-range codes must reach the pack expression untouched for the words to stay bit-identical
  __shared__ uint32_t s_codes[8][KB + 4];
  const int tid = threadIdx.x;
  const int64_t nT = blockIdx.y;
  const int64_t kb0 = (int64_t)blockIdx.x * KB;
  // load: 8 rows x 512 ints = 1024 x int4
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * 256 + tid;
    const int rr = idx >> 7, c4 = idx & 127;
    const int64_t row = nT * 8 + rr, kk = kb0 + c4 * 4;
    int4 v = {0, 0, 0, 0};
    if (row < n && kk < k) v = *reinterpret_cast<const int4*>(in + row * k + kk);  // k % 32 == 0 -> whole int4 in range
    *reinterpret_cast<int4*>(&s_codes[rr][c4 * 4]) = v;
  }
  __syncthreads();
  // words of this tile: [kS_local][t][j], KB/(16 I) super-tiles x 32 x I/2 = KB words
  constexpr int WORDS = KB;  // 8 rows * KB / 8
#pragma unroll
  for (int it = 0; it < WORDS / 256; ++it) {
    const int wi = it * 256 + tid;
    const int j = wi % (I / 2);
    const int t = (wi / (I / 2)) & 31;
    const int ksl = wi / (16 * I);
    const int64_t ks = kb0 / (16 * I) + ksl;
    if (ks >= ksuper) continue;
    const int rr = t >> 2, q = t & 3;
    const int kl = (ksl * I + 2 * j) * 16 + 2 * q;
    const uint32_t* src = &s_codes[rr][kl];
    uint32_t v[8];
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      v[2 * pr] = src[8 * pr];
      v[2 * pr + 1] = src[8 * pr + 1];
    }
    const uint32_t pack = (v[7] << 28) | (v[5] << 24) | (v[3] << 20) | (v[1] << 16) | (v[6] << 12) | (v[4] << 8) | (v[2] << 4) | v[0];
    out[((nT * ksuper + ks) * 32 + t) * (I / 2) + j] = (int32_t)pack;
  }
}

// Aint4: tile = 16 rows (one m-tile) x KB k.   ref TinyGemmConvertA.cu:226-285
template <int I>
__global__ void __launch_bounds__(256) pack_Aint4_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        int64_t m, int64_t k, int64_t ksuper) {
  constexpr int KB = 256;
  __shared__ uint32_t s_codes[16][KB + 4];  // full 32-bit codes, see pack_Bint4_kernel
  const int tid = threadIdx.x;
  const int64_t mT = blockIdx.y;
  const int64_t kb0 = (int64_t)blockIdx.x * KB;
  const bool vec_ok = (k & 3) == 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * 256 + tid;
    const int rr = idx >> 6, c4 = idx & 63;
    const int64_t row = mT * 16 + rr, kk = kb0 + c4 * 4;
    int4 v = {0, 0, 0, 0};
    if (row < m) {
      if (vec_ok && kk + 3 < k) {
        v = *reinterpret_cast<const int4*>(in + row * k + kk);
      } else {
        if (kk < k) v.x = in[row * k + kk];
        if (kk + 1 < k) v.y = in[row * k + kk + 1];
        if (kk + 2 < k) v.z = in[row * k + kk + 2];
        if (kk + 3 < k) v.w = in[row * k + kk + 3];
      }
    }
    *reinterpret_cast<int4*>(&s_codes[rr][c4 * 4]) = v;
  }
  __syncthreads();
  // words of this tile: [kS_local][t][inner]: KB/16 k-tiles x 32 = 512 words
  constexpr int WORDS = KB * 2;
#pragma unroll
  for (int it = 0; it < WORDS / 256; ++it) {
    const int wi = it * 256 + tid;
    const int inner = wi % I;
    const int t = (wi / I) & 31;
    const int ksl = wi / (32 * I);
    const int64_t ks = kb0 / (16 * I) + ksl;
    if (ks >= ksuper) continue;
    const int m0 = t >> 2, q = t & 3;
    const int kl = (ksl * I + inner) * 16 + 2 * q;
    const uint32_t v0 = s_codes[m0][kl], v1 = s_codes[m0][kl + 1];              // (m0,k0) (m0,k1)
    const uint32_t v2 = s_codes[m0 + 8][kl], v3 = s_codes[m0 + 8][kl + 1];      // (m1,k0) (m1,k1)
    const uint32_t v4 = s_codes[m0][kl + 8], v5 = s_codes[m0][kl + 9];          // (m0,k2) (m0,k3)
    const uint32_t v6 = s_codes[m0 + 8][kl + 8], v7 = s_codes[m0 + 8][kl + 9];  // (m1,k2) (m1,k3)
    const uint32_t pack = (v7 << 28) | (v5 << 24) | (v3 << 20) | (v1 << 16) | (v6 << 12) | (v4 << 8) | (v2 << 4) | v0;
    out[((mT * ksuper + ks) * 32 + t) * I + inner] = (int32_t)pack;
  }
}

// ---- unpack: one thread per code; the index arithmetic is the packers' read backwards (TinyGemmConvertA.cu:226-285,
// TinyGemmConvertB.cu:252-308: pack = v7<<28 | v5<<24 | v3<<20 | v1<<16 | v6<<12 | v4<<8 | v2<<4 | v0) ----
__global__ void __launch_bounds__(256) unpack_int4_kernel(const uint32_t* __restrict__ packed, int32_t* __restrict__ codes, int layout_a,
                                                          int64_t rows, int64_t k, int I, int64_t ksuper) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * k) return;
  const int64_t r = idx / k, kk = idx - r * k;
  const int64_t kt = kk >> 4;
  const int kq = (int)(kk & 15);
  int64_t word;
  int v;
  if (layout_a) {  // v = [(m0,k0),(m0,k1),(m1,k0),(m1,k1),(m0,k2),(m0,k3),(m1,k2),(m1,k3)], k0 = 2 (t % 4), k2 = k0 + 8
    const int rr = (int)(r & 15), m0 = rr & 7, hi = rr >> 3;
    const int t = 4 * m0 + ((kq & 7) >> 1);
    v = (kq >> 3) * 4 + hi * 2 + (kq & 1);
    word = (((r >> 4) * ksuper + kt / I) * 32 + t) * I + kt % I;
  } else {         // word j of a lane: k-tiles 2j (v0..v3) and 2j + 1 (v4..v7) of the super-tile, k = base + 2 (t % 4) + {0, 1, 8, 9}
    const int t = 4 * (int)(r & 7) + ((kq & 7) >> 1);
    const int ktl = (int)(kt % I);
    v = (ktl & 1) * 4 + (kq & 1) + 2 * (kq >> 3);
    word = (((r >> 3) * ksuper + kt / I) * 32 + t) * (I / 2) + (ktl >> 1);
  }
  const int shift = (v & 1) * 16 + (v >> 1) * 4;
  codes[idx] = (int32_t)((packed[word] >> shift) & 15u);
}

// ---- dequantise a Bint4-packed weight matrix into row-major 16-bit values (what a GEMM library multiplies for MANY activation rows) ----
// w[r][k] = RNE16(fma(f32(lut[r][code]), f32(scale[g][r]), f32(zero[g][r]))) -- the reference's dequantisation, element for element
// (MatrixLayoutB.cuh:1042-1046; int4: lut = code - 8, Dequantization.cuh:136-178).  Thread = (row, 64-k super-tile of innerKTiles 4 /
// 32-k of 2 / 128-k of 8): its words are 4 lanes x I / 2 words = 8 I contiguous bytes of the packed layout (ConvertB.cu:252-308), its
// output 32 I contiguous bytes of the row.
template <typename DT, int I, int CHK>
__global__ void __launch_bounds__(256) dequant_w4_kernel(const uint32_t* __restrict__ packed, const uint16_t* __restrict__ qinfo, const uint16_t* __restrict__ lut,
                                                        uint16_t* __restrict__ out, int64_t rows, int64_t wrows_q, int64_t k, int64_t ksuper, int gshift, int qtype) {
  constexpr int W = I / 2;   // words per lane of the packed layout = 32-k runs per super-tile
  // lane = (super-tile, word column j, run h of 8 consecutive k) of a 512-k chunk: a quad of lanes writes 64 contiguous bytes, the 4 W lanes
  // of a super-tile 32 I contiguous bytes, consecutive super-tiles follow: whole lines per wave-store; the 4 words a lane needs (lanes
  // 0 ... 3 of its row, column j) are the same for the four h -- one request per quad.
  // A WAVE is CHK consecutive 512-k chunks of ONE row (host: k a multiple of 512 CHK): at most 16 quantisation groups per chunk.  Their
  // dequantised tables -- 16 values RNE16(fma(lut[e], scale, zero)) per group, one fma per lane and round of 64 -- go to the wave's own LDS,
  // and every weight is then ONE 2-byte LDS read at table + 2 code (a 32-byte table is 8 banks: different entries never collide, equal
  // ones broadcast) instead of an 8-way select and an fma per element (~150 vector ops per 16 bytes of output: 31 us for a 4096 x 4096
  // matrix against 14 with one chunk per wave; CHK = 4: every load of the wave's 2048 k in flight before the first table is built).
  __shared__ uint16_t tables[4][CHK][16][16];  // [wave][chunk][group of the chunk][entry]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // blockIdx.y (+ 65535 blockIdx.z) = the row, blockIdx.x = a 256-thread piece of it: no 64-bit division by the run-time row length
  const int per_row = (int)(k >> 3) / CHK;             // threads per row (a multiple of 64)
  const int64_t r = (int64_t)blockIdx.y + (int64_t)blockIdx.z * 65535;
  const int tr = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= rows || tr - lane >= per_row) return;       // (wave-uniform)
  const int64_t k0w = (int64_t)(tr - lane) * 8 * CHK;  // first k of the wave
  const int ngw = (512 >> gshift) > 0 ? (512 >> gshift) : 1;   // groups of a chunk (g = 256 / 128 / 64 / 32: 2 / 4 / 8 / 16)
  // ---- requests: the packed words of every chunk, then the table inputs ----
  uint32_t wd[CHK][4];
  int hh[CHK];
  const uint16_t* tb[CHK];
#pragma unroll
  for (int c = 0; c < CHK; ++c) {
    const int t = (int)((k0w >> 3) + c * 64 + lane);   // this lane's 8-k run of the row
    const int h = t & 3, j = (t >> 2) % W;
    const int64_t s = t / (4 * W);
    const uint32_t* src = packed + (((r >> 3) * ksuper + s) * 32 + 4 * (r & 7)) * W + j;
#pragma unroll
    for (int i = 0; i < 4; ++i) wd[c][i] = src[i * W];
    hh[c] = h;
    const int64_t k0 = s * (16 * I) + j * 32;
    tb[c] = &tables[wave][c][(int)((k0 >> gshift) - ((k0w + c * 512) >> gshift))][0];
  }
  for (int t = lane; t < CHK * ngw * 16; t += 64) {
    const int e = t & 15, cg = t >> 4, c = cg / ngw, gw = cg - c * ngw;
    float lv;
    if (qtype == TG_Q_INT4) lv = (float)(e - 8);
    else lv = DT::lo_f32((uint32_t)lut[(qtype == TG_Q_ANY4_ROWWISE ? r * 16 : 0) + e]);
    const uint32_t sz = reinterpret_cast<const uint32_t*>(qinfo)[(((k0w + c * 512) >> gshift) + gw) * wrows_q + r];
    tables[wave][c][gw][e] = DT::from_f32(__builtin_fmaf(lv, DT::lo_f32(sz), DT::hi_f32(sz)));
  }
  // (the region is the wave's own and a wave's LDS operations execute in order: no barrier)
  // word i holds k = 2 i + {0, 1, 8, 9, 16, 17, 24, 25} of the run of 32 in the nibbles (v & 1) * 16 + (v >> 1) * 4, v = 0 ... 7: the pair
  // (k, k + 1) = (2 i + 8 h, 2 i + 8 h + 1) sits at bits 4 h and 16 + 4 h
#pragma unroll
  for (int c = 0; c < CHK; ++c) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t c0 = (wd[c][i] >> (hh[c] * 4)) & 15u, c1 = (wd[c][i] >> (16 + hh[c] * 4)) & 15u;
      o[i] = (uint32_t)tb[c][c0] | ((uint32_t)tb[c][c1] << 16);
    }
    *reinterpret_cast<u32x4*>(out + r * k + k0w + (int64_t)(c * 64 + lane) * 8) = o;
  }
}

// ---- 16-bit fragment-order conversions (pure data movement) ------------------------------------
// ref TinyGemmConvertA.cu:19-141 / 442-546 and TinyGemmConvertB.cu:20-66 / 136-176
__global__ void __launch_bounds__(256) to_A16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                    int64_t m, int64_t k, int64_t mTiles, int64_t kTiles) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= mTiles * kTiles * 32) return;
  const int t = gid & 31;
  const int64_t kT = (gid >> 5) % kTiles, mT = (gid >> 5) / kTiles;
  const int64_t m0 = mT * 16 + (t >> 2), m1 = m0 + 8;
  const int64_t k0 = kT * 16 + (t & 3) * 2;
  uint16_t v[8];
  auto at = [&](int64_t rr, int64_t cc) -> uint16_t { return (rr < m && cc < k) ? in[rr * k + cc] : (uint16_t)0; };
  v[0] = at(m0, k0); v[1] = at(m0, k0 + 1); v[2] = at(m1, k0); v[3] = at(m1, k0 + 1);
  v[4] = at(m0, k0 + 8); v[5] = at(m0, k0 + 9); v[6] = at(m1, k0 + 8); v[7] = at(m1, k0 + 9);
  u32x4 o = {v[0] | ((uint32_t)v[1] << 16), v[2] | ((uint32_t)v[3] << 16), v[4] | ((uint32_t)v[5] << 16), v[6] | ((uint32_t)v[7] << 16)};
  *reinterpret_cast<u32x4*>(out + gid * 8) = o;
}

__global__ void __launch_bounds__(256) from_A16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                      int64_t m, int64_t k, int64_t mTiles, int64_t kTiles) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= mTiles * kTiles * 32) return;
  const int t = gid & 31;
  const int64_t kT = (gid >> 5) % kTiles, mT = (gid >> 5) / kTiles;
  const u32x4 o = *reinterpret_cast<const u32x4*>(in + gid * 8);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t rr = mT * 16 + (t >> 2) + 8 * ((e >> 1) & 1);
    const int64_t cc = kT * 16 + (t & 3) * 2 + 8 * (e >> 2) + (e & 1);
    const uint16_t val = (uint16_t)(o[e >> 1] >> (16 * (e & 1)));
    if (rr < m && cc < k) out[rr * k + cc] = val;
  }
}

__global__ void __launch_bounds__(256) to_B16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                    int64_t n, int64_t k, int64_t nTiles, int64_t totalK, int inner) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= nTiles * totalK * 32) return;
  const int t = gid & 31;
  const int64_t kT = (gid >> 5) % totalK, nT = (gid >> 5) / totalK;
  const int64_t n0 = nT * 8 + (t >> 2);
  const int64_t k0 = kT * 16 + (t & 3) * 2;
  auto at = [&](int64_t cc) -> uint32_t { return (n0 < n && cc < k) ? in[n0 * k + cc] : 0u; };
  u32x2 o = {at(k0) | (at(k0 + 1) << 16), at(k0 + 8) | (at(k0 + 9) << 16)};
  uint16_t* dst = out + ((nT * (totalK / inner) + kT / inner) * 32 + t) * (4 * inner) + (kT % inner) * 4;
  *reinterpret_cast<u32x2*>(dst) = o;
}

__global__ void __launch_bounds__(256) from_B16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                      int64_t n, int64_t k, int64_t nTiles, int64_t kTiles,
                                                      int64_t outerK, int inner) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= nTiles * kTiles * 32) return;
  const int t = gid & 31;
  const int64_t kT = (gid >> 5) % kTiles, nT = (gid >> 5) / kTiles;
  const int64_t n0 = nT * 8 + (t >> 2);
  if (n0 >= n) return;
  const uint16_t* src = in + ((nT * outerK + kT / inner) * 32 + t) * (4 * inner) + (kT % inner) * 4;
  const u32x2 o = *reinterpret_cast<const u32x2*>(src);
  const int64_t k0 = kT * 16 + (t & 3) * 2;
  const int64_t ks[4] = {k0, k0 + 1, k0 + 8, k0 + 9};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (ks[e] < k) out[n0 * k + ks[e]] = (uint16_t)(o[e >> 1] >> (16 * (e & 1)));
}

// debug op, ref TinyGemmDequantize.cu:19-34 (grid-stride, one word -> 8 bf16 = 16 bytes)
__global__ void __launch_bounds__(256) dequant_int4_kernel(const int32_t* __restrict__ in, u32x4* __restrict__ out, int64_t count) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < count; idx += (int64_t)gridDim.x * 256) {
    const uint32_t w = (uint32_t)in[idx];
    u32x4 o;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const float lo = (float)((int)((w >> (4 * ii)) & 0xfu) - 8);
      const float hi = (float)((int)((w >> (4 * ii + 16)) & 0xfu) - 8);
      o[ii] = BF16::pack2(lo, hi);
    }
    out[idx] = o;
  }
}

// ---- int8 packers (reference TinyGemmConvertB.cu:366-411, TinyGemmConvertA.cu:337-397): one thread per output word.
// The OR of the shifted 32-bit inputs is kept exactly as written there (inputs above 255 bleed into higher bytes).
template <int I>
__global__ void __launch_bounds__(256) pack_Bint8_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n,
                                                         int64_t k, int64_t ksuper, int64_t total) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int j = (int)(o % I), t = (int)((o / I) % 32);
    const int64_t ks_ = (o / (I * 32)) % ksuper, nt = o / (I * 32 * ksuper);
    const int64_t n0 = nt * 8 + t / 4, kb = (ks_ * I + j) * 16 + (t % 4) * 2;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (n0 < n) {
      const int32_t* r = in + n0 * k;
      if (kb < k) v[0] = (uint32_t)r[kb];
      if (kb + 1 < k) v[1] = (uint32_t)r[kb + 1];
      if (kb + 8 < k) v[2] = (uint32_t)r[kb + 8];
      if (kb + 9 < k) v[3] = (uint32_t)r[kb + 9];
    }
    out[o] = (int32_t)((v[3] << 24) | (v[1] << 16) | (v[2] << 8) | v[0]);
  }
}

template <int I>
__global__ void __launch_bounds__(256) pack_Aint8_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t m,
                                                         int64_t k, int64_t kouter, int64_t total) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int w = (int)(o % 2), j = (int)((o / 2) % I), t = (int)((o / (2 * I)) % 32);
    const int64_t ko = (o / (2 * I * 32)) % kouter, mt = o / (2 * I * 32 * kouter);
    const int64_t m0 = mt * 16 + t / 4, m1 = m0 + 8;
    const int64_t ka = (ko * I + j) * 16 + (t % 4) * 2 + 8 * w;  // word 0: k0, k0+1; word 1: k0+8, k0+9
    uint32_t v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;                 // (m0,ka) (m0,ka+1) (m1,ka) (m1,ka+1)
    if (m0 < m && ka < k) v0 = (uint32_t)in[m0 * k + ka];
    if (m0 < m && ka + 1 < k) v1 = (uint32_t)in[m0 * k + ka + 1];
    if (m1 < m && ka < k) v2 = (uint32_t)in[m1 * k + ka];
    if (m1 < m && ka + 1 < k) v3 = (uint32_t)in[m1 * k + ka + 1];
    out[o] = (int32_t)((v3 << 24) | (v1 << 16) | (v2 << 8) | v0);
  }
}
