// f16_gemm.cuh -- the 16-bit-weight GEMM of tg_gemm_f16 (reference TinyGemm_bf16.cu:163-327; included by tinygemm_hip.hip).
#pragma once

// ---- 16-bit weights (reference TinyGemm_bf16.cu) ---------------------------------------------
// Same tile/split-K structure; the A operand is gathered dword-wise from the fragment-order
// tensor (each dword = two adjacent k of one row), no dequantisation.
struct F16GemmParams {
  const char* x;
  const char* w;
  char* y;
  int32_t m, wrows, k;
  int32_t ktiles_padded;  // k-tiles present in the TC tensor (size(1) * I)
  int32_t inner;          // I
};

template <typename DT, bool LAYOUT_A, int WAVES, int I>
__global__ void __launch_bounds__(WAVES * 64) f16_gemm_kernel(const F16GemmParams p) {
  __shared__ f32x4 s_red[WAVES * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, Q = lane >> 4, r = i & 7;
  const int rt = blockIdx.x, ct = blockIdx.y;
  const int row0 = rt * 16, row = row0 + i;
  const bool row_ok = row < p.wrows;
  // Lane (i, Q) reads the fragment words of ITS OWN lane slot t = 4 (i & 7) + Q of the m16n8k16 layouts, as stored:
  // per k-tile the dwords (k0,k1) and (k0+8,k0+9) with k0 = 2Q, so one K-slot (two k-tiles) is the 8 k values
  // {2Q, 2Q+1, 2Q+8, 2Q+9} + {0, 16} and the X fragment is four dwords at byte offsets 4Q + {0, 16, 32, 48} of the slot
  // (the mapping of w8_gemm.cuh).  One 16-byte (A16, B16 I = 2) or 8-byte (B16 I = 1) load per k-tile pair / k-tile.
  const uint32_t* wd = reinterpret_cast<const uint32_t*>(p.w);
  const int xrow = min(ct * 16 + i, p.m - 1);
  const bool xcol = ct * 16 + i < p.m;
  const int ktiles = p.k >> 4;  // k % 32 == 0
  const int nsteps_total = ktiles >> 1;
  const int t = 4 * r + Q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // A ring of F16_RING steps in flight per wave.  Every load is unconditional per lane with clamped addresses and nothing of a step is touched
  // before it is consumed (round 6: a load under a lane mask makes hipcc wait vmcnt(0) right behind it -- every step then exposed the whole
  // memory latency); rows / columns beyond the problem are masked at the consumer.
  constexpr int F16_RING = 4;
  struct Step { u32x4 w0, w1, x; };
  const int rt_c = rt;  // (row tiles are never out of range: the grid is exact; rows beyond wrows within the last tile are masked below)
  auto load_step = [&](int s, Step& st) {
    const int sc = min(s, nsteps_total - 1);
    if constexpr (LAYOUT_A) {
      // [mT][kT][32][8 halfs] = 4 dwords per lane slot: (m0;k0,k1) (m1;k0,k1) (m0;k8,k9) (m1;k8,k9)
      st.w0 = *reinterpret_cast<const u32x4*>(wd + (((int64_t)rt_c * p.ktiles_padded + 2 * sc) * 32 + t) * 4);
      st.w1 = *reinterpret_cast<const u32x4*>(wd + (((int64_t)rt_c * p.ktiles_padded + 2 * sc + 1) * 32 + t) * 4);
    } else {
      // [nT][kT/I][32][4 I halfs]: per k-tile the dwords (k0,k1) (k8,k9)
      const int tile = min(2 * rt + (i >> 3), (p.wrows + 7) / 8 - 1);
      if constexpr (I == 2) {
        st.w0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wd + (((int64_t)tile * (p.ktiles_padded / 2) + sc) * 32 + t) * 4));
        st.w1 = st.w0;
      } else {
        const u32x2 v0 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wd + (((int64_t)tile * p.ktiles_padded + 2 * sc) * 32 + t) * 2));
        const u32x2 v1 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(wd + (((int64_t)tile * p.ktiles_padded + 2 * sc + 1) * 32 + t) * 2));
        st.w0 = u32x4{v0[0], v0[1], v1[0], v1[1]};
        st.w1 = st.w0;
      }
    }
    st.x = *reinterpret_cast<const u32x4*>(p.x + ((int64_t)xrow * p.k + 32 * sc) * 2 + 16 * Q);   // dwords 4Q ... 4Q + 3: transposed at the consumer
  };
  auto compute_step = [&](const Step& st) {
    u32x4 a;
    if constexpr (LAYOUT_A) {
      const int h = i >> 3;
      a = u32x4{h ? st.w0[1] : st.w0[0], h ? st.w0[3] : st.w0[2], h ? st.w1[1] : st.w1[0], h ? st.w1[3] : st.w1[2]};
    } else {
      a = st.w0;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = row_ok ? a[e] : 0u;
    const u32x4 xt = transpose_rows4(st.x);
    const u32x4 xv = {xcol ? xt[0] : 0u, xcol ? xt[1] : 0u, xcol ? xt[2] : 0u, xcol ? xt[3] : 0u};
    acc = DT::mfma(a, xv, acc);
  };
  {
    // this wave's steps: wave, wave + WAVES, ...: nw of them.  Rounds of F16_RING steps whose refills are all in range run without a branch
    // around a load (exact vmcnt); the last round(s) only consume (a refill past the end would be real work for the vector-memory path).
    const int nw = (nsteps_total - wave + WAVES - 1) / WAVES;
    Step ring[F16_RING];
#pragma unroll
    for (int j = 0; j < F16_RING; ++j) load_step(wave + j * WAVES, ring[j]);   // (clamped: a wave with fewer steps loads its last one again)
    int base = 0;
    for (; base + 2 * F16_RING <= nw; base += F16_RING) {
#pragma unroll
      for (int j = 0; j < F16_RING; ++j) {
        compute_step(ring[j]);
        load_step(wave + (base + F16_RING + j) * WAVES, ring[j]);
      }
    }
    // the remainder: fewer than two rounds; refills only where a step exists
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int j = 0; j < F16_RING; ++j) {
        const int jj = base + r * F16_RING + j;
        if (jj < nw) {
          compute_step(ring[j]);
          if (jj + F16_RING < nw) load_step(wave + (jj + F16_RING) * WAVES, ring[j]);
        }
      }
    }
  }
  s_red[wave * 64 + lane] = acc;
  __syncthreads();
  if (tid < 256) {
    const int c = tid >> 4, rr = tid & 15;
    const float* red = reinterpret_cast<const float*>(s_red);
    const int src = (((rr >> 2) * 16 + c) << 2) + (rr & 3);
    float sum = 0.f;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) sum += red[wv * 256 + src];
    const int col = ct * 16 + c, rowg = row0 + rr;
    if (col < p.m && rowg < p.wrows) reinterpret_cast<uint16_t*>(p.y)[(int64_t)col * p.wrows + rowg] = DT::from_f32(sum);
  }
}
