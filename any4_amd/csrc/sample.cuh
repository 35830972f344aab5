// sample.cuh -- sample_kernel: temperature / top-k / top-p sampling of a row of 16-bit logits in ONE launch, without a sort and without a
// [vocab] temporary (dg_sample, include/decode_glue_hip.h; the definition is any4_amd/sampling.py: sample_ref).  Included inside
// tg_sample.hip's anonymous namespace.
//
// One workgroup of 1024 threads per row; everything between the row and the token lives in LDS.
//
// A 16-bit logit has an order-preserving 16-bit key (dkey: 0 = the largest value, -0 counted as +0), and every token of one key has the same
// weight, so the rank order (logit descending, index ascending) is: keys ascending, and inside a key the index.  The kernel therefore only
// COUNTS tokens per key and walks the counts:
//   pass 1   the smallest key of the row (= l_max) and which of the 1024 COARSE bins (64 consecutive keys) are non-empty.  The non-empty
//            coarse bins get consecutive SLOTS; 512 slots (512 x 64 counters = 128 KiB) are one WINDOW of the key space.  4 randn in
//            fp16 fills ~450 slots at vocab 128256, in bf16 ~60: one window.  A row with more non-empty coarse bins takes two windows:
//            the LDS tables hold one at a time, so a walk that needs the other one rebuilds it (a zero of the table and a pass over
//            the row each time, up to six per launch); a window's totals are kept, so a walk steps over a window it does not end in.
//   pass 2   the count of every key of the window (LDS integer atomics), then per slot the pair (tokens, mass) and its prefix over the slots.
//            The mass of a key is count x w, w = floor(expf((l - l_max) / temperature) x 2^shift) a 64-bit INTEGER (2^shift x vocab < 2^62):
//            integer sums are the same in every order, which makes the prefixes of slots, of keys inside a slot and of tokens inside a key
//            consistent with each other and the result bit-deterministic whatever the arrival order of the atomics.
//   find     three walks over those prefixes, each "the first rank whose inclusive mass reaches THR, but at most rank LIMIT - 1":
//            Z_k = mass of the first k ranks (THR never reached, LIMIT = k); the nucleus (THR = ceil(top_p Z_k), LIMIT = k) -> kept ranks and
//            their mass Z; the draw (THR = floor(u Z) + 1, LIMIT = kept).  A walk finds its slot by 512 threads, then its key and the rank
//            inside the key by one wave.  With one window nothing is rebuilt between the walks.
//   pass 3   the answer is the j-th token of that key in index order: waves own contiguous pieces of the row, count their matches, and
//            the wave that holds the j-th finds it by an ordered count over its lanes.
// temperature == 0 skips pass 2 and the walks: the first token of the smallest key.
//
// Rows need no alignment beyond their element's: a row is addressed as the 16-byte vectors of the aligned stream it lies in; a vector that
// lies inside the row is one 16-byte load, the first and the last (partly outside) are read element by element.
#pragma once

constexpr int SMP_THREADS = 1024, SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_COARSE = 1024;              // coarse bins: 64 keys each
constexpr int SMP_SLOTS = 512;                // slots of a window
constexpr int SMP_FINE = SMP_SLOTS * 64;      // counters of a window
constexpr int SMP_WINDOWS = SMP_COARSE / SMP_SLOTS;  // windows a row can need
constexpr int SMP_BATCH = 8;                  // 16-byte loads a lane has in flight

struct SampleParams {
  const uint16_t* logits;
  int64_t ld;
  const int64_t* ctr;
  const float* temperature;
  const int32_t* top_k;
  const float* top_p;
  const int64_t* seed;
  const float* u_in;
  int64_t* token_out;
  float* u_out;
  int64_t ctr_add;
  int32_t vocab, per_sequence, shift;
};

// LDS, all of it dynamic (prepare_lds_kernel: the kernel has no static LDS)
struct SampleShared {
  uint32_t fine[SMP_FINE];           // tokens per key of the window, [slot][key & 63]
  uint64_t pre_m[SMP_SLOTS + 1];     // mass / tokens in front of slot s of the window ([SMP_SLOTS]: the window's total)
  uint32_t pre_c[SMP_SLOTS + 1];
  uint16_t slot_of[SMP_COARSE];      // coarse bin -> its slot (counted over all windows)
  uint16_t coarse_of[SMP_COARSE];    // slot -> coarse bin
  uint8_t nonempty[SMP_COARSE];
  uint64_t wave_m[SMP_WAVES];
  uint32_t wave_c[SMP_WAVES];
  uint32_t min_key;
  int32_t cross;                     // the slot a walk crosses in (-1: not in this window)
  uint32_t res_key, res_j, res_rank; // a walk's answer: key, rank inside the key, rank in the row ...
  uint64_t res_mass;                 // ... and the inclusive mass there
};
static_assert(sizeof(SampleShared) <= 160 * 1024, "LDS of a CU");

// Philox4x32-10 (any4_amd/sampling.py: philox4x32_10), first output word
__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// key of a 16-bit float (bf16 and fp16 alike: sign, exponent, mantissa): ascending key = descending value; -0 is +0
__device__ __forceinline__ uint32_t smp_dkey(uint32_t bits) {
  bits &= 0xffffu;
  if (bits == 0x8000u) bits = 0;
  return (bits & 0x8000u) ? bits : 0x7fffu - bits;
}
__device__ __forceinline__ uint32_t smp_bits_of(uint32_t dkey) { return dkey < 0x8000u ? 0x7fffu - dkey : dkey; }

// Integer sums over a wave on the vector ALU's own data paths (tg_common.cuh, namespace tgl: no LDS round trip per step): rotations
// within the 16-lane rows, then the row swaps.  Every lane gets the sum.
template <int CTRL>
__device__ __forceinline__ uint32_t smp_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t smp_dpp(uint64_t v) {
  return (uint64_t)smp_dpp<CTRL>((uint32_t)v) | ((uint64_t)smp_dpp<CTRL>((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint32_t smp_swap16_sum(uint32_t v) {
  const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  return (uint32_t)sw[0] + (uint32_t)sw[1];
}
__device__ __forceinline__ uint32_t smp_swap32_sum(uint32_t v) {
  const auto sw = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return (uint32_t)sw[0] + (uint32_t)sw[1];
}
__device__ __forceinline__ uint64_t smp_swap16_sum(uint64_t v) {
  const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(v >> 32), (uint32_t)(v >> 32), false, false);
  return ((uint64_t)(uint32_t)lo[0] | ((uint64_t)(uint32_t)hi[0] << 32)) + ((uint64_t)(uint32_t)lo[1] | ((uint64_t)(uint32_t)hi[1] << 32));
}
__device__ __forceinline__ uint64_t smp_swap32_sum(uint64_t v) {
  const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(v >> 32), (uint32_t)(v >> 32), false, false);
  return ((uint64_t)(uint32_t)lo[0] | ((uint64_t)(uint32_t)hi[0] << 32)) + ((uint64_t)(uint32_t)lo[1] | ((uint64_t)(uint32_t)hi[1] << 32));
}
template <typename T>
__device__ __forceinline__ T smp_wave_sum(T v) {
  v += smp_dpp<0x128>(v);  // row_ror 8, 4, 2, 1
  v += smp_dpp<0x124>(v);
  v += smp_dpp<0x122>(v);
  v += smp_dpp<0x121>(v);
  return smp_swap32_sum(smp_swap16_sum(v));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return smp_wave_sum(v); }
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) { return smp_wave_sum(v); }
// inclusive prefix sums over the lanes of a wave
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// A row as 16-byte vectors of the aligned stream it lies in: token i is element (i + off) & 7 of vector (i + off) >> 3.
struct SampleRow {
  const uint16_t* row;  // token 0
  int32_t vocab, off, nvec;
  // the 8 elements of vector v (two per word) and which of them are tokens of the row
  __device__ __forceinline__ uint32_t load_raw(int32_t v, u32x4& w) const {
    const int32_t t0 = v * 8 - off;  // token of element 0
    if (t0 >= 0 && t0 + 8 <= vocab) {
      w = *reinterpret_cast<const u32x4*>(row + t0);
      return 0xffu;
    }
    uint32_t valid = 0;
    w = u32x4{0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int32_t t = t0 + e;
      if (t >= 0 && t < vocab) {
        w[e >> 1] |= (uint32_t)row[t] << (16 * (e & 1));
        valid |= 1u << e;
      }
    }
    return valid;
  }
  static __device__ __forceinline__ void keys_of(const u32x4& w, uint32_t (&key)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      key[2 * e] = smp_dkey(w[e] & 0xffffu);
      key[2 * e + 1] = smp_dkey(w[e] >> 16);
    }
  }
  // the keys of vector v and which of its 8 elements are tokens of the row
  __device__ __forceinline__ uint32_t load(int32_t v, uint32_t (&key)[8]) const {
    u32x4 w;
    const uint32_t valid = load_raw(v, w);
    keys_of(w, key);
    return valid;
  }
  // f(v, key, valid) for every vector of [v_begin, v_end) this lane owns (v = v_begin + lane, + 64, ...), in that order.  A pass is bound
  // by the latency of its loads, not by their bytes (one workgroup reads the row): SMP_BATCH loads are in flight before the first is used.
  template <typename F>
  __device__ __forceinline__ void for_each(int32_t v_begin, int32_t v_end, int lane, F&& f) const {
    for (int32_t v0 = v_begin; v0 < v_end; v0 += 64 * SMP_BATCH) {
      u32x4 w[SMP_BATCH];
      uint32_t valid[SMP_BATCH];
#pragma unroll
      for (int i = 0; i < SMP_BATCH; ++i) {
        const int32_t v = v0 + i * 64 + lane;
        valid[i] = 0;
        if (v < v_end) valid[i] = load_raw(v, w[i]);
      }
#pragma unroll
      for (int i = 0; i < SMP_BATCH; ++i)
        if (valid[i]) {
          uint32_t key[8];
          keys_of(w[i], key);
          f(v0 + i * 64 + lane, key, valid[i]);
        }
    }
  }
};

template <typename DT>
__device__ __forceinline__ uint64_t smp_weight(uint32_t dkey, float lmax, float temperature, int shift) {
  const float x = DT::to_f32((uint16_t)smp_bits_of(dkey));
  // in [0, 1]: the largest logit has weight 1 (the clamp only bounds the integer sums for a temperature < 0, which is out of contract)
  // The argument in float64, rounded once: the difference of two bf16 logits can exceed float32's range.
  const float arg = (float)(((double)x - (double)lmax) / (double)temperature);
  const float w = fminf(expf(arg), 1.f);
  return (uint64_t)((double)w * (double)(1ull << shift));
}

template <typename DT>
__global__ void __launch_bounds__(SMP_THREADS) sample_kernel(SampleParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smp_lds[];
  SampleShared& S = *reinterpret_cast<SampleShared*>(smp_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t c_read = P.ctr[P.per_sequence ? b : 0];
  if (c_read < 0) {  // an inactive sequence
    if (tid == 0) {
      P.token_out[b] = -1;
      if (P.u_out) P.u_out[b] = 0.f;
    }
    return;
  }
  const float temperature = P.temperature[b], top_p = P.top_p[b];
  const int32_t V = P.vocab, top_k = P.top_k[b];
  float u;
  if (P.u_in) {
    u = P.u_in[b];
  } else {
    const uint64_t c = (uint64_t)(c_read + P.ctr_add), sd = (uint64_t)P.seed[b];
    u = (float)(philox4x32_10_word0((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32)) >> 8) * 0x1p-24f;
  }
  if (tid == 0 && P.u_out) P.u_out[b] = u;

  SampleRow R;
  R.row = P.logits + b * P.ld;
  R.vocab = V;
  R.off = (int32_t)((reinterpret_cast<uintptr_t>(R.row) & 15u) >> 1);
  R.nvec = (int32_t)(((int64_t)R.off + V + 7) >> 3);
  // a wave owns a contiguous piece of the row (pass 3 needs the index order), its lanes consecutive vectors
  const int32_t per_wave = (R.nvec + SMP_WAVES - 1) / SMP_WAVES;
  const int32_t v_begin = min(wave * per_wave, R.nvec), v_end = min(v_begin + per_wave, R.nvec);

  // ---- pass 1: the smallest key, the non-empty coarse bins ----
  if (tid < SMP_COARSE / 4) reinterpret_cast<uint32_t*>(S.nonempty)[tid] = 0;
  if (tid == 0) S.min_key = 0xffffu;
  __syncthreads();
  {
    uint32_t kmin = 0xffffu;
    R.for_each(v_begin, v_end, lane, [&](int32_t, const uint32_t (&key)[8], uint32_t valid) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (valid >> e & 1) {
          kmin = min(kmin, key[e]);
          S.nonempty[key[e] >> 6] = 1;
        }
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, 64));
    if (lane == 0) atomicMin(&S.min_key, kmin);
  }
  __syncthreads();
  const uint32_t min_key = S.min_key;

  uint32_t ans_key = min_key, ans_j = 0;  // temperature == 0: the first token of the largest value
  if (temperature != 0.f) {
    // slots of the non-empty coarse bins, in key order
    {
      const bool ne = S.nonempty[tid] != 0;  // SMP_COARSE == SMP_THREADS
      const unsigned long long bal = __ballot(ne);
      if (lane == 0) S.wave_c[wave] = (uint32_t)__popcll(bal);
      __syncthreads();
      uint32_t base = 0;
      for (int w = 0; w < wave; ++w) base += S.wave_c[w];
      const uint32_t slot = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      S.slot_of[tid] = ne ? (uint16_t)slot : (uint16_t)0xffffu;
      if (ne) S.coarse_of[slot] = (uint16_t)tid;
    }
    uint32_t nslots = 0;
    for (int w = 0; w < SMP_WAVES; ++w) nslots += S.wave_c[w];
    __syncthreads();  // (wave_c is reused below)
    const int nwin = (int)((nslots + SMP_SLOTS - 1) / SMP_SLOTS);
    const float lmax = DT::to_f32((uint16_t)smp_bits_of(min_key));

    const uint32_t K = (top_k <= 0 || top_k >= V) ? (uint32_t)V : (uint32_t)top_k;
    uint64_t Zk = 0, Z = 0;
    uint32_t kept = K;
    int built = -1;  // the window the LDS tables hold
    // (tokens, mass) of each window once it has been built: a later walk steps over a window it does not end in without rebuilding it
    uint64_t total_m[SMP_WINDOWS] = {};
    uint32_t total_c[SMP_WINDOWS] = {};
    bool known[SMP_WINDOWS] = {};
    for (int phase = 0; phase < 3; ++phase) {
      uint64_t THR;
      uint32_t LIMIT = K;
      if (phase == 0) {
        THR = 1ull << 63;  // never reached: the walk ends at rank K - 1
      } else if (phase == 1) {
        if (!(top_p < 1.f)) {
          Z = Zk;
          continue;
        }
        THR = (uint64_t)ceil((double)top_p * (double)Zk);
        if (THR < 1) THR = 1;
      } else {
        THR = (uint64_t)floor((double)u * (double)Z) + 1;
        LIMIT = kept;
      }
      uint64_t carry_m = 0;
      uint32_t carry_c = 0;
      for (int win = 0; win < nwin; ++win) {
        if (known[win] && !(carry_m + total_m[win] >= THR || carry_c + total_c[win] >= LIMIT)) {  // (the same in every thread)
          carry_m += total_m[win];
          carry_c += total_c[win];
          continue;
        }
        if (built != win) {
          // ---- pass 2: the counts of the window's keys ----
          for (int i = tid; i < SMP_FINE / 4; i += SMP_THREADS) reinterpret_cast<u32x4*>(S.fine)[i] = u32x4{0, 0, 0, 0};
          __syncthreads();
          const uint32_t slot0 = (uint32_t)win * SMP_SLOTS;
          R.for_each(v_begin, v_end, lane, [&](int32_t, const uint32_t (&key)[8], uint32_t valid) {
            uint32_t run = 0;  // equal neighbours share an atomic
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              if (!(valid >> e & 1)) continue;
              ++run;
              const bool last = e == 7 || !(valid >> (e + 1) & 1) || key[e + 1] != key[e];
              if (last) {
                const uint32_t s = (uint32_t)S.slot_of[key[e] >> 6] - slot0;
                if (s < (uint32_t)SMP_SLOTS) atomicAdd(&S.fine[s * 64 + (key[e] & 63u)], run);
                run = 0;
              }
            }
          });
          __syncthreads();
          // per slot (tokens, mass): a wave per slot, a lane per key
          const uint32_t here = min(nslots - slot0, (uint32_t)SMP_SLOTS);
          for (uint32_t s = wave; s < (uint32_t)SMP_SLOTS; s += SMP_WAVES) {
            uint32_t c = s < here ? S.fine[s * 64 + lane] : 0u;
            uint64_t m = 0;
            if (c) m = (uint64_t)c * smp_weight<DT>((uint32_t)S.coarse_of[slot0 + s] * 64u + lane, lmax, temperature, P.shift);
            if (s < here) {  // (the same in every lane)
              c = wave_sum_u32(c);
              m = wave_sum_u64(m);
            }
            if (lane == 0) {
              S.pre_c[s + 1] = c;
              S.pre_m[s + 1] = m;
            }
          }
          __syncthreads();
          // ... and their prefix over the slots
          uint32_t c = 0;
          uint64_t m = 0;
          if (tid < SMP_SLOTS) {
            c = wave_scan_u32(S.pre_c[tid + 1], lane);
            m = wave_scan_u64(S.pre_m[tid + 1], lane);
            if (lane == 63) {
              S.wave_c[wave] = c;
              S.wave_m[wave] = m;
            }
          }
          __syncthreads();
          if (tid < SMP_SLOTS) {
            for (int w = 0; w < wave; ++w) {
              c += S.wave_c[w];
              m += S.wave_m[w];
            }
            S.pre_c[tid + 1] = c;
            S.pre_m[tid + 1] = m;
          }
          if (tid == 0) {
            S.pre_c[0] = 0;
            S.pre_m[0] = 0;
          }
          built = win;
        }
        if (tid == 0) S.cross = -1;
        __syncthreads();
        // ---- the slot in which the walk ends ----
        if (tid < SMP_SLOTS) {
          const bool before = carry_m + S.pre_m[tid] >= THR || carry_c + S.pre_c[tid] >= LIMIT;
          const bool after = carry_m + S.pre_m[tid + 1] >= THR || carry_c + S.pre_c[tid + 1] >= LIMIT;
          if (after && !before) S.cross = tid;
        }
        __syncthreads();
        total_m[win] = S.pre_m[SMP_SLOTS];
        total_c[win] = S.pre_c[SMP_SLOTS];
        known[win] = true;
        const int cross = S.cross;
        if (cross >= 0) {
          // ---- the key in which it ends, and the rank inside the key ----
          if (wave == 0) {
            const uint32_t key = (uint32_t)S.coarse_of[(uint32_t)win * SMP_SLOTS + cross] * 64u + lane;
            const uint32_t c = S.fine[cross * 64 + lane];
            const uint64_t w = c ? smp_weight<DT>(key, lmax, temperature, P.shift) : 0;
            const uint32_t c1 = carry_c + S.pre_c[cross] + wave_scan_u32(c, lane);
            const uint64_t m1 = carry_m + S.pre_m[cross] + wave_scan_u64((uint64_t)c * w, lane);
            const uint32_t c0 = c1 - c;
            const uint64_t m0 = m1 - (uint64_t)c * w;
            if ((m1 >= THR || c1 >= LIMIT) && !(m0 >= THR || c0 >= LIMIT)) {
              uint64_t n = LIMIT - c0;                                    // tokens of this key up to rank LIMIT - 1 ...
              if (w > 0) n = min(n, (THR - m0 + w - 1) / w);              // ... and up to the one whose mass reaches THR
              S.res_key = key;
              S.res_j = (uint32_t)n - 1;
              S.res_rank = c0 + (uint32_t)n - 1;
              S.res_mass = m0 + n * w;
            }
          }
          __syncthreads();
          break;
        }
        carry_m += total_m[win];
        carry_c += total_c[win];
      }
      if (phase == 0) {
        Zk = S.res_mass;
      } else if (phase == 1) {
        kept = S.res_rank + 1;
        Z = S.res_mass;
      } else {
        ans_key = S.res_key;
        ans_j = S.res_j;
      }
      __syncthreads();  // (the next walk writes the answer again)
    }
  }

  // ---- pass 3: token number ans_j (in index order) among those with key ans_key ----
  {
    uint32_t mine = 0;
    R.for_each(v_begin, v_end, lane, [&](int32_t, const uint32_t (&key)[8], uint32_t valid) {
#pragma unroll
      for (int e = 0; e < 8; ++e) mine += (valid >> e & 1) && key[e] == ans_key;
    });
    mine = wave_sum_u32(mine);
    if (lane == 0) S.wave_c[wave] = mine;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += S.wave_c[w];
    if (ans_j >= before && ans_j < before + mine) {  // this wave holds it
      uint32_t run = before;
      for (int32_t v0 = v_begin; v0 < v_end && run <= ans_j; v0 += 64 * SMP_BATCH) {
        uint32_t match[SMP_BATCH];  // which elements of this lane's vectors have the key (the loads of a batch in flight together)
#pragma unroll
        for (int i = 0; i < SMP_BATCH; ++i) {
          const int32_t v = v0 + i * 64 + lane;
          match[i] = 0;
          if (v < v_end) {
            uint32_t key[8];
            const uint32_t valid = R.load(v, key);
#pragma unroll
            for (int e = 0; e < 8; ++e) match[i] |= (uint32_t)((valid >> e & 1) && key[e] == ans_key) << e;
          }
        }
#pragma unroll
        for (int i = 0; i < SMP_BATCH; ++i) {
          if (run > ans_j || __ballot(match[i] != 0) == 0) continue;  // (the same in every lane)
          const uint32_t n = (uint32_t)__popc(match[i]);
          const uint32_t inc = run + wave_scan_u32(n, lane);
          if (ans_j >= inc - n && ans_j < inc) {
            uint32_t skip = ans_j - (inc - n);
            int e = 0;
            for (; e < 8; ++e)
              if (match[i] >> e & 1) {
                if (skip == 0) break;
                --skip;
              }
            P.token_out[b] = (int64_t)(v0 + i * 64 + lane) * 8 + e - R.off;
          }
          run = __shfl(inc, 63, 64);
        }
      }
    }
  }
}
