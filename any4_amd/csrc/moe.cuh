// moe.cuh -- mixture-of-experts decode (dg_moe_route / dg_moe_launch's DG_MOE_GEMV, include/decode_glue_hip.h): the top-k router and the expert-indexed
// W4A16 GEMV.  Included inside tg_moe.hip's anonymous namespace.  The definition is any4_amd/moe.py: moe_ref.
//
//   moe_route_kernel   l[i][e] = sum_c router_w[e][c] x[i][c] (f32, not rounded), p = softmax(l[i]) over all E, the top_k largest p by
//                      (p descending, index ascending), gates g = p_s / sum of the selected p.
//                      One workgroup per activation row.  Its MR_THREADS lanes walk k together, 8 elements (16 bytes) per lane and pass,
//                      MR_J router rows at a time; a lane chains its products per expert, the wave sums them (tgl::wave_sum), the MR_WAVES
//                      partials meet in LDS and are added in wave order (lora_shrink_kernel's pattern).  Wave 0 then holds logit e in lane
//                      e: softmax and selection are wave reductions, top_k rounds of (wave maximum, ballot, lowest set bit).  A round
//                      whose ballot is empty (NaN: out of contract) takes the lowest index left, so every id written is in [0, E).
//
//   moe_w4_kernel      the GEMV of w4_gemv.cuh with the weights picked by ids [m][top_k] on the device.  Same layout (Bint4 words at
//                      innerKTiles 4, scale | zero words per group and row, int4 / any4 with a global or row-wise LUT), same numerics
//                      (TG_NUM_FAST: pair-table lookups, v_dot2 into f32, the group's affine map applied to the f32 partial sums).
//     grid      workgroup b owns the 16-row units [b upw, (b + 1) upw) of the packed layout (a unit = two 8-row tiles = one gate / up
//               block of the SwiGLU store) and the whole k; nothing is reduced across workgroups, there are no atomics.
//     experts   every wave reads the <= 64 ids itself (lane = pair, an id outside [0, E) becomes "none" and forms no address); the
//               workgroup walks e = 0 ... E - 1 and skips an expert whose ballot is empty: its bytes are never requested.  A selected
//               expert is served in sweeps of up to `np` of its pairs (8 where LDS allows: the host's plan): a sweep stages those pairs'
//               activation rows in LDS (the byte order of w4_gemm_pair.cuh, with the f32 sums of every half super-tile next to them) and
//               streams the expert's rows of the range ONCE, contracting each 16-byte load with every pair of the sweep -- the loop
//               over pairs stops at the sweep's count, so the vector work follows the rows that chose the expert, not m.
//     pass      16 weight rows; lane = (row = lane & 15, sub = lane >> 4): sub picks (super-tile of the step, half of it), a step is two
//               64-k super-tiles.  The 8 waves split k by super-tiles (spw each; a wave past the end of k has no step that counts);
//               MW_D steps per lane are in flight, and the ring runs across passes, sweeps and experts: a pass's last round requests the
//               first steps of the workgroup's NEXT (expert, unit), so the weight stream does not drain at a pass's barriers (a pass
//               of 16 rows at k = 4096 is one round).  Per pass the partial sums meet in LDS and are added in wave order.
//     tables    [256 byte values][64 columns] x 4 bytes at LDS address 0, address = byte << 8 | column << 2 (one v_perm_b32), column =
//               lane & 31 (columns c and c + 16 hold the same row: the 32 lanes of an LDS access group use 32 distinct columns); rebuilt
//               per (expert, pass).
//     stores    DG_MOE_GATE_UP: row pair of y gets swiglu16(gate sum, up sum) of its expert; rows of pairs without a valid id are
//               zero-filled.  DG_MOE_DOWN: acc[i][row] (f32, LDS, zero at the start) = fma(gates[pair], d, acc) as the experts come by
//               -- ascending expert id, within one expert ascending pair index --, and after the last expert y = RNE16(acc + residual).
//               The order depends on ids alone: the same inputs give the same bits on every launch.

constexpr int MR_THREADS = 512;
constexpr int MR_WAVES = MR_THREADS / 64;
constexpr int MR_J = 8;                    // router rows per walk over k
constexpr int MR_PASS = 8 * MR_THREADS;    // elements of k per pass
constexpr int MOE_MAX_E = 64;
constexpr int MOE_MAX_TOPK = 8;

struct MoeRouteParams {
  const uint16_t* x;    // [m][k]
  const uint16_t* rw;   // [E][k]
  int32_t* ids;         // [m][top_k]
  float* gates;         // [m][top_k]
  int32_t k, E, top_k;
};

template <typename DT>
__global__ __launch_bounds__(MR_THREADS) void moe_route_kernel(const MoeRouteParams P) {
  __shared__ float part[MR_WAVES][MOE_MAX_E];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint16_t* xr = P.x + row * P.k;
  for (int e0 = 0; e0 < P.E; e0 += MR_J) {
    float acc[MR_J] = {};
    for (int c = tid * 8; c < P.k; c += MR_PASS) {  // (k % 8 == 0: a lane's 8 elements are inside or outside as a whole)
      const u32x4 xv = *reinterpret_cast<const u32x4*>(xr + c);
      u32x4 av[MR_J];
#pragma unroll
      for (int j = 0; j < MR_J; ++j)  // (rows past E re-read row E - 1; their sums are dropped)
        av[j] = *reinterpret_cast<const u32x4*>(P.rw + (int64_t)min(e0 + j, P.E - 1) * P.k + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = DT::lo_f32(xv[e]), hi = DT::hi_f32(xv[e]);
#pragma unroll
        for (int j = 0; j < MR_J; ++j) {
          acc[j] = fmaf(DT::lo_f32(av[j][e]), lo, acc[j]);
          acc[j] = fmaf(DT::hi_f32(av[j][e]), hi, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MR_J; ++j) {
      acc[j] = tgl::wave_sum(acc[j]);
      if (lane == 0 && e0 + j < P.E) part[wave][e0 + j] = acc[j];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const bool in = lane < P.E;
  float l = 0.f;
  if (in) {
#pragma unroll
    for (int w = 0; w < MR_WAVES; ++w) l += part[w][lane];
  }
  const float mx = tgl::wave_max(in ? l : -INFINITY);
  const float ex = in ? expf(l - mx) : 0.f;
  const float p = ex / tgl::wave_sum(ex);
  uint64_t left = P.E == 64 ? ~0ull : ((1ull << P.E) - 1ull);
  int my_id = 0;
  float my_p = 0.f, sel = 0.f;
#pragma unroll
  for (int s = 0; s < MOE_MAX_TOPK; ++s) {
    if (s < P.top_k) {  // (uniform)
      const float cand = ((left >> lane) & 1ull) ? p : -1.f;
      const float best = tgl::wave_max(cand);
      uint64_t c = __ballot(cand == best) & left;
      if (c == 0) c = left;  // NaN (out of contract): the lowest index that is left (top_k <= E: there is one)
      const int idx = __builtin_ctzll(c);
      left &= ~(1ull << idx);
      const float pb = __shfl(p, idx);
      sel += pb;  // s ascending
      if (lane == s) { my_id = idx; my_p = pb; }
    }
  }
  if (lane < P.top_k) {
    P.ids[row * P.top_k + lane] = my_id;
    P.gates[row * P.top_k + lane] = my_p / sel;
  }
}

// ---- the expert-indexed GEMV ----
constexpr int MW_THREADS = 512;
constexpr int MW_WAVES = MW_THREADS / 64;
constexpr int MW_NP = 8;     // pairs per sweep at most
constexpr int MW_D = 4;      // steps per lane in flight
constexpr int MW_MAX_UPW = 16;  // units per workgroup at most (the DOWN accumulators: m x 16 upw floats of LDS)
constexpr int MW_TABLE_BYTES = 65536;

struct MoeW4Params {
  const char* x;         // GATE_UP [m][k]; DOWN [m top_k][k]
  const char* w;         // [E] x stride_w
  const char* qinfo;
  const char* lut;
  char* y;               // GATE_UP [m top_k][wrows / 2]; DOWN [m][wrows]
  const int32_t* ids;    // [m][top_k]
  const float* gates;    // DOWN
  const char* residual;  // DOWN, optional
  int64_t stride_w, stride_qinfo, stride_lut;  // bytes per expert
  int32_t m, top_k, E, wrows, k, ksuper, qtype;
  int32_t sg_shift;      // log2(super-tiles per group)
  int32_t stage;
  int32_t units, upw;    // 16-row units of the matrix, units per workgroup
  int32_t spw;           // super-tiles per wave
  int32_t np;            // pairs per sweep
  int32_t x_pitch, xs_pitch;            // bytes per staged activation row / per row of sums
  int32_t lds_x, lds_xs, lds_red, lds_acc;  // LDS byte offsets
};

template <typename DT>
__global__ void __launch_bounds__(MW_THREADS) moe_w4_kernel(const MoeW4Params p) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u0 = blockIdx.x * p.upw, u1 = min(u0 + p.upw, p.units);
  if (u0 >= u1) return;
  const int nrows = (u1 - u0) * 16;
  const int npairs = p.m * p.top_k;
  const bool down = p.stage == DG_MOE_DOWN;
  const int half_rows = p.wrows >> 1;

  // this lane's pair: its id, or -1 -- the only place an id is read, and nothing below indexes with a value that failed this test
  int id = -1;
  if (lane < npairs) {
    id = p.ids[lane];
    if (id < 0 || id >= p.E) id = -1;
  }
  if (down) {
    for (int i = tid; i < p.m * nrows; i += MW_THREADS) *(lds_fptr)((uint32_t)p.lds_acc + (uint32_t)i * 4u) = 0.f;
  } else {
    uint64_t none = __ballot(lane < npairs && id < 0);
    while (none) {  // (uniform) a pair without a valid expert: a row of zeros
      const int pr = __builtin_ctzll(none);
      none &= none - 1;
      for (int c = tid; c < (u1 - u0) * 8; c += MW_THREADS) *reinterpret_cast<uint16_t*>(p.y + ((int64_t)pr * half_rows + u0 * 8 + c) * 2) = 0;
    }
  }

  const int row_l = lane & 15, sub = lane >> 4, h = sub & 1, ss = sub >> 1;
  const int s_begin = wave * p.spw, s_end = min(s_begin + p.spw, p.ksuper);
  const int nsteps = (p.spw + 1) >> 1;
  const uint32_t colreg = (uint32_t)((lane & 31) * 4);
  const uint32_t lds_x = (uint32_t)p.lds_x, lds_xs = (uint32_t)p.lds_xs, lds_red = (uint32_t)p.lds_red, lds_acc = (uint32_t)p.lds_acc;
  const uint32_t qrow_bytes = (uint32_t)p.wrows * 4u;
  const int tc = tid & 31, thi = tid >> 5;  // table: this thread's column and high nibble

  // ---- the items of this workgroup: (expert, sweep, unit) -- experts ascending, a sweep's units ascending.  The ring of MW_D steps runs
  // ACROSS items: an item occupies a whole number of rounds of MW_D slots (slots past its last step re-read it and are skipped), and its
  // last round refills with the first steps of the NEXT item, so the weight stream does not drain at an item's barriers, table build
  // or -- at a new sweep -- activation staging. ----
  uint64_t present = 0;  // (uniform) experts that some pair selected
  for (int e = 0; e < p.E; ++e) present |= (__ballot(id == e) != 0 ? 1ull : 0ull) << e;
  struct Slot { u32x4 w; uint32_t q; };
  auto lane_w = [&](int e, int unit) -> const char* {
    const int row = unit * 16 + row_l;
    return p.w + (int64_t)e * p.stride_w + ((int64_t)(row >> 3) * p.ksuper * 256 + (row & 7) * 32 + h * 16);
  };
  auto lane_q = [&](int e, int unit) -> const char* { return p.qinfo + (int64_t)e * p.stride_qinfo + (int64_t)(unit * 16 + row_l) * 4; };
  auto load = [&](const char* wl, const char* ql, int i) -> Slot {  // step i of the wave (clamped: a step past the end re-reads, and is not counted)
    const int su = min(s_begin + 2 * min(i, nsteps - 1) + ss, p.ksuper - 1);
    Slot sl;
    sl.w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wl + (uint32_t)su * 256u));
    sl.q = *reinterpret_cast<const uint32_t*>(ql + (uint32_t)(su >> p.sg_shift) * qrow_bytes);
    return sl;
  };
  // the 16 LUT values of this thread's table column for an item (requested one item ahead, like the ring; int4 has none)
  auto load_lut = [&](int e, int unit, u32x4& l0, u32x4& l1) {
    if (p.qtype == TG_Q_INT4) return;
    const char* lsrc = p.lut + (int64_t)e * p.stride_lut + (p.qtype == TG_Q_ANY4_ROWWISE ? (int64_t)(unit * 16 + (tc & 15)) * 32 : 0);
    l0 = reinterpret_cast<const u32x4*>(lsrc)[0];
    l1 = reinterpret_cast<const u32x4*>(lsrc)[1];
  };
  const int rounds = (nsteps + MW_D - 1) / MW_D;
  if (present) {
    int e = __builtin_ctzll(present), unit = u0;
    uint64_t mask = __ballot(id == e);  // the expert's pairs not yet served
    bool new_sweep = true;
    const char* wl = lane_w(e, unit);
    const char* ql = lane_q(e, unit);
    Slot ring[MW_D];
#pragma unroll
    for (int d = 0; d < MW_D; ++d) ring[d] = load(wl, ql, d);
    u32x4 l0 = {0, 0, 0, 0}, l1 = {0, 0, 0, 0};
    load_lut(e, unit, l0, l1);
    int pj[MW_NP], cnt = 0;
#pragma unroll
    for (int j = 0; j < MW_NP; ++j) pj[j] = 0;
    while (true) {
      if (new_sweep) {  // up to np pairs of this expert
        cnt = 0;
#pragma unroll
        for (int j = 0; j < MW_NP; ++j) {
          if (j < p.np && mask) {
            pj[j] = __builtin_ctzll(mask);
            mask &= mask - 1;
            cnt = j + 1;
          }
        }
      }
      // the next item: the sweep's next unit, else the expert's next sweep, else the next selected expert
      int ne = e, nunit = unit + 1;
      bool has_next = true;
      if (nunit == u1) {
        nunit = u0;
        if (!mask) {
          const uint64_t rest = e >= 63 ? 0ull : present & ~((2ull << e) - 1ull);
          if (rest) ne = __builtin_ctzll(rest);
          else has_next = false;
        }
      }
      const char* wln = has_next ? lane_w(ne, nunit) : wl;
      const char* qln = has_next ? lane_q(ne, nunit) : ql;
      u32x4 l0n = l0, l1n = l1;
      if (has_next) load_lut(ne, nunit, l0n, l1n);
      if (new_sweep) {
        __syncthreads();  // the previous sweep's reads of the staged rows are over
#pragma unroll
        for (int j = 0; j < MW_NP; ++j) {
          if (j < cnt) {  // (uniform)
            const char* xr = p.x + (int64_t)(down ? pj[j] : pj[j] / p.top_k) * p.k * 2;
            for (int u = tid; u < p.ksuper * 2; u += MW_THREADS) {  // a thread stages one half super-tile: four 16-byte pieces and their sum
              const int su = u >> 1, hh = u & 1;
              float sum = 0.f;
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const int jc = t >> 1, q = 2 * hh + (t & 1);
                const char* src = xr + (su * 2 + jc) * 64 + q * 4;
                const uint32_t d0 = *reinterpret_cast<const uint32_t*>(src), d1 = *reinterpret_cast<const uint32_t*>(src + 16);
                const uint32_t d2 = *reinterpret_cast<const uint32_t*>(src + 32), d3 = *reinterpret_cast<const uint32_t*>(src + 48);
                u32x4 o;
                o[0] = __builtin_amdgcn_perm(d1, d0, 0x05040100u);  // x[2q]     x[2q+8]
                o[1] = __builtin_amdgcn_perm(d3, d2, 0x05040100u);  // x[2q+16]  x[2q+24]
                o[2] = __builtin_amdgcn_perm(d1, d0, 0x07060302u);  // x[2q+1]   x[2q+9]
                o[3] = __builtin_amdgcn_perm(d3, d2, 0x07060302u);  // x[2q+17]  x[2q+25]
#pragma unroll
                for (int v = 0; v < 4; ++v) sum = dot2_ones<DT>(o[v], sum);
                *(lds_u32x4ptr)(lds_x + (uint32_t)(j * p.x_pitch + (su * 8 + jc * 4 + q) * 16)) = o;
              }
              *(lds_fptr)(lds_xs + (uint32_t)(j * p.xs_pitch + u * 4)) = sum;
            }
          }
        }
      }
      // ---- the pass's pair table: entry[byte][column] = (lut[byte & 15], lut[byte >> 4]) of row unit * 16 + (column & 15) ----
      uint32_t lp[8];
      if (p.qtype == TG_Q_INT4) {
#pragma unroll
        for (int v = 0; v < 16; v += 2) lp[v >> 1] = DT::pack2((float)(v - 8), (float)(v - 7));
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) { lp[v] = l0[v]; lp[4 + v] = l1[v]; }
      }
      {
        uint32_t hsel = lp[0];
#pragma unroll
        for (int v = 1; v < 8; ++v) hsel = (thi >> 1) == v ? lp[v] : hsel;
        const uint32_t hv = (thi & 1) ? (hsel & 0xffff0000u) : (hsel << 16);
        const lds_u32ptr tb = (lds_u32ptr)((uint32_t)(thi * 16 * 256 + tc * 4));
#pragma unroll
        for (int lo = 0; lo < 16; ++lo) {
          const uint32_t lv = (lo & 1) ? (lp[lo >> 1] >> 16) : (lp[lo >> 1] & 0xffffu);
          tb[lo * 64] = lv | hv;
        }
      }
      __syncthreads();  // table and (new sweep) staged rows are there; the previous item's reads of `red` are over

      // ---- stream the expert's 16 rows of this unit ----
      float acc[MW_NP];
#pragma unroll
      for (int j = 0; j < MW_NP; ++j) acc[j] = 0.f;
      auto consume = [&](const Slot& sl, int i) {
        const int su_l = s_begin + 2 * i + ss;
        const bool on = su_l < s_end;  // (per lane: the second super-tile of a step may lie past the wave's slice)
        const int su = min(su_l, p.ksuper - 1);
        const uint32_t xa = lds_x + (uint32_t)(su * 128 + h * 32);
        const uint32_t xsa = lds_xs + (uint32_t)((su * 2 + h) * 4);
        uint32_t ev[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int jc = u >> 1, qq = u & 1;  // 32-k chunk of the super-tile, quad of the half
          const uint32_t w = sl.w[qq * 2 + jc];
#pragma unroll
          for (int v = 0; v < 4; ++v) ev[u][v] = *(lds_cu32ptr)(__builtin_amdgcn_perm(w, colreg, 0x0c0c0400u + ((uint32_t)v << 8)));
        }
        const float sc = DT::lo_f32(sl.q), zz = DT::hi_f32(sl.q);
#pragma unroll
        for (int j = 0; j < MW_NP; ++j) {
          if (j < cnt) {  // (uniform)
            float dsum = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const u32x4 xf = *(lds_cu32x4ptr)(xa + (uint32_t)(j * p.x_pitch + (u >> 1) * 64 + (u & 1) * 16));
#pragma unroll
              for (int v = 0; v < 4; ++v) dsum = dot2<DT>(ev[u][v], xf[v], dsum);
            }
            const float xs = *(lds_cfptr)(xsa + (uint32_t)(j * p.xs_pitch));
            const float t = __builtin_fmaf(zz, xs, __builtin_fmaf(sc, dsum, acc[j]));
            acc[j] = on ? t : acc[j];
          }
        }
      };
      for (int r = 0; r < rounds; ++r) {
        const bool last = r + 1 == rounds;  // (uniform) the item's last round refills with the next item's first steps
        const char* wr = last ? wln : wl;
        const char* qr = last ? qln : ql;
#pragma unroll
        for (int d = 0; d < MW_D; ++d) {
          if (r * MW_D + d < nsteps) consume(ring[d], r * MW_D + d);
          ring[d] = load(wr, qr, last ? d : (r + 1) * MW_D + d);
        }
      }
      // the four sub-slots of a row sit in lanes row + 16 sub: every lane gets the wave's sum
#pragma unroll
      for (int j = 0; j < MW_NP; ++j) {
        if (j < cnt) {
          const float v = tgl::halves32_sum(tgl::rows16_sum(acc[j]));
          if (lane < 16) *(lds_fptr)(lds_red + (uint32_t)(((wave * MW_NP + j) * 16 + lane) * 4)) = v;
        }
      }
      __syncthreads();
      auto red_sum = [&](int j, int r) -> float {  // wave order
        float s = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < MW_WAVES; ++w8) s += *(lds_cfptr)(lds_red + (uint32_t)(((w8 * MW_NP + j) * 16 + r) * 4));
        return s;
      };
      if (!down) {
        if (tid < cnt * 8) {  // thread = (pair of the sweep, gate row): rows r and r + 8 of the unit are a gate / up pair
          const int j = tid >> 3, r = tid & 7;
          int pr = pj[0];
#pragma unroll
          for (int v = 1; v < MW_NP; ++v) pr = j == v ? pj[v] : pr;
          *reinterpret_cast<uint16_t*>(p.y + ((int64_t)pr * half_rows + unit * 8 + r) * 2) = swiglu16<DT>(red_sum(j, r), red_sum(j, r + 8));
        }
      } else if (tid < 16) {  // thread = row of the unit; the sweep's pairs in ascending order (two of them may belong to one token)
#pragma unroll
        for (int j = 0; j < MW_NP; ++j) {
          if (j < cnt) {
            const uint32_t a = lds_acc + (uint32_t)(((pj[j] / p.top_k) * nrows + (unit - u0) * 16 + tid) * 4);
            *(lds_fptr)a = __builtin_fmaf(p.gates[pj[j]], red_sum(j, tid), *(lds_cfptr)a);
          }
        }
      }
      if (!has_next) break;
      new_sweep = unit + 1 == u1;
      if (ne != e) {
        e = ne;
        mask = __ballot(id == e);
      }
      unit = nunit;
      wl = wln;
      ql = qln;
      l0 = l0n;
      l1 = l1n;
    }
  }
  if (down) {
    __syncthreads();
    for (int i = tid; i < p.m * nrows; i += MW_THREADS) {
      const int a = i / nrows, r = i - a * nrows;
      const int64_t o = (int64_t)a * p.wrows + u0 * 16 + r;
      float v = *(lds_cfptr)(lds_acc + (uint32_t)i * 4u);
      if (p.residual) v += DT::to_f32(*reinterpret_cast<const uint16_t*>(p.residual + o * 2));
      *reinterpret_cast<uint16_t*>(p.y + o * 2) = DT::from_f32(v);
    }
  }
}
