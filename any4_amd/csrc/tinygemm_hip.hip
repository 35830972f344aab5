// tinygemm_hip.hip -- hand-written gfx950 (MI355X / CDNA4) kernels + the C ABI of
// include/tinygemm_hip.h.  Written for wave64 + v_mfma_f32_16x16x32_{bf16,f16}; there is no
// CUDA path, no hipify output and no multi-backend dispatch in this file.
//
// Reference behaviour being replaced (facebookresearch/any4 @ 2025-07-18, file:line):
//   tinygemm_lib/TinyGemmImpl.cuh:23-345      the split-K tile kernel
//   tinygemm_lib/MatrixLayoutA.cuh:375-816    weights-as-A int4 load + dequant
//   tinygemm_lib/MatrixLayoutB.cuh:686-1101   weights-as-B int4 load + dequant
//   tinygemm_lib/Dequantization.cuh:17-178, 331-351
//   tinygemm_lib/TinyGemm_int4.cu:294-548     host validation / dispatch
//   tinygemm_lib/TinyGemm_bf16.cu:163-327     16-bit weights
//   tinygemm_lib/TinyGemmConvert{A,B}.cu      layout / packing kernels
//   tinygemm_lib/TinyGemmDequantize.cu:19-58  debug dequant op
//
// Design notes live in DESIGN.md; the short version of the GEMM kernel:
//   * one workgroup = one 16-row weight tile, split-K over its waves (step = one 16-byte
//     packed-weight load per lane = 1 KiB per wave, streamed with non-temporal loads);
//   * W is the MFMA A operand (16 weight rows x 32 k), X the B operand (32 k x 16 activation
//     rows).  The reference's packed words are consumed AS STORED: a 2x2 / 4x4 word transpose
//     between the four 16-lane rows of the wave (v_permlane16_swap / v_permlane32_swap) gives
//     every lane a contiguous k-chunk, so the X fragment is one contiguous 16-byte load;
//   * the 16-entry LUT lives in LDS as f32, one private bank column per lane
//     ([16 entries][64 lanes]) so the 8 data-dependent lookups per word never conflict;
//     the lookup address is built with one v_perm_b32 per nibble;
//   * dequant = v_fma_f32(lut, scale, zero) then v_cvt_pk_bf16_f32 (RNE): the f32 product of
//     two 16-bit floats is exact, so this equals the reference's single-rounding bf16 fma;
//   * fp32 partial tiles meet in LDS, a fixed-order sum gives a deterministic result.

#include <stddef.h>
#include "tg_common.cuh"

namespace {

#include "w8_gemm.cuh"

#include "f16_gemm.cuh"
#include "tg_convert.cuh"


// Launch geometry.  Streaming shapes (many tiles) use 8-wave workgroups, two per CU, and the
// smallest split-K that still puts >= ~16 waves on every CU; a single small matrix (one tile per
// CU) uses one 16-wave workgroup per tile with split-K 16.
struct Geometry {
  int waves, splitk;
};

inline Geometry pick_geometry(int64_t rowtiles, int64_t coltiles, int64_t batch, int64_t nsteps) {
  const int64_t tiles = rowtiles * coltiles * batch;
  const int64_t want_waves = 256 * 16;  // 256 CUs x 16 waves
  Geometry g;
  if (tiles * 8 <= want_waves) {
    g.waves = 16;
    g.splitk = 16;
  } else {
    g.waves = 8;
    int sk = 1;
    while (sk < 8 && tiles * sk * 2 <= want_waves) sk *= 2;
    g.splitk = sk;
  }
  while (g.splitk > 1 && g.splitk > nsteps) g.splitk >>= 1;
  return g;
}


template <typename DT, bool LAYOUT_A, int I>
int launch_w8(const GemmParams& p) {
  constexpr int WAVES = 8;
  const int64_t tiles = (int64_t)p.rowtiles * coltiles(p) * p.batch;
  const int nsteps = (p.k / 16 + 3) / 4;
  int sk = 1;
  while (sk < WAVES && tiles * sk < 256 * 16 && sk * 2 <= nsteps) sk *= 2;
  const int tpb = WAVES / sk;
  dim3 grid((unsigned)((p.rowtiles + tpb - 1) / tpb), (unsigned)coltiles(p), (unsigned)p.batch);
  hipLaunchKernelGGL((w8_gemm_kernel<DT, LAYOUT_A, I, WAVES>), grid, dim3(WAVES * 64), 0, p.st, splitk_params(p, sk));
  return launch_status();
}


// The dispatcher's half of the workspace protocol: a family is offered the call with ws_need = 0, and assigns it only where it accepts.
template <typename F>
int offer(F& family, GemmParams& p) {
  p.ws_need = 0;
  return family(p);
}

// Dispatch of one validated 4-bit GEMM call to a kernel family (each family's launch path is its own translation unit, tg_common.cuh).
int launch_w4(GemmParams& p) {
  const bool LAYOUT_A = !p.on_right;
  const int KSTEP = LAYOUT_A ? 64 : 128;
  const Geometry g = pick_geometry(p.rowtiles, coltiles(p), p.batch, (p.k + KSTEP - 1) / KSTEP);
  // TG_NUM_FAST, weights on the B side: the pair-table kernel (group-scaled numerics) whenever its LDS plan fits
  // (mx4 in BOTH numerics: its dequantised weights, fp4 * 2^(e - 127), are exact 16-bit values however they are formed, so the
  //  pair-table kernels -- which convert them with v_cvt_scalef32_pk_bf16_fp4 -- ARE the reference arithmetic for it)
  if (p.numerics == TG_NUM_FAST || p.numerics == TG_NUM_FAST_MFMA || p.qmx) {
    int rc;
    if (!LAYOUT_A) {
      // one layer per launch with up to 4 activation rows (a decode step's GEMMs): its own kernel (w4_gemv.cuh)
      rc = p.numerics == TG_NUM_FAST_MFMA ? (int)TG_PAIR_NA : offer(tgx::gemv, p);  // (w4_gemv contracts with v_dot2)
      if (rc != TG_PAIR_NA) return rc;
      // STACKED launches of one activation row in the default numerics: the contraction tg_m1_default_contraction() names
      // (TG_M1_DEFAULT_MFMA; TG_NUM_FAST_DOT2 / TG_NUM_FAST_MFMA pin either one for A/B runs -- p.dot2 is set by the entry point)
      if (TG_M1_DEFAULT_MFMA && p.numerics == TG_NUM_FAST && p.m == 1 && !p.dot2 && !p.qmx) p.numerics = TG_NUM_FAST_MFMA;
      rc = offer(tgx::pair_xr, p);
      if (rc != TG_PAIR_NA) return rc;
      // one layer per launch with more 16-row tiles than CUs (5 ... 16 rows, k = 4096): in front of the persistent kernel, which would
      // take it from 192 64-row items on (12288 rows: 15.6 us per graph node)
      rc = offer(tgx::pair16_loop, p);
      if (rc != TG_PAIR_NA) return rc;
    }
    rc = LAYOUT_A ? offer(tgx::pair_a, p) : offer(tgx::pair, p);
    if (rc != TG_PAIR_NA) return rc;
    if (!LAYOUT_A) {
      if (p.m > 8) {
        rc = offer(tgx::pair_b16, p);
        if (rc != TG_PAIR_NA) return rc;
      }
      rc = offer(tgx::pair16, p);
      if (rc != TG_PAIR_NA) return rc;
    }
  }
  if (p.x_tc || p.y_tc) return TG_E_LAYOUT;  // only the pair-table kernels read / write fragment order themselves
  if (p.norm_w || p.epilogue) return TG_E_FUSION;  // ... and only they carry the fused norm / SwiGLU stages
#ifdef TG_DEV_MIN  // developer A/B builds carry the pair-table kernels only (a third of the build time)
  return TG_E_SHAPE;
#else
  // Streaming shapes go to the lane-owns-group kernel when the quantisation group covers at least one
  // unit of its walk (Bint4: g >= 128, Aint4: g >= 64).
  // m = 1 always streams: with private X slabs its split-K variants beat the latency kernel down to one matrix
  if ((g.waves == 8 || p.m == 1) && (1 << p.gshift) >= (LAYOUT_A ? 64 : 128)) return tgx::stream(p);
  if (p.dry) return TG_PLAN_SPLITK;
  return tgx::splitk(p, g.waves, g.splitk);
#endif
}

}  // namespace


extern "C" {

int tg_abi_version(void) { return TG_ABI_VERSION; }
int tg_m1_default_contraction(void) { return TG_M1_DEFAULT_MFMA ? 1 : 0; }

const char* tg_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case TG_E_NULL: return "a required tensor is missing (null data pointer)";
    case TG_E_INNER_K: return "innerKTiles is not valid for this layout (Aint4/A: 1,2,4; Bint4: 2,4,8; B16: 1,2; A16: 1)";
    case TG_E_K_DIV: return "k must be a multiple of 32 and of innerKTiles * 16 (isEvenDivisor(k, 32), isEvenDivisor(kTiles, innerKTiles))";
    case TG_E_GROUP: return "qGroupSize must be 32, 64, 128 or 256 and divide k";
    case TG_E_DTYPE: return "activation dtype must be bfloat16 or float16 (mx4: bfloat16 only)";
    case TG_E_QTYPE: return "unknown 4-bit quantization type";
    case TG_E_SHAPE: return "inconsistent or non-positive sizes";
    case TG_E_ALIGN: return "device buffers must be 16-byte aligned";
    case TG_E_DEVICE: return "could not select the requested device";
    case TG_E_SIZE: return "an operand is too large for the kernels' 32-bit byte offsets (activations, packed weights or quantisation info of one problem must stay below 2 GiB; at most 65535 16-row activation tiles)";
    case TG_E_INTERNAL: return "internal error: a kernel that addresses LDS from offset 0 was built with static LDS";
    case TG_E_STRUCT: return "tg_w4_gemm.struct_bytes must be sizeof(struct tg_w4_gemm) of the header the caller was built with (at least the ABI-1 prefix, at most this library's struct); dg_attn.struct_bytes must be this library's sizeof(struct dg_attn)";
    case TG_E_FUSION: return "no kernel with the requested fused stage (norm_weight / epilogue) for this problem: run that stage as its own launch (include/decode_glue_hip.h)";
    case TG_E_LAYOUT: return "no kernel for this layout / cache layout: fragment-order activations / outputs (x_layout, y_layout) are not available for this problem (convert with tg_convert_{from,to}_A16 around a row-major call), or dg_attn names a (kernel, flags) pair that DG_ATTN_FLAVOURS does not list";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown tinygemm error";
  }
}

int tg_convert_to_Bint4(const int32_t* in, int64_t n, int64_t k, int I, int32_t* out, int device, tg_stream_t stream) {
  if (!in || !out) return TG_E_NULL;
  if (!(I == 2 || I == 4 || I == 8)) return TG_E_INNER_K;  // ConvertB.cu:327
  if (n <= 0 || k <= 0) return TG_E_SHAPE;
  if (k % (I * 16) != 0) return TG_E_K_DIV;               // ConvertB.cu:337
  if (!aligned16(in)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t nTiles = cdiv(n, 8), ksuper = k / (I * 16);
  dim3 grid((unsigned)cdiv(k, 512), (unsigned)nTiles);
  hipStream_t st = (hipStream_t)stream;
  return pick<2, 4, 8>(I, [&](auto I_) {
    hipLaunchKernelGGL(pack_Bint4_kernel<decltype(I_)::value>, grid, dim3(256), 0, st, in, out, n, k, ksuper);
    return launch_status();
  });
}

int tg_convert_to_Aint4(const int32_t* in, int64_t m, int64_t k, int I, int32_t* out, int device, tg_stream_t stream) {
  if (!in || !out) return TG_E_NULL;
  if (!(I == 1 || I == 2 || I == 4)) return TG_E_INNER_K;  // ConvertA.cu:299
  if (m <= 0 || k <= 0) return TG_E_SHAPE;
  if (!aligned16(in)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t mTiles = cdiv(m, 16), ksuper = cdiv(k, I * 16);
  dim3 grid((unsigned)cdiv(ksuper * I * 16, 256), (unsigned)mTiles);
  hipStream_t st = (hipStream_t)stream;
  return pick<1, 2, 4>(I, [&](auto I_) {
    hipLaunchKernelGGL(pack_Aint4_kernel<decltype(I_)::value>, grid, dim3(256), 0, st, in, out, m, k, ksuper);
    return launch_status();
  });
}

int tg_unpack_int4(const int32_t* packed, int layout_a, int64_t rows, int64_t k, int I, int32_t* codes, int device, tg_stream_t stream) {
  if (!packed || !codes) return TG_E_NULL;
  if (layout_a ? !(I == 1 || I == 2 || I == 4) : !(I == 2 || I == 4 || I == 8)) return TG_E_INNER_K;
  if (rows <= 0 || k <= 0 || rows * k / 256 > INT32_MAX) return TG_E_SHAPE;
  if (!layout_a && k % (16 * I) != 0) return TG_E_K_DIV;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t ksuper = cdiv(k, 16 * I);
  hipLaunchKernelGGL(unpack_int4_kernel, dim3((unsigned)cdiv(rows * k, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(packed), codes, layout_a, rows, k, I, ksuper);
  return launch_status();
}

int tg_dequant_w4(const void* packed, const void* qinfo, const void* lut, int64_t wrows, int64_t k, int group, int qtype, int dtype, int I, void* out,
                  int device, tg_stream_t stream) {
  return tg_dequant_w4_panel(packed, qinfo, lut, wrows, wrows, k, group, qtype, dtype, I, out, device, stream);
}

int tg_dequant_w4_panel(const void* packed, const void* qinfo, const void* lut, int64_t wrows, int64_t wrows_q, int64_t k, int group, int qtype,
                        int dtype, int I, void* out, int device, tg_stream_t stream) {
  if (!packed || !qinfo || !out) return TG_E_NULL;
  if (wrows_q < wrows) return TG_E_SHAPE;
  if (!(qtype == TG_Q_INT4 || qtype == TG_Q_ANY4_GLOBAL || qtype == TG_Q_ANY4_ROWWISE)) return TG_E_QTYPE;
  if (qtype != TG_Q_INT4 && !lut) return TG_E_NULL;
  if (!(dtype == TG_BF16 || dtype == TG_F16)) return TG_E_DTYPE;
  if (!(I == 2 || I == 4 || I == 8)) return TG_E_INNER_K;
  if (wrows <= 0 || k <= 0 || wrows % 8 != 0 || wrows > INT32_MAX || k > INT32_MAX) return TG_E_SHAPE;
  if (k % (16 * I) != 0 || k % 32 != 0) return TG_E_K_DIV;
  if (k % 512 != 0) return TG_E_K_DIV;   // (a wave of the kernel is 512 consecutive k of one row)
  if (!(group == 32 || group == 64 || group == 128 || group == 256) || k % group != 0) return TG_E_GROUP;
  if (!aligned16(packed) || !aligned16(out) || (reinterpret_cast<uintptr_t>(qinfo) & 3u) || (lut && !aligned16(lut))) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t ksuper = k / (16 * I);
  const int gshift = group_shift(group);
  const int chk = k % 2048 == 0 ? 4 : 1;   // chunks of 512 k per wave
  const unsigned bs = k / 8 / chk < 256 ? (unsigned)(k / 8 / chk) : 256u;   // (a row's threads: a multiple of 64)
  const dim3 grid((unsigned)cdiv(k / 8 / chk, 256), (unsigned)(wrows < 65535 ? wrows : 65535), (unsigned)cdiv(wrows, 65535));
  return pick_dt(dtype, [&](auto DT_) {
    return pick<2, 4, 8>(I, [&](auto I_) {
      return pick<4, 1>(chk, [&](auto CHK_) {
        hipLaunchKernelGGL((dequant_w4_kernel<decltype(DT_), decltype(I_)::value, decltype(CHK_)::value>), grid, dim3(bs), 0, (hipStream_t)stream,
                           (const uint32_t*)packed, (const uint16_t*)qinfo, (const uint16_t*)lut, (uint16_t*)out, wrows, wrows_q, k, ksuper, gshift, qtype);
        return launch_status();
      });
    });
  });
}

int tg_convert_to_A16(const void* rm, int64_t m, int64_t k, void* tc, int device, tg_stream_t stream) {
  if (!rm || !tc) return TG_E_NULL;
  if (m <= 0 || k <= 0) return TG_E_SHAPE;
  if (!aligned16(tc)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t mT = cdiv(m, 16), kT = cdiv(k, 16);
  hipLaunchKernelGGL(to_A16_kernel, dim3((unsigned)cdiv(mT * kT * 32, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)rm, (uint16_t*)tc, m, k, mT, kT);
  return launch_status();
}

int tg_convert_from_A16(const void* tc, int64_t m, int64_t k, void* rm, int device, tg_stream_t stream) {
  if (!rm || !tc) return TG_E_NULL;
  if (m <= 0 || k <= 0) return TG_E_SHAPE;
  if (!aligned16(tc)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t mT = cdiv(m, 16), kT = cdiv(k, 16);
  hipLaunchKernelGGL(from_A16_kernel, dim3((unsigned)cdiv(mT * kT * 32, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)tc, (uint16_t*)rm, m, k, mT, kT);
  return launch_status();
}

int tg_convert_to_B16(const void* rm, int64_t n, int64_t k, int I, void* tc, int device, tg_stream_t stream) {
  if (!rm || !tc) return TG_E_NULL;
  if (!(I == 1 || I == 2)) return TG_E_INNER_K;  // ConvertB.cu:84
  if (n <= 0 || k <= 0) return TG_E_SHAPE;
  if (!aligned16(tc)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t nT = cdiv(n, 8), totalK = cdiv(k, 16 * I) * I;
  hipLaunchKernelGGL(to_B16_kernel, dim3((unsigned)cdiv(nT * totalK * 32, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)rm, (uint16_t*)tc, n, k, nT, totalK, I);
  return launch_status();
}

int tg_convert_from_B16(const void* tc, int64_t n, int64_t k, int I, void* rm, int device, tg_stream_t stream) {
  if (!rm || !tc) return TG_E_NULL;
  if (!(I == 1 || I == 2)) return TG_E_INNER_K;
  if (n <= 0 || k <= 0) return TG_E_SHAPE;
  if (!aligned16(tc)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t nT = cdiv(n, 8), kT = cdiv(k, 16), outerK = cdiv(k, 16 * I);
  hipLaunchKernelGGL(from_B16_kernel, dim3((unsigned)cdiv(nT * kT * 32, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)tc, (uint16_t*)rm, n, k, nT, kT, outerK, I);
  return launch_status();
}

int tg_dequant_int4(const int32_t* in, int64_t count, void* out_bf16, int device, tg_stream_t stream) {
  if (!in || !out_bf16) return TG_E_NULL;
  if (count <= 0) return TG_E_SHAPE;
  if (!aligned16(out_bf16)) return TG_E_ALIGN;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t blocks = cdiv(count, 256);
  hipLaunchKernelGGL(dequant_int4_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                     (hipStream_t)stream, in, (u32x4*)out_bf16, count);
  return launch_status();
}

// The caller's struct, as long as IT says it is (tg_w4_gemm.struct_bytes), into a zero-filled struct of this library's length:
// fields the caller's header did not have read as zero = off.  Never reads past struct_bytes.
static int take_args(const tg_w4_gemm* a, tg_w4_gemm* full) {
  if (!a) return TG_E_NULL;
  const size_t prefix = offsetof(tg_w4_gemm, stride_y) + sizeof(a->stride_y);  // ABI 1
  const size_t n = a->struct_bytes;
  if (n < prefix || n > sizeof(tg_w4_gemm) || a->struct_reserved != 0) return TG_E_STRUCT;
  memset(full, 0, sizeof(*full));
  memcpy(full, a, n);
  return 0;
}

// ---- the preconditions of a tg_w4_gemm, for the four entry points that take one -----------------------------------------------
// `a` is the zero-extended struct (take_args).  Return codes AND their precedence are ABI: a struct that breaks several preconditions
// gets the code of the first check below that fails.  Where an entry point's order differs from tg_gemm_w4's (dx says what it does not
// do before it looks at the sizes; w8 looks at the sizes before the batch stride of the bias and the workspace), its checks sit at
// that entry's own place.  dq (tg_gemm_w4_dq) takes the FORWARD call's struct and checks it as dx does, except that `y` is not read
// and mx4 -- no float parameters -- is refused.
enum GemmEntry { ENTRY_W4, ENTRY_DX, ENTRY_W8, ENTRY_DQ };

static bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

static bool bad_w_format(const tg_w4_gemm* a) {
  return !(a->w_format == TG_WFMT_M16N8K16 || a->w_format == TG_WFMT_ROWS) || (a->w_format && a->w_on_right) || a->reserved6 != 0;
}
static bool bad_numerics(const tg_w4_gemm* a) {
  return !(a->numerics == TG_NUM_FAST || a->numerics == TG_NUM_REFERENCE || a->numerics == TG_NUM_FAST_MFMA || a->numerics == TG_NUM_FAST_DOT2) ||
         a->reserved != 0;
}
static bool bad_workspace(const tg_w4_gemm* a) { return a->workspace && (!aligned16(a->workspace) || a->workspace_bytes < 0); }
static bool bad_bias_row_stride(const tg_w4_gemm* a) { return a->bias_row_stride < 0 || (a->bias_row_stride && !a->bias) || (a->bias_row_stride & 3); }

// the kernels address one problem's operands with 32-bit byte offsets
static bool too_large(const tg_w4_gemm* a, GemmEntry e) {
  const int64_t lim = (int64_t)1 << 31;
  const int64_t w_bytes = e == ENTRY_W8 ? a->wrows * a->k : a->wrows * a->k / 2;
  if (a->m * a->k * 2 >= lim || w_bytes >= lim || (a->k / a->group) * a->wrows * 4 >= lim) return true;
  // dx: its output is addressed that way as well, and its grid has no dimension of 16-row activation tiles
  return e == ENTRY_DX || e == ENTRY_DQ ? a->m * a->wrows * 2 >= lim : cdiv(a->m, 16) > 65535;
}

static int check_gemm(const tg_w4_gemm* a, GemmEntry e) {
  const bool dq = e == ENTRY_DQ, dx = e == ENTRY_DX || dq, w8 = e == ENTRY_W8;
  if (!a->x || !a->w || !a->qinfo || (!dq && !a->y)) return TG_E_NULL;
  // w8: its own quantisation type -- no LUT, not mx4, so the LUT and mx4 checks below cannot fail for it
  if (w8 ? a->qtype != TG_Q_INT8 : (a->qtype < TG_Q_INT4 || a->qtype > TG_Q_MX4)) return TG_E_QTYPE;
  if (dq && a->qtype == TG_Q_MX4) return TG_E_QTYPE;
  if ((a->qtype == TG_Q_ANY4_GLOBAL || a->qtype == TG_Q_ANY4_ROWWISE) && !a->lut) return TG_E_NULL;
  if (!(a->dtype == TG_BF16 || a->dtype == TG_F16)) return TG_E_DTYPE;
  if (a->qtype == TG_Q_MX4 && a->dtype != TG_BF16) return TG_E_DTYPE;  // TinyGemm_int4.cu:758,782
  if (dx) {
    // one problem, no fused stage, row-major dY / dX, Bint4 words; `numerics` is accepted and ignored, but must be a valid value
    if (a->batch > 1) return TG_E_SHAPE;
    if (a->bias || a->bias_row_stride || a->norm_weight || a->epilogue) return TG_E_FUSION;
    if (a->x_layout != TG_LAYOUT_RM || a->y_layout != TG_LAYOUT_RM) return TG_E_LAYOUT;
    if (bad_w_format(a)) return TG_E_SHAPE;
    if (!a->w_on_right && a->w_format != TG_WFMT_ROWS) return TG_E_LAYOUT;   // the reference's Aint4 words: repack to the native format
    if (bad_numerics(a)) return TG_E_SHAPE;
  }
  if (a->m <= 0 || a->wrows <= 0 || a->k <= 0 || a->m > INT32_MAX || a->wrows > INT32_MAX || a->k > INT32_MAX) return TG_E_SHAPE;
  // innerKTiles of the packed layout.  Bint4: 2, 4, 8; Aint4: 1, 2, 4 (TinyGemm_int4.cu); Bint8: 1, 2, 4; Aint8: 1, 2 (TinyGemm_int8.cu:262, 286)
  const int I = a->inner_k_tiles;
  const bool right = a->w_on_right != 0;
  const int i_min = !w8 && right ? 2 : 1, i_max = w8 ? (right ? 4 : 2) : (right ? 8 : 4);
  if (!(I == 1 || I == 2 || I == 4 || I == 8) || I < i_min || I > i_max) return TG_E_INNER_K;
  // TinyGemmImpl.cuh:370-376: kTiles % innerKTiles == 0, k % 32 == 0
  if (a->k % 32 != 0 || a->k % (16 * I) != 0) return TG_E_K_DIV;
  const int g = a->group;
  if (!(g == 32 || g == 64 || g == 128 || g == 256) || a->k % g != 0) return TG_E_GROUP;  // TinyGemm_int4.cu:379-387, TinyGemm_int8.cu:293-301
  if (a->wrows % (right ? 8 : 16) != 0) return TG_E_SHAPE;                                 // whole tiles of the packed tensor
  if (e == ENTRY_W4 && bad_w_format(a)) return TG_E_SHAPE;   // (w8 has one format per side and does not read the field)
  // x: 16-byte loads of the activation fragments (rows are k * 2 bytes with k % 32 == 0).  w: 16-byte loads of the 4-bit words, 4-byte
  // loads of the 8-bit ones.  y: dx stores 16 bytes per lane, w8 four rows (8 bytes), the 4-bit kernels' stores need the element's own
  // alignment only.  qinfo: (scale, zero) pairs.  LUT rows are read as two 16-byte vectors (w8 has none and ignores the pointer).
  if (misaligned(a->x, 16) || misaligned(a->w, w8 ? 4 : 16) || misaligned(a->qinfo, 4) || misaligned(a->y, dq ? 1 : dx ? 16 : w8 ? 8 : 1)) return TG_E_ALIGN;
  if (w8 && a->batch > 1 && (a->stride_x & 15)) return TG_E_ALIGN;   // (w4 checks its batch strides further down, behind the fused stages)
  if (!w8 && a->lut && misaligned(a->lut, 16)) return TG_E_ALIGN;
  if (a->bias && misaligned(a->bias, 8)) return TG_E_ALIGN;          // (dx: no bias got this far)
  switch (e) {
    case ENTRY_W4: {
      const bool on_right = right || a->w_format == TG_WFMT_ROWS;    // (make_params)
      if (bad_numerics(a)) return TG_E_SHAPE;
      if (bad_workspace(a)) return TG_E_ALIGN;
      if (!(a->x_layout == TG_LAYOUT_RM || a->x_layout == TG_LAYOUT_TC_A) || !(a->y_layout == TG_LAYOUT_RM || a->y_layout == TG_LAYOUT_TC_A)) return TG_E_LAYOUT;
      if ((a->x_layout || a->y_layout) && (!on_right || a->m % 16 != 0 || a->bias)) return TG_E_LAYOUT;
      if (bad_bias_row_stride(a)) return TG_E_SHAPE;
      if (!(a->epilogue == TG_EPI_NONE || a->epilogue == TG_EPI_SWIGLU)) return TG_E_SHAPE;
      if (a->norm_weight && !aligned16(a->norm_weight)) return TG_E_ALIGN;
      // the fused stages exist in the TG_NUM_FAST pair-table kernels only (row-major operands)
      if ((a->norm_weight || a->epilogue) && (a->numerics == TG_NUM_REFERENCE || a->x_layout || a->y_layout)) return TG_E_FUSION;
      if (a->norm_weight && a->k % 2048 != 0) return TG_E_FUSION;
      if (a->epilogue == TG_EPI_SWIGLU && (!on_right || a->bias || a->wrows % 16 != 0)) return TG_E_FUSION;
      if (a->batch > 1 && ((a->stride_x | a->stride_w | a->stride_lut) & 15)) return TG_E_ALIGN;
      if (a->batch > 1 && a->bias && (a->stride_bias & 7)) return TG_E_ALIGN;
      return too_large(a, e) ? (int)TG_E_SIZE : 0;
    }
    case ENTRY_DX:
    case ENTRY_DQ:
      if (bad_workspace(a)) return TG_E_ALIGN;
      return too_large(a, e) ? (int)TG_E_SIZE : 0;
    case ENTRY_W8:
      // the fields later ABI versions added for the 4-bit kernels (numerics, layouts, w_format) are not read; a fused stage is refused
      if (a->reserved != 0) return TG_E_SHAPE;
      if (a->norm_weight || a->epilogue) return TG_E_FUSION;
      if (bad_bias_row_stride(a)) return TG_E_SHAPE;
      if (too_large(a, e)) return TG_E_SIZE;
      if (a->batch > 1 && a->bias && (a->stride_bias & 7)) return TG_E_ALIGN;
      return bad_workspace(a) ? (int)TG_E_ALIGN : 0;
  }
  return TG_E_INTERNAL;
}

// GemmParams of a validated call.  dry: 0 launch, 1 report the kernel family, 2 report the workspace the fastest kernel wants.
static GemmParams make_params(const tg_w4_gemm* a, GemmEntry e, tg_stream_t stream, int dry) {
  const bool batched = a->batch > 1;
  GemmParams p;
  memset(&p, 0, sizeof p);   // (ws_need: the planner's answer)
  p.x = (const char*)a->x;
  p.w = (const char*)a->w;
  p.qinfo = (const char*)a->qinfo;
  p.lut = (const char*)a->lut;
  p.y = (char*)a->y;
  p.m = (int32_t)a->m;
  p.wrows = (int32_t)a->wrows;
  p.k = (int32_t)a->k;
  // The packed words the call holds.  TG_WFMT_ROWS: the A-shaped tensor holds Bint4 words (rows padded to 16), so from here on this IS
  // a weights-on-the-right call -- both sides produce [activation row][weight row] (TinyGemm_int4.cu:450-456).
  // (w8 has one packed format per side and does not read w_format)
  const bool rows = e != ENTRY_W8 && a->w_format == TG_WFMT_ROWS;
  p.on_right = rows || a->w_on_right != 0;
  p.inner = rows ? (a->k % 64 == 0 ? 4 : 2) : a->inner_k_tiles;
  p.ntiles = (int32_t)(a->wrows / (p.on_right ? 8 : 16));
  p.ksuper = (int32_t)(a->k / (16 * p.inner));
  p.gshift = group_shift(a->group);
  p.ngroups = (int32_t)(a->k / a->group);
  p.qtype = a->qtype;
  p.rowtiles = (int32_t)cdiv(a->wrows, 16);
  p.dt = a->dtype;
  p.qmx = a->qtype == TG_Q_MX4;
  p.batch = batched ? a->batch : 1;
  p.st = (hipStream_t)stream;
  p.numerics = a->numerics == TG_NUM_FAST_DOT2 ? (int)TG_NUM_FAST : a->numerics;
  p.dot2 = a->numerics == TG_NUM_FAST_DOT2;
  p.dry = dry != 0;
  p.dry_detail = dry == 3;
  p.stride_x = batched ? a->stride_x : 0;
  p.stride_w = batched ? a->stride_w : 0;
  p.stride_qinfo = batched ? a->stride_qinfo : 0;
  p.stride_lut = batched ? a->stride_lut : 0;
  p.stride_y = batched ? a->stride_y : 0;
  p.bias = (const char*)a->bias;
  p.stride_bias = batched ? a->stride_bias : 0;
  p.bias_row_stride = a->bias_row_stride;
  p.norm_w = (const char*)a->norm_weight;
  p.norm_eps = a->norm_eps;
  p.epilogue = a->epilogue;
  p.ws = (char*)a->workspace;
  p.ws_bytes = a->workspace ? a->workspace_bytes : 0;
  p.ws_query = dry == 2;
  p.x_tc = a->x_layout == TG_LAYOUT_TC_A;
  p.y_tc = a->y_layout == TG_LAYOUT_TC_A;
  return p;
}

// dry: 0 launch, 1 report the kernel family (tg_gemm_w4_plan), 2 report the workspace the fastest kernel wants, 3 as 1 but naming the
// lean m = 1 pair kernel (tg_gemm_w4_plan_detail)
static int gemm_w4_impl(const tg_w4_gemm* caller, int device, tg_stream_t stream, int dry, int64_t* ws_need = nullptr) {
  tg_w4_gemm full;
  int rc0 = take_args(caller, &full);
  if (rc0 == 0) rc0 = check_gemm(&full, ENTRY_W4);
  if (rc0 != 0) return rc0;
  GemmParams p = make_params(&full, ENTRY_W4, stream, dry);
  DeviceScope ds(dry ? -1 : device);
  if (!dry && !ds.ok) return TG_E_DEVICE;
  // MANY activation rows (a prefill through the modules, a wide decode batch): the LDS-tiled MFMA GEMM that dequantises the weights once per
  // 128-row tile of m instead of once per 16 rows (w4_gemm_tile.cuh; the reference's weights bit for bit, so it serves both numerics
  // settings).  From 65 rows; ONE layer from 17 rows when the caller's workspace allows a split-K launch (tg_tile.hip).  4096^2 at m = 128 / 256 / 1024:
  // 17.9 / 25.5 / 52 us against 37.8 / 44.5 / 166 on the stream kernel and 55 / 102 / 427 in 16-row blocks.
  if (p.on_right && p.m >= TG_TILE_MIN_M_SPLIT) {
    const int trc = offer(tgx::tile, p);
    if (trc != TG_PAIR_NA) {
      if (ws_need) *ws_need = p.ws_need;
      return trc;
    }
  }
  // More than 16 activation rows in the default numerics (row-major operands, weights on the B side): the group-scaled kernels hold at
  // most one 16-row MFMA tile of activations, so the call is issued as ceil(m / 16) launches of up to 16 rows each on the caller's stream
  // (the reference's own grid walks the 16-row tiles of m the same way and re-reads the weights per tile, TinyGemmImpl.cuh:379-392).
  // Stacked 4096^2 layers at m = 17 ... 32: 5.2-5.3 us per layer on the reference-numerics stream kernel (22 % of the roofline for
  // ONE pass over the weights) against 3.0-3.3 here; one layer per graph node at m = 32 / 64: 15.3 / 35.5 us against 14 / 28.
  // Up to 64 rows: from 128 rows on the stream kernel's ONE launch (its 16-row tiles of m run concurrently and share the weights in
  // L2) wins -- one 4096^2 layer per graph node at m = 128 / 256 / 1024: 37.8 / 44.5 / 166 us against 55 / 102 / 427 in blocks
  // (profiles/r05_row_blocks_large_m.txt).
#ifndef TG_ROW_BLOCKS_MAX_M
#define TG_ROW_BLOCKS_MAX_M 64
#endif
  if (p.on_right && p.m > 16 && p.m <= TG_ROW_BLOCKS_MAX_M && (p.numerics == TG_NUM_FAST || p.numerics == TG_NUM_FAST_MFMA) && !p.x_tc && !p.y_tc &&
      !p.norm_w && !p.epilogue) {
    // the rows [m0, m0 + mb) of the call as a call of their own
    auto row_block = [&](int64_t m0, int mb) {
      GemmParams q = p;
      q.m = mb;
      q.x = p.x + m0 * p.k * 2;
      q.y = p.y + m0 * p.wrows * 2;
      if (q.bias && q.bias_row_stride) q.bias = p.bias + m0 * q.bias_row_stride * 2;
      return q;
    };
    // decided on a dry pass over the two block shapes of the call (16 rows, the ragged last block): both on a group-scaled kernel, or the
    // whole call stays on the path below
    auto block_plan = [&](int mb) {
      GemmParams q = row_block(0, mb);
      q.dry = true;
      return launch_w4(q);
    };
    auto group_scaled = [](int rc) { return rc == TG_PLAN_PAIR || rc == TG_PLAN_PAIR_XR || rc == TG_PLAN_GEMV; };
    const int last = p.m % 16 ? p.m % 16 : 16;
    const int r16 = block_plan(16), rl = last == 16 ? r16 : block_plan(last);
    if (group_scaled(r16) && group_scaled(rl)) {
      int64_t need = 0;
      for (int m0 = 0; m0 < p.m; m0 += 16) {
        GemmParams q = row_block(m0, p.m - m0 < 16 ? p.m - m0 : 16);
        const int rc = launch_w4(q);
        if (rc < 0) return rc;
        if (rc == TG_PLAN_PAIR || rc == TG_PLAN_PAIR_XR) need = q.ws_need > need ? q.ws_need : need;
      }
      if (ws_need) *ws_need = need;
      return dry ? r16 : 0;
    }
  }
  const int rc = launch_w4(p);
  if (ws_need) *ws_need = (rc == TG_PLAN_PAIR || rc == TG_PLAN_PAIR_XR) ? p.ws_need : 0;
  return rc;
}

int tg_gemm_w4(const tg_w4_gemm* a, int device, tg_stream_t stream) { return gemm_w4_impl(a, device, stream, 0); }

int tg_gemm_w4_plan(const tg_w4_gemm* a, int device) { return gemm_w4_impl(a, device, nullptr, 1); }

int tg_gemm_w4_plan_detail(const tg_w4_gemm* a, int device) { return gemm_w4_impl(a, device, nullptr, 3); }

int64_t tg_gemm_w4_workspace_bytes(const tg_w4_gemm* a) {
  int64_t need = 0;
  const int rc = gemm_w4_impl(a, -1, nullptr, 2, &need);
  return rc < 0 ? rc : need;
}

// ---- input gradient dX = dY . W (tg_gemm_w4_dx; the kernel and its launch path: w4_gemm_dx.cuh, tg_dx.hip) ----
// dry: 0 launch, 2 report the workspace of the split.  Every check runs before any HIP call.
static int gemm_dx_impl(const tg_w4_gemm* caller, int device, tg_stream_t stream, int dry, int64_t* ws_need = nullptr) {
  tg_w4_gemm full;
  const tg_w4_gemm* a = &full;
  int rc0 = take_args(caller, &full);
  if (rc0 == 0) rc0 = check_gemm(a, ENTRY_DX);
  if (rc0 != 0) return rc0;
  GemmParams p = make_params(a, ENTRY_DX, stream, dry);
  DeviceScope ds(dry ? -1 : device);
  if (!dry && !ds.ok) return TG_E_DEVICE;
  const int rc = tgx::gemm_dx(p);
  if (ws_need) *ws_need = p.ws_need;
  return rc;
}

int tg_gemm_w4_dx(const tg_w4_gemm* a, int device, tg_stream_t stream) { return gemm_dx_impl(a, device, stream, 0); }

int64_t tg_gemm_w4_dx_workspace_bytes(const tg_w4_gemm* a) {
  int64_t need = 0;
  const int rc = gemm_dx_impl(a, -1, nullptr, 2, &need);
  return rc < 0 ? rc : need;
}

// ---- gradients of scales, zeros and LUT (tg_gemm_w4_dq; the kernels and their launch path: w4_gemm_dq.cuh, tg_dq.hip) ----
// query: report the workspace, look at nothing but the struct.  Every check runs before any HIP call.
static int gemm_dq_impl(const tg_w4_gemm* caller, const void* dy, float* d_qinfo, float* d_lut, int device, tg_stream_t stream, bool query,
                        int64_t* ws_need = nullptr) {
  tg_w4_gemm full;
  const tg_w4_gemm* a = &full;
  int rc0 = take_args(caller, &full);
  if (rc0 == 0) rc0 = check_gemm(a, ENTRY_DQ);
  if (rc0 != 0) return rc0;
  GemmParams plan = make_params(a, ENTRY_DQ, stream, 2);
  tgx::gemm_dq(plan, nullptr, nullptr, nullptr);
  if (ws_need) *ws_need = plan.ws_need;
  if (query) return 0;
  if (a->qtype == TG_Q_INT4) d_lut = nullptr;
  if (!dy || (!d_qinfo && !d_lut)) return TG_E_NULL;
  if (misaligned(dy, 16) || (d_qinfo && misaligned(d_qinfo, 16)) || (d_lut && misaligned(d_lut, 16))) return TG_E_ALIGN;
  if (!a->workspace) return TG_E_NULL;
  if (a->workspace_bytes < plan.ws_need) return TG_E_SHAPE;
  GemmParams p = make_params(a, ENTRY_DQ, stream, 0);
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  return tgx::gemm_dq(p, (const char*)dy, d_qinfo, d_lut);
}

int tg_gemm_w4_dq(const tg_w4_gemm* a, const void* dy, float* d_qinfo, float* d_lut, int device, tg_stream_t stream) {
  return gemm_dq_impl(a, dy, d_qinfo, d_lut, device, stream, false);
}

int64_t tg_gemm_w4_dq_workspace_bytes(const tg_w4_gemm* a) {
  int64_t need = 0;
  const int rc = gemm_dq_impl(a, nullptr, nullptr, nullptr, -1, nullptr, true, &need);
  return rc < 0 ? rc : need;
}

int tg_convert_to_Bint8(const int32_t* in, int64_t n, int64_t k, int I, int32_t* out, int device, tg_stream_t stream) {
  if (!in || !out) return TG_E_NULL;
  if (!(I == 1 || I == 2 || I == 4)) return TG_E_INNER_K;  // ConvertB.cu:428
  if (n <= 0 || k <= 0) return TG_E_SHAPE;
  if (k % (I * 16) != 0) return TG_E_K_DIV;                // ConvertB.cu:438
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t ksuper = k / (I * 16), total = cdiv(n, 8) * ksuper * 32 * I;
  const unsigned blocks = (unsigned)(cdiv(total, 256) < 8192 ? cdiv(total, 256) : 8192);
  hipStream_t st = (hipStream_t)stream;
  return pick<1, 2, 4>(I, [&](auto I_) {
    hipLaunchKernelGGL(pack_Bint8_kernel<decltype(I_)::value>, dim3(blocks), dim3(256), 0, st, in, out, n, k, ksuper, total);
    return launch_status();
  });
}

int tg_convert_to_Aint8(const int32_t* in, int64_t m, int64_t k, int I, int32_t* out, int device, tg_stream_t stream) {
  if (!in || !out) return TG_E_NULL;
  if (!(I == 1 || I == 2)) return TG_E_INNER_K;  // ConvertA.cu:413
  if (m <= 0 || k <= 0) return TG_E_SHAPE;
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  const int64_t kouter = cdiv(cdiv(k, 16), I), total = cdiv(m, 16) * kouter * 32 * I * 2;
  const unsigned blocks = (unsigned)(cdiv(total, 256) < 8192 ? cdiv(total, 256) : 8192);
  hipStream_t st = (hipStream_t)stream;
  return pick<1, 2>(I, [&](auto I_) {
    hipLaunchKernelGGL(pack_Aint8_kernel<decltype(I_)::value>, dim3(blocks), dim3(256), 0, st, in, out, m, k, kouter, total);
    return launch_status();
  });
}

// dry: 0 launch, 2 report the workspace the fastest kernel wants (tg_gemm_w8_workspace_bytes)
static int gemm_w8_impl(const tg_w4_gemm* caller, int device, tg_stream_t stream, int dry, int64_t* ws_need) {
  tg_w4_gemm full;
  const tg_w4_gemm* a = &full;
  int rc0 = take_args(caller, &full);
  if (rc0 == 0) rc0 = check_gemm(a, ENTRY_W8);
  if (rc0 != 0) return rc0;
  GemmParams p = make_params(a, ENTRY_W8, stream, dry);
  // what the struct says for the 4-bit kernels only was not validated and does not reach an int8 kernel
  p.lut = nullptr; p.stride_lut = 0; p.numerics = TG_NUM_REFERENCE; p.dot2 = 0; p.norm_eps = 0.f; p.x_tc = p.y_tc = 0;
  DeviceScope ds(dry ? -1 : device);
  if (!dry && !ds.ok) return TG_E_DEVICE;
#ifdef TG_DEV_MIN
  return TG_E_SHAPE;
#else
  // many activation rows: the LDS-tiled MFMA GEMM's int8 flavour (w4_gemm_tile.cuh; the same weights bit for bit), split-K with the caller's workspace
  {
    const int trc = offer(tgx::tile_w8, p);
    if (ws_need) *ws_need = p.ws_need;
    if (trc != TG_PAIR_NA) return trc == TG_PLAN_TILE ? 0 : trc;
    if (dry) return 0;
  }
  return pick_dt(p.dt, [&](auto DT_) {
    return pick<0, 1>(!p.on_right, [&](auto LAYOUT_A_) {
      return pick<1, 2, 4>(p.inner, [&](auto I_) {  // (innerKTiles 1, 2, 4 on the right; 1, 2 on the left)
        constexpr bool LAYOUT_A = decltype(LAYOUT_A_)::value != 0;
        constexpr int I = decltype(I_)::value;
        if constexpr (LAYOUT_A && I == 4) {
          return (int)TG_PAIR_NA;
        } else {
          return launch_w8<decltype(DT_), LAYOUT_A, I>(p);
        }
      });
    });
  });
#endif
}

int tg_gemm_w8(const tg_w4_gemm* a, int device, tg_stream_t stream) { return gemm_w8_impl(a, device, stream, 0, nullptr); }

int64_t tg_gemm_w8_workspace_bytes(const tg_w4_gemm* a) {
  int64_t need = 0;
  const int rc = gemm_w8_impl(a, -1, nullptr, 2, &need);
  return rc < 0 ? rc : need;
}

int tg_gemm_f16(const void* x, const void* w, void* y, int64_t m, int64_t wrows, int64_t k, int dtype,
                int w_on_right, int I, int device, tg_stream_t stream) {
  if (!x || !w || !y) return TG_E_NULL;
  if (!(dtype == TG_BF16 || dtype == TG_F16)) return TG_E_DTYPE;
  if (m <= 0 || wrows <= 0 || k <= 0 || m > INT32_MAX || wrows > INT32_MAX || k > INT32_MAX) return TG_E_SHAPE;
  if (w_on_right ? !(I == 1 || I == 2) : I != 1) return TG_E_INNER_K;
  if (k % 32 != 0) return TG_E_K_DIV;  // TinyGemmImpl.cuh:376
  if (wrows % (w_on_right ? 8 : 16) != 0) return TG_E_SHAPE;
  if (!aligned16(x) || !aligned16(w)) return TG_E_ALIGN;
  F16GemmParams p;
  p.x = (const char*)x;
  p.w = (const char*)w;
  p.y = (char*)y;
  p.m = (int32_t)m;
  p.wrows = (int32_t)wrows;
  p.k = (int32_t)k;
  p.inner = I;
  p.ktiles_padded = (int32_t)(cdiv(k, 16 * I) * I);
  DeviceScope ds(device);
  if (!ds.ok) return TG_E_DEVICE;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)cdiv(wrows, 16), (unsigned)cdiv(m, 16));
  constexpr int WAVES = 8;
  return pick_dt(dtype, [&](auto DT_) {
    return pick<0, 1>(!w_on_right, [&](auto LAYOUT_A_) {
      return pick<1, 2>(I, [&](auto I_) {  // (innerKTiles 1, 2 on the right; 1 on the left)
        constexpr bool LAYOUT_A = decltype(LAYOUT_A_)::value != 0;
        if constexpr (LAYOUT_A && decltype(I_)::value == 2) {
          return (int)TG_PAIR_NA;
        } else {
          hipLaunchKernelGGL((f16_gemm_kernel<decltype(DT_), LAYOUT_A, WAVES, decltype(I_)::value>), grid, dim3(WAVES * 64), 0, st, p);
          return launch_status();
        }
      });
    });
  });
}

}  // extern "C"

#include "decode_glue.cuh"
#include "peer_gather.cuh"
