// moe_call.cuh -- one mixture-of-experts call is the public struct dg_moe (include/decode_glue_hip.h); this is what the library does with
// it in front of a launch: its validation for both kernels (check_moe) and the sizes of the group workspace that the grouped path's
// check, planner, sorter and GEMM agree on.  Host-only, as attn_call.cuh is: no kernel receives a dg_moe, every kernel keeps its own
// parameter block.  Included inside the anonymous namespace of tg_moe.hip (dg_moe_launch, dg_moe_plan, the GEMV launcher) and
// tg_moe_tile.hip (the grouped launcher and planner), behind moe.cuh (MOE_MAX_E, MOE_MAX_TOPK); a launcher gets a call that check_moe
// accepted and keeps only its parameter block, DeviceScope, grid, LDS size and the choice of kernel.

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// ---- the group workspace (int32 units): what dg_moe_group writes and the grouped GEMM reads ----
constexpr int MG_HDR = 0;        // n_tiles, n_invalid, n_valid, BM
constexpr int MG_COUNT = 4;      // [64]
constexpr int MG_OFFSET = 68;    // [65], padded to 68
constexpr int MG_PERM = 136;     // [P]; then invalid [P]; then tiles [bound][3]
constexpr int MG_THREADS = 256;
constexpr int MG_MAX_PAIRS = 65536;
constexpr int MG_BM = 128;       // the tile height of the grouped GEMM
constexpr int MG_BN = 64;

inline int64_t mg_bound(int64_t P, int64_t E, int64_t bm) { return (P + bm - 1) / bm + (E < P ? E : P); }
inline int64_t mg_ints(int64_t P, int64_t E, int64_t bm) { return MG_PERM + 2 * P + 3 * mg_bound(P, E, bm); }

// TG_E_SIZE, where the kernels differ on purpose: the GEMV indexes pairs in int32 with room to spare, the grouped path sorts at most
// MG_MAX_PAIRS of them in one workgroup; an expert's rows and bytes are bounded alike.  (m first: m * top_k must not wrap.)
inline bool moe_too_large(const dg_moe& c) {
  const int64_t max_pairs = c.kernel == DG_MOE_GROUPED ? MG_MAX_PAIRS : INT32_MAX / 2;
  return c.m > max_pairs || c.m * c.top_k > max_pairs || c.wrows > (1 << 24) || c.wrows * c.k / 2 > INT32_MAX;
}

// Everything of a call that needs no device, behind `call == NULL` and struct_bytes.  The codes in their order of precedence: layout
// (kernel, stage), null, dtype, qtype, shape, size, innerKTiles, group, alignment.  A field that the call's kernel and stage do not use
// is not read: gates and residual belong to DOWN, the workspaces to a GROUPED launch (plan: the planner tells their sizes and looks at
// neither), f32_ws to its DOWN stage.
inline int check_moe(const dg_moe& c, bool plan) {
  if ((c.kernel != DG_MOE_GEMV && c.kernel != DG_MOE_GROUPED) || (c.stage != DG_MOE_GATE_UP && c.stage != DG_MOE_DOWN)) return TG_E_LAYOUT;
  const bool any4 = c.qtype == TG_Q_ANY4_GLOBAL || c.qtype == TG_Q_ANY4_ROWWISE;
  const bool down = c.stage == DG_MOE_DOWN;
  const bool group_ws = c.kernel == DG_MOE_GROUPED && !plan, f32_ws = group_ws && down;
  if (!c.x || !c.w || !c.qinfo || !c.y || !c.ids || (any4 && !c.lut) || (down && !c.gates) || (group_ws && !c.group_ws) || (f32_ws && !c.f32_ws))
    return TG_E_NULL;
  if (c.dtype != TG_BF16 && c.dtype != TG_F16) return TG_E_DTYPE;
  if (c.qtype != TG_Q_INT4 && !any4) return TG_E_QTYPE;
  if (c.m < 1 || c.E < 1 || c.E > MOE_MAX_E || c.top_k < 1 || c.top_k > MOE_MAX_TOPK || c.top_k > c.E) return TG_E_SHAPE;
  if (c.k < 64 || (c.k % 64) != 0 || c.wrows < 16 || (c.wrows % 16) != 0) return TG_E_SHAPE;
  if (moe_too_large(c)) return TG_E_SIZE;
  const int64_t pairs = c.m * c.top_k;
  if ((group_ws && c.group_ws_bytes < 4 * mg_ints(pairs, c.E, MG_BM)) || (f32_ws && c.f32_ws_bytes < pairs * c.wrows * 4)) return TG_E_SIZE;
  if (c.inner_k_tiles != 4) return TG_E_INNER_K;
  if ((c.group != 64 && c.group != 128 && c.group != 256) || (c.k % c.group) != 0) return TG_E_GROUP;
  if (!aligned16(c.x) || !aligned16(c.w) || !aligned16(c.qinfo) || !aligned16(c.lut) || !aligned16(c.y) || !aligned4(c.ids) ||
      (down && (!aligned4(c.gates) || !aligned16(c.residual))) || (group_ws && !aligned4(c.group_ws)) || (f32_ws && !aligned16(c.f32_ws)) ||
      (c.stride_w % 16) != 0 || (c.stride_qinfo % 16) != 0 || (c.stride_lut % 16) != 0)
    return TG_E_ALIGN;
  return 0;
}
