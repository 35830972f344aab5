// attn_call.cuh -- one attention call of the decode stack is the public struct dg_attn (include/decode_glue_hip.h); this is what the library
// does with it in front of a launch: which (kernel, flags) pairs exist (attn_flavour), which fields a pair uses (attn_used_fields), and its
// validation for every kind of kernel (check_attn).  Host-only, as GemmParams is: no kernel receives a dg_attn, every kernel keeps its own
// argument list.  Included by decode_glue.cuh (tinygemm_hip.hip: dg_attn_launch, the decode launchers) and tg_prefill.hip (prefill_launch);
// a launcher validates the call with check_attn and keeps only DeviceScope, LDS size, grid and the choice of kernel.
#pragma once
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
#include "kv_paged.cuh"

// DG_ATTN_PREFILL's launcher: defined in tg_prefill.hip, called by dg_attn_launch from the other translation unit; not exported
__attribute__((visibility("hidden"))) int prefill_launch(const dg_attn& c, int device, tg_stream_t stream);

namespace {

// check_attn's kinds are the public DG_ATTN_* kernels and this one -- dg_decode_attn: q is already roped (dg_attn::qkv holds it), no tables
constexpr int ATTN_UNFUSED = -1;

// DG_ATTN_FLAVOURS is the definition of what dg_attn_launch accepts
inline bool attn_flavour(int32_t kernel, uint32_t flags) {
#define DG_ATTN_PAIR(name, k, f) {k, f},
  static const struct { int32_t kernel; uint32_t flags; } pairs[] = {DG_ATTN_FLAVOURS(DG_ATTN_PAIR)};
#undef DG_ATTN_PAIR
  for (const auto& p : pairs)
    if (p.kernel == kernel && p.flags == flags) return true;
  return false;
}

// The caller's struct as check_attn and the launchers read it -- the one place where a call is copied: a field that the call's kernel and
// flags do not use (the positional entry points up to ABI 8 did not have the parameter) holds what a call without it holds.
inline dg_attn attn_used_fields(const dg_attn& call) {
  dg_attn c = call;
  if (!(c.flags & DG_ATTN_MX8)) c.k_exp = c.v_exp = nullptr;
  if (!(c.flags & DG_ATTN_PAGED)) { c.table = nullptr; c.page_size = c.num_pages = 0; }
  if (c.kernel != DG_ATTN_SPLIT) { c.scratch = nullptr; c.scratch_bytes = 0; c.nsplit = 1; }
  if (c.kernel != DG_ATTN_PREFILL) c.T = 1;
  if (c.kernel != DG_ATTN_PREFILL || !(c.flags & DG_ATTN_SEQ)) { c.len = c.slot = nullptr; c.cache_bs = c.bs; }  // sequence i lives in slot i
  return c;
}

// dg_attn::flags by name
struct AttnFlags {
  bool seq;          // DG_ATTN_SEQ: `pos` holds a position per sequence
  bool kv8;          // DG_ATTN_MX8: mx8 caches, k_exp / v_exp their exponent bytes
  bool paging;       // DG_ATTN_PAGED: k_cache / v_cache are pools [num_pages][kvl][page_size][d] behind `table` int32 [cache_bs][max_seq / page_size]
                     // (with kv8: k_exp / v_exp are pools [num_pages][kvl][page_size][d / 32] behind the same table, and both rule sets hold)
  bool one_barrier;  // DG_ATTN_ONE_BARRIER: a split call that must run the one-barrier kernel: that kernel's d and alignment
  explicit AttnFlags(const dg_attn& c)
      : seq(c.flags & DG_ATTN_SEQ), kv8(c.flags & DG_ATTN_MX8), paging(c.flags & DG_ATTN_PAGED), one_barrier(c.flags & DG_ATTN_ONE_BARRIER) {}
};

// The split kind's scratch buffer: one int counter per head (rounded up to 16 bytes), then [head][chunk][max, sum, d outputs] floats.
struct SplitScratch {
  int64_t part_offset, bytes;
};
inline SplitScratch split_scratch(int64_t bs, int hl, int d, int nsplit) {
  const int64_t counters = ((bs * hl * 4 + 15) / 16) * 16;
  return {counters, counters + bs * hl * (int64_t)nsplit * (d + 2) * 4};
}

// The kernels' paging argument of a paged call that check_attn accepts
inline KvPages kv_pages(const dg_attn& c) {
  int shift = 0;
  while (((int64_t)1 << shift) < c.page_size) ++shift;
  return {c.table, shift, (int32_t)(c.max_seq / c.page_size), (int32_t)c.num_pages};
}

// The codes in their order of precedence: null, dtype, shape (the split kind's scratch size last), alignment.  Where the kinds differ they
// differ on purpose; each such line says why.
inline int check_attn(int kind, const dg_attn& c) {
  const bool online = kind == DG_ATTN_ONLINE, split = kind == DG_ATTN_SPLIT, prefill = kind == DG_ATTN_PREFILL;
  const auto [seq, kv8, paging, one_barrier] = AttnFlags(c);
  const int64_t bs = c.bs, max_seq = c.max_seq;
  const int d = c.d;
  // dg_decode_attn has no tables; only the split kind has a scratch buffer, only an mx8 call exponent tensors
  if (!c.qkv || !c.pos || !c.k_cache || !c.v_cache || !c.out || (kind != ATTN_UNFUSED && (!c.cos || !c.sin)) || (split && !c.scratch) ||
      (kv8 && (!c.k_exp || !c.v_exp)) || (paging && !c.table))
    return TG_E_NULL;
  if (!(c.dtype == TG_BF16 || c.dtype == TG_F16)) return TG_E_DTYPE;
  if (bs <= 0 || c.hl <= 0 || c.kvl <= 0 || c.hl % c.kvl != 0 || max_seq <= 0) return TG_E_SHAPE;
  // d: the one-barrier and the prefill kernel are instantiated for 64 / 128 (every paged call runs one of the two, and so does a split
  // call held to the one-barrier kernel); a 256-thread block of the others works in d / 8 columns
  if (online || prefill || paging || one_barrier ? !(d == 64 || d == 128) : (d < 8 || d % 8 != 0 || d > 256 || (256 % (d / 8)) != 0)) return TG_E_SHAPE;
  // max_seq: LDS holds a score per cache position (8192; prefill fills those caches) or per position of a chunk (split: 65536, the launcher
  // refuses what does not fit); the one-barrier kernel keeps no scores: its bound is the 32-bit byte offset of a row within a head
  // (paged: that offset is taken within a page; the decode entry points keep the split kind's 65536)
  if (online && !paging ? max_seq * d * 2 >= ((int64_t)1 << 32) : max_seq > (split || online ? 65536 : 8192)) return TG_E_SHAPE;
  // paged: a page is a power of two of at least 64 positions (it holds a kernel's unit -- 32 / 64 rows, a 64-position tile -- whole) and
  // max_seq is whole pages; page ids are int32
  if (paging && (c.page_size < 64 || c.page_size > max_seq || (c.page_size & (c.page_size - 1)) != 0 || max_seq % c.page_size != 0 ||
                  c.num_pages <= 0 || c.num_pages > INT32_MAX))
    return TG_E_SHAPE;
  // grid: bs * hl is grid.x of the decode kernels; prefill counts its grid in the launcher (TG_E_SIZE), but bs is grid.y of its cache append
  // and the token rows bs * T are int32 with room to spare
  if (prefill ? (bs > 65535 || c.T <= 0 || bs * c.T > INT32_MAX / 2) : bs * c.hl > INT32_MAX) return TG_E_SHAPE;
  // prefill, seq: slots are int32, and without `slot` sequence i lives in slot i
  if (prefill && seq && (c.cache_bs <= 0 || c.cache_bs > INT32_MAX || (!c.slot && bs != c.cache_bs))) return TG_E_SHAPE;
  // split: the combine walks 1 ... 64 partials, an mx8 row is whole 32-element blocks; then, last of the shape tests, the caller's scratch
  if (split && (c.nsplit < 1 || c.nsplit > 64 || (kv8 && d % 32 != 0))) return TG_E_SHAPE;
  if (split && c.scratch_bytes < split_scratch(bs, c.hl, d, c.nsplit).bytes) return TG_E_SHAPE;
  // alignment: every kernel reads cache rows (exponents, scratch: null where a call has none) in 16-byte pieces; qkv and the tables only the
  // one-barrier and the prefill kernel (and with them every paged call), and only prefill stores `out` that way; the block table is read in
  // single entries and aligned by contract
  if (!aligned16(c.k_cache) || !aligned16(c.v_cache) || !aligned16(c.k_exp) || !aligned16(c.v_exp) || !aligned16(c.scratch)) return TG_E_ALIGN;
  if (!aligned16(c.table)) return TG_E_ALIGN;
  if ((online || prefill || paging || one_barrier) && (!aligned16(c.qkv) || !aligned16(c.cos) || !aligned16(c.sin))) return TG_E_ALIGN;
  if (prefill && !aligned16(c.out)) return TG_E_ALIGN;
  return 0;
}

}  // namespace
