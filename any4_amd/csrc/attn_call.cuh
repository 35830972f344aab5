// attn_call.cuh -- one attention call of the decode stack, described once (include/decode_glue_hip.h: dg_decode_attn, dg_rope_attn*,
// dg_prefill_attn*, the _paged, the _online_mx8 and the _mx8_paged ones among them).  Host-only, as GemmParams is: no kernel receives an AttnCall, every kernel keeps its own argument list.  Included by
// decode_glue.cuh (tinygemm_hip.hip) and tg_prefill.hip; an entry point builds the call (attn_call), sets what only it takes and hands it
// to its kind's launcher, which validates it with check_attn and keeps only DeviceScope, LDS size, grid and the choice of kernel.
#pragma once
#include "tg_common.cuh"
#include "../../include/decode_glue_hip.h"
#include "kv_paged.cuh"

namespace {

enum AttnKind {
  ATTN_UNFUSED,  // dg_decode_attn: q is already roped (AttnCall::qkv holds it), no tables
  ATTN_GENERAL,  // dg_rope_attn(_seq): one 256-thread block per head, any d % 8 == 0
  ATTN_ONLINE,   // dg_rope_attn_online(_seq, _paged): the one-barrier kernel, d = 64 / 128
  ATTN_SPLIT,    // dg_rope_attn_split(_seq, _mx8, _mx8_seq, _paged), dg_rope_attn_online_mx8(_seq, _paged): nsplit blocks per head and a scratch buffer
  ATTN_PREFILL,  // dg_prefill_attn(_seq, _mx8, _mx8_seq, _paged, _mx8_paged): T tokens per sequence
};

struct AttnCall {
  const void* qkv;
  const float *cos, *sin;
  const int64_t* pos;
  void *k_cache, *v_cache, *out;
  void *k_exp = nullptr, *v_exp = nullptr;          // kv8: the exponent bytes of the mx8 caches
  const int64_t *len = nullptr, *slot = nullptr;    // prefill, seq: tokens and cache slot per sequence (either may stay null)
  void* scratch = nullptr;                          // split
  int64_t scratch_bytes = 0;
  int64_t bs, T = 1, cache_bs;  // T: tokens per sequence (prefill); cache_bs: sequences the caches hold (prefill, seq; otherwise bs)
  int hl, kvl, d;
  int64_t max_seq;
  float scale;
  int nsplit = 1;  // split
  int dtype, device;
  tg_stream_t stream;
  bool seq = false;  // `pos` holds a position per sequence (the _seq entry points)
  bool kv8 = false;  // mx8 caches (the _mx8 entry points)
  bool one_barrier = false;  // a split call that must run the one-barrier kernel (dg_rope_attn_online_mx8): that kernel's d and alignment
  // paged: k_cache / v_cache are pools [num_pages][kvl][page_size][d] behind `table` int32 [cache_bs][max_seq / page_size] (the _paged entry points;
  // with kv8, the _mx8_paged ones: k_exp / v_exp are pools [num_pages][kvl][page_size][d / 32] behind the same table, and both rule sets hold)
  bool paging = false;
  const int32_t* table = nullptr;
  int64_t page_size = 0, num_pages = 0;

  // what an entry point takes on top of the sixteen common arguments (attn_call)
  AttnCall& per_sequence() { seq = true; return *this; }
  AttnCall& mx8(void* ke, void* ve) { kv8 = true; k_exp = ke; v_exp = ve; return *this; }
  AttnCall& online() { one_barrier = true; return *this; }
  AttnCall& split(void* s, int64_t bytes, int n) { scratch = s; scratch_bytes = bytes; nsplit = n; return *this; }
  AttnCall& chunk(int64_t tokens) { T = tokens; return *this; }
  AttnCall& slots(const int64_t* l, const int64_t* s, int64_t n) { len = l; slot = s; cache_bs = n; return per_sequence(); }
  AttnCall& paged(const int32_t* t, int64_t ps, int64_t np) { paging = true; table = t; page_size = ps; num_pages = np; return per_sequence(); }
};

// the sixteen arguments every entry point takes
inline AttnCall attn_call(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* k_cache, void* v_cache, void* out,
                          int64_t bs, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device, tg_stream_t stream) {
  AttnCall c;
  c.qkv = qkv; c.cos = cos; c.sin = sin; c.pos = pos; c.k_cache = k_cache; c.v_cache = v_cache; c.out = out;
  c.bs = c.cache_bs = bs; c.hl = hl; c.kvl = kvl; c.d = d; c.max_seq = max_seq; c.scale = scale;
  c.dtype = dtype; c.device = device; c.stream = stream;
  return c;
}

// The split kind's scratch buffer: one int counter per head (rounded up to 16 bytes), then [head][chunk][max, sum, d outputs] floats.
struct SplitScratch {
  int64_t part_offset, bytes;
};
inline SplitScratch split_scratch(int64_t bs, int hl, int d, int nsplit) {
  const int64_t counters = ((bs * hl * 4 + 15) / 16) * 16;
  return {counters, counters + bs * hl * (int64_t)nsplit * (d + 2) * 4};
}

// The kernels' paging argument of a paged call that check_attn accepts
inline KvPages kv_pages(const AttnCall& c) {
  int shift = 0;
  while (((int64_t)1 << shift) < c.page_size) ++shift;
  return {c.table, shift, (int32_t)(c.max_seq / c.page_size), (int32_t)c.num_pages};
}

// The codes in their order of precedence: null, dtype, shape (the split kind's scratch size last), alignment.  Where the kinds differ they
// differ on purpose; each such line says why.
inline int check_attn(AttnKind kind, const AttnCall& c) {
  const bool online = kind == ATTN_ONLINE, split = kind == ATTN_SPLIT, prefill = kind == ATTN_PREFILL;
  const int64_t bs = c.bs, max_seq = c.max_seq;
  const int d = c.d;
  // dg_decode_attn has no tables; only the split kind has a scratch buffer, only an mx8 call exponent tensors
  if (!c.qkv || !c.pos || !c.k_cache || !c.v_cache || !c.out || (kind != ATTN_UNFUSED && (!c.cos || !c.sin)) || (split && !c.scratch) ||
      (c.kv8 && (!c.k_exp || !c.v_exp)) || (c.paging && !c.table))
    return TG_E_NULL;
  if (!(c.dtype == TG_BF16 || c.dtype == TG_F16)) return TG_E_DTYPE;
  if (bs <= 0 || c.hl <= 0 || c.kvl <= 0 || c.hl % c.kvl != 0 || max_seq <= 0) return TG_E_SHAPE;
  // d: the one-barrier and the prefill kernel are instantiated for 64 / 128 (every paged call runs one of the two, and so does a split
  // call held to the one-barrier kernel); a 256-thread block of the others works in d / 8 columns
  if (online || prefill || c.paging || c.one_barrier ? !(d == 64 || d == 128) : (d < 8 || d % 8 != 0 || d > 256 || (256 % (d / 8)) != 0)) return TG_E_SHAPE;
  // max_seq: LDS holds a score per cache position (8192; prefill fills those caches) or per position of a chunk (split: 65536, the launcher
  // refuses what does not fit); the one-barrier kernel keeps no scores: its bound is the 32-bit byte offset of a row within a head
  // (paged: that offset is taken within a page; the decode entry points keep the split kind's 65536)
  if (online && !c.paging ? max_seq * d * 2 >= ((int64_t)1 << 32) : max_seq > (split || online ? 65536 : 8192)) return TG_E_SHAPE;
  // paged: a page is a power of two of at least 64 positions (it holds a kernel's unit -- 32 / 64 rows, a 64-position tile -- whole) and
  // max_seq is whole pages; page ids are int32
  if (c.paging && (c.page_size < 64 || c.page_size > max_seq || (c.page_size & (c.page_size - 1)) != 0 || max_seq % c.page_size != 0 ||
                  c.num_pages <= 0 || c.num_pages > INT32_MAX))
    return TG_E_SHAPE;
  // grid: bs * hl is grid.x of the decode kernels; prefill counts its grid in the launcher (TG_E_SIZE), but bs is grid.y of its cache append
  // and the token rows bs * T are int32 with room to spare
  if (prefill ? (bs > 65535 || c.T <= 0 || bs * c.T > INT32_MAX / 2) : bs * c.hl > INT32_MAX) return TG_E_SHAPE;
  // prefill, seq: slots are int32, and without `slot` sequence i lives in slot i
  if (prefill && c.seq && (c.cache_bs <= 0 || c.cache_bs > INT32_MAX || (!c.slot && bs != c.cache_bs))) return TG_E_SHAPE;
  // split: the combine walks 1 ... 64 partials, an mx8 row is whole 32-element blocks; then, last of the shape tests, the caller's scratch
  if (split && (c.nsplit < 1 || c.nsplit > 64 || (c.kv8 && d % 32 != 0))) return TG_E_SHAPE;
  if (split && c.scratch_bytes < split_scratch(bs, c.hl, d, c.nsplit).bytes) return TG_E_SHAPE;
  // alignment: every kernel reads cache rows (exponents, scratch: null where a call has none) in 16-byte pieces; qkv and the tables only the
  // one-barrier and the prefill kernel (and with them every paged call), and only prefill stores `out` that way; the block table is read in
  // single entries and aligned by contract
  if (!aligned16(c.k_cache) || !aligned16(c.v_cache) || !aligned16(c.k_exp) || !aligned16(c.v_exp) || !aligned16(c.scratch)) return TG_E_ALIGN;
  if (!aligned16(c.table)) return TG_E_ALIGN;
  if ((online || prefill || c.paging || c.one_barrier) && (!aligned16(c.qkv) || !aligned16(c.cos) || !aligned16(c.sin))) return TG_E_ALIGN;
  if (prefill && !aligned16(c.out)) return TG_E_ALIGN;
  return 0;
}

}  // namespace
