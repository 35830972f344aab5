/* decode_glue_hip.h -- C ABI of the non-GEMM kernels of the decode stack: one decode step (one new token per sequence,
 * SURVEY.md 8f row N2) and the prompt prefill in front of it (DG_ATTN_PREFILL: a chunk of tokens per sequence).
 *
 * Not part of the tinygemm drop-in boundary (include/tinygemm_hip.h).  The reference times model-level
 * decode through HuggingFace `transformers` (benchmark.py:113-215 -> LlamaDecoderLayer, an external
 * dependency that is not vendored in the reference): per layer that is ~45 small elementwise / reduction
 * launches around the 4 (fused) quantized GEMMs, which at batch 1 cost 3x the GEMMs themselves.  These
 * five kernels replace them so that the model-level number measures the GEMM path, not launch gaps:
 *
 *   dg_add_rmsnorm   h' = h + delta;  y = rmsnorm(h') * w          (residual add + LlamaRMSNorm)
 *   dg_rope_kv       rotary embedding of q and k, k/v written into the static KV cache at *pos
 *   dg_decode_attn   grouped-query attention of one new token against cache[0 .. *pos]
 *   dg_attn_launch   the two above fused (what the decode harness launches), and a chunk of T tokens: rotary embedding, T cache rows
 *                    appended, causal flash attention over cache + chunk -- one call struct for every kernel and cache layout
 *   dg_swiglu        silu(gate) * up
 *
 * Conventions are those of include/tinygemm_hip.h: raw device pointers, caller-owned outputs, explicit
 * stream, no allocation, no host sync, graph-capturable (`pos` is read on the device, so a captured graph
 * can be replayed for the next position), return 0 / TG_E_* (negative) / hipError_t (positive).
 * All 16-bit tensors are bf16 (TG_BF16) or fp16 (TG_F16); cos/sin tables are float32.
 * Rounding points follow the plain-torch formulation in any4_amd/decode.py (tests compare the two).
 */
#ifndef DECODE_GLUE_HIP_H
#define DECODE_GLUE_HIP_H

#include "tinygemm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* h_out[r][:] = h[r][:] + delta[r][:] (delta may be NULL: h_out = h; h_out may alias h);
 * y[r][:] = to16(float(h_out) * rsqrt(mean(float(h_out)^2) + eps)) * w   (y may be NULL: residual add only).
 * dim % 8 == 0, dim <= 16384. */
TG_API int dg_add_rmsnorm(const void* h, const void* delta, const void* w, void* h_out, void* y,
                          int64_t rows, int64_t dim, float eps, int dtype, int device, tg_stream_t stream);

/* qkv [bs][(hl + 2 kvl) * d] (q heads, then k heads, then v heads); cos/sin float32 [max_seq][d]
 * (both halves filled, HF convention); *pos = sequence position (int64 on the device).
 * q_out [bs][hl][d] = rope(q); k_cache[b][kv][*pos][:] = rope(k); v_cache[b][kv][*pos][:] = v.
 * rope(x)[j] = to16(RN(x[j] cos[j]) + RN(rotate_half(x)[j] sin[j])) in f32: two rounded products, a rounded sum, never an FMA
 * (any4_amd/csrc/stage_math.cuh) -- the bits of the torch ops in decode._rope, and the same in every kernel below that ropes
 * (dg_rope_attn, dg_rope_attn_online, dg_rope_attn_split, dg_prefill_attn; tests/test_gpu_glue_f64.py compares > 4e6 elements each).
 * caches are [bs][kvl][max_seq][d]; d even, d <= 256. */
TG_API int dg_rope_kv(const void* qkv, const float* cos, const float* sin, const int64_t* pos, void* q_out,
                      void* k_cache, void* v_cache, int64_t bs, int hl, int kvl, int d, int64_t max_seq,
                      int dtype, int device, tg_stream_t stream);

/* out[b][h][:] = softmax_s( to16(q[b][h] . k_cache[b][h / (hl/kvl)][s]) * scale ) over s <= *pos, applied to
 * v_cache; probabilities rounded to 16 bit before the value contraction, fp32 accumulation, one rounding of
 * the output.  d % 8 == 0, d <= 256, max_seq <= 8192. */
TG_API int dg_decode_attn(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos, void* out,
                          int64_t bs, int hl, int kvl, int d, int64_t max_seq, float scale, int dtype, int device,
                          tg_stream_t stream);

/* out[b][j] = to16(silu(gu[b][j])) * gu[b][il + j], j < il; gu [bs][2 il]; il % 8 == 0. */
TG_API int dg_swiglu(const void* gu, void* out, int64_t bs, int64_t il, int dtype, int device, tg_stream_t stream);

/* y[m][n] = RNE16(x[m][k] . w[n][k]^T), ROW-MAJOR 16-bit weights (an nn.Linear's), f32 accumulation: the LM head of the decode step,
 * which the reference leaves un-quantised (quantize.py:34-36).  m = 1 ... 4 at k = 2048 / 4096, 1 ... 2 at k = 8192 (TG_E_SHAPE otherwise: the caller
 * keeps its GEMM); x and w 16-byte aligned. */
TG_API int dg_linear16(const void* x, const void* w, void* y, int64_t m, int64_t n, int64_t k, int dtype, int device, tg_stream_t stream);

/* ---- fused attention: one call struct (dg_attn), one entry point (dg_attn_launch) ----
 * A call names its kernel (`kernel`, one of DG_ATTN_GENERAL / ONLINE / SPLIT / PREFILL) and says what its caches are and how `pos` is
 * read (`flags`, DG_ATTN_SEQ | MX8 | PAGED | ONE_BARRIER).  Nothing is inferred from null pointers.  DG_ATTN_FLAVOURS below lists the
 * nineteen accepted (kernel, flags) pairs under the names they had as functions of their own up to ABI 8 (any4_amd/decode_ops.py keeps
 * those names for its functions, and the text below uses them for "the call with that pair").
 *
 * The four kernels, for 16-bit caches [bs][kvl][max_seq][d] and a scalar position (flags = 0):
 *
 * DG_ATTN_GENERAL (dg_rope_attn): dg_rope_kv followed by dg_decode_attn in ONE launch (a hipGraph of dependent kernels advances at ~5 us
 *   per node on MI355X): same arithmetic in the same order, bit-identical results; q is not materialised.  d % 8 == 0,
 *   d <= 256, max_seq <= 8192.
 *
 * DG_ATTN_ONLINE (dg_rope_attn_online): dg_rope_attn for latency (what the decode harness launches at d = 64 / 128): every load of the
 *   launch is issued behind the read of `pos`, scores are reduced with DPP, the softmax statistics are kept per row group and combined
 *   once (flash-decoding style, ONE barrier), so probabilities are normalised after the value contraction: the cache rows written are
 *   bit-identical to dg_rope_kv's, the output agrees with dg_rope_attn within 16-bit rounding.  qkv and the rotary tables 16-byte aligned.
 *
 * DG_ATTN_SPLIT (dg_rope_attn_split): dg_rope_attn with the sequence split over `nsplit` blocks per head (flash-decoding style combine by
 *   the last block to arrive): fills the GPU at batch 1 and long contexts.  With d = 64 / 128 (and 16-byte aligned qkv / tables) it is
 *   dg_rope_attn_online's one-barrier kernel with gridDim.y = nsplit: block c of a head takes the 32-row iterations c, c + nsplit, ... of
 *   the context; what crosses blocks goes through agent-scope atomics, not through a device-scope fence.  `scratch`:
 *   dg_rope_attn_split_scratch_bytes bytes, 16-byte aligned, ZEROED ONCE by the caller before the first launch (the kernel leaves its
 *   counters at zero again); launches sharing a scratch buffer must be stream-ordered.  Probabilities are normalised after the value
 *   contraction, so results agree with dg_rope_attn within 16-bit rounding, not bit for bit.  max_seq / nsplit <= ~15000.
 *
 * DG_ATTN_PREFILL (dg_prefill_attn): a chunk of T new tokens per sequence.  qkv [bs * T][(hl + 2 kvl) * d], row b * T + t = token t of
 *   sequence b (q heads, k heads, v heads, as in dg_rope_kv); *pos = p0 = sequence position of token 0 (int64 on the device, read by the
 *   kernel).
 *     k_cache[b][kv][p0 + t][:] = rope(k, p0 + t);  v_cache[b][kv][p0 + t][:] = v          -- the bits dg_rope_kv writes
 *     out[b * T + t][h * d ...] = softmax_{s <= p0 + t}( (rope(q) . k_cache[b][h / (hl/kvl)][s]) * scale ) applied to v_cache
 *   i.e. token t sees the cache rows [0, p0) that earlier calls wrote and rows [p0, p0 + t] of its own chunk.  q is roped and rounded to
 *   16 bit like k; scores and softmax statistics in f32 (online softmax over 64-position tiles), probabilities rounded to 16 bit for the
 *   value product, f32 accumulation, normalised once, one rounding of the output (dg_rope_attn_online's recipe).  Two launches (cache
 *   append, then attention), no scratch memory, no atomics: a call repeated gives the same bits.  A token whose position p0 + t is
 *   outside [0, max_seq) writes no cache row, is seen by nobody and leaves its output row unwritten; cache rows outside [p0, p0 + T) are
 *   not written, rows above a token's own position are not read.  d = 64 / 128, hl % kvl == 0, max_seq <= 8192, bs <= 65535 (TG_E_SHAPE
 *   otherwise); qkv, the tables, the caches and out 16-byte aligned. */
enum {
  DG_ATTN_GENERAL = 0,
  DG_ATTN_ONLINE = 1,
  DG_ATTN_SPLIT = 2,
  DG_ATTN_PREFILL = 3
};

/* DG_ATTN_SEQ -- a position per sequence (ragged batches).  The decode kernels (the _seq flavours): their namesakes' arithmetic, rounding
 *   points, shape limits and scratch protocol, with `pos` an int64[bs] on the device: sequence b sits at pos[b] (one read per workgroup,
 *   as `*pos` is).  A sequence whose pos[b] is outside [0, max_seq) -- an inactive batch slot, by convention -1 -- writes no cache row and
 *   leaves its row of `out` unwritten, which is what a scalar-position call does for the whole batch.  For every other sequence the cache
 *   rows and the output row are, bit for bit, those of the namesake called for that sequence alone.
 *   DG_ATTN_PREFILL (dg_prefill_attn_seq): position, length and cache slot per sequence.  qkv [bs * T][(hl + 2 kvl) * d]: row i * T + t =
 *   token t of chunk-sequence i, rows padded to the common T; out [bs * T][hl * d] likewise.  All three arrays are int64 on the device:
 *     pos  [bs]           position of token 0 of sequence i
 *     len  [bs] or NULL   only tokens t < min(len[i], T) exist (NULL: all T); later rows write nothing, are seen by nobody and leave
 *                         their output rows unwritten; len[i] <= 0 makes sequence i a no-op
 *     slot [bs] or NULL   sequence i lives in k_cache[slot[i]] / v_cache[slot[i]] of caches [cache_bs][kvl][max_seq][d] (NULL: slot i,
 *                         and bs == cache_bs is required); a slot outside [0, cache_bs) makes sequence i a no-op.  Slots must be
 *                         distinct (the caller's obligation); whatever the three arrays hold, nothing outside the caches is indexed.
 *   Everything else is dg_prefill_attn's: two launches, no scratch, no atomics; rows above a token's own position are never read, tile
 *   rows beyond a workgroup's last valid position are zero-filled on chip; d = 64 / 128, max_seq <= 8192, bs <= 65535.  For an existing
 *   token the cache rows and the output row are, bit for bit, dg_prefill_attn's for that sequence alone with T = len[i].
 *
 * DG_ATTN_MX8 -- mx8 KV cache: block-scaled 8-bit rows (OCP MXFP8; any4_amd/kvcache.py mx8_encode is the definition).  k_cache / v_cache
 *   [bs][kvl][max_seq][d] hold one E4M3 code per element, k_exp / v_exp [bs][kvl][max_seq][d / 32] one E8M0 exponent byte per 32
 *   consecutive elements of a row: value = code * 2^(E - 127); E = 255 marks a block with a non-finite element, which reads as NaN in all
 *   32 places.  The _mx8 flavours keep their namesakes' guards, scratch protocol and rounding points:
 *     writers  the roped k row keeps dg_rope_kv's 16-bit bits; that row and the raw v row are encoded per block -- byte for byte
 *              mx8_encode(rope(k)) / mx8_encode(v).  Rows that are not written keep their codes AND their exponent bytes.
 *     readers  a cached row is converted to the 16-bit type (exact) and enters the namesake's arithmetic in the namesake's order.  In
 *              dg_rope_attn_split_mx8 the new token's own k / v enter the scores and the value sum as their DECODED rows (what later
 *              steps read), not as the unquantised ones.
 *   dg_rope_attn_split_mx8 and its _seq flavour always run the 256-thread split kernel (dg_rope_attn_split's for a d other than 64 / 128):
 *   nsplit = 1 is accepted, max_seq / nsplit <= ~15000; d % 32 == 0 (TG_E_SHAPE otherwise, nothing is touched).  dg_prefill_attn_mx8 and
 *   its _seq flavour: d = 64 / 128.  All four tensors 16-byte aligned; a null k_exp or v_exp is TG_E_NULL.  fp16 stacks whose |k|, |v|
 *   exceed fp16's range after decoding are out of contract.
 *
 * DG_ATTN_ONE_BARRIER -- a DG_ATTN_SPLIT | DG_ATTN_MX8 call held to the one-barrier kernel (dg_rope_attn_online_mx8 and its _seq flavour):
 *   always dg_rope_attn_online's one-barrier kernel in its 8-bit flavour with `nsplit` blocks per head (nsplit = 1: neither partials nor
 *   counters are used; the scratch layout and protocol are dg_rope_attn_split's).  A row lies across d / 8 lanes as the 16-bit rows do: a
 *   lane's piece is 8 code bytes and the exponent byte of its block, every wave-load is contiguous, the first 256 rows are requested
 *   before `pos` is known; pieces are converted to the 16-bit type on use, and behind the conversion every sum and rounding point is the
 *   16-bit kernel's -- on a 16-bit cache that holds the decoded values dg_rope_attn_online / _online_seq (nsplit = 1) and
 *   dg_rope_attn_split / _split_seq give the same output bit for bit.  Writer and new token as in dg_rope_attn_split_mx8: byte for byte
 *   mx8_encode(rope(k)) / mx8_encode(v), entering the sums as the DECODED rows; rows that are not written keep their codes and exponent
 *   bytes, and whatever `pos` holds nothing outside [0, max_seq) of the four tensors is indexed.  In this order: a null pointer (k_exp,
 *   v_exp, scratch included) is TG_E_NULL; d other than 64 / 128, nsplit outside 1 ... 64, max_seq > 65536 or a scratch that is too small
 *   TG_E_SHAPE; caches, exponents, scratch, qkv, cos or sin off a 16-byte boundary TG_E_ALIGN; nothing is touched in any of these cases.
 *
 * DG_ATTN_PAGED -- paged KV cache: a pool of fixed-size pages behind a block table.  Per layer k_cache / v_cache are the POOLS
 *   [num_pages][kvl][page_size][d] in the 16-bit type; one table, int32 [cache_bs][max_seq / page_size] on the device, serves every layer:
 *   logical position p of the sequence in cache slot s is row p % page_size of page table[s][p / page_size] (-1: unmapped, by convention).
 *   page_size is a power of two, 64 <= page_size <= max_seq, max_seq % page_size == 0, num_pages > 0 (TG_E_SHAPE otherwise); d = 64 / 128
 *   in all three; max_seq <= 65536 for the decode kernels, <= 8192 for prefill; the table 16-byte aligned like the other tensors
 *   (TG_E_ALIGN), not null (TG_E_NULL); in every such case nothing is touched.  The contiguous caches [bs][kvl][max_seq][d] ARE the pool
 *   with page_size = max_seq and the identity table.
 *     dg_rope_attn_online_paged   dg_rope_attn_online_seq behind the table
 *     dg_rope_attn_split_paged    the same on dg_rope_attn_split_seq; always the one-barrier kernel with nsplit blocks per head
 *     dg_prefill_attn_paged       the same on dg_prefill_attn_seq; slot[i] picks the table ROW, cache_bs is the number of table rows
 *   A position per sequence always: DG_ATTN_PAGED goes with DG_ATTN_SEQ, and the caller says so (there is no scalar-position paged
 *   flavour); the position, length and slot guards are the _seq ones.  Whatever the table holds, nothing outside the pools is indexed: an
 *   entry outside [0, num_pages) is read as page 0 (that sequence's output is then unspecified), and a row whose OWN entry is outside
 *   [0, num_pages) is not written -- neither pool changes.  Pages of different sequences that are written by one call must be distinct
 *   (the caller's obligation, as distinct slots are).  The kernels walk the context in units that a page holds whole (32- / 64-row
 *   iterations, 64-position tiles); paging changes where a unit's base comes from (one scalar table read) and nothing else: partition of
 *   work, order of every sum, masks and rounding points are the _seq namesakes', so for tables that map the same rows the cache rows
 *   written and the output rows are, bit for bit, theirs.
 *
 * DG_ATTN_PAGED | DG_ATTN_MX8 -- paged mx8 KV cache: 8-bit page pools behind the block table.  Per layer FOUR pools behind the one table:
 *   k_cache / v_cache [num_pages][kvl][page_size][d] hold one E4M3 code BYTE per element, k_exp / v_exp [num_pages][kvl][page_size][d / 32]
 *   one E8M0 exponent byte per 32 consecutive elements of a row (the mx8 format above); logical position p of the sequence in slot s is row
 *   p % page_size of page table[s][p / page_size] in all four.  A page holds at least 64 rows, so the codes and the exponents of a (page,
 *   kv head) begin on 16-byte boundaries when the pools do.
 *     dg_rope_attn_online_mx8_paged   always the one-barrier kernel with nsplit blocks per head (nsplit = 1: neither partials nor counters
 *                                     are used), the one decode flavour
 *     dg_prefill_attn_mx8_paged       dg_prefill_attn_paged on the four pools
 *   Both obey the paged AND the mx8 rules, in the order null, dtype, shape, alignment: a null pointer (table, k_exp, v_exp, scratch
 *   included) is TG_E_NULL; d other than 64 / 128, a page_size that is no power of two in [64, max_seq] or does not divide max_seq,
 *   num_pages <= 0, nsplit outside 1 ... 64 or a scratch that is too small TG_E_SHAPE; pools, exponents, table, scratch, qkv, cos or sin
 *   off a 16-byte boundary TG_E_ALIGN; nothing is touched in any of these cases.  The page lookup is the paged flavours' (an entry outside
 *   [0, num_pages) reads page 0; a row whose OWN entry is outside the pool writes neither codes nor exponent bytes), the rows' bytes and
 *   the arithmetic are the contiguous mx8 flavours': for tables that map the same rows, the bytes written and the output rows are, bit
 *   for bit, those of dg_rope_attn_online_mx8_seq (same nsplit) / dg_prefill_attn_mx8_seq. */
#define DG_ATTN_SEQ 1u
#define DG_ATTN_MX8 2u
#define DG_ATTN_PAGED 4u
#define DG_ATTN_ONE_BARRIER 8u

/* The accepted calls: X(name up to ABI 8, kernel, flags).  Every other pair is TG_E_LAYOUT. */
#define DG_ATTN_FLAVOURS(X)                                                                                         \
  X(dg_rope_attn, DG_ATTN_GENERAL, 0)                                                                               \
  X(dg_rope_attn_seq, DG_ATTN_GENERAL, DG_ATTN_SEQ)                                                                 \
  X(dg_rope_attn_online, DG_ATTN_ONLINE, 0)                                                                         \
  X(dg_rope_attn_online_seq, DG_ATTN_ONLINE, DG_ATTN_SEQ)                                                           \
  X(dg_rope_attn_online_paged, DG_ATTN_ONLINE, DG_ATTN_SEQ | DG_ATTN_PAGED)                                         \
  X(dg_rope_attn_split, DG_ATTN_SPLIT, 0)                                                                           \
  X(dg_rope_attn_split_seq, DG_ATTN_SPLIT, DG_ATTN_SEQ)                                                             \
  X(dg_rope_attn_split_mx8, DG_ATTN_SPLIT, DG_ATTN_MX8)                                                             \
  X(dg_rope_attn_split_mx8_seq, DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_SEQ)                                           \
  X(dg_rope_attn_online_mx8, DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER)                                      \
  X(dg_rope_attn_online_mx8_seq, DG_ATTN_SPLIT, DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER | DG_ATTN_SEQ)                    \
  X(dg_rope_attn_split_paged, DG_ATTN_SPLIT, DG_ATTN_SEQ | DG_ATTN_PAGED)                                           \
  X(dg_rope_attn_online_mx8_paged, DG_ATTN_SPLIT, DG_ATTN_SEQ | DG_ATTN_PAGED | DG_ATTN_MX8 | DG_ATTN_ONE_BARRIER)  \
  X(dg_prefill_attn, DG_ATTN_PREFILL, 0)                                                                            \
  X(dg_prefill_attn_seq, DG_ATTN_PREFILL, DG_ATTN_SEQ)                                                              \
  X(dg_prefill_attn_mx8, DG_ATTN_PREFILL, DG_ATTN_MX8)                                                              \
  X(dg_prefill_attn_mx8_seq, DG_ATTN_PREFILL, DG_ATTN_MX8 | DG_ATTN_SEQ)                                            \
  X(dg_prefill_attn_paged, DG_ATTN_PREFILL, DG_ATTN_SEQ | DG_ATTN_PAGED)                                            \
  X(dg_prefill_attn_mx8_paged, DG_ATTN_PREFILL, DG_ATTN_SEQ | DG_ATTN_PAGED | DG_ATTN_MX8)

/* One call.  C: `struct dg_attn a = {sizeof a};`.  A field that the call's kernel and flags do not use is not read: k_exp / v_exp
 * without DG_ATTN_MX8; table, page_size, num_pages without DG_ATTN_PAGED; scratch, scratch_bytes, nsplit outside DG_ATTN_SPLIT; T outside
 * DG_ATTN_PREFILL; len, slot, cache_bs outside DG_ATTN_PREFILL with DG_ATTN_SEQ.  Pointers and 64-bit fields stand in front of the 32-bit
 * ones, so the struct has no hidden padding. */
typedef struct dg_attn {
  uint32_t struct_bytes;  /* sizeof(struct dg_attn); anything else is TG_E_STRUCT (the first version: there is no shorter prefix) */
  int32_t kernel;         /* DG_ATTN_GENERAL ... DG_ATTN_PREFILL */
  const void* qkv;        /* [bs * T][(hl + 2 kvl) * d], 16-bit */
  const float* cos;       /* float32 [max_seq][d] */
  const float* sin;
  const int64_t* pos;     /* on the device: one position, or [bs] with DG_ATTN_SEQ */
  void* k_cache;          /* the caches; with DG_ATTN_PAGED the pools */
  void* v_cache;
  void* out;              /* [bs * T][hl * d] */
  void* k_exp;            /* DG_ATTN_MX8: the exponent bytes of the caches / pools */
  void* v_exp;
  const int64_t* len;     /* DG_ATTN_PREFILL with DG_ATTN_SEQ: [bs] or NULL */
  const int64_t* slot;    /* DG_ATTN_PREFILL with DG_ATTN_SEQ: [bs] or NULL */
  const int32_t* table;   /* DG_ATTN_PAGED: int32 [cache_bs][max_seq / page_size] */
  void* scratch;          /* DG_ATTN_SPLIT */
  int64_t scratch_bytes;  /* DG_ATTN_SPLIT: at least dg_rope_attn_split_scratch_bytes */
  int64_t bs;             /* sequences of the call */
  int64_t T;              /* DG_ATTN_PREFILL: tokens per sequence */
  int64_t cache_bs;       /* DG_ATTN_PREFILL with DG_ATTN_SEQ: sequences the caches hold / rows of the table */
  int64_t max_seq;
  int64_t page_size;      /* DG_ATTN_PAGED */
  int64_t num_pages;      /* DG_ATTN_PAGED */
  uint32_t flags;         /* DG_ATTN_SEQ | DG_ATTN_MX8 | DG_ATTN_PAGED | DG_ATTN_ONE_BARRIER */
  int32_t hl;             /* query heads, kv heads (hl % kvl == 0), head dimension */
  int32_t kvl;
  int32_t d;
  int32_t nsplit;         /* DG_ATTN_SPLIT: blocks per head, 1 ... 64 */
  int32_t dtype;          /* TG_BF16 / TG_F16 */
  float scale;
  uint32_t reserved;      /* padding to 8 bytes; not read */
} dg_attn;

/* In this order: call == NULL is TG_E_NULL; struct_bytes != sizeof(struct dg_attn) is TG_E_STRUCT; a kernel outside the four, a flag bit
 * outside the four or a (kernel, flags) pair that DG_ATTN_FLAVOURS does not list is TG_E_LAYOUT, before any other field is read; then
 * the kernel's own checks -- null, dtype, shape, alignment -- and the launch. */
TG_API int dg_attn_launch(const dg_attn* call, int device, tg_stream_t stream);
TG_API int64_t dg_rope_attn_split_scratch_bytes(int64_t bs, int hl, int d, int nsplit);

/* ---- sampling: temperature, top-k, top-p (nucleus) and a counter-based draw, one launch per step ----
 * The definition is any4_amd/sampling.py (sample_ref, uniform, philox4x32_10), in float64; this is its kernel.  Per row b of
 * logits [bs][ld] (16-bit, ld >= vocab; rows need no alignment beyond 2 bytes):
 *   rank      tokens ordered by (logit descending, index ascending)
 *   weights   w_i = exp((l_i - l_max) / temperature[b]); temperature[b] == 0: the answer is rank 0 (argmax, lowest index among ties)
 *   top-k     the first top_k[b] ranks are kept (top_k <= 0 or >= vocab: all), Z_k their mass
 *   top-p     of those, the shortest rank prefix whose mass is >= top_p[b] * Z_k (top_p >= 1: all; at least one token), Z its mass
 *   draw      the first kept rank whose inclusive cumulative mass exceeds u * Z (the last kept rank if there is none)
 * u: u_in[b] when u_in is given, else (w >> 8) * 2^-24 with w the first word of Philox4x32-10 at counter (lo32(c), hi32(c), 0, 0) under
 * key (lo32(seed[b]), hi32(seed[b])), c = ctr[per_sequence ? b : 0] + ctr_add -- the index the new token will have in its sequence (a decode
 * step passes its position buffer and ctr_add = 1), so a draw depends on the seed and the place only.  When the value READ from ctr is
 * negative the sequence is inactive: token_out[b] = -1, u_out[b] = 0, its logits are not read.
 * token_out int64 [bs]; u_out float [bs] or NULL: the u used.  temperature / top_p float [bs], top_k int32 [bs], seed int64 [bs] (may be
 * NULL when u_in is given) are read on the device, so a captured graph sees values changed between replays.
 * Arithmetic: the kernel sorts nothing and keeps no [vocab] temporary; it counts tokens per 16-bit value, and a value's mass is
 * count x floor(expf((l - l_max) / temperature) x 2^s) as a 64-bit integer, s = 62 - bit_length(vocab); the argument is formed in float64
 * and rounded to float32 once.  Integer sums have no order, so the same inputs give the same token on every launch and every device.
 * A row whose values occupy more than 512 of the 1024 bins of 64 consecutive 16-bit values (both signs over most binades) is walked in
 * two windows, with extra passes over the row.  Against the float64 definition the normalised cumulative
 * masses differ by at most 2^-22 (3 + ln vocab) + 2^-27, 3.5e-6 at vocab 128256.  Out of contract: NaN or +inf logits, a row that is all -inf, temperature < 0.
 * scratch: dg_sample_scratch_bytes(bs, vocab) bytes, caller-owned; the answer is 0 today and scratch may then be NULL.
 * TG_E_NULL: a required pointer is NULL; TG_E_DTYPE; TG_E_SHAPE: bs < 1, vocab < 1 or ld < vocab; TG_E_SIZE: vocab > 2^30 or bs >= 2^31;
 * TG_E_ALIGN: a pointer off its element's alignment.  Nothing is touched in any of these cases. */
TG_API int dg_sample(const void* logits, const int64_t* ctr, const float* temperature, const int32_t* top_k, const float* top_p,
                     const int64_t* seed, const float* u_in, int64_t* token_out, float* u_out, void* scratch, int64_t scratch_bytes,
                     int64_t bs, int64_t vocab, int64_t ld, int per_sequence, int64_t ctr_add, int dtype, int device, tg_stream_t stream);
TG_API int64_t dg_sample_scratch_bytes(int64_t bs, int64_t vocab);

/* ---- per-sequence LoRA adapters on a linear's output: shrink (t = A x) and expand (y += scale B t), the "BGMV" pair ----
 * The definition is any4_amd/lora.py: lora_ref.  Adapter weights of ONE linear [n][k]: A [n_adapters][r][k] and B [n_adapters][n][r], 16-bit
 * row-major, scale float [n_adapters] (alpha / rank); an adapter of lower rank is zero-padded to r.  The adapter of activation row i is
 * idx[i / rows_per_id] (int32 on the device, ceil(m / rows_per_id) entries: 1 for a decode step, the chunk length for a prefill), read by
 * the kernels, so a captured graph sees ids changed between replays.  A value outside [0, n_adapters) means "no adapter": no address
 * is formed from it.
 *   dg_lora_shrink   t[i][j] = sum_c A[a][j][c] x~[i][c], f32.  x [m][k] 16-bit.  norm_weight NULL: x~ = x.  norm_weight g [k]: x~ =
 *                    RNE16(x g) and the sum is multiplied by rs = rsqrt(mean(x^2) + eps) in f32 -- the "sum" convention of the GEMV's
 *                    fused RMSNorm (tg_w4_gemm.norm_weight), so the adapter contracts the 16-bit activations the base GEMM contracts.
 *                    Rows without an adapter: t = 0.
 *   dg_lora_expand   y[i][c] = RNE16(fma(scale[a], sum_j B[a][c][j] t[i][j], f32(y[i][c]))), j ascending in f32, IN PLACE on y [m][ldy]
 *                    (16-bit, the first n columns of every row).  Rows without an adapter keep their bits: they are not rewritten.
 * Sums run in a fixed order without atomics: the same inputs give the same bits on every launch.  Any m >= 1.
 * TG_E_NULL: a required pointer is NULL; TG_E_DTYPE; TG_E_SHAPE: m, n_adapters or rows_per_id < 1, r outside {8, 16, ..., 64}, k < 8,
 * n < 8, n % 8, ldy < n, ldy % 8; TG_E_K_DIV: k % 8; TG_E_SIZE: m >= 2^31, k > 2^17, n > 65535 x 512; TG_E_ALIGN: x, norm_weight, A,
 * B, t or y off a 16-byte boundary, idx or scale off 4.  Nothing is launched in any of these cases.  No allocation, no synchronisation. */
TG_API int dg_lora_shrink(const void* x, const void* norm_weight, const void* A, const int32_t* idx, float* t, int64_t m, int64_t k,
                          int64_t r, int64_t n_adapters, int64_t rows_per_id, float eps, int dtype, int device, tg_stream_t stream);
TG_API int dg_lora_expand(const float* t, const void* B, const float* scale, const int32_t* idx, void* y, int64_t m, int64_t n, int64_t r,
                          int64_t ldy, int64_t n_adapters, int64_t rows_per_id, int dtype, int device, tg_stream_t stream);

/* ---- mixture of experts (MoE) for a decode step: a top-k router and a 4-bit GEMV whose weights are picked by expert ids on the device ----
 * The definition is any4_amd/moe.py: moe_ref.  Three launches serve one sparse MLP block: route, gate_up, down; all three read their
 * indices on the device, so a captured graph follows the router from replay to replay.  ONE call struct serves this path and the many-row path below
 * (struct dg_moe, dg_moe_launch, dg_moe_plan: ABI 10); the caller names the kernel, nothing is inferred from NULL pointers.
 *
 * dg_moe_route   x [m][k] 16-bit (already normed), router_w [E][k] 16-bit.  l[i][e] = sum_c router_w[e][c] x[i][c] in f32, NOT rounded to
 *   16 bit; p = softmax(l[i]) over all E in f32; the top_k largest p ordered by (p descending, expert index ascending: a tie goes to the
 *   lower index) -> ids int32 [m][top_k]; gates float [m][top_k], g[i][s] = p_s / (p_0 + ... + p_{top_k-1}), the sum in slot order.
 *   E in 1 ... 64, top_k in 1 ... min(E, 8), k % 8 == 0 (TG_E_K_DIV), any m >= 1.  NaN or infinite logits are out of contract; even then
 *   every id written is in [0, E) and a row's ids are distinct.  Sums run in a fixed order: the same inputs give the same bits.
 *   TG_E_NULL, TG_E_DTYPE, TG_E_SHAPE, TG_E_K_DIV, TG_E_SIZE (k > 2^20), TG_E_ALIGN (x, router_w off 16 bytes; ids, gates off 4).
 *
 * dg_moe_launch, kernel DG_MOE_GEMV   one layer's experts are STACKED: expert e of an operand sits at base + e * stride (bytes, a multiple of 16):
 *     w      Bint4 words [E][wrows / 8][k / 64][32][2] int32 (tg_convert_to_Bint4 at innerKTiles 4, per expert)
 *     qinfo  scales_and_zeros [E][k / group][wrows][2] 16-bit
 *     lut    [E][wrows][16] (TG_Q_ANY4_ROWWISE) or [E][16] (TG_Q_ANY4_GLOBAL) 16-bit; not read for TG_Q_INT4
 *   ids int32 [m][top_k]: pair (i, s) = activation row i, slot s.  An id outside [0, E) is never turned into an address.
 *   Numerics are TG_NUM_FAST's: f32 sums of the looked-up values times the activations per group, the group's scale and zero applied to
 *   the partial sums.
 *   stage DG_MOE_GATE_UP   x [m][k] (the top_k slots of a row share it); weight rows in blocks of 16 = 8 gate + 8 up rows (TG_EPI_SWIGLU's
 *                          order); y [m * top_k][wrows / 2], row i * top_k + s = RNE16(RNE16(silu(RNE16(gate))) RNE16(up)) of expert
 *                          ids[i][s] (dg_swiglu's rounding points).  A pair with an invalid id gets a row of zeros.
 *   stage DG_MOE_DOWN      x [m * top_k][k], one row per pair; gates float [m][top_k]; residual [m][wrows] 16-bit or NULL;
 *                          y[i] = RNE16(sum_s gates[i][s] d_s (+ residual[i])), d_s the unrounded f32 sum of pair (i, s).  The terms are
 *                          added by fused multiply-add in the order (expert id ascending, then slot ascending), the residual last: the
 *                          order depends on ids alone, so the same inputs give the same bits on every launch.  A pair with an invalid
 *                          id contributes nothing; a row without a valid pair gets RNE16(residual), or zeros.
 *   int4 and any4, inner_k_tiles 4, group 64 / 128 / 256, k % 64 == 0, wrows % 16 == 0.  m <= 8 is one launch; larger m is issued as
 *   ceil(m / 8) launches on the caller's stream (every block of 8 rows re-reads its experts: for many rows -- a prompt -- there is
 *   kernel DG_MOE_GROUPED below, which reads a selected expert once per 128 of its rows).
 *   Within a launch a selected expert's rows cross the memory interface once per workgroup range as long as at most `pairs per sweep`
 *   (dg_moe_plan: 8; fewer from k of about 4800 on, because the sweep's activation rows are staged in LDS) pairs chose it; an unselected
 *   expert's bytes are never requested.  No atomics, no scratch, no allocation, no synchronisation.
 *   In this order: call == NULL TG_E_NULL; struct_bytes TG_E_STRUCT; kernel or stage TG_E_LAYOUT; a required pointer (x, w, qinfo, y, ids; lut for
 *   any4; gates for DOWN) TG_E_NULL; TG_E_DTYPE; TG_E_QTYPE (mx4, int8); TG_E_SHAPE (m < 1, E outside 1 ... 64, top_k outside
 *   1 ... min(E, 8), k % 64, wrows % 16); TG_E_SIZE (an expert beyond 2^31 bytes, k beyond what LDS stages); TG_E_INNER_K; TG_E_GROUP;
 *   TG_E_ALIGN (an operand off 16 bytes, ids or gates off 4, a stride that is no multiple of 16).  Nothing is launched in these cases.
 *   group_ws, f32_ws and their sizes are not read.
 * dg_moe_plan, kernel DG_MOE_GEMV   the launch plan of the call's first row block, for tests and tools: out[0] workgroups, out[1] 16-row
 *   units per workgroup, out[2] pairs per sweep, out[3] waves that own part of k, out[4 ... 7] 0.  device < 0: planned for 256 compute
 *   units, without a device.  out == NULL: TG_E_NULL. */
#define DG_MOE_GATE_UP 0
#define DG_MOE_DOWN 1
#define DG_MOE_GEMV 0     /* dg_moe::kernel: the expert-indexed GEMV, a decode step's few rows */
#define DG_MOE_GROUPED 1  /* the grouped tile GEMM over the pairs dg_moe_group sorted, a prompt's many rows (below) */

/* One call.  C: `struct dg_moe c = {sizeof c};`.  Pointers and 64-bit fields stand in front of the 32-bit ones: no hidden padding.  A field
 * that the call's kernel and stage do not use is not read. */
typedef struct dg_moe {
  uint32_t struct_bytes;    /* sizeof(struct dg_moe); anything else is TG_E_STRUCT */
  int32_t kernel;           /* DG_MOE_GEMV / DG_MOE_GROUPED */
  const void* x;
  const void* w;
  const void* qinfo;
  const void* lut;
  void* y;
  const int32_t* ids;
  const float* gates;       /* DG_MOE_DOWN */
  const void* residual;     /* DG_MOE_DOWN, optional */
  const int32_t* group_ws;  /* DG_MOE_GROUPED */
  float* f32_ws;            /* DG_MOE_GROUPED, DG_MOE_DOWN */
  int64_t stride_w;         /* bytes between experts */
  int64_t stride_qinfo;
  int64_t stride_lut;
  int64_t m;
  int64_t wrows;
  int64_t k;
  int64_t group_ws_bytes;   /* DG_MOE_GROUPED */
  int64_t f32_ws_bytes;     /* DG_MOE_GROUPED, DG_MOE_DOWN */
  int32_t stage;            /* DG_MOE_GATE_UP / DG_MOE_DOWN */
  int32_t E;
  int32_t top_k;
  int32_t group;
  int32_t qtype;            /* TG_Q_INT4 / TG_Q_ANY4_GLOBAL / TG_Q_ANY4_ROWWISE */
  int32_t dtype;            /* TG_BF16 / TG_F16 */
  int32_t inner_k_tiles;    /* 4 */
  uint32_t reserved;        /* padding to 8 bytes; not read */
} dg_moe;

TG_API int dg_moe_route(const void* x, const void* router_w, int32_t* ids, float* gates, int64_t m, int64_t k, int64_t E, int64_t top_k,
                        int dtype, int device, tg_stream_t stream);
TG_API int dg_moe_launch(const dg_moe* call, int device, tg_stream_t stream);
TG_API int dg_moe_plan(const dg_moe* call, int device, int64_t* out /* [8] */);

/* ---- mixture of experts for MANY rows (a prompt): the pairs sorted by expert, then a grouped 4-bit tile GEMM ----
 * The definition is any4_amd/moe.py: moe_grouped_ref (the group workspace's: group_ref).  Four launches serve one sparse MLP block: dg_moe_route
 * (above), dg_moe_group, dg_moe_launch with kernel DG_MOE_GROUPED twice (DG_MOE_GATE_UP; DG_MOE_DOWN, which issues the combine behind its
 * GEMM).  Nothing is read on the host: the grid is sized by a bound, so a captured graph follows the router.
 *
 * NUMERICS are the tile GEMM's (tg_gemm_w4 at many rows), NOT DG_MOE_GEMV's: a weight is w = RNE16(fma(f32(lut[row][code]), f32(scale),
 *   f32(zero))) (int4: lut = code - 8), products are summed in f32 (v_mfma_f32_16x16x32), k ascending in 64-k super-tiles, never split: the
 *   bits of a row's sums do not depend on m, on the tile the row landed in or on the other rows.
 *
 * dg_moe_group   ids int32 [m][top_k] -> the group workspace (int32; P = m top_k pairs, pair p = i top_k + s; one launch of one workgroup,
 *   no atomics, the same ids give the same bytes):
 *     [0] n_tiles  [1] n_invalid  [2] n_valid  [3] bm
 *     [4 ... 67]    count[e]   pairs of expert e (0 from E on)
 *     [68 ... 135]  offset[e]  prefix of count, offset[E] = n_valid (0 beyond)
 *     [136 ...]     perm[P]    the pairs with an id in [0, E), sorted by (expert ascending, pair ascending) -- a stable counting sort --; -1 from
 *                              n_valid on
 *     then          invalid[P] the pairs whose id is outside [0, E), ascending; -1 from n_invalid on.  Such an id is never turned into an address.
 *     then          tiles[bound][3]  (expert, first position in perm, rows <= bm): an expert with c pairs has ceil(c / bm) tiles, experts
 *                              ascending; zeros from n_tiles on.  bound = ceil(P / bm) + min(E, P) >= n_tiles is the m-extent of the GEMM's grid.
 *   group_ws_bytes >= 4 * (136 + 2 P + 3 bound).  bm: the GEMM's tile height (dg_moe_plan out[0]).
 *   TG_E_NULL; TG_E_SHAPE (m < 1, E outside 1 ... 64, top_k outside 1 ... min(E, 8), bm not the GEMM's); TG_E_SIZE (P > 65536, workspace too
 *   small); TG_E_ALIGN (ids, group_ws off 4 bytes).  Nothing is launched in these cases.
 *
 * dg_moe_launch, kernel DG_MOE_GROUPED   the one struct, operands as DG_MOE_GEMV's (stacked experts: base + e * stride); group_ws as
 *   dg_moe_group left it for the same ids.
 *   An LDS-tiled MFMA GEMM, one workgroup per (tile of the list, n tile); a workgroup whose tile index is >= n_tiles exits before it touches
 *   memory; rows beyond a tile's `rows` are not stored.  Activation rows are gathered, results scattered to the pair's own row:
 *   stage DG_MOE_GATE_UP   x [m][k]; y [P][wrows / 2], row p = RNE16(RNE16(silu(RNE16(gate))) RNE16(up)) of expert ids[p]; rows of the pairs in
 *                          invalid[] are written as +0.
 *   stage DG_MOE_DOWN      x [P][k]; the GEMM stores the unrounded f32 sums d [P][wrows] to f32_ws (f32_ws_bytes >= 4 P wrows, 16-byte
 *                          aligned, not cleared: the row of an invalid pair is never read), then the combine: y[i] = RNE16(sum_s gates[i][s]
 *                          d[i top_k + s] (+ residual[i])), fused multiply-adds from 0 in the order (expert id ascending, then slot
 *                          ascending), the residual last -- DG_MOE_DOWN's order under DG_MOE_GEMV.  y may be residual.
 *   int4 and any4, inner_k_tiles 4, group 64 / 128 / 256, k % 64 == 0, wrows % 16 == 0, any m >= 1 with P <= 65536.  No atomics, no scratch,
 *   no allocation, no synchronisation.
 *   Refusals in DG_MOE_GEMV's order with its codes (no k that LDS cannot stage); the workspaces join them: group_ws (f32_ws for DOWN) NULL with the required pointers
 *   (TG_E_NULL), P > 65536 or a workspace too small with TG_E_SIZE, group_ws off 4 / f32_ws off 16 bytes with TG_E_ALIGN.  GATE_UP does not
 *   read f32_ws or its size.
 * dg_moe_plan, kernel DG_MOE_GROUPED   nothing launched, the workspaces are not looked at; out[0] bm (pairs per tile), out[1] weight rows per tile, out[2] the
 *   grid's m-extent (bound), out[3] n tiles, out[4] 64-k super-tiles per step (2 when k % 128 == 0), out[5] bytes of the group workspace,
 *   out[6] bytes of the f32 workspace (0 for GATE_UP), out[7] 0.  device < 0: without a device. */
TG_API int dg_moe_group(const int32_t* ids, int32_t* group_ws, int64_t group_ws_bytes, int64_t m, int64_t top_k, int64_t E, int64_t bm,
                        int device, tg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
