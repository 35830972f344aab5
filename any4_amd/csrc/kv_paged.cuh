// kv_paged.cuh -- the paged KV cache on the device (include/decode_glue_hip.h, the dg_*_paged entry points), shared by decode_glue.cuh
// and attn_prefill.cuh.  Per layer the pools are [num_pages][kvl][page_size][d]; one int32 table [cache_bs][max_seq / page_size] maps
// logical position p of the sequence in slot s to row p % page_size of page table[s][p / page_size].  The kernels walk the context in
// units that a page holds whole (page_size >= 64 and a power of two), so paging only changes where a unit's base address comes from:
// the page id is wave-uniform (a scalar read), the base a 64-bit scalar, the offset within the page the 32-bit one it was.
// mx8 pools (the dg_*_mx8_paged entry points; kv8.cuh): four pools behind the one table -- codes [num_pages][kvl][page_size][d] BYTES and
// exponents [num_pages][kvl][page_size][d / 32] bytes.  kv_page_base counts elements: the byte base of the codes of (page, kv head) is
// kv_page_base(G, page, kvl, kv, d), that of the exponents kv_page_base(G, page, kvl, kv, d / 32).
#pragma once

// What only the PAGED kernels read: their LAST argument.  The prefill kernels take PagedArg<PAGED>, an empty one for the contiguous
// flavours (which keep their argument offsets and their code); rope_attn_online_kernel reads gridDim from the implicit arguments behind
// the explicit ones, which even an empty struct would move, and takes KvPages as an optional last parameter instead.
struct KvPages {
  const int32_t* table;  // [cache_bs][entries]
  int32_t page_shift;    // log2(page_size)
  int32_t entries;       // max_seq / page_size: table entries per sequence
  int32_t num_pages;
};
template <bool PAGED> struct PagedArg {};
template <> struct PagedArg<true> : KvPages {};
// (a kernel that takes the argument as an optional last parameter, `PG... pages`: the one element of the pack)
__device__ __forceinline__ const KvPages& kv_pages_arg(const KvPages& g) { return g; }
// (... `KvPages, Kv8Exps`, the paged mx8 flavour: the first of the two)
template <typename REST> __device__ __forceinline__ const KvPages& kv_pages_arg(const KvPages& g, const REST&) { return g; }

// Page of logical row `r` (inside [0, max_seq)) of the sequence in slot `s`, for a READ: an entry outside [0, num_pages) -- unmapped is
// -1 by convention -- reads page 0, so nothing outside the pools is indexed (that sequence's output is then unspecified).
__device__ __forceinline__ int kv_page_read(const KvPages& G, int s, int r) {
  const int e = G.table[(int64_t)s * G.entries + (r >> G.page_shift)];
  return (uint32_t)e < (uint32_t)G.num_pages ? e : 0;
}
// ... for a WRITE: -1 when the entry is outside [0, num_pages) -- the write is dropped
__device__ __forceinline__ int kv_page_write(const KvPages& G, int s, int r) {
  const int e = G.table[(int64_t)s * G.entries + (r >> G.page_shift)];
  return (uint32_t)e < (uint32_t)G.num_pages ? e : -1;
}
// first element of (page, kv head) in a pool [num_pages][kvl][page_size][d]
__device__ __forceinline__ int64_t kv_page_base(const KvPages& G, int page, int kvl, int kv, int d) {
  return (((int64_t)page * kvl + kv) << G.page_shift) * d;
}
