// kv_paged.cuh -- where a KV-cache row is (every layout), and the paged cache on the device (include/decode_glue_hip.h, the dg_*_paged
// entry points); shared by decode_glue.cuh and attn_prefill.cuh.
// Everything here counts in ROWS of a cache or pool: row R of a 16-bit cache starts at byte R * d * 2, of mx8 codes at byte R * d, of mx8
// exponents at byte R * (d / 32) (kv8.cuh), so one row index serves every tensor of a layout.
//   contiguous  [cache_bs][kvl][max_seq] rows: logical row r of (slot s, kv head) is row kv_head_row(s, kvl, kv, max_seq) + r.
//   paged       per layer the pools are [num_pages][kvl][page_size] rows; one int32 table [cache_bs][max_seq / page_size] maps logical
//               row r of the sequence in slot s to row r % page_size of page table[s][r / page_size].  The kernels walk the context in
//               units that a page holds whole (page_size >= 64 and a power of two), so paging only changes where a unit's first row
//               comes from (kv_unit_row): the page id is wave-uniform (a scalar read), the unit's base a 64-bit scalar, the offset
//               within the unit the 32-bit one it was.  A page holds at least 64 rows, so a unit's code base (row * d bytes) and
//               exponent base (row * d / 32 bytes) are multiples of 16 bytes for d = 64 and 128.  mx8: four pools behind the one table.
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
// first row of (slot s, kv head) in a contiguous cache
__device__ __forceinline__ int64_t kv_head_row(int s, int kvl, int kv, int64_t max_seq) { return ((int64_t)s * kvl + kv) * max_seq; }
// pool row of logical row r, whose page is `page`, for the kv head
__device__ __forceinline__ int64_t kv_page_row(const KvPages& G, int page, int kvl, int kv, int r) {
  return (((int64_t)page * kvl + kv) << G.page_shift) + (r & ((1 << G.page_shift) - 1));
}
// READ: first pool row of the unit that starts at logical row r0 (inside [0, max_seq)) -- wave-uniform
__device__ __forceinline__ int64_t kv_unit_row(const KvPages& G, int s, int kvl, int kv, int r0) {
  return kv_page_row(G, __builtin_amdgcn_readfirstlane(kv_page_read(G, s, r0)), kvl, kv, r0);
}
// ... of the whole page that holds r0, for a caller that keeps the row within the page, r0 & (page_size - 1), in its 32-bit offset
__device__ __forceinline__ int64_t kv_unit_page_row(const KvPages& G, int s, int kvl, int kv, int r0) {
  return kv_page_row(G, __builtin_amdgcn_readfirstlane(kv_page_read(G, s, r0)), kvl, kv, 0);
}
// WRITE: pool row of position pos (inside [0, max_seq)); -1: dropped
__device__ __forceinline__ int64_t kv_write_row(const KvPages& G, int s, int kvl, int kv, int pos) {
  const int page = kv_page_write(G, s, pos);
  return page < 0 ? -1 : kv_page_row(G, page, kvl, kv, pos);
}
