// pair_walk.h -- the item walk of the lean m = 1 pair kernel (w4_pair_m1_lean_kernel, w4_gemm_pair.cuh): which work items a workgroup
// takes and where an item's rows start in every operand.  Plain C++ (no HIP), so that a host program can check it against the
// division-based decode of the general kernel (tests/native/pair_walk_check.cpp).
//
// A work item is one 64-row block of one problem of the batch: item = b * rblocks + rb.  A workgroup takes a contiguous range of items:
// one division finds the first, every further one is the next row block or the next problem's first (a comparison).  The per-lane part of
// every address is the same for all items (the rows of a block are a multiple of 64), so the kernel computes it once per launch; what
// moves from item to item are these wave-uniform byte offsets, b * stride + rb * step per operand: scalar multiplications, once per item.
// (Moving the offsets by increments instead -- + step, or + stride - (rblocks - 1) step behind a problem's last block -- measured equal,
//  the multiplications stay, they need no state.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TG_WALK_FN __host__ __device__ __forceinline__
#else
#define TG_WALK_FN inline
#endif

enum { PW_W = 0, PW_Q = 1, PW_LUT = 2, PW_N = 3 };  // packed words, scale | zero words, LUT rows

struct PairWalkGeom {
  int32_t rblocks;       // 64-row blocks per problem
  int64_t step[PW_N];    // bytes from one row block to the next of the same problem
  int64_t stride[PW_N];  // bytes from one problem to the next
};

struct PairWalk {
  int32_t b, rb;       // problem, row block
  int64_t off[PW_N];   // byte offset of the item's rows from the operand's start
};

// the items [begin, end) of workgroup `wg` of `wgs`
TG_WALK_FN void pair_walk_range(int wg, int wgs, int items, int& begin, int& end) {
  begin = (int)(((int64_t)wg * items) / wgs);
  end = (int)(((int64_t)(wg + 1) * items) / wgs);
}

// an item by its coordinates (multiplications only) ...
TG_WALK_FN PairWalk pair_walk_at(const PairWalkGeom& g, int b, int rb) {
  PairWalk e;
  e.b = b;
  e.rb = rb;
  for (int i = 0; i < PW_N; ++i) e.off[i] = (int64_t)b * g.stride[i] + (int64_t)rb * g.step[i];
  return e;
}

// ... by its number (the one division of a workgroup's walk) ...
TG_WALK_FN PairWalk pair_walk_first(const PairWalkGeom& g, int item) {
  const int b = item / g.rblocks;
  return pair_walk_at(g, b, item - b * g.rblocks);
}

// ... and the item behind `e`: no division
TG_WALK_FN void pair_walk_next(const PairWalkGeom& g, PairWalk& e) {
  const bool wrap = e.rb + 1 == g.rblocks;
  e = pair_walk_at(g, wrap ? e.b + 1 : e.b, wrap ? 0 : e.rb + 1);
}
