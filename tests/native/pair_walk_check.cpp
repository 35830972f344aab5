// pair_walk_check.cpp -- stand-alone host check of any4_amd/csrc/pair_walk.h (the item walk of w4_pair_m1_lean_kernel) against the
// division-based decode of the general pair kernel: for every grid of 1 ... 512 workgroups and a range of (items, rblocks), every
// workgroup's range is walked item by item (no division behind the first) and each item compared with item / rblocks, item % rblocks
// and the offsets b * stride + rb * step.  The ranges must also tile [0, items) without gap or overlap.  Built with -fsanitize=address,undefined by
// tests/test_pair_walk_cpu.py.  Exit status 0 = all equal.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../any4_amd/csrc/pair_walk.h"

static long long checked = 0;

static int check(int wgs, int items, int rblocks, const PairWalkGeom& g) {
  std::vector<PairWalk> seen;  // (heap: an index slip is the sanitizer's to catch)
  seen.reserve((size_t)items);
  int expect_begin = 0;
  for (int wg = 0; wg < wgs; ++wg) {
    int begin, end;
    pair_walk_range(wg, wgs, items, begin, end);
    if (begin != expect_begin || end < begin || end > items) {
      fprintf(stderr, "range: wgs %d items %d wg %d: [%d, %d), expected begin %d\n", wgs, items, wg, begin, end, expect_begin);
      return 1;
    }
    expect_begin = end;
    if (begin >= end) continue;
    PairWalk e = pair_walk_first(g, begin);
    for (int it = begin; it < end; ++it) {
      // the general kernel's decode(): per_problem = rblocks (one activation pass)
      const int b = it / rblocks, rb = it - b * rblocks;
      const PairWalk at = pair_walk_at(g, b, rb);
      bool ok = e.b == b && e.rb == rb;
      for (int i = 0; i < PW_N; ++i) {
        const int64_t want = (int64_t)b * g.stride[i] + (int64_t)rb * g.step[i];
        ok = ok && e.off[i] == want && at.off[i] == want;
      }
      if (!ok) {
        fprintf(stderr, "walk: wgs %d items %d rblocks %d item %d: got (b %d, rb %d), expected (%d, %d) or an offset differs\n", wgs, items,
                rblocks, it, e.b, e.rb, b, rb);
        return 1;
      }
      seen.push_back(e);
      ++checked;
      if (it + 1 < end) pair_walk_next(g, e);  // (the kernel's last item keeps its own rows)
    }
  }
  if (expect_begin != items || (int)seen.size() != items) {
    fprintf(stderr, "cover: wgs %d items %d: ranges end at %d, %zu items walked\n", wgs, items, expect_begin, seen.size());
    return 1;
  }
  return 0;
}

int main() {
  // the strides of a stacked 4096 x 4096 launch (bytes: packed words, scale | zero, per-row LUT), and a second set with padding between
  // the problems, one LUT per problem and problems far enough apart for offsets beyond 2^32
  const int rbs[] = {1, 2, 3, 5, 64};
  for (int rblocks : rbs) {
    for (int variant = 0; variant < 2; ++variant) {
      PairWalkGeom g;
      g.rblocks = rblocks;
      const int64_t ksuper = variant ? 224 : 64, wrows = 64LL * rblocks;
      g.step[PW_W] = ksuper * 2048; g.step[PW_Q] = 256; g.step[PW_LUT] = variant ? 0 : 2048;
      g.stride[PW_W] = g.step[PW_W] * rblocks + (variant ? (1LL << 33) + 4096 : 0);
      g.stride[PW_Q] = wrows * 4 * 32 + (variant ? 16 : 0);
      g.stride[PW_LUT] = variant ? 32 : wrows * 32;
      const int batches[] = {1, 2, 3, 7, 96, 173, 600};
      for (int batch : batches) {
        const int items = batch * rblocks;
        if (items > 1500) continue;  // (keeps the sanitizer build's run at about a second)
        for (int wgs = 1; wgs <= 512; ++wgs)
          if (check(wgs, items, rblocks, g)) return 1;
      }
    }
  }
  printf("pair_walk_check: %lld items equal to the division-based decode\n", checked);
  return 0;
}
