// tg_trace.cuh -- the developer trace (builds with -DGEMV_TRACE=1, dev/gemv_trace.py): a kernel stamps s_memrealtime at up to eight of
// its phases and one thread per workgroup writes the stamps to [workgroup][8] of a buffer the tool handed over (tg_dev_gemv_trace,
// tg_dev_p16_trace, tg_dev_attn_trace).  In every other build the macros below expand to nothing.
#pragma once
#ifndef GEMV_TRACE
#define GEMV_TRACE 0
#endif

#if GEMV_TRACE
#define TG_TRACE_BEGIN() unsigned long long tg_tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define TG_STAMP(i) tg_tr[i] = __builtin_amdgcn_s_memrealtime()
#define TG_STAMP_IF(cond, i) do { if (cond) TG_STAMP(i); } while (0)
// (values a stamp must wait for: asm operands, e.g. "v"(acc[0]))
#define TG_TRACE_KEEP(...) asm volatile("" ::__VA_ARGS__)
// the first n stamps to buf[workgroup][8], by the thread(s) for which `cond` holds
#define TG_TRACE_FLUSH(cond, buf, n)                                               \
  do {                                                                             \
    if (cond) {                                                                    \
      _Pragma("unroll") for (int tg_i = 0; tg_i < (n); ++tg_i) (buf)[(size_t)blockIdx.x * 8 + tg_i] = tg_tr[tg_i]; \
    }                                                                              \
  } while (0)

// Host side: the tool's buffer as a ring of [slots][512 workgroups][8 stamps]; every traced launch takes the next slot.
struct TraceRing {
  unsigned long long* buf = nullptr;
  int slots = 0, launch = 0;
  void set(unsigned long long* b, int n) { buf = b; slots = n; launch = 0; }
  unsigned long long* next() { return buf && slots > 0 ? buf + (size_t)(launch++ % slots) * 512 * 8 : nullptr; }
};
#else
#define TG_TRACE_BEGIN() do { } while (0)
#define TG_STAMP(i) do { } while (0)
#define TG_STAMP_IF(cond, i) do { } while (0)
#define TG_TRACE_KEEP(...) do { } while (0)
#define TG_TRACE_FLUSH(cond, buf, n) do { } while (0)
#endif
