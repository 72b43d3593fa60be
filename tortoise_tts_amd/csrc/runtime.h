// Host-side runtime pieces shared by the stage engines: device arena, the stream bridge that lets
// an engine run (and hipGraph-capture) on its own stream while staying ordered with the caller's,
// the operand-overflow guard, the kept hipGraph, and a thin GEMM call builder.
#pragma once
#include <algorithm>
#include <vector>
#include <stdlib.h>
#include "ops.h"

namespace tt {

// All engine workspaces come from hipMalloc at create time; nothing is allocated on the hot path.
struct Arena {
  std::vector<void*> ptrs;
  size_t total = 0;
  int alloc(void** out, size_t bytes, bool zero = true) {
    void* p = nullptr;
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      set_error("hipMalloc(%zu bytes) failed: %s (arena holds %zu bytes)", bytes, hipGetErrorString(e), total);
      return -2;
    }
    if (zero) {
      e = hipMemset(p, 0, bytes);
      if (e != hipSuccess) {
        set_error("hipMemset failed: %s", hipGetErrorString(e));
        return -2;
      }
    }
    ptrs.push_back(p);
    total += bytes;
    *out = p;
    return 0;
  }
  template <typename P> int alloc_t(P** out, size_t count, bool zero = true) { return alloc((void**)out, count * sizeof(P), zero); }
  void release() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
    total = 0;
  }
};

// The caller hands us any stream (often the legacy null stream, which cannot be captured).  run() enqueues an entry point's work
// on the engine's own stream, ordered after everything already queued on the caller's stream, and makes the caller's stream wait
// for it - on every path, so that a call failing half-way still leaves the caller's stream behind what it did enqueue.
struct StreamBridge {
  hipStream_t own = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  int init() {
    TT_CHECK_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    TT_CHECK_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    TT_CHECK_HIP(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    return 0;
  }
  // body(own) -> 0 or an error code; the first error is the one returned and reported by tt_last_error
  template <typename F>
  int run(hipStream_t user, F&& body) {
    TT_CHECK_HIP(hipEventRecord(ev_in, user));
    TT_CHECK_HIP(hipStreamWaitEvent(own, ev_in, 0));
    const int rc = body(own);
    if (rc) {
      if (hipEventRecord(ev_out, own) == hipSuccess) (void)hipStreamWaitEvent(user, ev_out, 0);
      return rc;
    }
    TT_CHECK_HIP(hipEventRecord(ev_out, own));
    TT_CHECK_HIP(hipStreamWaitEvent(user, ev_out, 0));
    return 0;
  }
  void destroy() {
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (own) (void)hipStreamDestroy(own);
    own = nullptr;
    ev_in = ev_out = nullptr;
  }
};

// Operand-overflow guard (fp16 operands saturate at 65504): dev[0] counts the kernels (workgroups) that met a non-finite value
// since the last reset; snapshot() copies it into the pinned host word at the end of a run, read() reports that copy.
struct OverflowGuard {
  int* dev = nullptr;   // [4] device counters
  int* host = nullptr;  // pinned copy of dev[0]
  int init(Arena& arena, const char* who) {
    TT_TRY(arena.alloc_t(&dev, 4));
    if (hipHostMalloc((void**)&host, 4 * sizeof(int)) != hipSuccess) {
      set_error("%s: hipHostMalloc failed", who);
      return -2;
    }
    host[0] = 0;
    return 0;
  }
  int snapshot(hipStream_t s) {
    TT_CHECK_HIP(hipMemcpyAsync(host, dev, sizeof(int), hipMemcpyDeviceToHost, s));
    return 0;
  }
  // The count as of the last snapshot (>= 0), or a negative error.  A non-zero count becomes the error message "<stage> stage: <count>
  // <met> (operand overflow in <detail>)".  reset != 0 clears it on stream s.
  int read(int reset, hipStream_t s, const char* who, const char* stage, const char* met, const char* detail) {
    const int n = host[0];
    if (n > 0) set_error("%s stage: %d %s (operand overflow in %s)", stage, n, met, detail);
    if (reset && n > 0) {  // (a clean counter needs no device work: this sits at the end of every utterance)
      if (hipMemsetAsync(dev, 0, 4 * sizeof(int), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reset failed", who);
        return -2;
      }
      host[0] = 0;
    }
    return n;
  }
  void release() {
    if (host) (void)hipHostFree(host);
    host = nullptr;
  }
};

// A captured hipGraph kept on a handle between calls.  `key` holds the bytes of everything the capture baked in that a later call
// could change: ensure() replays the kept graph while the key matches and re-captures otherwise.
struct KeptGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  std::vector<unsigned char> key;
  int captures = 0;  // successful captures so far (tt_*_stat: tests assert the kept graph is reused)
  void drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
    key.clear();
  }
  // Capture fn() -> 0 | error on stream s.  The capture is always ended; on any failure nothing is kept.
  template <typename F>
  int capture(hipStream_t s, const char* who, F&& fn) {
    drop();
    hipError_t ce = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (ce != hipSuccess) {
      set_error("%s: capture failed: %s", who, hipGetErrorString(ce));
      return -2;
    }
    int rc = fn();
    ce = hipStreamEndCapture(s, &graph);
    if (!rc && ce != hipSuccess) { set_error("%s: capture failed: %s", who, hipGetErrorString(ce)); rc = -2; }
    if (!rc && (ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
      set_error("%s: instantiate failed: %s", who, hipGetErrorString(ce));
      rc = -2;
    }
    if (rc) {
      drop();
      return rc;
    }
    captures += 1;
    return 0;
  }
  template <typename F>
  int ensure(hipStream_t s, const void* k, size_t bytes, const char* who, F&& fn) {
    const unsigned char* kb = (const unsigned char*)k;
    if (exec && key.size() == bytes && std::equal(kb, kb + bytes, key.begin())) return 0;
    TT_TRY(capture(s, who, fn));
    key.assign(kb, kb + bytes);
    return 0;
  }
  int launch(hipStream_t s, const char* who) {
    const hipError_t ce = hipGraphLaunch(exec, s);
    if (ce != hipSuccess) {
      set_error("%s: hipGraphLaunch: %s", who, hipGetErrorString(ce));
      return -2;
    }
    return 0;
  }
};

// What every engine handle (tt_ar, tt_clvp, ...) owns besides its own buffers.  open() comes first in a create; close() comes
// first in a destroy: it waits for the device, after which the handle's own buffers and graphs can go too.
struct EngineHandle {
  Arena arena;
  StreamBridge sb;
  OverflowGuard guard;  // allocated by the stages whose kernels count non-finite values (open(who, true))
  int open(const char* who, bool with_guard) {
    TT_TRY(sb.init());
    return with_guard ? guard.init(arena, who) : 0;
  }
  // The body of every tt_*_guard entry point `who`: the guard of the `stage` stage as of its last finished run; the fp16 case of the
  // message ends in the stage's advice.
  int read_guard(int reset, const char* who, const char* stage, int dtype, const char* met = "kernel(s) met non-finite values",
                 const char* f16_advice = "fp16: use bf16 operands for this stage") {
    return guard.read(reset, sb.own, who, stage, met, dtype == DT_F16 ? f16_advice : "bf16");
  }
  void close() {
    (void)hipDeviceSynchronize();
    guard.release();
    arena.release();
    sb.destroy();
  }
};

extern bool g_graph_replay;  // tt_graph_replay (common.hip): diagnostics switch, default on
static inline bool graphs_enabled() { return g_graph_replay; }

static inline GemmArgs gemm_args(const void* A, int lda, const void* W, int ldw, int M, int N, int K) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = M; g.N = N; g.K = K;
  g.taps = 1; g.seq_len = M; g.splitk = 1; g.q_scale = 1.f;
  return g;
}

static inline int elem_size(int dtype) { return dtype_bytes(dtype); }
// p + elems operand elements of `es` bytes (2: bf16 / fp16, 4: the fp32 verification mode)
static inline void* offset_t(void* p, size_t elems, int es = 2) { return (void*)((char*)p + elems * es); }
static inline const void* offset_t(const void* p, size_t elems, int es = 2) { return (const void*)((const char*)p + elems * es); }
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace tt
