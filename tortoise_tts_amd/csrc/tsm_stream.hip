// The time-stretch fed in chunks (include/tortoise_mi355x_tss.h): a stream at another speaking rate, bit for bit the whole-clip result of
// tsm.hip.  The counters and every argument check are host code (tsm_stream_host.h); a push hands the kernel one TssItem per pushed slot BY
// VALUE (no upload, no copy back) and is ONE launch.
//
//   tss_push_kernel      ONE WORKGROUP PER PUSHED SLOT (blockIdx.x = item), 256 threads, running the frames k0 .. k1 the push completes in
//                        sequence with the steps of tsm_steps.h: tsm_stretch_kernel's chain, so its bits.
//     position           position j of the stream comes from the slot's history for j < n_prev, from the chunk up to n_end, and is 0 before
//                        sample 0 and from n_end on.  Only a flush has frames that reach n_end: before one the host schedules frame k only
//                        when a_k + 1407 <= n_end (tsm_frames_done).  This reader is the one difference to tsm_stretch_kernel.
//     region             fetched into registers a frame ahead, as in tsm_stretch_kernel: no global load sits on the chain.
//     template           read from the slot at entry and written back at exit by the same thread for the same elements (no barrier
//                        needed); at frame 1 it is x[0 .. 768) = the region at 256, taken from the registers frame 1's region was
//                        fetched into.
//     history            two copies and a parity, as tt_rss has them: the workgroup reads the current copy (positions n_prev - 1664 ..
//                        n_prev - 1) and the chunk and writes the OTHER copy (n_end - 1664 .. n_end - 1) before its frames.  Nothing in
//                        this launch reads the copy being written - the slot has one workgroup and no other slot's workgroup touches it -
//                        and the next push is ordered behind this one on the handle's stream and reads that copy.  In place behind a
//                        barrier would save 6.5 KB per slot and cost a drained barrier in front of the frames, with the prefetch of frame
//                        k0 either held in registers across it or issued late; the copies cost nothing on the chain.
//     no frame           a push that completes no frame (k1 < k0) still advances the history.
//   Nothing a slot computes depends on which other slots are pushed with it.
#include <vector>
#include "runtime.h"
#include "tsm_stream_host.h"

namespace tt {

struct TssArgs {
  int n;
  TssItem it[TT_TSS_MAX_STREAMS];
};
static_assert(sizeof(TssArgs) + 7 * sizeof(void*) <= 4096, "the items travel as kernel arguments");

__global__ __launch_bounds__(kTsmThreads) void tss_push_kernel(TssArgs a, const float* __restrict__ audio, const float* __restrict__ window,
                                                               float* __restrict__ hist_all, float* __restrict__ tpl_all,
                                                               float* __restrict__ out, int* __restrict__ offsets,
                                                               const float* __restrict__ zero) {
  TT_TSM_LDS;
  if ((int)blockIdx.x >= a.n) return;  // (uniform over the workgroup)
  const TssItem it = a.it[blockIdx.x];
  const int t = threadIdx.x, u = t & (kTsmThreads / 2 - 1), half = t / (kTsmThreads / 2);
  const float* chunk = audio + it.in_off;
  const float* hist = hist_all + ((size_t)it.slot * 2 + it.parity) * TT_TSS_HIST;
  const int n_prev = it.n_prev, n_end = it.n_end, rq = it.rq;
  // One unconditional load: a position that reads 0 is loaded from `zero`, a device float that holds 0.  With a branch per case, or a
  // select behind the load, the compiler waits for each load where it is issued, and the prefetch of the next frame's region would sit
  // on the chain.
  auto sample = [&](int j) {
    const int e = j - n_prev + TT_TSS_HIST;  // (e < 0 is beyond the next frame's reach: tsm_stream_host.h, tortoise_mi355x_tss.h)
    const float* p = j >= n_prev ? chunk + (j - n_prev) : hist + e;
    return *(j >= 0 && j < n_end && e >= 0 ? p : zero);
  };
  {  // the history after this push, into the other copy
    float* next = hist_all + ((size_t)it.slot * 2 + (it.parity ^ 1)) * TT_TSS_HIST;
    float h[kTsmPre];  // (all loads in flight before the first store)
#pragma unroll
    for (int r = 0; r < kTsmPre; ++r) h[r] = sample(n_end - TT_TSS_HIST + min(r * kTsmThreads + t, TT_TSS_HIST - 1));
#pragma unroll
    for (int r = 0; r < kTsmPre; ++r)
      if (r * kTsmThreads + t < TT_TSS_HIST) next[r * kTsmThreads + t] = h[r];
  }
  const int k0 = it.k0, k1 = it.k1;
  if (k1 < k0) return;  // the push completes no frame
  float* tpl_g = tpl_all + (size_t)it.slot * kTsmW;
  float* y = out + it.out_off;
  const int limit = it.m1 - it.m0;  // outputs of this push: the hops of its frames, cut at n_out on a flush
  const int off0 = it.off_off + (k0 == 1) - k0;  // frame k's entry is offsets[off0 + k]: d_0 comes first in the push that runs frame 1
  const TsmWin w = tsm_window(window, t);
  // a frame whose whole region lies in the chunk - all but the first few of a piece-sized push - reads it as the whole-clip kernel reads the
  // inside of a clip, from one uniform base; the others take the reader above (some 25 address instructions more per load, which the chain
  // pays for: about 0.8 us per frame when every frame took it)
  auto fetch = [&](float (&pre)[kTsmPre], int k) {
    const int base = tsm_nominal(k, rq) - kTsmS;
    if (base >= n_prev && base + kTsmRegion <= n_end) {  // (uniform over the workgroup)
      tsm_fetch_inside(pre, chunk + (base - n_prev), t);
    } else {
      tsm_fetch(pre, k, rq, t, sample);
    }
  };
  float pre[kTsmPre];
  fetch(pre, k0);
  if (k0 == 1) {
    // frame 0 sits at p_0 = -Hs: frame 1's template is x[0 .. W), the region of frame 1 (from -256) at 256 .. 1023
#pragma unroll
    for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = pre[e + kTsmS / kTsmThreads];
    if (t == 0 && offsets) offsets[it.off_off] = 0;
  } else {
#pragma unroll
    for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = tpl_g[e * kTsmThreads + t];
  }
  for (int k = k0; k <= k1; ++k) {
    tsm_store_region(reg_s, sh_s, pre, t);
    if (k + 1 <= k1) fetch(pre, k + 1);  // in flight while this frame is searched
    __syncthreads();
    float cc[4], ee[4];
    tsm_search(reg_s, sh_s, tpl_s, u, half, cc, ee);
    const int cs = tsm_argmax(cc, ee, part_s, best_s, t, u, half);
    // hop k - 1 of the output
    tsm_overlap_add(w, reg_s, tpl_s, cs, t, y, (k - k0) * kTsmHs + t, limit);
    if (t == 0 && offsets) offsets[off0 + k] = cs - kTsmS;
    tsm_next_template(reg_s, tpl_s, cs, t);
  }
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_g[e * kTsmThreads + t] = tpl_s[e * kTsmThreads + t];  // (this thread wrote them)
}

}  // namespace tt

using namespace tt;

static_assert(kTsmS % kTsmThreads == 0 && kTsmPre * kTsmThreads >= TT_TSS_HIST, "frame 1's template starts at a whole register of the region; the history copy");

struct tt_tss : EngineHandle {
  TssBook book;
  float* window = nullptr;  // [W] the periodic Hann window, as tt_tsm has it
  float* hist = nullptr;    // [max_streams][2][TT_TSS_HIST]
  float* tpl = nullptr;     // [max_streams][W]
  float* zero = nullptr;    // [1] 0.f: what a position outside the stream reads
};

extern "C" {

int tt_tss_abi_version(void) { return 1; }  // ABI changes

int tt_tss_frames_done(int n, int rq) { return tss_count_ok(n, 0, rq) ? tsm_frames_done(n, rq) : -1; }

int tt_tss_ready(int n_before, int n_chunk, int rq, int flush) { return tss_ready(n_before, n_chunk, rq, flush); }

int tt_tss_create(int max_streams, tt_tss** out) {
  TT_REQUIRE(out, "tt_tss_create: null argument");
  TT_REQUIRE(max_streams >= 1 && max_streams <= TT_TSS_MAX_STREAMS, "tt_tss_create: max_streams %d (1 .. %d)", max_streams, TT_TSS_MAX_STREAMS);
  tt_tss* e = new tt_tss();
  e->book.init(max_streams);
  int rc = e->open("tt_tss_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->window, kTsmW, false);
  if (!rc) rc = e->arena.alloc_t(&e->hist, (size_t)max_streams * 2 * TT_TSS_HIST, true);
  if (!rc) rc = e->arena.alloc_t(&e->tpl, (size_t)max_streams * kTsmW, true);
  if (!rc) rc = e->arena.alloc_t(&e->zero, 1, true);
  if (!rc) {
    float w[kTsmW];
    for (int j = 0; j < kTsmW; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)kTsmW));  // tt_tsm_create's
    if (hipMemcpy(e->window, w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("tt_tss_create: the window upload failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_tss_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_tss_destroy(tt_tss* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_tss_open(tt_tss* e, int slot, int rq) {
  TT_REQUIRE(e, "tt_tss_open: null argument");
  char err[256];
  if (e->book.check_open(slot, rq, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  e->book.commit_open(slot, rq);
  return 0;
}

int tt_tss_close(tt_tss* e, int slot) {
  TT_REQUIRE(e, "tt_tss_close: null argument");
  char err[256];
  if (e->book.close(slot, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  return 0;
}

int tt_tss_state(tt_tss* e, int slot, int* n_in, int* m_out, int* frames, int* finished) {
  TT_REQUIRE(e, "tt_tss_state: null argument");
  TT_REQUIRE(slot >= 0 && slot < e->book.max_streams(), "tt_tss_state: slot %d (0 .. %d)", slot, e->book.max_streams() - 1);
  const TssSlot& s = e->book.slots[(size_t)slot];
  TT_REQUIRE(s.state != kTssClosed, "tt_tss_state: slot %d is closed", slot);
  if (n_in) *n_in = s.n_in;
  if (m_out) *m_out = s.m_out;
  if (frames) *frames = s.frames;
  if (finished) *finished = s.state == kTssFinished;
  return 0;
}

int tt_tss_push(tt_tss* e, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, int* offsets,
                void* stream) {
  TT_REQUIRE(e && audio && out, "tt_tss_push: null argument");
  char err[256];
  std::vector<TssItem> items;
  if (e->book.plan(n_push, slots, n_chunk, flush, &items, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  TssArgs a;
  a.n = n_push;
  for (int i = 0; i < n_push; ++i) a.it[i] = items[(size_t)i];
  const int rc = e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    tss_push_kernel<<<n_push, kTsmThreads, 0, s>>>(a, audio, e->window, e->hist, e->tpl, out, offsets, e->zero);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  e->book.commit(items, flush);
  return 0;
}

}  // extern "C"
