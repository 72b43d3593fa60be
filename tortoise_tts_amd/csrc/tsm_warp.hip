// WSOLA along a rate map (include/tortoise_mi355x_tsw.h): the time-stretch of tsm.hip with a speaking rate that changes inside the clip.
//
//   tsw_stretch_kernel   ONE WORKGROUP PER CLIP (blockIdx.x = clip), 256 threads, the frames in sequence - tsm_stretch_kernel with one
//                        difference: the nominal position a_k comes from the clip's table of segments instead of one rate.  a_k still does
//                        not depend on the path, so the region is fetched a frame ahead as before, and every step is csrc/tsm_steps.h's:
//                        the table (0, 0, rq) gives tsm_stretch_kernel's bits.
//     table              copied to LDS (at most 64 x 3 integers) and checked there by every thread alike (tsw_out_samples of
//                        tsm_warp_host.h, the code the host plans with) before anything is written.
//     cursor             the current segment (m_i, a_i, rq_i) and the next border m_(i+1) live in uniform values (readfirstlane of the
//                        LDS reads: scalar registers).  The frames' outputs (k - 1) Hs increase, so the cursor only moves forward; it
//                        is advanced inside the one-frame-ahead prefetch, where tsm_stretch_kernel calls tsm_nominal.  A frame that
//                        crosses no border - all but S - 1 of a clip - costs one scalar compare more than a constant rate; a crossing
//                        reads three LDS words, ahead of the barrier that waits for LDS anyway.  Nothing new sits on the frame chain.
//   Nothing a clip computes depends on where it stands in the batch.
#include <limits.h>
#include <math.h>
#include "runtime.h"
#include "tsm_steps.h"
#include "tsm_warp_host.h"

namespace tt {

// Code placement.  The search loop of tsm_search is 708 bytes of 8-byte instructions (v_pk_fma_f32, ds_read_b128) with one wave per SIMD
// and nothing to hide an instruction fetch behind.  As first built its head stood at an address = 4 mod 8 and the kernel ran 4.7 .. 5.4 %
// slower per frame than tsm_stretch_kernel (head = 0 mod 8) with the same instructions in the frame loop, the search loop's in the
// same order (profiles/r24_tsmap.txt).  One 4-byte s_nop ahead of the frame loop, executed once per clip, moves the head to 0 mod 8.  This
// depends on the compiler's layout: after a change of the kernel or the toolchain, look at the loop head's address again.
#ifndef TT_TSW_PLACE
#define TT_TSW_PLACE asm volatile("s_nop 0")
#endif

__global__ __launch_bounds__(kTsmThreads) void tsw_stretch_kernel(const float* __restrict__ audio, const int* __restrict__ in_off,
                                                                  const int* __restrict__ seg, const int* __restrict__ seg_off,
                                                                  const float* __restrict__ window, int max_samples, int max_segments,
                                                                  float* __restrict__ out, const int* __restrict__ out_off,
                                                                  int* __restrict__ offsets, const int* __restrict__ frame_off,
                                                                  int* __restrict__ status) {
  TT_TSM_LDS;
  __shared__ int tab_s[3 * TT_TSW_MAX_SEGMENTS];
  const int c = blockIdx.x, t = threadIdx.x, u = t & (kTsmThreads / 2 - 1), half = t / (kTsmThreads / 2);
  const int i0 = in_off[c], n = in_off[c + 1] - i0;
  const int s0 = seg_off[c], S = seg_off[c + 1] - s0;
  const int o0 = out_off[c], f0 = frame_off[c];
  // (every test below is uniform over the workgroup)
  if (i0 < 0 || n < 0) {
    if (t == 0) status[c] = TT_TSW_REFUSED;
    return;
  }
  if (n == 0) {
    if (t == 0) status[c] = TT_TSW_EMPTY;
    return;
  }
  if (n > max_samples || s0 < 0 || S < 1 || S > max_segments) {
    if (t == 0) status[c] = TT_TSW_REFUSED;
    return;
  }
  if (t < 3 * S) tab_s[t] = seg[3 * (long long)s0 + t];  // (3 S <= 192 < the 256 threads)
  __syncthreads();
  const int n_out = tsw_out_samples(n, S, tab_s);  // 0: the table breaks a rule
  if (n_out == 0 || o0 < 0 || f0 < 0 || out_off[c + 1] - o0 != n_out || frame_off[c + 1] - f0 != tsm_frames(n_out)) {  // nothing is written outside the clip's own slices
    if (t == 0) status[c] = TT_TSW_REFUSED;
    return;
  }
  const int K = tsm_frames(n_out);
  const float* x = audio + i0;
  auto sample = [&](int i) { return i >= 0 && i < n ? x[i] : 0.f; };
  float* y = out + o0;
  int* off = offsets + f0;
  const TsmWin w = tsm_window(window, t);
  // frame 0 sits at p_0 = -Hs: frame 1's template is x[0 .. W)
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = sample(e * kTsmThreads + t);
  if (t == 0) off[0] = 0;
  // the cursor: segment `cur` = (cm, ca, crq), the next border at output sample nm (none: INT_MAX)
  auto entry = [&](int i) { return __builtin_amdgcn_readfirstlane(tab_s[i]); };
  int cur = 0, cm = 0, ca = 0, crq = entry(2), nm = S > 1 ? entry(3) : INT_MAX;
  float pre[kTsmPre];
  auto fetch = [&](int k) {
    const int m = (k - 1) * kTsmHs;
    while (m >= nm) {  // (uniform; a segment shorter than a hop is passed over)
      ++cur;
      cm = nm; ca = entry(3 * cur + 1); crq = entry(3 * cur + 2);
      nm = cur + 1 < S ? entry(3 * cur + 3) : INT_MAX;
    }
    const int base = tsw_position(m, cm, ca, crq) - kTsmS;
    if (base >= 0 && base + kTsmRegion <= n)  // (uniform over the workgroup) all but the first and the last few frames of a clip
      tsm_fetch_inside(pre, x + base, t);
    else
      tsm_fetch_at(pre, base, t, sample);
  };
  TT_TSW_PLACE;
  fetch(1);
  for (int k = 1; k < K; ++k) {
    tsm_store_region(reg_s, sh_s, pre, t);
    if (k + 1 < K) fetch(k + 1);  // in flight while this frame is searched
    __syncthreads();
    float cc[4], ee[4];
    tsm_search(reg_s, sh_s, tpl_s, u, half, cc, ee);
    const int cs = tsm_argmax(cc, ee, part_s, best_s, t, u, half);
    // hop k - 1 of the output
    tsm_overlap_add(w, reg_s, tpl_s, cs, t, y, (k - 1) * kTsmHs + t, n_out);
    if (t == 0) off[k] = cs - kTsmS;
    tsm_next_template(reg_s, tpl_s, cs, t);
  }
  if (t == 0) status[c] = TT_TSW_OK;
}

}  // namespace tt

using namespace tt;

struct tt_tsw : EngineHandle {
  int max_samples = 0, max_clips = 0, max_segments = 0;
  float* window = nullptr;  // [W] the periodic Hann window, fp64 values rounded to f32 (tt_tsm_create's)
};

extern "C" {

int tt_tsw_abi_version(void) { return 1; }  // ABI changes

int tt_tsw_plan(int n, int n_segments, const int* starts, const int* rqs, int* table_out) {
  char err[256];
  if (tsw_plan(n, n_segments, starts, rqs, table_out, err, sizeof(err)) != 0) {
    set_error("%s", err);
    return -1;
  }
  return 0;
}

int tt_tsw_out_samples(int n, int n_segments, const int* table) { return table ? tsw_out_samples(n, n_segments, table) : 0; }

int tt_tsw_frames(int n, int n_segments, const int* table) { return table ? tsw_frames(n, n_segments, table) : 0; }

int tt_tsw_create(int max_samples, int max_clips, int max_segments, tt_tsw** out) {
  char err[256];
  TT_REQUIRE(out, "tt_tsw_create: null argument");
  TT_REQUIRE(tsw_check_create(max_samples, max_clips, max_segments, err, sizeof(err)) == 0, "%s", err);
  tt_tsw* e = new tt_tsw();
  e->max_samples = max_samples; e->max_clips = max_clips; e->max_segments = max_segments;
  int rc = e->open("tt_tsw_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->window, kTsmW, false);
  if (!rc) {
    float w[kTsmW];
    for (int j = 0; j < kTsmW; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)kTsmW));
    if (hipMemcpy(e->window, w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("tt_tsw_create: the window upload failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_tsw_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_tsw_destroy(tt_tsw* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_tsw_stretch(tt_tsw* e, int n_clips, const float* audio, const int* in_off, const int* seg, const int* seg_off, float* out,
                   const int* out_off, int* offsets, const int* frame_off, int* status, void* stream) {
  char err[256];
  TT_REQUIRE(tsw_check_stretch(e && audio && in_off && seg && seg_off && out && out_off && offsets && frame_off && status, n_clips,
                               e ? e->max_clips : 0, err, sizeof(err)) == 0, "%s", err);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    tsw_stretch_kernel<<<n_clips, kTsmThreads, 0, s>>>(audio, in_off, seg, seg_off, e->window, e->max_samples, e->max_segments, out, out_off,
                                                       offsets, frame_off, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
