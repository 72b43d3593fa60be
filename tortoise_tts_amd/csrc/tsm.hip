// WSOLA time-scale modification (include/tortoise_mi355x_tsm.h): the same speech, faster or slower, at the same pitch.
//
//   tsm_stretch_kernel   ONE WORKGROUP PER CLIP (blockIdx.x = clip), 256 threads, the frames in sequence: frame k's template is what
//                        follows frame k - 1's choice, so the chain is a latency chain and a clip has no parallelism beyond one frame's search.
//     region             the nominal position a_k does not depend on the path: the 1663 samples x[a_k - 256 ..) that frame k can touch (512
//                        candidate windows of 768, and the 768 behind any choice + Hs: the NEXT template) are fetched into registers a
//                        frame ahead, while the current frame's search runs, and written to LDS when the search is done.  No global load
//                        sits on the chain.  A region that lies inside the clip - every frame's but the first and the last few - is
//                        fetched from one uniform base without a bounds test per sample (tsm_fetch_inside).
//     template           copied LDS -> LDS from the region at the chosen offset (16-byte aligned again, so its reads are ds_read_b128 broadcasts).
//     search             thread (half, u) owns the adjacent candidates 4u .. 4u + 3 over j in [384 half, 384 half + 384): its region reads
//                        are 16-byte aligned ds_read_b128, consecutive over the lanes (no bank conflict), each value feeds all four
//                        candidates, the template read is a ds_read_b128 broadcast, and the next j's reads are issued before this j's
//                        FMAs (one workgroup per CU: the low-occupancy case).  The region is kept twice, the second copy one sample on:
//                        the window slides by one sample per j, and with both copies every pair of neighbouring values a packed FMA
//                        takes is an aligned register pair of a read (no moves between the reads and the FMAs).  c and E are direct sums, one FMA per term: ascending j within a
//                        half, then lower half + upper half (through LDS).
//     argmax             a packed 64-bit key (order-preserving score bits | tie order), reduced over the wave with shuffles and over the
//                        four waves through LDS.
//     overlap-add        y of hop k - 1 needs frame k - 1 (the template's first half) and frame k (the region at the chosen offset): both
//                        are in LDS; one coalesced store per sample.
//   Nothing a clip computes depends on where it stands in the batch.
//   The steps are csrc/tsm_steps.h's, shared with the chunked kernel of tsm_stream.hip.
#include <math.h>
#include "runtime.h"
#include "tsm_steps.h"

namespace tt {

__global__ __launch_bounds__(kTsmThreads) void tsm_stretch_kernel(const float* __restrict__ audio, const int* __restrict__ in_off,
                                                                  const int* __restrict__ rqs, const float* __restrict__ window, int max_samples,
                                                                  float* __restrict__ out, const int* __restrict__ out_off,
                                                                  int* __restrict__ offsets, const int* __restrict__ frame_off,
                                                                  int* __restrict__ status) {
  TT_TSM_LDS;
  const int c = blockIdx.x, t = threadIdx.x, u = t & (kTsmThreads / 2 - 1), half = t / (kTsmThreads / 2);
  const int i0 = in_off[c], n = in_off[c + 1] - i0, rq = rqs[c];
  const int o0 = out_off[c], f0 = frame_off[c];
  // (every test below is uniform over the workgroup)
  if (i0 < 0 || n < 0) {
    if (t == 0) status[c] = TT_TSM_REFUSED;
    return;
  }
  if (n == 0) {
    if (t == 0) status[c] = TT_TSM_EMPTY;
    return;
  }
  if (n > max_samples || !tsm_rate_ok(rq)) {
    if (t == 0) status[c] = TT_TSM_REFUSED;
    return;
  }
  const int n_out = tsm_out_samples(n, rq), K = tsm_frames(n_out);
  if (o0 < 0 || f0 < 0 || out_off[c + 1] - o0 != n_out || frame_off[c + 1] - f0 != K) {  // nothing is written outside the clip's own slices
    if (t == 0) status[c] = TT_TSM_REFUSED;
    return;
  }
  const float* x = audio + i0;
  auto sample = [&](int i) { return i >= 0 && i < n ? x[i] : 0.f; };
  float* y = out + o0;
  int* off = offsets + f0;
  const TsmWin w = tsm_window(window, t);
  // frame 0 sits at p_0 = -Hs: frame 1's template is x[0 .. W)
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = sample(e * kTsmThreads + t);
  if (t == 0) off[0] = 0;
  float pre[kTsmPre];
  auto fetch = [&](int k) {
    const int base = tsm_nominal(k, rq) - kTsmS;
    if (base >= 0 && base + kTsmRegion <= n)  // (uniform over the workgroup) all but the first and the last few frames of a clip
      tsm_fetch_inside(pre, x + base, t);
    else
      tsm_fetch(pre, k, rq, t, sample);
  };
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
  if (t == 0) status[c] = TT_TSM_OK;
}

}  // namespace tt

using namespace tt;

struct tt_tsm : EngineHandle {
  int max_samples = 0, max_clips = 0;
  float* window = nullptr;  // [W] the periodic Hann window, fp64 values rounded to f32
};

extern "C" {

int tt_tsm_abi_version(void) { return 1; }  // ABI changes

int tt_tsm_out_samples(int n, int rq) { return n >= 1 && n <= TT_TSM_MAX_SAMPLES && tsm_rate_ok(rq) ? tsm_out_samples(n, rq) : 0; }

int tt_tsm_frames(int n, int rq) { return n >= 1 && n <= TT_TSM_MAX_SAMPLES && tsm_rate_ok(rq) ? tsm_frames(tsm_out_samples(n, rq)) : 0; }

int tt_tsm_create(int max_samples, int max_clips, tt_tsm** out) {
  TT_REQUIRE(out, "tt_tsm_create: null argument");
  TT_REQUIRE(max_samples >= 1 && max_samples <= TT_TSM_MAX_SAMPLES, "tt_tsm_create: max_samples %d (1 .. %d)", max_samples, TT_TSM_MAX_SAMPLES);
  TT_REQUIRE(max_clips >= 1 && max_clips <= TT_TSM_MAX_CLIPS, "tt_tsm_create: max_clips %d (1 .. %d)", max_clips, TT_TSM_MAX_CLIPS);
  tt_tsm* e = new tt_tsm();
  e->max_samples = max_samples; e->max_clips = max_clips;
  int rc = e->open("tt_tsm_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->window, kTsmW, false);
  if (!rc) {
    float w[kTsmW];
    for (int j = 0; j < kTsmW; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)kTsmW));
    if (hipMemcpy(e->window, w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("tt_tsm_create: the window upload failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_tsm_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_tsm_destroy(tt_tsm* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_tsm_stretch(tt_tsm* e, int n_clips, const float* audio, const int* in_off, const int* rq, float* out, const int* out_off, int* offsets,
                   const int* frame_off, int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && rq && out && out_off && offsets && frame_off && status, "tt_tsm_stretch: null argument");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_tsm_stretch: %d clips (1 .. %d)", n_clips, e->max_clips);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    tsm_stretch_kernel<<<n_clips, kTsmThreads, 0, s>>>(audio, in_off, rq, e->window, e->max_samples, out, out_off, offsets, frame_off, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
