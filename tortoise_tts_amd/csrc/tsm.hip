// WSOLA time-scale modification (include/tortoise_mi355x_tsm.h): the same speech, faster or slower, at the same pitch.
//
//   tsm_stretch_kernel   ONE WORKGROUP PER CLIP (blockIdx.x = clip), 256 threads, the frames in sequence: frame k's template is what
//                        follows frame k - 1's choice, so the chain is a latency chain and a clip has no parallelism beyond one frame's search.
//     region             the nominal position a_k does not depend on the path: the 1663 samples x[a_k - 256 ..) that frame k can touch (512
//                        candidate windows of 768, and the 768 behind any choice + Hs: the NEXT template) are fetched into registers a
//                        frame ahead, while the current frame's search runs, and written to LDS when the search is done.  No global load
//                        sits on the chain.
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
#include <math.h>
#include "runtime.h"
#include "../../include/tortoise_mi355x_tsm.h"

namespace tt {

constexpr int kTsmW = TT_TSM_WINDOW, kTsmHs = TT_TSM_HOP, kTsmS = TT_TSM_SEARCH;
constexpr int kTsmThreads = 256;                           // 128 x four candidates, x the two halves of j
constexpr int kTsmRegion = 2 * kTsmS - 1 + kTsmHs + kTsmW;  // 1663 samples from a_k - kTsmS
constexpr int kTsmRegionPad = 1664;
constexpr int kTsmPre = (kTsmRegion + kTsmThreads - 1) / kTsmThreads;  // region samples a thread holds of the next frame (7)
static_assert(4 * (kTsmThreads / 2) == 2 * kTsmS && kTsmW == 2 * kTsmHs && kTsmW % 8 == 0 && kTsmW == 3 * kTsmThreads, "tsm_stretch_kernel's thread mapping");

typedef float tsm_f2 __attribute__((ext_vector_type(2)));  // (8- and 16-byte aligned: ds_read_b64 / ds_read_b128)
typedef float tsm_f4 __attribute__((ext_vector_type(4)));

__host__ __device__ static inline bool tsm_rate_ok(int rq) { return rq >= TT_TSM_RATE_MIN && rq <= TT_TSM_RATE_MAX; }
__host__ __device__ static inline int tsm_out_samples(int n, int rq) {
  const long long v = ((long long)n * TT_TSM_RATE_ONE + rq / 2) / rq;
  return v < 1 ? 1 : (int)v;
}
__host__ __device__ static inline int tsm_frames(int n_out) { return (n_out + kTsmHs - 1) / kTsmHs + 1; }
__host__ __device__ static inline int tsm_nominal(int k, int rq) { return (int)(((long long)(k - 1) * kTsmHs * rq + 32768) >> 16); }

// (score, tie order) as one unsigned key: a greater score wins; among equal scores the smaller |d|, and of +-d the negative one
__device__ __forceinline__ unsigned long long tsm_key(float s, int cand) {
  s += 0.f;  // (-0 -> +0: equal scores have equal bits)
  unsigned u = __float_as_uint(s);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  const int d = cand - kTsmS;
  const unsigned pos = d < 0 ? (unsigned)(-2 * d - 1) : (unsigned)(2 * d);  // 0, -1, 1, -2, 2, ... -> 0, 1, 2, 3, 4, ...
  return ((unsigned long long)u << 32) | (unsigned)(2 * kTsmS - 1 - pos);
}
__device__ __forceinline__ int tsm_key_cand(unsigned long long key) {
  const int pos = 2 * kTsmS - 1 - (int)(key & (2 * kTsmS - 1));
  return kTsmS + ((pos & 1) ? -((pos + 1) >> 1) : (pos >> 1));
}

__global__ __launch_bounds__(kTsmThreads) void tsm_stretch_kernel(const float* __restrict__ audio, const int* __restrict__ in_off,
                                                                  const int* __restrict__ rqs, const float* __restrict__ window, int max_samples,
                                                                  float* __restrict__ out, const int* __restrict__ out_off,
                                                                  int* __restrict__ offsets, const int* __restrict__ frame_off,
                                                                  int* __restrict__ status) {
  __shared__ __align__(16) float reg_s[kTsmRegionPad];
  __shared__ __align__(16) float sh_s[kTsmRegionPad];  // reg_s one sample on: sh_s[i] = reg_s[i + 1]
  __shared__ __align__(16) float tpl_s[kTsmW];
  __shared__ float part_s[8 * kTsmThreads / 2];  // c and E of the upper half of j, [4 + 4][128]
  __shared__ unsigned long long best_s[kTsmThreads / 64];
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
  // the window values of this thread's output samples t and t + 256 of every hop: first half (the entering frame), second half (the leaving one)
  const bool two = t + kTsmThreads < kTsmHs;
  const float w_in0 = window[t], w_out0 = window[t + kTsmHs];
  const float w_in1 = two ? window[t + kTsmThreads] : 0.f, w_out1 = two ? window[t + kTsmThreads + kTsmHs] : 0.f;
  // frame 0 sits at p_0 = -Hs: frame 1's template is x[0 .. W)
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = sample(e * kTsmThreads + t);
  if (t == 0) off[0] = 0;
  float pre[kTsmPre];
  auto fetch = [&](int k) {
    const int base = tsm_nominal(k, rq) - kTsmS;
#pragma unroll
    for (int e = 0; e < kTsmPre; ++e) {
      const int i = e * kTsmThreads + t;
      pre[e] = i < kTsmRegion ? sample(base + i) : 0.f;
    }
  };
  fetch(1);
  for (int k = 1; k < K; ++k) {
    // (the previous frame's reads of reg_s ended before its last barrier)
#pragma unroll
    for (int e = 0; e < kTsmPre; ++e) {
      const int i = e * kTsmThreads + t;
      if (i < kTsmRegionPad) reg_s[i] = pre[e];
      if (i >= 1 && i < kTsmRegionPad) sh_s[i - 1] = pre[e];
    }
    if (k + 1 < K) fetch(k + 1);  // in flight while this frame is searched
    __syncthreads();
    // candidates 4u .. 4u + 3 over this thread's half of j: the window reg_s[4u + j ..] is 16-byte aligned for every j = 0 mod 4
    const tsm_f4* r4 = (const tsm_f4*)reg_s + u + half * (kTsmW / 8);
    const tsm_f4* s4 = (const tsm_f4*)sh_s + u + half * (kTsmW / 8);
    const tsm_f4* t4 = (const tsm_f4*)tpl_s + half * (kTsmW / 8);
    tsm_f2 c01 = {0.f, 0.f}, c23 = {0.f, 0.f}, e01 = {0.f, 0.f}, e23 = {0.f, 0.f};  // (c, E) of candidates 4u + (0, 1) and 4u + (2, 3)
    auto step = [&](float tj, tsm_f2 a, tsm_f2 b) {  // one j: the window values of candidates (0, 1) and (2, 3), register pairs as read
      c01 = __builtin_elementwise_fma(tsm_f2{tj, tj}, a, c01);
      c23 = __builtin_elementwise_fma(tsm_f2{tj, tj}, b, c23);
      e01 = __builtin_elementwise_fma(a, a, e01);
      e23 = __builtin_elementwise_fma(b, b, e23);
    };
    // x0 = region[4u + j .. + 3], x1 = the same one sample on (the shifted copy): every pair a step needs is an aligned half of a read
    tsm_f4 tv = t4[0], x0 = r4[0], x1 = s4[0];
#pragma unroll 4
    for (int q = 0; q < kTsmW / 8; ++q) {
      const tsm_f4 y0 = r4[q + 1], y1 = s4[q + 1], tn = t4[q + 1 < kTsmW / 8 ? q + 1 : q];  // the next j's reads, in flight over this j's FMAs
      step(tv.x, x0.xy, x0.zw);  // ascending j
      step(tv.y, x1.xy, x1.zw);
      step(tv.z, x0.zw, y0.xy);
      step(tv.w, x1.zw, y1.xy);
      tv = tn; x0 = y0; x1 = y1;
    }
    const float cc[4] = {c01.x, c01.y, c23.x, c23.y}, ee[4] = {e01.x, e01.y, e23.x, e23.y};
    if (half) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        part_s[g * kTsmThreads / 2 + u] = cc[g];
        part_s[(4 + g) * kTsmThreads / 2 + u] = ee[g];
      }
    }
    __syncthreads();
    unsigned long long key = 0;  // (below every candidate's key)
    if (!half) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float cg = cc[g] + part_s[g * kTsmThreads / 2 + u], eg = ee[g] + part_s[(4 + g) * kTsmThreads / 2 + u];
        const unsigned long long kg = tsm_key(cg / sqrtf(eg + 1e-20f), 4 * u + g);
        key = kg > key ? kg : key;
      }
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(key, m);
      key = o > key ? o : key;
    }
    if ((t & 63) == 0) best_s[t >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < kTsmThreads / 64; ++wv) key = best_s[wv] > key ? best_s[wv] : key;
    const int cs = tsm_key_cand(key);  // 0 .. 511, the same in every thread
    // hop k - 1 of the output: frame k - 1 leaves (the template's first half), frame k enters (the region at the chosen offset)
    const int m0 = (k - 1) * kTsmHs + t;
    if (m0 < n_out) y[m0] = fmaf(w_in0, reg_s[cs + t], w_out0 * tpl_s[t]);
    if (two && m0 + kTsmThreads < n_out) y[m0 + kTsmThreads] = fmaf(w_in1, reg_s[cs + t + kTsmThreads], w_out1 * tpl_s[t + kTsmThreads]);
    if (t == 0) off[k] = cs - kTsmS;
    // the next template: what follows this frame's choice, x[p_k + Hs + j]
    float nt[kTsmW / kTsmThreads];
#pragma unroll
    for (int e = 0; e < kTsmW / kTsmThreads; ++e) nt[e] = reg_s[cs + kTsmHs + e * kTsmThreads + t];
    __syncthreads();  // every read of tpl_s, reg_s and best_s of this frame is done
#pragma unroll
    for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = nt[e];
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
