// The steps the WSOLA kernels share (include/tortoise_mi355x_tsm.h, include/tortoise_mi355x_tss.h): the integers of a rate, and one frame's
// region store, search, argmax, overlap-add and template copy.  tsm.hip (whole clips) and tsm_stream.hip (streams) are built from these and
// differ only in how a position of the input is read, so their arithmetic cannot drift: a streamed sample is the whole-clip sample to the bit.
//
// The integer part (everything above `#ifdef __HIPCC__`) is plain C++ as well: the streaming bookkeeping (tsm_stream_host.h) and its
// stand-alone check compile it without the device toolchain.
//
// Why WSOLA streams exactly.  The clip's length n enters the whole-clip kernel in n_out, in K and in the zeros read at and beyond n; nothing
// else.  Frame k >= 1 reads its region x[a_k - S .. a_k - S + kTsmRegion) = x[a_k - 256 .. a_k + 1407) and the template the previous frame
// left, and a_k does not depend on the path.  So frame k is what the whole-clip kernel computes as soon as a_k + kTsmLook <= (inputs so far),
// whatever follows; the frames of a stream are a prefix of the clip's frames (tsm_frames_done) until the flush runs the rest against zeros.
#pragma once
#include <math.h>
#include "../../include/tortoise_mi355x_tsm.h"

#ifdef __HIPCC__
#define TT_TSM_HD __host__ __device__
#else
#define TT_TSM_HD
#endif

namespace tt {

constexpr int kTsmW = TT_TSM_WINDOW, kTsmHs = TT_TSM_HOP, kTsmS = TT_TSM_SEARCH;
constexpr int kTsmThreads = 256;                           // 128 x four candidates, x the two halves of j
constexpr int kTsmRegion = 2 * kTsmS - 1 + kTsmHs + kTsmW;  // 1663 samples from a_k - kTsmS
constexpr int kTsmRegionPad = 1664;
constexpr int kTsmLook = kTsmRegion - kTsmS;                // 1407: frame k reads x[.. a_k + kTsmLook)
constexpr int kTsmPre = (kTsmRegion + kTsmThreads - 1) / kTsmThreads;  // region samples a thread holds of the next frame (7)
static_assert(4 * (kTsmThreads / 2) == 2 * kTsmS && kTsmW == 2 * kTsmHs && kTsmW % 8 == 0 && kTsmW == 3 * kTsmThreads, "the kernels' thread mapping");
static_assert(kTsmLook == 1407 && kTsmS + kTsmW <= kTsmRegion, "the look-ahead the headers name; frame 1's template x[0 .. W) lies in its region");

TT_TSM_HD static inline bool tsm_rate_ok(int rq) { return rq >= TT_TSM_RATE_MIN && rq <= TT_TSM_RATE_MAX; }
TT_TSM_HD static inline int tsm_out_samples(int n, int rq) {
  const long long v = ((long long)n * TT_TSM_RATE_ONE + rq / 2) / rq;
  return v < 1 ? 1 : (int)v;
}
TT_TSM_HD static inline int tsm_frames(int n_out) { return (n_out + kTsmHs - 1) / kTsmHs + 1; }
TT_TSM_HD static inline int tsm_nominal(int k, int rq) { return (int)(((long long)(k - 1) * kTsmHs * rq + 32768) >> 16); }

// The frames 1 .. done complete once n samples are in: the k >= 1 with a_k + kTsmLook <= n.  a_k does not decrease in k, so they are a
// prefix, and a_k <= A  <=>  (k - 1) Hs rq + 32768 < (A + 1) 65536  <=>  k - 1 <= ((A + 1) 65536 - 32768 - 1) / (Hs rq).
TT_TSM_HD static inline int tsm_frames_done(int n, int rq) {
  if (n < kTsmLook) return 0;
  return (int)(((((long long)n - kTsmLook + 1) << 16) - 32768 - 1) / ((long long)kTsmHs * rq)) + 1;
}

#ifdef __HIPCC__

typedef float tsm_f2 __attribute__((ext_vector_type(2)));  // (8- and 16-byte aligned: ds_read_b64 / ds_read_b128)
typedef float tsm_f4 __attribute__((ext_vector_type(4)));

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

// The LDS of a workgroup that runs frames: the region twice (the second copy one sample on: sh_s[i] = reg_s[i + 1]), the template, c and E
// of the upper half of j ([4 + 4][128]) and the four waves' best keys.
#define TT_TSM_LDS                                         \
  __shared__ __align__(16) float reg_s[kTsmRegionPad];     \
  __shared__ __align__(16) float sh_s[kTsmRegionPad];      \
  __shared__ __align__(16) float tpl_s[kTsmW];             \
  __shared__ float part_s[8 * kTsmThreads / 2];            \
  __shared__ unsigned long long best_s[kTsmThreads / 64]

// the window values of thread t's output samples t and t + 256 of every hop: first half (the entering frame), second half (the leaving one)
struct TsmWin {
  bool two;
  float in0, out0, in1, out1;
};
__device__ __forceinline__ TsmWin tsm_window(const float* __restrict__ window, int t) {
  TsmWin w;
  w.two = t + kTsmThreads < kTsmHs;
  w.in0 = window[t]; w.out0 = window[t + kTsmHs];
  w.in1 = w.two ? window[t + kTsmThreads] : 0.f; w.out1 = w.two ? window[t + kTsmThreads + kTsmHs] : 0.f;
  return w;
}

// region: frame k's 1663 samples x[a_k - S ..) into the thread's registers; `sample(i)` is how the kernel reads position i
template <class Sample>
__device__ __forceinline__ void tsm_fetch(float (&pre)[kTsmPre], int k, int rq, int t, Sample sample) {
  const int base = tsm_nominal(k, rq) - kTsmS;
#pragma unroll
  for (int e = 0; e < kTsmPre; ++e) {
    const int i = e * kTsmThreads + t;
    pre[e] = i < kTsmRegion ? sample(base + i) : 0.f;
  }
}

// region from a base the kernel computed itself (a rate map's nominal position, tsm_warp.hip): the samples x[base ..), read through `sample`
template <class Sample>
__device__ __forceinline__ void tsm_fetch_at(float (&pre)[kTsmPre], int base, int t, Sample sample) {
#pragma unroll
  for (int e = 0; e < kTsmPre; ++e) {
    const int i = e * kTsmThreads + t;
    pre[e] = i < kTsmRegion ? sample(base + i) : 0.f;
  }
}

// region, the common case: the whole region lies inside the input, at p[0 .. kTsmRegion) - one base that is uniform over the workgroup and
// seven plain loads, no bounds test per sample (the tests of tsm_fetch cost the chain some 0.3 us per frame).  The pad entry 1663 repeats
// the last sample instead of holding 0: no step reads it (the search reads reg_s / sh_s below 1280, the overlap-add and the template
// copy reg_s up to 511 + 384 + 767 = 1662).
__device__ __forceinline__ void tsm_fetch_inside(float (&pre)[kTsmPre], const float* p, int t) {
#pragma unroll
  for (int e = 0; e < kTsmPre; ++e) {
    const int i = e * kTsmThreads + t;
    pre[e] = p[i < kTsmRegion ? i : kTsmRegion - 1];
  }
}

// region store: the registers into both copies (the previous frame's reads of reg_s ended before its last barrier)
__device__ __forceinline__ void tsm_store_region(float* reg_s, float* sh_s, const float (&pre)[kTsmPre], int t) {
#pragma unroll
  for (int e = 0; e < kTsmPre; ++e) {
    const int i = e * kTsmThreads + t;
    if (i < kTsmRegionPad) reg_s[i] = pre[e];
    if (i >= 1 && i < kTsmRegionPad) sh_s[i - 1] = pre[e];
  }
}

// search: c and E of candidates 4u .. 4u + 3 over this thread's half of j; the window reg_s[4u + j ..] is 16-byte aligned for every j = 0 mod 4
__device__ __forceinline__ void tsm_search(const float* reg_s, const float* sh_s, const float* tpl_s, int u, int half, float (&cc)[4],
                                           float (&ee)[4]) {
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
  cc[0] = c01.x; cc[1] = c01.y; cc[2] = c23.x; cc[3] = c23.y;
  ee[0] = e01.x; ee[1] = e01.y; ee[2] = e23.x; ee[3] = e23.y;
}

// key and argmax: lower half + upper half of j (through LDS), the score, the best key over the wave (shuffles) and the four waves (LDS)
// -> the chosen candidate 0 .. 511, the same in every thread.  Two barriers.
__device__ __forceinline__ int tsm_argmax(const float (&cc)[4], const float (&ee)[4], float* part_s, unsigned long long* best_s, int t, int u,
                                          int half) {
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
  return tsm_key_cand(key);
}

// overlap-add of one hop: the previous frame leaves (the template's first half), this frame enters (the region at the chosen offset).
// m0 = (the hop's first output) + t as an index into y; outputs at and beyond `limit` are not written.
__device__ __forceinline__ void tsm_overlap_add(const TsmWin& w, const float* reg_s, const float* tpl_s, int cs, int t, float* y, int m0, int limit) {
  if (m0 < limit) y[m0] = fmaf(w.in0, reg_s[cs + t], w.out0 * tpl_s[t]);
  if (w.two && m0 + kTsmThreads < limit) y[m0 + kTsmThreads] = fmaf(w.in1, reg_s[cs + t + kTsmThreads], w.out1 * tpl_s[t + kTsmThreads]);
}

// template copy: what follows this frame's choice, x[p_k + Hs + j], becomes the next frame's template.  One barrier: every read of tpl_s,
// reg_s and best_s of this frame is done before tpl_s changes (and before the next frame's region store).
__device__ __forceinline__ void tsm_next_template(const float* reg_s, float* tpl_s, int cs, int t) {
  float nt[kTsmW / kTsmThreads];
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) nt[e] = reg_s[cs + kTsmHs + e * kTsmThreads + t];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kTsmW / kTsmThreads; ++e) tpl_s[e * kTsmThreads + t] = nt[e];
}

#endif  // __HIPCC__

}  // namespace tt
