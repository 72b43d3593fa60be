// Loudness normalisation and true-peak limiting (include/tortoise_mi355x_loud.h): BS.1770 integrated loudness, a 4x oversampled true peak
// and the gain to a target under a ceiling, for a ragged batch of 24 kHz clips.
//
// The host knows no clip length (every pointer is a device pointer), so every kernel that works below the clip level runs a fixed grid
// over WORK ITEMS: each workgroup counts the items of every clip (at most 64 clips), and takes the items blockIdx.x, + gridDim.x, ...
// An item belongs to one clip and reads nothing but that clip; what a clip computes does not depend on where it stands in the batch.
//
//   loud_begin_kernel    one thread per clip: an EMPTY / REFUSED clip gets its status (and nothing else, here or later); the true peaks
//                        of the others are set to 0 for the atomic maxima below.
//   loud_filter_kernel   item = 64 segments of 150 samples (four hops), one THREAD per segment, 64 threads: the item's samples are loaded
//                        coalesced into LDS (rows of 151 words: the lanes' reads fall into different banks), each thread runs the K-weighting
//                        cascade over its segment in f64.  PASS 0 from a zero state, leaving the four end values; PASS 1 from the true
//                        state, accumulating y^2.  The dependent chain is one fma per section and sample: 150 samples a thread.
//   loud_carry_kernel    one wave per clip: state' = M state + end values, segment after segment (the only sequential part: 16 fma per 150
//                        samples), 64 segments' end values at a time through LDS; the states overwrite the end values in place.
//   loud_peak_kernel     item = 2400 samples, 256 threads: three 16-tap phases per sample out of LDS, a wave and workgroup maximum, one
//                        atomicMax on the bits of the clip's (non-negative) f32 peak - a maximum does not depend on the order.
//   loud_gate_kernel     one workgroup per clip: hop energies from the segments' sums, block energies, both gates (sums over the blocks in a
//                        fixed order: thread-strided, then a fixed tree), L, the gain, the status.
//   loud_apply_kernel    item = 2400 samples: y = g x; in LOOKAHEAD mode P, r, the sliding minimum and the Hann smoothing of a tile with its
//                        halo of 2 Lh + 9 samples all stay in LDS (P is recomputed, not stored: 48 fma per sample).
// The steps of the arithmetic are loudness_steps.h's, shared with the streaming leveler (loudness_stream.hip).
#include <math.h>
#include "runtime.h"
#include "loudness_steps.h"

namespace tt {

constexpr int kLdSegs = 64;                  // segments (threads) of a filter item
constexpr int kLdItem = kLdSegs * kLdS;      // 9600 samples
constexpr int kLdTile = 2400;                // samples of a peak / apply item
constexpr int kLdHalo = 2 * kLdLh + 1 + 8;   // 249: r reaches 2 Lh, P one more, the oversampler 8 more
static_assert(kLdItem == kLdB, "loudness.hip's item mapping");

struct LoudBatch {
  const float* audio;
  const int* in_off;
  const int* hop_off;
  const float* target;   // null: measure
  const float* ceiling;
  int n_clips, max_total;
};

struct LoudClip {
  int i0, n, h0, seg0;
  int early;  // -1: measured; TT_LOUD_EMPTY / TT_LOUD_REFUSED: status and nothing else
};

__host__ __device__ static inline int loud_hops(int n) { return (n + kLdH - 1) / kLdH; }
__host__ __device__ static inline int loud_blocks(int n) { return n >= kLdB ? (n - kLdB) / kLdH + 1 : 0; }

__device__ static inline LoudClip loud_clip(const LoudBatch& b, int c) {
  LoudClip k;
  const int i1 = b.in_off[c + 1];
  k.i0 = b.in_off[c]; k.n = i1 - k.i0; k.h0 = b.hop_off[c];
  k.seg0 = 0; k.early = -1;
  if (k.i0 < 0 || k.n < 0) { k.early = TT_LOUD_REFUSED; return k; }
  for (int j = 0; j < c; ++j)  // (a clip that starts before an earlier clip's start or end: the segment slots would overlap)
    if (b.in_off[j] > k.i0) { k.early = TT_LOUD_REFUSED; return k; }
  if (k.n == 0) { k.early = TT_LOUD_EMPTY; return k; }
  if (i1 > b.max_total || k.h0 < 0 || b.hop_off[c + 1] - k.h0 != loud_hops(k.n)) { k.early = TT_LOUD_REFUSED; return k; }
  if (b.target) {
    const float T = b.target[c], cl = b.ceiling[c];
    if (!(fabsf(T) <= 1e30f) || !(cl > 0.f && cl <= 1e30f)) { k.early = TT_LOUD_REFUSED; return k; }
  }
  k.seg0 = k.i0 / kLdS + c;  // (the clips' segment ranges are disjoint and end below max_total / 150 + n_clips)
  return k;
}

// pre[c] = items before clip c (pre[n_clips] = all); every thread of the workgroup calls it
__device__ static inline void loud_plan(const LoudBatch& b, int item, int* pre) {
  const int t = threadIdx.x;
  if (t < b.n_clips) {
    const LoudClip k = loud_clip(b, t);
    pre[t + 1] = k.early < 0 ? (k.n + item - 1) / item : 0;
  }
  __syncthreads();
  if (t == 0) {
    pre[0] = 0;
    for (int c = 0; c < b.n_clips; ++c) pre[c + 1] += pre[c];
  }
  __syncthreads();
}
__device__ static inline int loud_owner(const int* pre, int n_clips, int w) {
  int c = 0;
  while (c + 1 < n_clips && pre[c + 1] <= w) ++c;
  return c;
}

__global__ void loud_begin_kernel(LoudBatch b, float* __restrict__ true_peak, float* __restrict__ out_true_peak, int* __restrict__ status) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= b.n_clips) return;
  const LoudClip k = loud_clip(b, c);
  if (k.early >= 0) {
    status[c] = k.early;
    return;
  }
  true_peak[c] = 0.f;
  if (out_true_peak) out_true_peak[c] = 0.f;
}

__device__ __forceinline__ int loud_row(int i) { return (i / kLdS) * (kLdS + 1) + i % kLdS; }  // sample i of an item -> its LDS word

template <int PASS>
__global__ __launch_bounds__(kLdSegs) void loud_filter_kernel(LoudBatch b, LoudCoef k, double* __restrict__ state, double* __restrict__ seg_e) {
  __shared__ float xs[kLdSegs * (kLdS + 1) + 2];  // the item's samples from two before its first
  __shared__ int pre[TT_LOUD_MAX_CLIPS + 1];
  const int t = threadIdx.x;
  loud_plan(b, kLdItem, pre);
  for (int w = blockIdx.x; w < pre[b.n_clips]; w += gridDim.x) {
    const int c = loud_owner(pre, b.n_clips, w);
    const LoudClip cl = loud_clip(b, c);
    const int first = (w - pre[c]) * kLdSegs, s0 = first * kLdS;  // first segment and sample of the item
    const int cnt = min(kLdItem, cl.n - s0);
    const float* x = b.audio + cl.i0;
    for (int i = t; i < cnt + 2; i += kLdSegs) {
      const int src = s0 - 2 + i;
      xs[loud_row(i)] = src >= 0 ? x[src] : 0.f;
    }
    __syncthreads();
    const int off = t * kLdS, len = min(kLdS, cnt - off);
    if (len > 0) {
      const size_t slot = (size_t)(cl.seg0 + first + t);
      LoudMem m = {(double)xs[loud_row(off + 1)], (double)xs[loud_row(off)], 0.0, 0.0, 0.0, 0.0};
      double e = 0.0;
      if (PASS == 1) {
        m.v1 = state[4 * slot]; m.v2 = state[4 * slot + 1]; m.y1 = state[4 * slot + 2]; m.y2 = state[4 * slot + 3];
      }
      loud_segment<PASS>(k, [&](int j) { return (double)xs[loud_row(off + 2 + j)]; }, len, m, e);
      if (PASS == 0) {
        state[4 * slot] = m.v1; state[4 * slot + 1] = m.v2; state[4 * slot + 2] = m.y1; state[4 * slot + 3] = m.y2;
      } else {
        seg_e[slot] = e;
      }
    }
    __syncthreads();  // (xs is loaded again)
  }
}

__global__ __launch_bounds__(64) void loud_carry_kernel(LoudBatch b, LoudCoef k, double* __restrict__ state) {
  __shared__ double zs[64][4];
  const int c = blockIdx.x, t = threadIdx.x;
  const LoudClip cl = loud_clip(b, c);
  if (cl.early >= 0) return;
  const int nseg = (cl.n + kLdS - 1) / kLdS;
  double* st = state + 4 * (size_t)cl.seg0;
  double S[4] = {0.0, 0.0, 0.0, 0.0};  // (the same in every lane)
  for (int base = 0; base < nseg; base += 64) {
    const int s = base + t;
    if (s < nseg) {
#pragma unroll
      for (int r = 0; r < 4; ++r) zs[t][r] = st[4 * (size_t)s + r];
    }
    __syncthreads();
    const int m = min(64, nseg - base);
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < m; ++i) {
      if (t == i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[r] = S[r];
      }
      loud_carry_step(k, zs[i], S);
    }
    if (s < nseg) {
#pragma unroll
      for (int r = 0; r < 4; ++r) st[4 * (size_t)s + r] = mine[r];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLdThreads) void loud_peak_kernel(LoudBatch b, const float* __restrict__ src, const float* __restrict__ table,
                                                               float* __restrict__ peak) {
  __shared__ float xs[kLdTile + kLdTaps];
  __shared__ float hs[3 * kLdTaps];
  __shared__ float red[kLdThreads / 64];
  __shared__ int pre[TT_LOUD_MAX_CLIPS + 1];
  const int t = threadIdx.x;
  if (t < 3 * kLdTaps) hs[t] = table[t];
  loud_plan(b, kLdTile, pre);
  for (int w = blockIdx.x; w < pre[b.n_clips]; w += gridDim.x) {
    const int c = loud_owner(pre, b.n_clips, w);
    const LoudClip cl = loud_clip(b, c);
    const int t0 = (w - pre[c]) * kLdTile, cnt = min(kLdTile, cl.n - t0);
    const float* x = src + cl.i0;
    for (int i = t; i < kLdTile + kLdTaps; i += kLdThreads) {
      const int s = t0 - 7 + i;
      xs[i] = s >= 0 && s < cl.n ? x[s] : 0.f;
    }
    __syncthreads();
    float mx = 0.f;
    for (int i = t; i < cnt; i += kLdThreads) mx = fmaxf(mx, loud_peak_at(xs + i, hs));
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    if (t == 0) {
      for (int q = 1; q < kLdThreads / 64; ++q) mx = fmaxf(mx, red[q]);
      atomicMax((unsigned*)peak + c, __float_as_uint(mx));  // (non-negative floats order as their bits)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLdThreads) void loud_gate_kernel(LoudBatch b, LoudCoef k, const double* __restrict__ seg_e, int mode,
                                                               double* __restrict__ lufs, const float* __restrict__ true_peak,
                                                               int* __restrict__ blocks_abs, int* __restrict__ blocks_rel,
                                                               double* __restrict__ hop_energy, float* __restrict__ gain, int* __restrict__ status) {
  __shared__ double red[kLdThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  const LoudClip cl = loud_clip(b, c);
  if (cl.early >= 0) return;  // (uniform)
  const int nseg = (cl.n + kLdS - 1) / kLdS, nh = loud_hops(cl.n), nb = loud_blocks(cl.n);
  const double* se = seg_e + cl.seg0;
  double* q = hop_energy + cl.h0;
  constexpr int per = kLdH / kLdS;
  for (int h = t; h < nh; h += kLdThreads) {
    double a = 0.0;
    for (int s = h * per; s < min(h * per + per, nseg); ++s) a += se[s];
    q[h] = a;
  }
  __threadfence();  // (the hop energies are read back below by other threads of the workgroup)
  __syncthreads();
  const LoudGates gt = loud_gates(q, nb, k.z_abs, red);
  const double L = gt.L, na = gt.na, nr = gt.nr;
  const int st = gt.st;
  if (t != 0) return;
  lufs[c] = L;
  blocks_abs[c] = (int)na;
  blocks_rel[c] = (int)nr;
  status[c] = st;
  if (gain) {
    float g = 1.f;
    if (st == TT_LOUD_OK) {
      g = loud_gain_of_db((double)b.target[c] - L);
      if (mode == TT_LOUD_SCALE) g = fminf(g, b.ceiling[c] / true_peak[c]);
    }
    gain[c] = g;
  }
}

__global__ __launch_bounds__(kLdThreads) void loud_apply_kernel(LoudBatch b, const float* __restrict__ table, int mode, const float* __restrict__ gain,
                                                                const int* __restrict__ status, float* __restrict__ out) {
  __shared__ float xs[kLdTile + 2 * kLdHalo];       // x[t0 - 249 ..]
  __shared__ float Ps[kLdTile + 4 * kLdLh + 1];     // P[t0 - 241 ..]
  __shared__ float rs[kLdTile + 4 * kLdLh];         // r[t0 - 240 ..]
  __shared__ float ds[kLdTile + 2 * kLdLh];         // 1 - m[t0 - 120 ..]
  __shared__ float tab[kLdTable];
  __shared__ int pre[TT_LOUD_MAX_CLIPS + 1];
  const int t = threadIdx.x;
  for (int i = t; i < kLdTable; i += kLdThreads) tab[i] = table[i];
  loud_plan(b, kLdTile, pre);
  for (int w = blockIdx.x; w < pre[b.n_clips]; w += gridDim.x) {
    const int c = loud_owner(pre, b.n_clips, w);
    const LoudClip cl = loud_clip(b, c);
    const int t0 = (w - pre[c]) * kLdTile, cnt = min(kLdTile, cl.n - t0);
    const float* x = b.audio + cl.i0;
    float* y = out + cl.i0;
    const float g = gain[c];
    if (mode != TT_LOUD_LOOKAHEAD_MODE || status[c] != TT_LOUD_OK) {  // (uniform; g is 1 for SHORT and SILENT: the samples, bit for bit)
      for (int i = t; i < cnt; i += kLdThreads) y[t0 + i] = g * x[t0 + i];
      continue;
    }
    const float ceil_c = b.ceiling[c];
    for (int i = t; i < kLdTile + 2 * kLdHalo; i += kLdThreads) {
      const int s = t0 - kLdHalo + i;
      xs[i] = s >= 0 && s < cl.n ? x[s] : 0.f;
    }
    __syncthreads();
    for (int i = t; i < kLdTile + 4 * kLdLh + 1; i += kLdThreads) {
      const int s = t0 - (2 * kLdLh + 1) + i;  // xs index of x[s - 7] is i + 1
      Ps[i] = s >= 0 && s < cl.n ? loud_peak_at(xs + i + 1, tab) : 0.f;
    }
    __syncthreads();
    for (int i = t; i < kLdTile + 4 * kLdLh; i += kLdThreads) {
      const int s = t0 - 2 * kLdLh + i;
      rs[i] = s >= 0 && s < cl.n ? loud_ratio(ceil_c, g, Ps[i], Ps[i + 1]) : 1.f;
    }
    __syncthreads();
    for (int i = t; i < kLdTile + 2 * kLdLh; i += kLdThreads) ds[i] = loud_slide(rs + i);
    __syncthreads();
    const float* wn = tab + 3 * kLdTaps;
    for (int i = t; i < cnt; i += kLdThreads) {
      const float s = loud_smooth(wn, ds + i, rs[i + 2 * kLdLh]);
      y[t0 + i] = (g * xs[i + kLdHalo]) * s;
    }
    __syncthreads();
  }
}

// Phases 1 .. 3 of the oversampler, taps t = -7 .. 8: the header's formula evaluated in fp64 and rounded to f32.  The f32 values are part of
// the specification, so they are tabulated (tests/test_loudness_cpu.py holds them to the reference's, bit for bit), not left to a libm.
const float kLoudTaps[3][TT_LOUD_TAPS] = {
    {-0x1.5e5d38p-11f, 0x1.0bcebcp-8f, -0x1.7339acp-7f, 0x1.873e28p-6f, -0x1.6df07ep-5f, 0x1.4ec604p-4f, -0x1.5aed62p-3f, 0x1.cbc246p-1f, 0x1.2ca176p-2f, -0x1.d2edaap-4f, 0x1.ed2db0p-5f, -0x1.0de388p-5f, 0x1.1370bcp-6f, -0x1.d4dc34p-8f, 0x1.01fc3cp-9f, -0x1.2538c6p-14f},
    {-0x1.ab6476p-12f, 0x1.0e553ap-8f, -0x1.a54124p-7f, 0x1.d23d36p-6f, -0x1.bd0464p-5f, 0x1.957982p-4f, -0x1.8dd350p-3f, 0x1.42b1c6p-1f, 0x1.42b1c6p-1f, -0x1.8dd350p-3f, 0x1.957982p-4f, -0x1.bd0464p-5f, 0x1.d23d36p-6f, -0x1.a54124p-7f, 0x1.0e553ap-8f, -0x1.ab6476p-12f},
    {-0x1.2538c6p-14f, 0x1.01fc3cp-9f, -0x1.d4dc34p-8f, 0x1.1370bcp-6f, -0x1.0de388p-5f, 0x1.ed2db0p-5f, -0x1.d2edaap-4f, 0x1.2ca176p-2f, 0x1.cbc246p-1f, -0x1.5aed62p-3f, 0x1.4ec604p-4f, -0x1.6df07ep-5f, 0x1.873e28p-6f, -0x1.7339acp-7f, 0x1.0bcebcp-8f, -0x1.5e5d38p-11f}};

}  // namespace tt

using namespace tt;

struct tt_loud : EngineHandle {
  int max_total = 0, max_clips = 0;
  LoudCoef coef;
  float* table = nullptr;   // [kLdTable] oversampler phases 1 .. 3 and the smoothing window, fp64 values rounded to f32
  double* state = nullptr;  // [segments][4] end values of the zero-state pass, then the true states
  double* seg_e = nullptr;  // [segments] sum of y^2
};

namespace {

int loud_run(tt_loud* e, hipStream_t s, const LoudBatch& b, int mode, float* out, double* lufs, float* true_peak, int* blocks_abs, int* blocks_rel,
             double* hop_energy, float* gain, float* out_true_peak, int* status) {
  const int items = std::min(e->max_total / kLdItem + b.n_clips, 2048), tiles = std::min(e->max_total / kLdTile + b.n_clips, 4096);
  loud_begin_kernel<<<1, TT_LOUD_MAX_CLIPS, 0, s>>>(b, true_peak, out_true_peak, status);
  loud_filter_kernel<0><<<items, kLdSegs, 0, s>>>(b, e->coef, e->state, e->seg_e);
  loud_carry_kernel<<<b.n_clips, 64, 0, s>>>(b, e->coef, e->state);
  loud_filter_kernel<1><<<items, kLdSegs, 0, s>>>(b, e->coef, e->state, e->seg_e);
  loud_peak_kernel<<<tiles, kLdThreads, 0, s>>>(b, b.audio, e->table, true_peak);
  loud_gate_kernel<<<b.n_clips, kLdThreads, 0, s>>>(b, e->coef, e->seg_e, mode, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, gain, status);
  if (out) {
    loud_apply_kernel<<<tiles, kLdThreads, 0, s>>>(b, e->table, mode, gain, status, out);
    loud_peak_kernel<<<tiles, kLdThreads, 0, s>>>(b, out, e->table, out_true_peak);
  }
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int tt_loud_abi_version(void) { return 1; }  // ABI changes

int tt_loud_hops(int n) { return n >= 1 && n <= TT_LOUD_MAX_SAMPLES ? loud_hops(n) : 0; }

int tt_loud_blocks(int n) { return n >= 1 && n <= TT_LOUD_MAX_SAMPLES ? loud_blocks(n) : 0; }

int tt_loud_create(int max_total_samples, int max_clips, tt_loud** out) {
  TT_REQUIRE(out, "tt_loud_create: null argument");
  TT_REQUIRE(max_total_samples >= 1 && max_total_samples <= TT_LOUD_MAX_SAMPLES, "tt_loud_create: max_total_samples %d (1 .. %d)", max_total_samples,
             TT_LOUD_MAX_SAMPLES);
  TT_REQUIRE(max_clips >= 1 && max_clips <= TT_LOUD_MAX_CLIPS, "tt_loud_create: max_clips %d (1 .. %d)", max_clips, TT_LOUD_MAX_CLIPS);
  tt_loud* e = new tt_loud();
  e->max_total = max_total_samples; e->max_clips = max_clips;
  loud_design(&e->coef);
  const size_t segments = (size_t)max_total_samples / kLdS + (size_t)max_clips + 1;
  int rc = e->open("tt_loud_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->table, kLdTable, false);
  if (!rc) rc = e->arena.alloc_t(&e->state, 4 * segments);
  if (!rc) rc = e->arena.alloc_t(&e->seg_e, segments);
  if (!rc) {
    float tab[kLdTable];
    loud_table(tab);
    if (hipMemcpy(e->table, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("tt_loud_create: the table upload failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_loud_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_loud_destroy(tt_loud* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_loud_measure(tt_loud* e, int n_clips, const float* audio, const int* in_off, const int* hop_off, double* lufs, float* true_peak,
                    int* blocks_abs, int* blocks_rel, double* hop_energy, int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && hop_off && lufs && true_peak && blocks_abs && blocks_rel && hop_energy && status, "tt_loud_measure: null argument");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_loud_measure: %d clips (1 .. %d)", n_clips, e->max_clips);
  const LoudBatch b = {audio, in_off, hop_off, nullptr, nullptr, n_clips, e->max_total};
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    return loud_run(e, s, b, TT_LOUD_NONE, nullptr, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, nullptr, nullptr, status);
  });
}

int tt_loud_normalize(tt_loud* e, int n_clips, const float* audio, const int* in_off, const int* hop_off, const float* target,
                      const float* ceiling, int mode, float* out, double* lufs, float* true_peak, int* blocks_abs, int* blocks_rel,
                      double* hop_energy, float* gain, float* out_true_peak, int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && hop_off && target && ceiling && out && lufs && true_peak && blocks_abs && blocks_rel && hop_energy && gain &&
                 out_true_peak && status,
             "tt_loud_normalize: null argument");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_loud_normalize: %d clips (1 .. %d)", n_clips, e->max_clips);
  TT_REQUIRE(mode == TT_LOUD_NONE || mode == TT_LOUD_SCALE || mode == TT_LOUD_LOOKAHEAD_MODE, "tt_loud_normalize: mode %d (0 .. 2)", mode);
  const LoudBatch b = {audio, in_off, hop_off, target, ceiling, n_clips, e->max_total};
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    return loud_run(e, s, b, mode, out, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, gain, out_true_peak, status);
  });
}

}  // extern "C"
