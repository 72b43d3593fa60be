// The steps the F0 kernels share (include/tortoise_mi355x_f0.h, include/tortoise_mi355x_f0v.h): a workgroup's plan, the status of a clip, and
// the stage / slots / scan / power / pick / parabola steps of a group of frames.  f0.hip (one pick a frame) and f0_viterbi.hip (the
// candidates of a frame) are built from these, so d' and tt_f0_track's own pick cannot drift between them: the bits are the same.
//
//   stage     the group's span, (kF0G + 3) 240 + 480 = 2160 floats, into LDS, zero outside the clip.
//   slots     the register tiling of tsm_search: thread (u, h), u < 120, owns the four adjacent lags 4u + 1 .. 4u + 4 and half h of every
//             slot (120 samples, ascending).  Per four samples one broadcast ds_read_b128 of x[j ..] and one new aligned ds_read_b128 of
//             x[j + 4u ..], consecutive over the lanes; the eight values held feed all 16 (sample, lag) terms.  A term is one v_sub_f32
//             and one v_fma_f32.  After slot s >= 3 the thread adds its last four slot sums, oldest first, ((S_s-3 + S_s-2) + S_s-1) + S_s:
//             its half of d of frame s - 3, to LDS.  d = half 0 + half 1.  At most 120 + 3 + 1 + 1 rounded operations on a path.
//   scan      one wave a frame.  Lane l holds lags 8l + 1 .. 8l + 8: a local f64 running sum, a shuffle scan of the lanes' totals,
//             c = (sum of the lanes before) + local; d' in f64 to the wave's LDS table.
//   power     P is 15 samples a lane and a butterfly.
//   pick      lane l looks at lags l, l + 64, ...: both searches are min-index reductions over the wave, the argmin a (value, index)
//             reduction.  No lane walks the table.
//   parabola  delta of a lag from its three table entries.
// Nothing about a frame depends on where its clip stands in the batch: the order of every sum is fixed by the frame's index in its own clip.
#pragma once
#include <math.h>
#include "runtime.h"
#include "f0_host.h"

namespace tt {

constexpr int kF0H = TT_F0_HOP, kF0W = TT_F0_WINDOW, kF0T = TT_F0_LAG_MAX, kF0Lead = TT_F0_LEAD;
#ifndef TT_F0_G
#define TT_F0_G 4  // a multiple of 4, at most 8 (the LDS plan below).  4: 39 KB of LDS, four workgroups a CU, one round of scan and pick; 8: 0.79 of
#endif             // the terms, 59 KB, two a CU, two rounds - and the slower of the two as measured (profiles/r27_f0.txt)
constexpr int kF0G = TT_F0_G;                             // frames of a workgroup
constexpr int kF0Threads = 256;
constexpr int kF0Waves = kF0Threads / 64;
constexpr int kF0Slots = kF0G + kF0W / kF0H - 1;          // 7 slots of kF0H samples
constexpr int kF0Span = kF0Slots * kF0H + kF0T;           // 2160 floats
constexpr int kF0Quads = kF0T / 4;                        // 120 threads of a half own the lags
constexpr int kF0Half = kF0H / 2;                         // samples of a thread's part of a slot
constexpr int kF0Row = kF0T + 4;                          // doubles of a wave's d' table (entries 0 .. T)
constexpr int kF0PerLane = 8;                             // lags of a lane in the scan
constexpr int kF0None = 0x7fffffff;
static_assert(kF0W == 4 * kF0H && kF0Lead == kF0W - kF0H && kF0T % 4 == 0 && kF0Half % 4 == 0 && kF0Span % 4 == 0, "a frame is four slots");
static_assert(2 * 128 == kF0Threads && kF0Quads <= 128 && kF0G % kF0Waves == 0 && 64 * kF0PerLane >= kF0T && kF0W % 64 == 0, "thread plan");
static_assert((kF0Span + kF0G * 2 * kF0T) * sizeof(float) + kF0Waves * kF0Row * sizeof(double) <= 64 * 1024, "LDS plan");

typedef float f0_f4 __attribute__((ext_vector_type(4)));

struct F0Args {
  int n_clips, max_samples;
  const float* audio;
  const int* in_off;
  const int* par;
  const double* thr;
  const int* frm_off;
};

// the status of clip c before its audio is read; *n_p its samples when it is TT_F0_OK
__device__ static inline int f0_clip(const F0Args& a, int c, int* n_p) {
  const int i0 = a.in_off[c], i1 = a.in_off[c + 1];
  const int st = f0_clip_status(i0, i1, a.max_samples, a.par[2 * c], a.par[2 * c + 1], a.thr[2 * c], a.thr[2 * c + 1], a.frm_off[c], a.frm_off[c + 1]);
  *n_p = st == TT_F0_OK ? i1 - i0 : 0;
  return st;
}

__device__ static inline int f0_wave_min(int v) {
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

// stage: x_s[e] = x[fg H - 720 + e] for the ns slots of the group that begins at frame fg (the caller's barrier follows)
__device__ static inline void f0_stage(float* x_s, const float* __restrict__ x, int n, int fg, int ns, int t) {
  const int b0 = fg * kF0H - kF0Lead, span = ns * kF0H + kF0T;
  for (int e = t; e < span; e += kF0Threads) {
    const int i = b0 + e;
    x_s[e] = i >= 0 && i < n ? x[i] : 0.f;
  }
}

// slots: part_s[frame][half][lag - 1] of the group's ns - 3 frames (the caller's barrier follows)
__device__ static inline void f0_slots(const float* x_s, float* part_s, int ns, int t) {
  const int u = t & 127, h = t >> 7;
  if (u < kF0Quads) {
    const f0_f4* x4 = (const f0_f4*)x_s;
    float p0[4] = {0.f, 0.f, 0.f, 0.f}, p1[4] = {0.f, 0.f, 0.f, 0.f}, p2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ns; ++s) {
      const f0_f4* xa = x4 + s * (kF0H / 4) + h * (kF0Half / 4);  // (the last read below: float4 (ns - 1) 60 + 30 + 29 + 1 + 119 < span / 4)
      const f0_f4* xb = xa + u;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      f0_f4 B0 = xb[0];
#pragma unroll 2
      for (int q = 0; q < kF0Half / 4; ++q) {
        const f0_f4 A = xa[q], B1 = xb[q + 1];
        const float av[4] = {A.x, A.y, A.z, A.w};
        const float y[8] = {B0.x, B0.y, B0.z, B0.w, B1.x, B1.y, B1.z, B1.w};  // x[j0 + 4u ..], j0 = the first of these four samples
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float e = av[i] - y[i + 1 + k];  // x[j] - x[j + tau], tau = 4u + 1 + k
            acc[k] = fmaf(e, e, acc[k]);
          }
        }
        B0 = B1;
      }
      if (s >= 3) {
        f0_f4 d;
        d.x = ((p0[0] + p1[0]) + p2[0]) + acc[0];
        d.y = ((p0[1] + p1[1]) + p2[1]) + acc[1];
        d.z = ((p0[2] + p1[2]) + p2[2]) + acc[2];
        d.w = ((p0[3] + p1[3]) + p2[3]) + acc[3];
        *(f0_f4*)(part_s + ((s - 3) * 2 + h) * kF0T + 4 * u) = d;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p0[k] = p1[k];
        p1[k] = p2[k];
        p2[k] = acc[k];
      }
    }
  }
}

// scan: d'(0 .. T) of the group's frame i into the wave's table dp (the caller's barrier follows)
__device__ static inline void f0_scan(const float* part_s, double* dp, int i, int lane) {
  const float* pa = part_s + (i * 2) * kF0T + lane * kF0PerLane;
  float dv[kF0PerLane];
  double loc[kF0PerLane];
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < kF0PerLane; ++k) {
    const bool in = lane * kF0PerLane + k < kF0T;
    dv[k] = in ? pa[k] + pa[kF0T + k] : 0.f;
    run += (double)dv[k];
    loc[k] = run;
  }
  double tot = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(tot, d);
    if (lane >= d) tot = o + tot;
  }
  double before = __shfl_up(tot, 1);
  if (lane == 0) before = 0.0;
#pragma unroll
  for (int k = 0; k < kF0PerLane; ++k) {
    const int tau = lane * kF0PerLane + k + 1;
    if (tau <= kF0T) {
      const double cs = before + loc[k];
      dp[tau] = cs > 0.0 ? ((double)dv[k] * (double)tau) / cs : 1.0;
    }
  }
  if (lane == 0) dp[0] = 1.0;
}

// power: P of the group's frame i, on every lane of its wave
__device__ static inline double f0_power(const float* x_s, int i, int lane) {
  double P = 0.0;
  const float* xf = x_s + i * kF0H + lane * (kF0W / 64);
#pragma unroll
  for (int k = 0; k < kF0W / 64; ++k) {
    const double v = (double)xf[k];
    P = fma(v, v, P);
  }
  for (int m = 32; m >= 1; m >>= 1) P += __shfl_xor(P, m);
  return P;
}

// pick: t^ of a frame from its table, on every lane of its wave; *has_t0: a lag of [lo, hi] lies below thr
__device__ static inline int f0_pick(const double* dp, int lo, int hi, double thr, int lane, bool* has_t0) {
  int t0 = kF0None;
  for (int tau = lane; tau <= hi; tau += 64)
    if (tau >= lo && dp[tau] < thr) t0 = min(t0, tau);
  t0 = f0_wave_min(t0);
  *has_t0 = t0 != kF0None;
  int th;
  if (t0 != kF0None) {  // (uniform) the end of the descent from t0
    th = kF0None;
    for (int tau = lane; tau <= hi; tau += 64)
      if (tau >= t0 && (tau == hi || dp[tau + 1] >= dp[tau])) th = min(th, tau);
    th = f0_wave_min(th);
  } else {  // the first argmin over [lo, hi]
    double bv = 0.0;
    int bi = kF0None;
    for (int tau = lane; tau <= hi; tau += 64)
      if (tau >= lo && (bi == kF0None || dp[tau] < bv)) bv = dp[tau], bi = tau;
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (oi != kF0None && (bi == kF0None || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
    }
    th = bi;
  }
  return th;
}

// parabola: delta of lag th from d'(th - 1), d'(th), d'(th + 1); 0 at the table's ends and where the three do not curve upwards
__device__ static inline double f0_parabola(const double* dp, int th) {
  const double bq = dp[th];
  double delta = 0.0;
  if (th >= 2 && th <= kF0T - 1) {
    const double aq = dp[th - 1], cq = dp[th + 1];
    const double den = (aq - 2.0 * bq) + cq;
    if (den > 0.0) delta = fmin(1.0, fmax(-1.0, 0.5 * (aq - cq) / den));
  }
  return delta;
}

}  // namespace tt
