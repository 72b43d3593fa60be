// The steps the whole-clip loudness kernels (loudness.hip) and the streaming leveler (loudness_stream.hip) share: the K-weighting cascade of
// one sample, a segment's run, the carry with M, the gate sums, the true-peak phases and the limiter's ratio / sliding minimum / Hann sum.
// A kernel of either form that uses a step computes that step's bits (include/tortoise_mi355x_loud.h is the text).
#pragma once
#include <math.h>
#include "../../include/tortoise_mi355x_loud.h"

namespace tt {

constexpr int kLdH = TT_LOUD_HOP, kLdB = TT_LOUD_BLOCK, kLdS = TT_LOUD_SEGMENT, kLdLh = TT_LOUD_LOOKAHEAD, kLdTaps = TT_LOUD_TAPS;
constexpr int kLdThreads = 256;
constexpr int kLdW = 2 * kLdLh + 1;          // 241 window taps
constexpr int kLdTable = 3 * kLdTaps + kLdW; // phases 1 .. 3, then the window
static_assert(kLdH % kLdS == 0 && kLdTaps == 16, "the hop is a whole number of segments");

struct LoudCoef {
  double b0, b1, b2, na1, na2;  // shelf (the feedback coefficients negated)
  double nc1, nc2;              // high-pass feedback, negated; its b is (1, -2, 1)
  double M[4][4];               // transition of kLdS samples over (shelf y[n-1], y[n-2], high-pass y[n-1], y[n-2])
  double z_abs;                 // 10^(-6.9309): the absolute gate in the linear domain
};

// the recurrence's memory: two inputs, two shelf outputs, two high-pass outputs
struct LoudMem {
  double x1, x2, v1, v2, y1, y2;
};

// ---- host: the tables a handle of either form is made with
// Phases 1 .. 3 of the oversampler, taps t = -7 .. 8, f32: tabulated in loudness.hip (they are part of the specification)
extern const float kLoudTaps[3][TT_LOUD_TAPS];

// one K-weighting section's feedback pair (and the shelf's b) for fs = 24000
static inline void loud_design(LoudCoef* k) {
  const double fs = (double)TT_LOUD_SAMPLE_RATE;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
    k->b0 = (Vh + Vb * K / Q + K * K) / a0;
    k->b1 = 2.0 * (K * K - Vh) / a0;
    k->b2 = (Vh - Vb * K / Q + K * K) / a0;
    k->na1 = -(2.0 * (K * K - 1.0) / a0);
    k->na2 = -((1.0 - K / Q + K * K) / a0);
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / fs), a0 = 1.0 + K / Q + K * K;
    k->nc1 = -(2.0 * (K * K - 1.0) / a0);
    k->nc2 = -((1.0 - K / Q + K * K) / a0);
  }
  // M: the recurrence without input on the four unit states, kLdS samples, in extended precision
  for (int q = 0; q < 4; ++q) {
    long double v1 = q == 0, v2 = q == 1, y1 = q == 2, y2 = q == 3;
    for (int j = 0; j < kLdS; ++j) {
      const long double v = (long double)k->na1 * v1 + (long double)k->na2 * v2;
      const long double y = v - 2.0L * v1 + v2 + (long double)k->nc1 * y1 + (long double)k->nc2 * y2;
      v2 = v1; v1 = v; y2 = y1; y1 = y;
    }
    k->M[0][q] = (double)v1; k->M[1][q] = (double)v2; k->M[2][q] = (double)y1; k->M[3][q] = (double)y2;
  }
  k->z_abs = pow(10.0, (-70.0 + 0.691) / 10.0);
}

static inline void loud_table(float* tab) {
  for (int p = 0; p < 3; ++p)
    for (int q = 0; q < kLdTaps; ++q) tab[p * kLdTaps + q] = kLoudTaps[p][q];
  double w[kLdW], sum = 0.0;
  for (int q = 0; q < kLdW; ++q) {
    w[q] = 0.5 + 0.5 * cos(M_PI * (double)(q - kLdLh) / (double)(kLdLh + 1));
    sum += w[q];
  }
  for (int q = 0; q < kLdW; ++q) tab[3 * kLdTaps + q] = (float)(w[q] / sum);
}

#ifdef __HIPCC__

// one sample through the cascade: the K-weighted sample; the memory moves on
__device__ __forceinline__ double loud_sample(const LoudCoef& k, double x0, LoudMem& m) {
  double v = k.b0 * x0;  // the five terms in the header's order: the a1 term last, it alone waits for the previous sample
  v = fma(k.b1, m.x1, v);
  v = fma(k.b2, m.x2, v);
  v = fma(k.na2, m.v2, v);
  v = fma(k.na1, m.v1, v);
  double y = v;
  y = fma(-2.0, m.v1, y);
  y = y + m.v2;
  y = fma(k.nc2, m.y2, y);
  y = fma(k.nc1, m.y1, y);
  m.x2 = m.x1; m.x1 = x0; m.v2 = m.v1; m.v1 = v; m.y2 = m.y1; m.y1 = y;
  return y;
}

// len samples of a segment, read(j) the j-th as f64: PASS 0 only moves the memory (from a zero state: the end values), PASS 1 adds y^2 to e
template <int PASS, typename Read>
__device__ __forceinline__ void loud_segment(const LoudCoef& k, Read read, int len, LoudMem& m, double& e) {
  for (int j = 0; j < len; ++j) {
    const double y = loud_sample(k, read(j), m);
    if (PASS == 1) e = fma(y, y, e);
  }
}

// state' = M state + z, the four rows in turn, four fused multiply-adds each onto z
__device__ __forceinline__ void loud_carry_step(const LoudCoef& k, const double* z, double (&S)[4]) {
  double nx[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double a = z[r];
#pragma unroll
    for (int q = 0; q < 4; ++q) a = fma(k.M[r][q], S[q], a);
    nx[r] = a;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) S[r] = nx[r];
}

// P[n] from w[0 .. 15] = x[n - 7 .. n + 8]; h = phases 1 .. 3
__device__ __forceinline__ float loud_peak_at(const float* w, const float* h) {
  float P = fabsf(w[7]);  // phase 0 is the exact delta
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < kLdTaps; ++q) a = fmaf(h[p * kLdTaps + q], w[q], a);
    P = fmaxf(P, fabsf(a));
  }
  return P;
}

// a + the values of the other threads (kLdThreads of them), in a fixed tree
__device__ static inline double loud_sum(double a, double* red) {
  const int t = threadIdx.x;
  red[t] = a;
  __syncthreads();
  for (int s = kLdThreads / 2; s >= 1; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

struct LoudGates {
  double L, na, nr;  // L (-HUGE_VAL without one), the blocks above the absolute gate and above both
  int st;            // TT_LOUD_OK / SHORT / SILENT
};

// Both gates and L over the blocks 0 .. nb - 1 of the hop energies q (nb + 3 of them), by the whole workgroup of kLdThreads threads:
// thread-strided sums, then the fixed tree.  Every thread gets the result.
__device__ static inline LoudGates loud_gates(const double* q, int nb, double z_abs, double* red) {
  const int t = threadIdx.x;
  auto z = [&](int j) { return (((q[j] + q[j + 1]) + q[j + 2]) + q[j + 3]) / (double)kLdB; };
  double sa = 0.0, na = 0.0;
  for (int j = t; j < nb; j += kLdThreads) {
    const double zj = z(j);
    if (zj > z_abs) { sa += zj; na += 1.0; }
  }
  sa = loud_sum(sa, red);
  na = loud_sum(na, red);
  double L = -HUGE_VAL, nr = 0.0;
  int st = nb == 0 ? TT_LOUD_SHORT : TT_LOUD_SILENT;
  if (na > 0.0) {
    const double rel = 0.1 * (sa / na);
    double sr = 0.0;
    for (int j = t; j < nb; j += kLdThreads) {
      const double zj = z(j);
      if (zj > z_abs && zj > rel) { sr += zj; nr += 1.0; }
    }
    sr = loud_sum(sr, red);
    nr = loud_sum(nr, red);
    L = -0.691 + 10.0 * log10(sr / nr);
    st = TT_LOUD_OK;
  }
  return {L, na, nr, st};
}

// the gain to a target: (f32) 10^((T - L) / 20), or of a level in dB, the power in f64
__device__ __forceinline__ float loud_gain_of_db(double db) { return (float)pow(10.0, db / 20.0); }

// the limiter: r from the ceiling, the gain and two neighbouring peaks; 1 - the minimum of kLdW ratios; the Hann sum over kLdW of those
__device__ __forceinline__ float loud_ratio(float ceil_c, float g, float P0, float P1) { return fminf(1.f, ceil_c / (g * fmaxf(P0, P1))); }
__device__ __forceinline__ float loud_slide(const float* rs) {
  float m = rs[0];
  for (int q = 1; q < kLdW; ++q) m = fminf(m, rs[q]);
  return 1.f - m;
}
__device__ __forceinline__ float loud_smooth(const float* wn, const float* ds, float r) {
  float a = 0.f;
  for (int q = 0; q < kLdW; ++q) a = fmaf(wn[q], ds[q], a);
  return fminf(r, 1.f - a);
}

#endif  // __HIPCC__

}  // namespace tt
