// The steps the resampler's kernels share (include/tortoise_mi355x_rs.h, include/tortoise_mi355x_rss.h): the integers of a ratio, the
// prototype table, one tap's weight and one output sample.  resample.hip (whole clips) and resample_stream.hip (streams, both forms) are
// built from these, so their arithmetic cannot drift: a streamed sample is the whole-clip sample to the bit.
//
// The integer part (everything above `#ifdef __HIPCC__`) is plain C++ as well: the streaming bookkeeping (resample_stream_host.h) and its
// stand-alone check compile it without the device toolchain.
#pragma once
#include <math.h>
#include "../../include/tortoise_mi355x_rs.h"

#ifdef __HIPCC__
#define TT_RS_HD __host__ __device__
#else
#define TT_RS_HD
#endif

namespace tt {

constexpr int kRsTab = TT_RS_ZEROS * TT_RS_PER_ZERO;  // Z L = 16384: taps with k >= kRsTab are zero
constexpr long long kRsOne = (long long)kRsTab << 16;                                               // Z L 65536
constexpr long long kRsCqNum = (long long)TT_RS_RHO_NUM * TT_RS_PER_ZERO * 65536;                   // 9 L 65536
constexpr int kRsCqMin = (int)(kRsCqNum / ((long long)TT_RS_RHO_DEN * TT_RS_MAX_RATIO));            // cq at P / Q = 8
constexpr int kRsHMax = (int)((kRsOne + kRsCqMin - 1) / kRsCqMin);                                  // 285
static_assert(TT_RS_TABLE == kRsTab + 1 && kRsHMax == 285, "the header's table and the widest filter");
static_assert(kRsOne + 2 * (kRsCqNum / TT_RS_RHO_DEN) < (1ll << 32), "u <= (H + 1) cq < Z L 65536 + 2 cq fits 32 bits");

TT_RS_HD static inline int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}
TT_RS_HD static inline bool rs_ratio_ok(int P, int Q) {
  if (P < 1 || Q < 1 || P > TT_RS_MAX_TERM || Q > TT_RS_MAX_TERM) return false;
  if ((long long)P > (long long)TT_RS_MAX_RATIO * Q || (long long)Q > (long long)TT_RS_MAX_RATIO * P) return false;
  return Q == TT_RS_PITCH_ONE || rs_gcd(P, Q) == 1;
}
TT_RS_HD static inline int rs_out_samples(int n, int P, int Q) { return (int)(((long long)n * Q + P - 1) / P); }
TT_RS_HD static inline unsigned rs_cq(int P, int Q) {
  return P > Q ? (unsigned)(kRsCqNum * Q / ((long long)TT_RS_RHO_DEN * P)) : (unsigned)(kRsCqNum / TT_RS_RHO_DEN);
}
TT_RS_HD static inline int rs_half_width(unsigned cq) { return (int)((kRsOne + cq - 1) / cq); }
TT_RS_HD static inline float rs_c32(int P, int Q) { return (float)(0.9 * (P > Q ? (double)Q / (double)P : 1.0)); }

// I0 by its power series, sum_k ((x / 2)^k / k!)^2: the same double operations in the same order as tests/resample_reference.py
static inline double rs_i0(double x) {
  const double y = x / 2;
  double term = 1, sum = 1;
  for (int k = 1; k < 500; ++k) {
    const double f = y / k;
    term *= f * f;
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// tab[0 .. TT_RS_TABLE): the prototype in fp64, rounded to f32 (host)
static inline void rs_fill_table(float* tab) {
  const double i0b = rs_i0((double)TT_RS_BETA);
  for (int t = 0; t <= kRsTab; ++t) {
    const double x = (double)t / TT_RS_PER_ZERO, q = (double)t / kRsTab;
    const double s = t ? sin(M_PI * x) / (M_PI * x) : 1.0;
    tab[t] = (float)(s * rs_i0(TT_RS_BETA * sqrt(1.0 - q * q)) / i0b);
  }
}

#ifdef __HIPCC__

// h_j of the header for the table position u (16.16): three rounded f32 operations; 0 beyond the last zero crossing.  `tab` is the
// prototype wherever the caller keeps it (LDS in the kernels that gather per tap, global memory where a phase bank is built once).
__device__ static inline float rs_tap_weight(const float* tab, unsigned u, float c32) {
  const unsigned k = u >> 16;
  const unsigned kc = k < (unsigned)kRsTab ? k : (unsigned)kRsTab - 1;
  const float a = (float)(u & 65535u) * (1.f / 65536.f);
  const float t0 = tab[kc], t1 = tab[kc + 1];
  return k < (unsigned)kRsTab ? c32 * fmaf(a, t1 - t0, t0) : 0.f;
}

// f = floor(r cq / Q) and g = ceil(r cq / Q) of an output's phase r: with them the header's per-tap division is not executed, u = |d| cq + f
// for d = j - i <= 0 and u = d cq - g for d >= 1, exactly
__device__ static inline void rs_phase(int r, unsigned cq, int Q, unsigned* f, unsigned* g_up) {
  const unsigned long long rc = (unsigned long long)r * cq;
  *f = (unsigned)(rc / (unsigned)Q);
  *g_up = *f + (rc % (unsigned)Q != 0);
}

// u of tap d = -H .. H + 1 of an output whose phase gave (f, g_up)
__device__ static inline unsigned rs_tap_u(int d, unsigned cq, unsigned f, unsigned g_up) {
  return d <= 0 ? (unsigned)(-d) * cq + f : (unsigned)d * cq - g_up;
}

// One output sample of phase r: xs[0 .. 2 H + 2) are the inputs x[i - H .. i + H + 1] (zeros where the clip has none), taken in ascending
// order with one FMA each; u walks down by cq to the centre and up again.
__device__ static inline float rs_output(const float* tab, const float* xs, int H, unsigned cq, int Q, int r, float c32) {
  unsigned f, g_up;
  rs_phase(r, cq, Q, &f, &g_up);
  float acc = 0.f;
  unsigned u = (unsigned)H * cq + f;  // d = -H .. 0: u = |d| cq + f
  for (int d = 0; d <= H; ++d, u -= cq) acc = fmaf(rs_tap_weight(tab, u, c32), xs[d], acc);
  u = cq - g_up;                      // d = 1 .. H + 1: u = d cq - g
  for (int d = 1; d <= H + 1; ++d, u += cq) acc = fmaf(rs_tap_weight(tab, u, c32), xs[H + d], acc);
  return acc;
}

#endif  // __HIPCC__

}  // namespace tt
