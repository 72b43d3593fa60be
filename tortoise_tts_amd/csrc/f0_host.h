// The integers and parameter rules of the F0 tracker (include/tortoise_mi355x_f0.h): the frame count, the per-clip parameter checks the
// kernels make, the lag range of a frequency range, and every argument check of tt_f0_create / tt_f0_track that does not need the data.
// Plain C++ with no device part, so that csrc/checks/f0_host_check.cpp can run it under the host sanitizers; the frame count and the
// parameter rules are host and device functions, so that the kernels of f0.hip refuse a clip with the very code the host check runs.
#pragma once
#include <math.h>
#include <stdio.h>
#include "../../include/tortoise_mi355x_f0.h"

#if defined(__HIPCC__)
#define TT_F0_HD __host__ __device__
#else
#define TT_F0_HD
#endif

namespace tt {

// F = ceil(n / H) for 1 <= n <= TT_F0_MAX_SAMPLES (the caller checks the range)
TT_F0_HD static inline int f0_frames(int n) { return (n + TT_F0_HOP - 1) / TT_F0_HOP; }
TT_F0_HD static inline bool f0_lags_ok(int lo, int hi) { return lo >= TT_F0_LAG_MIN && lo <= hi && hi <= TT_F0_LAG_MAX; }
// thr in [0, 2], floor_e >= 0 and finite (NaN fails every comparison)
TT_F0_HD static inline bool f0_thr_ok(double thr, double floor_e) { return thr >= 0.0 && thr <= 2.0 && floor_e >= 0.0 && floor_e <= 1.7e308; }

// the status of a clip from its numbers alone: offsets i0 .. i1 of its samples, its frame slice f0_ .. f1, its parameters
TT_F0_HD static inline int f0_clip_status(int i0, int i1, int max_samples, int lo, int hi, double thr, double floor_e, int fo0, int fo1) {
  const long long n = (long long)i1 - i0;
  if (i0 < 0 || n < 0) return TT_F0_REFUSED;
  if (n == 0) return TT_F0_EMPTY;
  if (n > max_samples) return TT_F0_REFUSED;
  if (!f0_lags_ok(lo, hi) || !f0_thr_ok(thr, floor_e)) return TT_F0_REFUSED;
  if (fo0 < 0 || (long long)fo1 - fo0 < f0_frames((int)n)) return TT_F0_REFUSED;
  return TT_F0_OK;
}

// lag_hi = floor(24000 / fmin), lag_lo = ceil(24000 / fmax) for 50 <= fmin <= fmax <= 1000 Hz; false (nothing written) otherwise.  The
// quotients of integers up to 24000 are at least 1 / 1000 from an integer unless they are one, so the rounded division decides correctly.
static inline bool f0_lag_from_hz(double fmin, double fmax, int* lo, int* hi) {
  const double least = (double)TT_F0_SAMPLE_RATE / TT_F0_LAG_MAX, most = (double)TT_F0_SAMPLE_RATE / TT_F0_LAG_MIN;
  if (!lo || !hi || !(fmin >= least && fmin <= fmax && fmax <= most)) return false;
  const int l = (int)ceil(TT_F0_SAMPLE_RATE / fmax), h = (int)floor(TT_F0_SAMPLE_RATE / fmin);
  if (!f0_lags_ok(l, h)) return false;  // (fmin and fmax between the same two lags: no lag lies in the range)
  *lo = l;
  *hi = h;
  return true;
}

static inline int f0_fail(char* err, size_t n, const char* fmt, int a, int b) {
  snprintf(err, n, fmt, a, b);
  return -1;
}

static inline int f0_check_create(bool have_out, int max_samples, int max_clips, char* err, size_t en) {
  if (!have_out) return f0_fail(err, en, "tt_f0_create: null argument", 0, 0);
  if (max_samples < 1 || max_samples > TT_F0_MAX_SAMPLES) return f0_fail(err, en, "tt_f0_create: max_samples %d (1 .. %d)", max_samples, TT_F0_MAX_SAMPLES);
  if (max_clips < 1 || max_clips > TT_F0_MAX_CLIPS) return f0_fail(err, en, "tt_f0_create: max_clips %d (1 .. %d)", max_clips, TT_F0_MAX_CLIPS);
  return 0;
}

static inline int f0_check_track(bool have_all, int n_clips, int max_clips, char* err, size_t en) {
  if (!have_all) return f0_fail(err, en, "tt_f0_track: null argument", 0, 0);
  if (n_clips < 1 || n_clips > max_clips) return f0_fail(err, en, "tt_f0_track: %d clips (1 .. %d)", n_clips, max_clips);
  return 0;
}

}  // namespace tt
