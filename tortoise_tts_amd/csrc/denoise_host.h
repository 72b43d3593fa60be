// Host arithmetic of the spectral-subtraction denoiser (include/tortoise_mi355x_nr.h): the rank of the order statistic, the frames of a
// noise region, a clip's status and the checks of tt_nr_params.  Plain C++ with no device part, so that csrc/checks/nr_host_check.cpp can
// run it under the sanitizers; csrc/denoise.hip uses the same functions.
#pragma once
#include <math.h>
#include "../../include/tortoise_mi355x_nr.h"

#ifdef __HIPCC__
#define TT_NR_HD __host__ __device__
#else
#define TT_NR_HD
#endif

namespace tt {

// The k-th smallest (k = 0: the minimum) of a multiset of 32-bit patterns, given only below(x) = how many of them are < x: the largest x with
// below(x) <= k, built from the most significant bit down.  below is monotone, so 32 evaluations decide it, whatever the values are.
template <class Below>
TT_NR_HD inline unsigned nr_bisect(int k, const Below& below) {
  unsigned ans = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = ans | (1u << bit);
    if (below(cand) <= k) ans = cand;
  }
  return ans;
}

// k = floor(q (frames - 1)), q = quantile_num / TT_NR_QUANTILE_DEN, in 64-bit integers; -1 for an argument out of range
static inline int nr_rank(int quantile_num, int frames) {
  if (quantile_num < 0 || quantile_num > TT_NR_QUANTILE_DEN || frames < 1) return -1;
  return (int)((long long)quantile_num * (long long)(frames - 1) / TT_NR_QUANTILE_DEN);
}

// the frames t < frames with start <= t hop and t hop + hop <= end; -1 for an argument out of range
static inline int nr_region(long long start, long long end, int hop, int frames, int* first, int* count) {
  if (!first || !count || start < 0 || end < start || hop < 1 || frames < 1) return -1;
  const long long lo = (start + hop - 1) / hop;  // the first t with t hop >= start
  long long hi = end / hop;                      // t + 1 <= end / hop
  if (hi > frames) hi = frames;
  *first = lo < frames ? (int)lo : frames;
  *count = hi > lo ? (int)(hi - lo) : 0;
  return 0;
}

// status of an accepted clip: what is decided from the lengths alone
static inline int nr_status(int frames, int noise_frames) { return noise_frames == 0 && frames < TT_NR_MIN_FRAMES ? TT_NR_SHORT : TT_NR_OK; }

// nullptr, or what is wrong with the region of a clip of `frames` frames
static inline const char* nr_region_fault(int first, int count, int frames) {
  if (count == 0) return nullptr;  // auto
  if (count < TT_NR_MIN_REGION) return "a noise region needs at least TT_NR_MIN_REGION = 8 frames";
  if (first < 0 || first > frames - count) return "the noise region is not inside the clip";
  return nullptr;
}

// nullptr, or what is wrong with the parameters
static inline const char* nr_params_fault(const tt_nr_params& p) {
  if (p.quantile_num < TT_NR_QUANTILE_DEN / 100 || p.quantile_num > TT_NR_QUANTILE_DEN / 2) return "quantile_num outside 100 .. 5000 (q = 0.01 .. 0.5)";
  if (!(p.quantile_scale > 0.f) || !isfinite(p.quantile_scale)) return "quantile_scale must be finite and positive";
  if (!(p.beta >= 1.f && p.beta <= 4.f)) return "beta outside 1 .. 4";
  if (!(p.g_min >= 0.01f && p.g_min < 1.f)) return "g_min outside 0.01 .. 1 (reduction_db 0 < .. 40)";
  if (p.smooth_frames < 0 || p.smooth_frames > TT_NR_MAX_SMOOTH) return "smooth_frames outside 0 .. 4";
  if (p.smooth_bins < 0 || p.smooth_bins > TT_NR_MAX_SMOOTH) return "smooth_bins outside 0 .. 4";
  return nullptr;
}

}  // namespace tt
