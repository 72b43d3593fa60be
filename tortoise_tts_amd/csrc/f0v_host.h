// The rules and the cost arithmetic of the Viterbi F0 path (include/tortoise_mi355x_f0v.h): the per-clip checks the kernels make, every
// argument check of tt_f0v_create / tt_f0v_track that does not need the data, the local and transition costs, and a plain C++ run of the
// recursion.  No device part is needed to compile it, so csrc/checks/f0v_host_check.cpp runs it under the host sanitizers; the status
// rules and the costs are host and device functions, so that f0_viterbi.hip refuses a clip and prices a step with the very code checked there.
#pragma once
#include <math.h>
#include <stdio.h>
#include "f0_host.h"
#include "../../include/tortoise_mi355x_f0v.h"

namespace tt {

constexpr int kF0vS = TT_F0V_STATES, kF0vU = TT_F0V_UNVOICED;

// every cost is one rounded f64 operation: never contracted into an FMA, on either side
TT_F0_HD static inline double f0v_add(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  const double r = a + b;
  return r;
#endif
}
TT_F0_HD static inline double f0v_mul(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  const double r = a * b;
  return r;
#endif
}

struct F0vCost {
  double oct, jump, vuv, uv;
};

// non-negative and finite (NaN fails every comparison)
TT_F0_HD static inline bool f0v_cost_ok(const F0vCost& k) {
  return k.oct >= 0.0 && k.oct <= 1.7e308 && k.jump >= 0.0 && k.jump <= 1.7e308 && k.vuv >= 0.0 && k.vuv <= 1.7e308 && k.uv >= 0.0 && k.uv <= 1.7e308;
}

// a voiced slot holds a candidate iff its lag is one of the table's, 1 .. T (0 is "absent"; anything else is read as absent too)
TT_F0_HD static inline bool f0v_present(int lag) { return lag >= 1 && lag <= TT_F0_LAG_MAX; }

// local(t, s): l2 = L2[lag] of a voiced state, l2lo = L2[lo]
TT_F0_HD static inline double f0v_local(int s, double dp, double l2, double l2lo, const F0vCost& k) {
  return s == kF0vU ? k.uv : f0v_add(dp, f0v_mul(k.oct, f0v_add(l2, -l2lo)));
}
// trans(j -> s): l2j, l2s = L2 of the two lags where the states are voiced
TT_F0_HD static inline double f0v_trans(int j, int s, double l2j, double l2s, const F0vCost& k) {
  if (j == kF0vU && s == kF0vU) return 0.0;
  if (j == kF0vU || s == kF0vU) return k.vuv;
  return f0v_mul(k.jump, fabs(f0v_add(l2s, -l2j)));
}

// tt_f0's status of a clip, and REFUSED for a cost out of range
TT_F0_HD static inline int f0v_clip_status(int i0, int i1, int max_samples, int lo, int hi, double thr, double floor_e, const F0vCost& k, int fo0,
                                           int fo1) {
  const int st = f0_clip_status(i0, i1, max_samples, lo, hi, thr, floor_e, fo0, fo1);
  return st == TT_F0_OK && !f0v_cost_ok(k) ? TT_F0_REFUSED : st;
}
// the status of a clip of F frames whose candidate tables the caller gives (tt_op_f0v_path)
TT_F0_HD static inline int f0v_path_status(int F, int max_frames, int lo, int hi, const F0vCost& k, int fo0, int fo1) {
  if (F < 0) return TT_F0_REFUSED;
  if (F == 0) return TT_F0_EMPTY;
  if (F > max_frames || !f0_lags_ok(lo, hi) || !f0v_cost_ok(k)) return TT_F0_REFUSED;
  if (fo0 < 0 || (long long)fo1 - fo0 < F) return TT_F0_REFUSED;
  return TT_F0_OK;
}

static inline bool f0v_table_ok(const double* L2) {
  for (int tau = 1; tau < TT_F0V_TABLE; ++tau)
    if (!(L2[tau] >= (tau > 1 ? L2[tau - 1] : -1.7e308) && L2[tau] <= 1.7e308)) return false;
  return true;
}

static inline int f0v_check_create(bool have_out, const double* L2, int max_samples, int max_clips, char* err, size_t en) {
  if (!have_out || !L2) return f0_fail(err, en, "tt_f0v_create: null argument", 0, 0);
  if (max_samples < 1 || max_samples > TT_F0_MAX_SAMPLES) return f0_fail(err, en, "tt_f0v_create: max_samples %d (1 .. %d)", max_samples, TT_F0_MAX_SAMPLES);
  if (max_clips < 1 || max_clips > TT_F0_MAX_CLIPS) return f0_fail(err, en, "tt_f0v_create: max_clips %d (1 .. %d)", max_clips, TT_F0_MAX_CLIPS);
  if (!f0v_table_ok(L2)) return f0_fail(err, en, "tt_f0v_create: the log2 table is not finite and non-decreasing over 1 .. %d", TT_F0_LAG_MAX, 0);
  return 0;
}

static inline int f0v_check_track(bool have_all, int n_clips, int max_clips, char* err, size_t en) {
  if (!have_all) return f0_fail(err, en, "tt_f0v_track: null argument", 0, 0);
  if (n_clips < 1 || n_clips > max_clips) return f0_fail(err, en, "tt_f0v_track: %d clips (1 .. %d)", n_clips, max_clips);
  return 0;
}

// The recursion of the header on the candidate tables of one clip: lag i32 [F][8] (f0v_present; slot 7 is not looked at), dp f64 [F][8],
// L2 the log2 table -> state [F] and the path's cost; false (nothing written) for F < 1.  Plain C++, one frame after the other.
static inline bool f0v_viterbi_host(int F, const int* lag, const double* dp, int lo, const double* L2, const F0vCost& k, int* state, double* cost) {
  if (F < 1 || !lag || !dp || !L2 || !state || !cost) return false;
  unsigned char* bp = new unsigned char[(size_t)F * kF0vS];
  double a[kF0vS], b[kF0vS];
  auto present = [&](int t, int s) { return s == kF0vU || f0v_present(lag[(size_t)t * kF0vS + s]); };
  auto l2 = [&](int t, int s) { return s == kF0vU ? 0.0 : L2[lag[(size_t)t * kF0vS + s]]; };
  for (int s = 0; s < kF0vS; ++s) {
    a[s] = present(0, s) ? f0v_local(s, dp[s], l2(0, s), L2[lo], k) : INFINITY;
    bp[s] = 0;
  }
  for (int t = 1; t < F; ++t) {
    for (int s = 0; s < kF0vS; ++s) {
      double best = INFINITY;
      int arg = 0;
      bool any = false;
      for (int j = 0; j < kF0vS; ++j) {
        if (!present(t - 1, j)) continue;
        const double v = f0v_add(a[j], present(t, s) ? f0v_trans(j, s, l2(t - 1, j), l2(t, s), k) : 0.0);
        if (!any || v < best) best = v, arg = j, any = true;
      }
      b[s] = present(t, s) ? f0v_add(f0v_local(s, dp[(size_t)t * kF0vS + s], l2(t, s), L2[lo], k), best) : INFINITY;
      bp[(size_t)t * kF0vS + s] = (unsigned char)arg;
    }
    for (int s = 0; s < kF0vS; ++s) a[s] = b[s];
  }
  int end = 0;
  for (int s = 1; s < kF0vS; ++s)
    if (a[s] < a[end]) end = s;
  *cost = a[end];
  for (int t = F - 1; t >= 0; --t) {
    state[t] = end;
    end = bp[(size_t)t * kF0vS + end];
  }
  delete[] bp;
  return true;
}

}  // namespace tt
