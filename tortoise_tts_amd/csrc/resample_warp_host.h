// The integers of a pitch map (include/tortoise_mi355x_rsw.h): the table's rules, its positions and length, the plan from input-domain
// segments, and every argument check of tt_rsw_create / tt_rsw_resample that does not need the data.  Plain C++ with no device part, so
// that csrc/checks/rsw_host_check.cpp can run it under the host sanitizers; the table's rules and the position are host and device
// functions, so that the kernels of resample_warp.hip check and read a table with the very code the host plans it with.
#pragma once
#include <stdio.h>
#include "../../include/tortoise_mi355x_rsw.h"
#include "resample_steps.h"

namespace tt {

// a table is i32 [4 S]: (m_i, thi_i, tlo_i, P_i)
TT_RS_HD static inline int rsw_m(const int* tab, int i) { return tab[4 * i]; }
TT_RS_HD static inline long long rsw_t(const int* tab, int i) { return (long long)tab[4 * i + 1] * 65536 + tab[4 * i + 2]; }
TT_RS_HD static inline int rsw_p(const int* tab, int i) { return tab[4 * i + 3]; }
TT_RS_HD static inline bool rsw_ratio_ok(int P) { return P >= TT_RSW_P_MIN && P <= TT_RSW_P_MAX; }

// the input position (16.16) of output sample m inside the segment (m_i, t_i, P_i), m >= m_i: exact
TT_RS_HD static inline long long rsw_position(int m, int m_i, long long t_i, int P_i) { return t_i + ((long long)m - m_i) * P_i; }

// n_out of a clip of n samples along the table, or 0 when the table breaks a rule: (0, 0) start, 0 <= tlo < 65536, m strictly increasing,
// ratios in range, continuity, t_(S-1) < n 65536.  With these every t_i < 2^39 and, as a step of one output advances by at least 32768,
// m_(S-1) <= t_(S-1) / 32768 < 2 n, so that n_out < 4 n + 1 fits 32 bits for n <= 2^23.  No product below leaves 64 bits for ANY i32
// entries: |m difference| < 2^32 and P <= 2^17 are checked before they are multiplied.
// The rules fall into one test per row and one of the table's end, so that the kernels check the rows of a table side by side, one thread
// each, and the host in a loop - with the same two functions.
TT_RS_HD static inline bool rsw_row_ok(int S, const int* tab, int i) {  // row i < S: its own entries, and its step to row i + 1
  if (i == 0 && (rsw_m(tab, 0) != 0 || tab[1] != 0 || tab[2] != 0)) return false;
  if (!rsw_ratio_ok(rsw_p(tab, i)) || tab[4 * i + 1] < 0 || tab[4 * i + 2] < 0 || tab[4 * i + 2] > 65535) return false;
  if (i + 1 < S) {
    if (rsw_m(tab, i + 1) <= rsw_m(tab, i)) return false;
    if (rsw_position(rsw_m(tab, i + 1), rsw_m(tab, i), rsw_t(tab, i), rsw_p(tab, i)) != rsw_t(tab, i + 1)) return false;
  }
  return true;
}
TT_RS_HD static inline int rsw_tail(int n, int S, const int* tab) {  // n_out of a table whose every row is ok, or 0: t_(S-1) >= n 65536
  const long long t = rsw_t(tab, S - 1), end = (long long)n * 65536;
  const int P = rsw_p(tab, S - 1);
  if (t >= end) return 0;
  return (int)(rsw_m(tab, S - 1) + (end - t + P - 1) / P);
}
TT_RS_HD static inline bool rsw_sizes_ok(int n, int S) { return n >= 1 && n <= TT_RS_MAX_SAMPLES && S >= 1 && S <= TT_RSW_MAX_SEGMENTS; }
TT_RS_HD static inline int rsw_out_samples(int n, int S, const int* tab) {
  if (!rsw_sizes_ok(n, S)) return 0;
  for (int i = 0; i < S; ++i)
    if (!rsw_row_ok(S, tab, i)) return 0;
  return rsw_tail(n, S, tab);
}

static inline int rsw_fail(char* err, size_t n, const char* fmt, int a, int b, int c) {
  snprintf(err, n, fmt, a, b, c);
  return -1;
}

// The plan from input-domain segments: starts b_0 .. b_(S-1) (b_S = n) and their ratios -> the table.  0, or -1 with a message in err and
// nothing written.
static inline int rsw_plan(int n, int S, const int* starts, const int* ps, int* tab, char* err, size_t en) {
  if (!starts || !ps || !tab) return rsw_fail(err, en, "tt_rsw_plan: null argument", 0, 0, 0);
  if (n < 1 || n > TT_RS_MAX_SAMPLES) return rsw_fail(err, en, "tt_rsw_plan: a clip of %d samples (1 .. %d)", n, TT_RS_MAX_SAMPLES, 0);
  if (S < 1 || S > TT_RSW_MAX_SEGMENTS) return rsw_fail(err, en, "tt_rsw_plan: %d segments (1 .. %d)", S, TT_RSW_MAX_SEGMENTS, 0);
  if (starts[0] != 0) return rsw_fail(err, en, "tt_rsw_plan: segment 0 starts at sample %d, not at 0", starts[0], 0, 0);
  for (int i = 0; i < S; ++i) {
    const long long end = i + 1 < S ? starts[i + 1] : n;
    if (end - starts[i] < TT_RSW_MIN_SEGMENT)
      return rsw_fail(err, en, "tt_rsw_plan: segment %d starts at sample %d and ends at %d: the starts increase, and a segment covers at least 2 samples",
                      i, starts[i], (int)end);
    if (!rsw_ratio_ok(ps[i])) return rsw_fail(err, en, "tt_rsw_plan: segment %d: ratio %d / 65536 is outside %d .. 131072", i, ps[i], TT_RSW_P_MIN);
  }
  int m = 0;
  long long t = 0;
  for (int i = 0; i < S; ++i) {
    tab[4 * i] = m; tab[4 * i + 1] = (int)(t >> 16); tab[4 * i + 2] = (int)(t & 65535); tab[4 * i + 3] = ps[i];
    if (i + 1 < S) {
      long long L = ((long long)starts[i + 1] * 65536 - t + ps[i] - 1) / ps[i];  // (the numerator is positive: t < (b_i + 2) 65536 <= b_(i+1) 65536)
      if (L < 1) L = 1;
      m += (int)L;
      t += L * ps[i];
    }
  }
  return 0;
}

static inline int rsw_check_create(int max_samples, int max_clips, int max_segments, char* err, size_t en) {
  if (max_samples < 1 || max_samples > TT_RS_MAX_SAMPLES) return rsw_fail(err, en, "tt_rsw_create: max_samples %d (1 .. %d)", max_samples, TT_RS_MAX_SAMPLES, 0);
  if (max_clips < 1 || max_clips > TT_RS_MAX_CLIPS) return rsw_fail(err, en, "tt_rsw_create: max_clips %d (1 .. %d)", max_clips, TT_RS_MAX_CLIPS, 0);
  if (max_segments < 1 || max_segments > TT_RSW_MAX_SEGMENTS)
    return rsw_fail(err, en, "tt_rsw_create: max_segments %d (1 .. %d)", max_segments, TT_RSW_MAX_SEGMENTS, 0);
  return 0;
}

static inline int rsw_check_resample(bool pointers, int n_clips, int max_clips, char* err, size_t en) {
  if (!pointers) return rsw_fail(err, en, "tt_rsw_resample: null argument", 0, 0, 0);
  if (n_clips < 1 || n_clips > max_clips) return rsw_fail(err, en, "tt_rsw_resample: %d clips (1 .. %d)", n_clips, max_clips, 0);
  return 0;
}

}  // namespace tt
