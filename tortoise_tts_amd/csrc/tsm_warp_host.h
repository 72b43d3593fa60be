// The integers of a rate map (include/tortoise_mi355x_tsw.h): the table's rules, its nominal positions and lengths, the plan from
// input-domain segments, and every argument check of tt_tsw_create / tt_tsw_stretch that does not need the data.  Plain C++ with no
// device part, so that csrc/checks/tsw_host_check.cpp can run it under the host sanitizers; the table's rules and the nominal position are
// host and device functions, so that the kernel of tsm_warp.hip checks and reads a table with the very code the host plans it with.
#pragma once
#include <stdio.h>
#include "../../include/tortoise_mi355x_tsw.h"
#include "tsm_steps.h"

namespace tt {

// a table is i32 [3 S]: (m_i, a_i, rq_i)
TT_TSM_HD static inline int tsw_m(const int* tab, int i) { return tab[3 * i]; }
TT_TSM_HD static inline int tsw_a(const int* tab, int i) { return tab[3 * i + 1]; }
TT_TSM_HD static inline int tsw_rq(const int* tab, int i) { return tab[3 * i + 2]; }

// the input advance of `len` output samples at rate rq (continuity, and the nominal position within a segment)
TT_TSM_HD static inline long long tsw_advance(long long len, int rq) { return (len * rq + 32768) >> 16; }

// a_k of an output sample m = (k - 1) Hs inside the segment (m_i, a_i, rq_i), m >= m_i
TT_TSM_HD static inline int tsw_position(int m, int m_i, int a_i, int rq_i) { return a_i + (int)tsw_advance((long long)m - m_i, rq_i); }

// n_out of a clip of n samples along the table, or 0 when the table breaks a rule: (0, 0) start, m strictly increasing, rates in range,
// continuity, a_(S-1) < n.  With these, a_i is strictly increasing too (every step advances by at least (32768 + 32768) >> 16 = 1) and
// m_(S-1) < 2 n + S (a step of L outputs advances by at least (L - 1) / 2), so that n_out and every a_k fit 32 bits for n <= 2^23.
TT_TSM_HD static inline int tsw_out_samples(int n, int S, const int* tab) {
  if (n < 1 || n > TT_TSM_MAX_SAMPLES || S < 1 || S > TT_TSW_MAX_SEGMENTS) return 0;
  if (tsw_m(tab, 0) != 0 || tsw_a(tab, 0) != 0) return 0;
  for (int i = 0; i < S; ++i) {
    if (!tsm_rate_ok(tsw_rq(tab, i))) return 0;
    if (i + 1 < S) {
      if (tsw_m(tab, i + 1) <= tsw_m(tab, i)) return 0;
      if (tsw_a(tab, i) + tsw_advance((long long)tsw_m(tab, i + 1) - tsw_m(tab, i), tsw_rq(tab, i)) != tsw_a(tab, i + 1)) return 0;
    }
  }
  const int a = tsw_a(tab, S - 1), rq = tsw_rq(tab, S - 1);
  if (a >= n) return 0;
  const long long tail = ((long long)(n - a) * TT_TSM_RATE_ONE + rq / 2) / rq;
  return (int)(tsw_m(tab, S - 1) + (tail < 1 ? 1 : tail));
}
TT_TSM_HD static inline int tsw_frames(int n, int S, const int* tab) {
  const int n_out = tsw_out_samples(n, S, tab);
  return n_out ? tsm_frames(n_out) : 0;
}

// a_k of frame k >= 1 by a search from the table's start (the kernel keeps a cursor instead: the segment only moves forward)
static inline int tsw_nominal(int k, int S, const int* tab) {
  const int m = (k - 1) * kTsmHs;
  int i = 0;
  while (i + 1 < S && tsw_m(tab, i + 1) <= m) ++i;
  return tsw_position(m, tsw_m(tab, i), tsw_a(tab, i), tsw_rq(tab, i));
}

static inline int tsw_fail(char* err, size_t n, const char* fmt, int a, int b, int c) {
  snprintf(err, n, fmt, a, b, c);
  return -1;
}

// The plan from input-domain segments: starts b_0 .. b_(S-1) (b_S = n) and their rates -> the table.  0, or -1 with a message in err and
// nothing written.
static inline int tsw_plan(int n, int S, const int* starts, const int* rqs, int* tab, char* err, size_t en) {
  if (!starts || !rqs || !tab) return tsw_fail(err, en, "tt_tsw_plan: null argument", 0, 0, 0);
  if (n < 1 || n > TT_TSM_MAX_SAMPLES) return tsw_fail(err, en, "tt_tsw_plan: a clip of %d samples (1 .. %d)", n, TT_TSM_MAX_SAMPLES, 0);
  if (S < 1 || S > TT_TSW_MAX_SEGMENTS) return tsw_fail(err, en, "tt_tsw_plan: %d segments (1 .. %d)", S, TT_TSW_MAX_SEGMENTS, 0);
  if (starts[0] != 0) return tsw_fail(err, en, "tt_tsw_plan: segment 0 starts at sample %d, not at 0", starts[0], 0, 0);
  for (int i = 0; i < S; ++i) {
    const long long end = i + 1 < S ? starts[i + 1] : n;
    if (end - starts[i] < TT_TSW_MIN_SEGMENT)
      return tsw_fail(err, en, "tt_tsw_plan: segment %d starts at sample %d and ends at %d: the starts increase, and a segment covers at least 2 samples",
                      i, starts[i], (int)end);
    if (!tsm_rate_ok(rqs[i])) return tsw_fail(err, en, "tt_tsw_plan: segment %d: rate %d / 65536 is outside %d .. 131072", i, rqs[i], TT_TSM_RATE_MIN);
  }
  int m = 0, a = 0;
  for (int i = 0; i < S; ++i) {
    tab[3 * i] = m; tab[3 * i + 1] = a; tab[3 * i + 2] = rqs[i];
    if (i + 1 < S) {
      long long L = ((long long)(starts[i + 1] - a) * TT_TSM_RATE_ONE + rqs[i] / 2) / rqs[i];  // (starts[i + 1] - a >= 1: |a - b_i| <= 1)
      if (L < 1) L = 1;
      m += (int)L;
      a += (int)tsw_advance(L, rqs[i]);
    }
  }
  return 0;
}

static inline int tsw_check_create(int max_samples, int max_clips, int max_segments, char* err, size_t en) {
  if (max_samples < 1 || max_samples > TT_TSM_MAX_SAMPLES) return tsw_fail(err, en, "tt_tsw_create: max_samples %d (1 .. %d)", max_samples, TT_TSM_MAX_SAMPLES, 0);
  if (max_clips < 1 || max_clips > TT_TSM_MAX_CLIPS) return tsw_fail(err, en, "tt_tsw_create: max_clips %d (1 .. %d)", max_clips, TT_TSM_MAX_CLIPS, 0);
  if (max_segments < 1 || max_segments > TT_TSW_MAX_SEGMENTS)
    return tsw_fail(err, en, "tt_tsw_create: max_segments %d (1 .. %d)", max_segments, TT_TSW_MAX_SEGMENTS, 0);
  return 0;
}

static inline int tsw_check_stretch(bool pointers, int n_clips, int max_clips, char* err, size_t en) {
  if (!pointers) return tsw_fail(err, en, "tt_tsw_stretch: null argument", 0, 0, 0);
  if (n_clips < 1 || n_clips > max_clips) return tsw_fail(err, en, "tt_tsw_stretch: %d clips (1 .. %d)", n_clips, max_clips, 0);
  return 0;
}

}  // namespace tt
