// Stand-alone check of the denoiser's host code (denoise_host.h): the rank of the order statistic and the frames of a noise region against
// brute force from their definitions, the bisection select against a sort (ties, zeros, all-ones patterns, padding), and the status and
// parameter checks.  Its own main, no device, no library:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all nr_host_check.cpp -o nr_host_check && ./nr_host_check
// Exit status 0 and "nr_host_check: ok" when everything holds.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../denoise_host.h"

using namespace tt;

#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "nr_host_check: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 32);
}

int main() {
  long ranks = 0, regions = 0, selects = 0;
  // k = floor(q (T - 1)): the largest k with k DEN <= num (T - 1)
  for (int num : {0, 1, 100, 101, 1999, 2000, 2001, 3333, 4999, 5000, 9999, 10000})
    for (int T = 1; T <= 3000; T += (T < 80 ? 1 : 37)) {
      const int k = nr_rank(num, T);
      EXPECT(k >= 0 && k <= T - 1);
      EXPECT((long long)k * TT_NR_QUANTILE_DEN <= (long long)num * (T - 1) && (long long)(k + 1) * TT_NR_QUANTILE_DEN > (long long)num * (T - 1));
      ++ranks;
    }
  EXPECT(nr_rank(2000, 1) == 0 && nr_rank(2000, 6) == 1 && nr_rank(5000, 1025) == 512 && nr_rank(100, 16385) == 163);
  EXPECT(nr_rank(-1, 5) == -1 && nr_rank(10001, 5) == -1 && nr_rank(2000, 0) == -1);
  EXPECT(nr_rank(TT_NR_QUANTILE_DEN, 1 + TT_NR_MAX_SAMPLES / 8) == TT_NR_MAX_SAMPLES / 8);  // no overflow at the largest clip and the smallest hop

  // the frames of a region against enumeration
  for (int hop : {8, 256, 300})
    for (int frames : {1, 7, 8, 9, 40})
      for (long long start = 0; start <= 11LL * hop; start += (hop > 8 ? hop / 4 - 1 : 1))
        for (long long end = start; end <= 45LL * hop; end += (hop > 8 ? hop / 3 + 1 : 3)) {
          int first = -7, count = -7, want_first = frames, want = 0;
          EXPECT(nr_region(start, end, hop, frames, &first, &count) == 0);
          for (int t = frames - 1; t >= 0; --t)
            if (start <= (long long)t * hop && (long long)t * hop + hop <= end) { want_first = t; ++want; }
          EXPECT(count == want && (want == 0 || first == want_first) && first >= 0 && first <= frames && first + count <= frames);
          ++regions;
        }
  int f, c;
  EXPECT(nr_region(-1, 5, 8, 4, &f, &c) == -1 && nr_region(6, 5, 8, 4, &f, &c) == -1 && nr_region(0, 5, 0, 4, &f, &c) == -1 &&
         nr_region(0, 5, 8, 0, &f, &c) == -1 && nr_region(0, 5, 8, 4, nullptr, &c) == -1 && nr_region(0, 5, 8, 4, &f, nullptr) == -1);
  EXPECT(nr_region(0, 9223372036854775807LL, 8, 100, &f, &c) == 0 && f == 0 && c == 100);
  EXPECT(nr_region(9223372036854775000LL, 9223372036854775807LL, 256, 100, &f, &c) == 0 && f == 100 && c == 0);

  // the bisection against a sort: the count is the only thing it sees
  for (int trial = 0; trial < 400; ++trial) {
    const int T = 1 + (int)(rnd() % 200);
    std::vector<unsigned> v(T);
    const int kind = trial % 5;
    for (int i = 0; i < T; ++i)
      v[i] = kind == 0 ? rnd() : kind == 1 ? rnd() % 4 : kind == 2 ? 0x3F800000u : kind == 3 ? (rnd() % 3 ? 0u : 0xFFFFFFFFu) : rnd() >> (rnd() % 32);
    std::vector<unsigned> padded(v);
    padded.resize(T + trial % 64, 0xFFFFFFFFu);  // the register form's padding never changes a rank below T
    std::vector<unsigned> sorted(v);
    std::sort(sorted.begin(), sorted.end());
    for (int k : {0, T / 5, T / 2, T - 1}) {
      const unsigned got = nr_bisect(k, [&](unsigned x) { int n = 0; for (unsigned u : padded) n += u < x; return n; });
      EXPECT(got == sorted[k]);
      ++selects;
    }
  }

  // status, regions and parameters
  EXPECT(nr_status(31, 0) == TT_NR_SHORT && nr_status(32, 0) == TT_NR_OK && nr_status(9, 8) == TT_NR_OK && nr_status(1, 0) == TT_NR_SHORT);
  EXPECT(!nr_region_fault(0, 0, 5) && !nr_region_fault(123, 0, 5) && nr_region_fault(0, 7, 40) && !nr_region_fault(0, 8, 40) && !nr_region_fault(32, 8, 40) &&
         nr_region_fault(33, 8, 40) && nr_region_fault(-1, 8, 40) && nr_region_fault(0, 41, 40) && nr_region_fault(0, 2147483647, 40) &&
         nr_region_fault(2147483647, 8, 40));
  const tt_nr_params ok = {2000, 4.4814f, 2.0f, 0.251189f, 2, 2};
  EXPECT(!nr_params_fault(ok));
  tt_nr_params p = ok; p.quantile_num = 99; EXPECT(nr_params_fault(p));
  p = ok; p.quantile_num = 5001; EXPECT(nr_params_fault(p));
  p = ok; p.quantile_num = 100; EXPECT(!nr_params_fault(p));
  p = ok; p.quantile_num = 5000; EXPECT(!nr_params_fault(p));
  p = ok; p.quantile_scale = 0.f; EXPECT(nr_params_fault(p));
  p = ok; p.quantile_scale = NAN; EXPECT(nr_params_fault(p));
  p = ok; p.quantile_scale = INFINITY; EXPECT(nr_params_fault(p));
  p = ok; p.beta = 0.99f; EXPECT(nr_params_fault(p));
  p = ok; p.beta = 4.01f; EXPECT(nr_params_fault(p));
  p = ok; p.beta = NAN; EXPECT(nr_params_fault(p));
  p = ok; p.g_min = 1.f; EXPECT(nr_params_fault(p));
  p = ok; p.g_min = 0.0099f; EXPECT(nr_params_fault(p));
  p = ok; p.g_min = 0.01f; EXPECT(!nr_params_fault(p));
  p = ok; p.g_min = NAN; EXPECT(nr_params_fault(p));
  p = ok; p.smooth_frames = -1; EXPECT(nr_params_fault(p));
  p = ok; p.smooth_frames = 5; EXPECT(nr_params_fault(p));
  p = ok; p.smooth_bins = -1; EXPECT(nr_params_fault(p));
  p = ok; p.smooth_bins = 5; EXPECT(nr_params_fault(p));
  p = ok; p.smooth_frames = 0; p.smooth_bins = 4; EXPECT(!nr_params_fault(p));
  printf("nr_host_check: ok (%ld ranks, %ld regions, %ld selects)\n", ranks, regions, selects);
  return 0;
}
