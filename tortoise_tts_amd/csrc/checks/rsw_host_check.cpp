// Stand-alone check of the pitch map's host code (resample_warp_host.h): the one-segment table against the constant ratio's integers, random
// plans against the table's rules and 0 <= t_i - 65536 b_i < P_(i-1), the positions (monotone, inside the clip's reach), every refusal of
// the plan and of the table, the 64-bit edges (the longest clip, P at both ends, 64 segments of 2 samples) and the argument checks - no
// device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all rsw_host_check.cpp -o rsw_host_check && ./rsw_host_check
// Exit status 0 and "rsw_host_check: ok" when everything holds.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../resample_warp_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

int main() {
  const int ratios[] = {32768, 32769, 40000, 55109, 65535, 65536, 65537, 77936, 100000, 131071, 131072};
  char err[256];
  unsigned seed = 13579;
  auto rnd = [&](int k) {
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (unsigned)k);
  };

  // one segment (0, 0, 0, P) is the constant ratio: n_out, and every (index, phase)
  for (int P : ratios)
    for (int n : {1, 2, 37, 1000, 5000, 100001, TT_RS_MAX_SAMPLES}) {
      const int starts[1] = {0}, ps[1] = {P};
      int tab[4] = {-1, -1, -1, -1};
      if (n < TT_RSW_MIN_SEGMENT) {  // (a planned segment covers 2 samples; the table itself is fine)
        CHECK(rsw_plan(n, 1, starts, ps, tab, err, sizeof(err)) == -1 && strstr(err, "at least 2 samples") && tab[0] == -1);
        tab[0] = tab[1] = tab[2] = 0; tab[3] = P;
      } else {
        CHECK(rsw_plan(n, 1, starts, ps, tab, err, sizeof(err)) == 0 && tab[0] == 0 && tab[1] == 0 && tab[2] == 0 && tab[3] == P);
      }
      const int n_out = rsw_out_samples(n, 1, tab);
      CHECK(n_out == rs_out_samples(n, P, TT_RS_PITCH_ONE));
      for (int m : {0, std::min(1, n_out - 1), n_out / 2, n_out - 1}) {
        const long long pos = rsw_position(m, 0, 0, P);
        CHECK(pos >> 16 == (long long)m * P / TT_RS_PITCH_ONE && (pos & 65535) == (long long)m * P % TT_RS_PITCH_ONE && pos >> 16 < n);
      }
    }

  // random plans: the table obeys its own rules, 0 <= t_i - 65536 b_i < P_(i-1), the position is monotone and the last output reads inside the clip
  long plans = 0;
  long long worst = 0;
  for (int round = 0; round < 20000; ++round) {
    const int S = 1 + rnd(TT_RSW_MAX_SEGMENTS);
    const int n = std::max(2 * S + rnd(8), 2 + rnd(3998));
    std::vector<int> cut;  // S - 1 borders in 2 .. n - 2 with gaps of at least 2: distinct v_1 < .. in 1 .. n - 1 - S, b_i = v_i + i
    {
      std::vector<int> slots;
      for (int v = 1; v <= n - 1 - S; ++v) slots.push_back(v);
      CHECK((int)slots.size() >= S - 1);
      for (int i = 0; i < S - 1; ++i) std::swap(slots[(size_t)i], slots[(size_t)(i + rnd((int)slots.size() - i))]);
      cut.assign(slots.begin(), slots.begin() + (S - 1));
      std::sort(cut.begin(), cut.end());
      for (int i = 0; i < S - 1; ++i) cut[(size_t)i] += i + 1;
    }
    std::vector<int> starts(1, 0), ps, tab((size_t)(4 * S), -1);
    starts.insert(starts.end(), cut.begin(), cut.end());
    for (int i = 0; i < S; ++i) ps.push_back(rnd(4) == 0 ? (rnd(2) ? TT_RSW_P_MIN : TT_RSW_P_MAX) : TT_RSW_P_MIN + rnd(TT_RSW_P_MAX - TT_RSW_P_MIN + 1));
    CHECK(rsw_plan(n, S, starts.data(), ps.data(), tab.data(), err, sizeof(err)) == 0);
    for (int i = 0; i < S; ++i) {
      const long long over = rsw_t(tab.data(), i) - (long long)starts[(size_t)i] * 65536;
      CHECK(rsw_p(tab.data(), i) == ps[(size_t)i] && over >= 0 && over < (i ? ps[(size_t)(i - 1)] : 1));
      CHECK(tab[(size_t)(4 * i + 2)] >= 0 && tab[(size_t)(4 * i + 2)] < 65536);
      worst = std::max(worst, over);
    }
    const int n_out = rsw_out_samples(n, S, tab.data());
    CHECK(n_out >= rsw_m(tab.data(), S - 1) + 1);
    CHECK(n_out >= n / 2 && n_out <= 2 * n + 1);
    int cur = 0;
    long long prev = -1;
    for (int m = 0; m < n_out; ++m) {
      while (cur + 1 < S && m >= rsw_m(tab.data(), cur + 1)) ++cur;  // the kernel's forward step
      const long long pos = rsw_position(m, rsw_m(tab.data(), cur), rsw_t(tab.data(), cur), rsw_p(tab.data(), cur));
      CHECK(pos > prev && pos >> 16 < n);
      prev = pos;
    }
    CHECK(prev + rsw_p(tab.data(), S - 1) >= (long long)n * 65536);  // one more output would start at or beyond the end
    ++plans;
  }
  CHECK(worst < TT_RSW_P_MAX);

  // the 64-bit edges: the longest clip with P at both ends, 64 segments of 2 samples, and a long clip whose borders sit at its end
  for (int P : {TT_RSW_P_MIN, TT_RSW_P_MAX}) {
    const int n = TT_RS_MAX_SAMPLES;
    int starts[64], ps[64], tab[256];
    for (int i = 0; i < 64; ++i) { starts[i] = i ? n - 2 * (64 - i) : 0; ps[i] = i % 2 ? P : TT_RSW_P_MIN + TT_RSW_P_MAX - P; }
    CHECK(rsw_plan(n, 64, starts, ps, tab, err, sizeof(err)) == 0);
    const int n_out = rsw_out_samples(n, 64, tab);
    CHECK(n_out > 0 && rsw_t(tab, 63) < (long long)n * 65536 && rsw_t(tab, 63) >= (long long)(n - 2) * 65536 && tab[4 * 63 + 1] >= n - 2);
    const long long last = rsw_position(n_out - 1, rsw_m(tab, 63), rsw_t(tab, 63), rsw_p(tab, 63));
    CHECK(last >> 16 < n && last + rsw_p(tab, 63) >= (long long)n * 65536);
    const int one[1] = {0}, p1[1] = {P};
    CHECK(rsw_plan(n, 1, one, p1, tab, err, sizeof(err)) == 0 && rsw_out_samples(n, 1, tab) == (int)(((long long)n * 65536 + P - 1) / P));
    for (int i = 0; i < 64; ++i) { starts[i] = 2 * i; ps[i] = P; }
    CHECK(rsw_plan(128, 64, starts, ps, tab, err, sizeof(err)) == 0 && rsw_out_samples(128, 64, tab) == 128 * 65536 / P);
  }

  // refusals of the plan: nothing is written
  {
    int tab[4 * 66];
    std::fill(tab, tab + 4 * 66, -7);
    std::vector<int> many(66), ok_ps(66, 65536);
    for (int i = 0; i < 66; ++i) many[(size_t)i] = 2 * i;
    struct Bad { int n, S; int starts[3]; int ps[3]; const char* what; };
    const Bad bad[] = {
        {0, 1, {0, 0, 0}, {65536, 65536, 65536}, "a clip of 0 samples"},
        {TT_RS_MAX_SAMPLES + 1, 1, {0, 0, 0}, {65536, 65536, 65536}, "samples (1 .."},
        {100, 0, {0, 0, 0}, {65536, 65536, 65536}, "0 segments"},
        {100, 2, {1, 50, 0}, {65536, 65536, 65536}, "not at 0"},
        {100, 2, {0, 1, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 2, {0, 99, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 3, {0, 60, 40}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 3, {0, 40, 40}, {65536, 65536, 65536}, "at least 2 samples"},
        {1, 1, {0, 0, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 2, {0, 50, 0}, {65536, 32767, 65536}, "segment 1: ratio 32767"},
        {100, 2, {0, 50, 0}, {131073, 65536, 65536}, "segment 0: ratio 131073"},
        {100, 1, {0, 0, 0}, {0, 65536, 65536}, "ratio 0"},
        {100, 1, {0, 0, 0}, {-65536, 65536, 65536}, "ratio -65536"},
    };
    for (const Bad& b : bad) {
      CHECK(rsw_plan(b.n, b.S, b.starts, b.ps, tab, err, sizeof(err)) == -1 && strstr(err, b.what));
      CHECK(std::all_of(tab, tab + 4 * 66, [](int v) { return v == -7; }));
    }
    CHECK(rsw_plan(1000, 65, many.data(), ok_ps.data(), tab, err, sizeof(err)) == -1 && strstr(err, "65 segments (1 .. 64)") && tab[0] == -7);
    CHECK(rsw_plan(100, 1, nullptr, ok_ps.data(), tab, err, sizeof(err)) == -1 && strstr(err, "null argument"));
    CHECK(rsw_plan(100, 1, many.data(), nullptr, tab, err, sizeof(err)) == -1 && rsw_plan(100, 1, many.data(), ok_ps.data(), nullptr, err, sizeof(err)) == -1);
    CHECK(rsw_plan(1000, 64, many.data(), ok_ps.data(), tab, err, sizeof(err)) == 0 && rsw_out_samples(1000, 64, tab) == 1000);  // 64 is fine
    CHECK(rsw_plan(4, 2, many.data(), ok_ps.data(), tab, err, sizeof(err)) == 0 && rsw_out_samples(4, 2, tab) == 4);
  }

  // refusals of the table
  {
    const int starts[3] = {0, 1000, 1700}, ps[3] = {81920, 52429, 131072};
    int good[12];
    CHECK(rsw_plan(3000, 3, starts, ps, good, err, sizeof(err)) == 0);
    const int n_out = rsw_out_samples(3000, 3, good);
    CHECK(n_out == good[8] + (int)((3000ll * 65536 - rsw_t(good, 2) + 131071) / 131072));
    auto with = [&](int at, int v) {
      std::vector<int> tb(good, good + 12);
      tb[(size_t)at] = v;
      return tb;
    };
    for (int at : {0, 1, 2}) CHECK(rsw_out_samples(3000, 3, with(at, 1).data()) == 0);                                  // the start is (0, 0, 0)
    CHECK(rsw_out_samples(3000, 3, with(4, 0).data()) == 0 && rsw_out_samples(3000, 3, with(8, good[4]).data()) == 0);  // m increases
    CHECK(rsw_out_samples(3000, 3, with(8, good[4] - 1).data()) == 0 && rsw_out_samples(3000, 3, with(4, -5).data()) == 0);
    for (int at : {5, 6, 9, 10})
      for (int by : {-1, 1}) CHECK(rsw_out_samples(3000, 3, with(at, good[at] + by).data()) == 0);  // continuity, broken by one unit
    for (int at : {6, 10})
      for (int v : {-1, 65536, good[at] + 65536, good[at] - 65536, INT_MAX, INT_MIN}) CHECK(rsw_out_samples(3000, 3, with(at, v).data()) == 0);  // 0 <= tlo < 65536
    for (int at : {5, 9})
      for (int v : {-1, INT_MAX, INT_MIN}) CHECK(rsw_out_samples(3000, 3, with(at, v).data()) == 0);
    for (int at : {3, 7, 11})
      for (int v : {0, -1, 32767, 131073, INT_MAX, INT_MIN}) CHECK(rsw_out_samples(3000, 3, with(at, v).data()) == 0);
    CHECK(rsw_out_samples(good[9], 3, good) == 0 && rsw_out_samples(good[9] + 1, 3, good) == good[8] + 1);  // t_(S-1) < n 65536
    CHECK(rsw_out_samples(3000, 0, good) == 0 && rsw_out_samples(3000, 65, good) == 0 && rsw_out_samples(0, 3, good) == 0);
    CHECK(rsw_out_samples(TT_RS_MAX_SAMPLES + 1, 3, good) == 0 && rsw_out_samples(TT_RS_MAX_SAMPLES, 3, good) > 0);
    CHECK(rsw_out_samples(3000, 2, good) > 0 && rsw_out_samples(3000, 1, good) == rs_out_samples(3000, 81920, 65536));  // a prefix of a table is a table
    {  // entries that would overflow a careless product: the largest m and thi with a continuity that cannot hold
      int wild[8] = {0, 0, 0, 131072, INT_MAX, INT_MAX, 65535, 131072};
      CHECK(rsw_out_samples(3000, 2, wild) == 0);
    }
  }

  // the handle's and the call's arguments
  CHECK(rsw_check_create(1, 1, 1, err, sizeof(err)) == 0 && rsw_check_create(TT_RS_MAX_SAMPLES, TT_RS_MAX_CLIPS, TT_RSW_MAX_SEGMENTS, err, sizeof(err)) == 0);
  CHECK(rsw_check_create(0, 1, 1, err, sizeof(err)) == -1 && strstr(err, "max_samples 0"));
  CHECK(rsw_check_create(TT_RS_MAX_SAMPLES + 1, 1, 1, err, sizeof(err)) == -1 && rsw_check_create(1, 0, 1, err, sizeof(err)) == -1 && strstr(err, "max_clips 0"));
  CHECK(rsw_check_create(1, 65, 1, err, sizeof(err)) == -1 && rsw_check_create(1, 1, 0, err, sizeof(err)) == -1 && strstr(err, "max_segments 0"));
  CHECK(rsw_check_create(1, 1, 65, err, sizeof(err)) == -1 && strstr(err, "max_segments 65 (1 .. 64)"));
  CHECK(rsw_check_resample(true, 1, 16, err, sizeof(err)) == 0 && rsw_check_resample(true, 16, 16, err, sizeof(err)) == 0);
  CHECK(rsw_check_resample(false, 1, 16, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(rsw_check_resample(true, 0, 16, err, sizeof(err)) == -1 && rsw_check_resample(true, 17, 16, err, sizeof(err)) == -1 && strstr(err, "17 clips (1 .. 16)"));

  printf("rsw_host_check: ok (%ld random plans, worst t_i - 65536 b_i = %lld / 65536 samples)\n", plans, worst);
  return 0;
}
