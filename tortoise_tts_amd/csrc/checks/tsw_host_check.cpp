// Stand-alone check of the rate map's host code (tsm_warp_host.h): the one-segment table against the constant rate's integers, random plans
// against the table's rules and |a_i - b_i| <= 1, the nominal positions (monotone, and the cursor against the search from the start), the
// lengths, every refusal of the plan and of the table, and the argument checks - no device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tsw_host_check.cpp -o tsw_host_check && ./tsw_host_check
// Exit status 0 and "tsw_host_check: ok" when everything holds.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../tsm_warp_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

int main() {
  const int rates[] = {32768, 32769, 40000, 52429, 65535, 65536, 65537, 81920, 100000, 131071, 131072};
  char err[256];
  unsigned seed = 24680;
  auto rnd = [&](int k) {
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (unsigned)k);
  };

  // one segment (0, 0, rq) is the constant rate: n_out, K and every a_k
  for (int rq : rates)
    for (int n : {1, 2, 300, 767, 768, 769, 5000, 100001, TT_TSM_MAX_SAMPLES}) {
      const int starts[1] = {0}, rqs[1] = {rq};
      int tab[3] = {-1, -1, -1};
      if (n < TT_TSW_MIN_SEGMENT) {  // (a planned segment covers 2 samples; the table itself is fine)
        CHECK(tsw_plan(n, 1, starts, rqs, tab, err, sizeof(err)) == -1 && strstr(err, "at least 2 samples") && tab[0] == -1);
        tab[0] = tab[1] = 0; tab[2] = rq;
      } else {
        CHECK(tsw_plan(n, 1, starts, rqs, tab, err, sizeof(err)) == 0 && tab[0] == 0 && tab[1] == 0 && tab[2] == rq);
      }
      CHECK(tsw_out_samples(n, 1, tab) == tsm_out_samples(n, rq) && tsw_frames(n, 1, tab) == tsm_frames(tsm_out_samples(n, rq)));
      const int K = std::min(tsw_frames(n, 1, tab), 3000);
      for (int k = 1; k < K; ++k) CHECK(tsw_nominal(k, 1, tab) == tsm_nominal(k, rq));
    }

  // random plans: the table obeys its own rules, |a_i - b_i| <= 1, a_k does not decrease, the forward cursor is the search from the start
  long plans = 0, frames = 0;
  int worst = 0;
  for (int round = 0; round < 20000; ++round) {
    const int S = 1 + rnd(TT_TSW_MAX_SEGMENTS);
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
    std::vector<int> starts(1, 0), rqs, tab((size_t)(3 * S), -1);
    starts.insert(starts.end(), cut.begin(), cut.end());
    for (int i = 0; i < S; ++i) rqs.push_back(rnd(4) == 0 ? (rnd(2) ? TT_TSM_RATE_MIN : TT_TSM_RATE_MAX) : TT_TSM_RATE_MIN + rnd(TT_TSM_RATE_MAX - TT_TSM_RATE_MIN + 1));
    CHECK(tsw_plan(n, S, starts.data(), rqs.data(), tab.data(), err, sizeof(err)) == 0);
    for (int i = 0; i < S; ++i) {
      CHECK(std::abs(tsw_a(tab.data(), i) - starts[(size_t)i]) <= 1 && tsw_rq(tab.data(), i) == rqs[(size_t)i]);
      worst = std::max(worst, std::abs(tsw_a(tab.data(), i) - starts[(size_t)i]));
    }
    const int n_out = tsw_out_samples(n, S, tab.data()), K = tsw_frames(n, S, tab.data());
    CHECK(n_out >= tsw_m(tab.data(), S - 1) + 1 && K == tsm_frames(n_out));
    CHECK(n_out >= n / 2 - 3 * S && n_out <= 2 * n + 3 * S);  // (a rounding and a sample of offset per segment, at most)
    int cur = 0, prev = 0;
    for (int k = 1; k < K; ++k) {
      const int m = (k - 1) * kTsmHs;
      while (cur + 1 < S && m >= tsw_m(tab.data(), cur + 1)) ++cur;  // the kernel's cursor
      const int a = tsw_position(m, tsw_m(tab.data(), cur), tsw_a(tab.data(), cur), tsw_rq(tab.data(), cur));
      CHECK(a == tsw_nominal(k, S, tab.data()) && a >= prev && a >= 0);
      CHECK(a <= n + 2 * kTsmHs);  // the last frames reach past the end by less than two hops at rate 2
      prev = a;
      ++frames;
    }
    ++plans;
  }
  CHECK(worst == 1);

  // refusals of the plan: nothing is written
  {
    int tab[3 * 66];
    std::fill(tab, tab + 3 * 66, -7);
    std::vector<int> many(66), ok_rates(66, 65536);
    for (int i = 0; i < 66; ++i) many[(size_t)i] = 2 * i;
    struct Bad { int n, S; int starts[3]; int rqs[3]; const char* what; };
    const Bad bad[] = {
        {0, 1, {0, 0, 0}, {65536, 65536, 65536}, "a clip of 0 samples"},
        {TT_TSM_MAX_SAMPLES + 1, 1, {0, 0, 0}, {65536, 65536, 65536}, "samples (1 .."},
        {100, 0, {0, 0, 0}, {65536, 65536, 65536}, "0 segments"},
        {100, 2, {1, 50, 0}, {65536, 65536, 65536}, "not at 0"},
        {100, 2, {0, 1, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 2, {0, 99, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 3, {0, 60, 40}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 3, {0, 40, 40}, {65536, 65536, 65536}, "at least 2 samples"},
        {1, 1, {0, 0, 0}, {65536, 65536, 65536}, "at least 2 samples"},
        {100, 2, {0, 50, 0}, {65536, 32767, 65536}, "segment 1: rate 32767"},
        {100, 2, {0, 50, 0}, {131073, 65536, 65536}, "segment 0: rate 131073"},
        {100, 1, {0, 0, 0}, {0, 65536, 65536}, "rate 0"},
        {100, 1, {0, 0, 0}, {-65536, 65536, 65536}, "rate -65536"},
    };
    for (const Bad& b : bad) {
      CHECK(tsw_plan(b.n, b.S, b.starts, b.rqs, tab, err, sizeof(err)) == -1 && strstr(err, b.what));
      CHECK(std::all_of(tab, tab + 3 * 66, [](int v) { return v == -7; }));
    }
    CHECK(tsw_plan(1000, 65, many.data(), ok_rates.data(), tab, err, sizeof(err)) == -1 && strstr(err, "65 segments (1 .. 64)") && tab[0] == -7);
    CHECK(tsw_plan(100, 1, nullptr, ok_rates.data(), tab, err, sizeof(err)) == -1 && strstr(err, "null argument"));
    CHECK(tsw_plan(100, 1, many.data(), nullptr, tab, err, sizeof(err)) == -1 && tsw_plan(100, 1, many.data(), ok_rates.data(), nullptr, err, sizeof(err)) == -1);
    CHECK(tsw_plan(1000, 64, many.data(), ok_rates.data(), tab, err, sizeof(err)) == 0 && tsw_out_samples(1000, 64, tab) == 1000);  // 64 is fine
    CHECK(tsw_plan(4, 2, many.data(), ok_rates.data(), tab, err, sizeof(err)) == 0 && tsw_out_samples(4, 2, tab) == 4 && tsw_frames(4, 2, tab) == 2);
  }

  // refusals of the table
  {
    const int starts[3] = {0, 1000, 1700}, rqs[3] = {81920, 52429, 131072};
    int good[9];
    CHECK(tsw_plan(3000, 3, starts, rqs, good, err, sizeof(err)) == 0);
    const int n_out = tsw_out_samples(3000, 3, good);
    CHECK(n_out == good[6] + (int)(((long long)(3000 - good[7]) * 65536 + 65536) / 131072) && tsw_frames(3000, 3, good) == tsm_frames(n_out));
    auto with = [&](int at, int v) {
      std::vector<int> tb(good, good + 9);
      tb[(size_t)at] = v;
      return tb;
    };
    CHECK(tsw_out_samples(3000, 3, with(0, 1).data()) == 0 && tsw_out_samples(3000, 3, with(1, 1).data()) == 0);     // the start is (0, 0)
    CHECK(tsw_out_samples(3000, 3, with(3, 0).data()) == 0 && tsw_out_samples(3000, 3, with(6, good[3]).data()) == 0);  // m increases
    CHECK(tsw_out_samples(3000, 3, with(6, good[3] - 1).data()) == 0);
    for (int at : {4, 7})
      for (int by : {-1, 1}) CHECK(tsw_out_samples(3000, 3, with(at, good[at] + by).data()) == 0);  // continuity, broken by 1
    for (int at : {2, 5, 8})
      for (int v : {0, -1, 32767, 131073, INT_MAX, INT_MIN}) CHECK(tsw_out_samples(3000, 3, with(at, v).data()) == 0 && tsw_frames(3000, 3, with(at, v).data()) == 0);
    CHECK(tsw_out_samples(good[7], 3, good) == 0 && tsw_out_samples(good[7] + 1, 3, good) == good[6] + 1);  // a_(S-1) < n
    CHECK(tsw_out_samples(3000, 0, good) == 0 && tsw_out_samples(3000, 65, good) == 0 && tsw_out_samples(0, 3, good) == 0);
    CHECK(tsw_out_samples(TT_TSM_MAX_SAMPLES + 1, 3, good) == 0 && tsw_out_samples(TT_TSM_MAX_SAMPLES, 3, good) > 0);
    CHECK(tsw_out_samples(3000, 2, good) > 0 && tsw_out_samples(3000, 1, good) == tsm_out_samples(3000, 81920));  // a prefix of a table is a table
  }

  // the handle's and the call's arguments
  CHECK(tsw_check_create(1, 1, 1, err, sizeof(err)) == 0 && tsw_check_create(TT_TSM_MAX_SAMPLES, TT_TSM_MAX_CLIPS, TT_TSW_MAX_SEGMENTS, err, sizeof(err)) == 0);
  CHECK(tsw_check_create(0, 1, 1, err, sizeof(err)) == -1 && strstr(err, "max_samples 0"));
  CHECK(tsw_check_create(TT_TSM_MAX_SAMPLES + 1, 1, 1, err, sizeof(err)) == -1 && tsw_check_create(1, 0, 1, err, sizeof(err)) == -1 && strstr(err, "max_clips 0"));
  CHECK(tsw_check_create(1, 65, 1, err, sizeof(err)) == -1 && tsw_check_create(1, 1, 0, err, sizeof(err)) == -1 && strstr(err, "max_segments 0"));
  CHECK(tsw_check_create(1, 1, 65, err, sizeof(err)) == -1 && strstr(err, "max_segments 65 (1 .. 64)"));
  CHECK(tsw_check_stretch(true, 1, 16, err, sizeof(err)) == 0 && tsw_check_stretch(true, 16, 16, err, sizeof(err)) == 0);
  CHECK(tsw_check_stretch(false, 1, 16, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(tsw_check_stretch(true, 0, 16, err, sizeof(err)) == -1 && tsw_check_stretch(true, 17, 16, err, sizeof(err)) == -1 && strstr(err, "17 clips (1 .. 16)"));

  printf("tsw_host_check: ok (%ld random plans, %ld frames, worst |a_i - b_i| %d)\n", plans, frames, worst);
  return 0;
}
