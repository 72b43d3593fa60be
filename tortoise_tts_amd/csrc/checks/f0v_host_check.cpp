// Stand-alone check of the Viterbi F0 path's host code (f0v_host.h): the cost rules, a clip's status at every border, the argument checks,
// and f0v_viterbi_host against hand-worked answers (F = 1, every state absent but "unvoiced", a tie at every step, a state that is
// absent in the middle, an octave slip pulled back) - no device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all f0v_host_check.cpp -o f0v_host_check && ./f0v_host_check
// Exit status 0 and "f0v_host_check: ok" when everything holds.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../f0v_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

struct Tables {
  std::vector<int> lag;
  std::vector<double> dp;
  explicit Tables(int F) : lag((size_t)F * 8, 0), dp((size_t)F * 8, 0.0) {
    for (int t = 0; t < F; ++t) lag[(size_t)t * 8 + 7] = 48;  // slot 7: some pick of tt_f0_track's; the path does not look at it
  }
  void set(int t, int s, int l, double d) { lag[(size_t)t * 8 + s] = l, dp[(size_t)t * 8 + s] = d; }
};

int main() {
  char err[256];
  std::vector<double> L2(TT_F0V_TABLE, 0.0);
  for (int tau = 1; tau < TT_F0V_TABLE; ++tau) L2[tau] = log2((double)tau);
  const F0vCost def{0.01, 0.35, 0.14, 0.30}, zero{0.0, 0.0, 0.0, 0.0};

  // the cost rules
  CHECK(f0v_cost_ok(def) && f0v_cost_ok(zero) && f0v_cost_ok(F0vCost{1e300, 1e300, 1e300, 1e300}));
  for (int which = 0; which < 4; ++which)
    for (double bad : {-1e-300, -1.0, (double)NAN, (double)INFINITY, (double)-INFINITY}) {
      double v[4] = {0.01, 0.35, 0.14, 0.30};
      v[which] = bad;
      CHECK(!f0v_cost_ok(F0vCost{v[0], v[1], v[2], v[3]}));
    }
  CHECK(f0v_local(7, 123.0, 0.0, 0.0, def) == 0.30 && f0v_local(0, 0.05, L2[96], L2[48], def) == 0.05 + 0.01 * (L2[96] - L2[48]));
  CHECK(f0v_trans(7, 7, 0.0, 0.0, def) == 0.0 && f0v_trans(7, 3, 0.0, L2[100], def) == 0.14 && f0v_trans(2, 7, L2[100], 0.0, def) == 0.14);
  CHECK(f0v_trans(0, 1, L2[80], L2[160], def) == 0.35 * (L2[160] - L2[80]) && f0v_trans(1, 0, L2[160], L2[80], def) == 0.35 * (L2[160] - L2[80]) && f0v_trans(4, 4, L2[77], L2[77], def) == 0.0);

  // a clip's status: tt_f0's rules first, then the costs
  const int M = 12000;
  auto st = [&](int i0, int i1, const F0vCost& k, int f0_, int f1) { return f0v_clip_status(i0, i1, M, 48, 400, 0.15, 0.01, k, f0_, f1); };
  CHECK(st(0, 12000, def, 0, 50) == TT_F0_OK && st(0, 12000, zero, 0, 50) == TT_F0_OK && st(5, 6, def, 7, 8) == TT_F0_OK);
  CHECK(st(100, 100, def, 0, 0) == TT_F0_EMPTY && st(100, 100, F0vCost{-1.0, NAN, 0.0, 0.0}, 0, 0) == TT_F0_EMPTY);  // (nothing else is looked at)
  CHECK(st(0, 12001, def, 0, 51) == TT_F0_REFUSED && st(0, 12000, def, 0, 49) == TT_F0_REFUSED && st(-1, 100, def, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, F0vCost{-0.01, 0.35, 0.14, 0.30}, 0, 50) == TT_F0_REFUSED && st(0, 12000, F0vCost{0.01, NAN, 0.14, 0.30}, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, F0vCost{0.01, 0.35, INFINITY, 0.30}, 0, 50) == TT_F0_REFUSED && st(0, 12000, F0vCost{0.01, 0.35, 0.14, -INFINITY}, 0, 50) == TT_F0_REFUSED);
  CHECK(f0v_clip_status(0, 12000, M, 23, 400, 0.15, 0.01, def, 0, 50) == TT_F0_REFUSED && f0v_clip_status(0, 12000, M, 48, 400, 2.5, 0.01, def, 0, 50) == TT_F0_REFUSED);
  CHECK(f0v_clip_status(INT_MIN, INT_MAX, M, 48, 400, 0.15, 0.01, def, 0, 50) == TT_F0_REFUSED);
  // ... and of a clip given as tables
  auto ps = [&](int F, const F0vCost& k, int f0_, int f1) { return f0v_path_status(F, 50, 48, 400, k, f0_, f1); };
  CHECK(ps(1, def, 0, 1) == TT_F0_OK && ps(50, def, 10, 60) == TT_F0_OK && ps(0, def, 0, 0) == TT_F0_EMPTY && ps(-1, def, 0, 50) == TT_F0_REFUSED);
  CHECK(ps(51, def, 0, 51) == TT_F0_REFUSED && ps(50, def, 0, 49) == TT_F0_REFUSED && ps(50, def, -1, 50) == TT_F0_REFUSED && ps(INT_MAX, def, 0, INT_MAX) == TT_F0_REFUSED);
  CHECK(ps(50, F0vCost{0.01, 0.35, 0.14, NAN}, 0, 50) == TT_F0_REFUSED && f0v_path_status(50, 50, 48, 481, def, 0, 50) == TT_F0_REFUSED);
  CHECK(ps(50, def, INT_MAX, INT_MIN) == TT_F0_REFUSED && ps(50, def, 0, INT_MAX) == TT_F0_OK);

  // the handle's and the call's arguments
  CHECK(f0v_check_create(true, L2.data(), 1, 1, err, sizeof(err)) == 0 && f0v_check_create(true, L2.data(), TT_F0_MAX_SAMPLES, TT_F0_MAX_CLIPS, err, sizeof(err)) == 0);
  CHECK(f0v_check_create(false, L2.data(), 1, 1, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(f0v_check_create(true, nullptr, 1, 1, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(f0v_check_create(true, L2.data(), 0, 1, err, sizeof(err)) == -1 && strstr(err, "max_samples 0 (1 .. 8388608)"));
  CHECK(f0v_check_create(true, L2.data(), TT_F0_MAX_SAMPLES + 1, 1, err, sizeof(err)) == -1 && f0v_check_create(true, L2.data(), 1, 65, err, sizeof(err)) == -1 &&
        strstr(err, "max_clips 65 (1 .. 64)"));
  {
    std::vector<double> bad = L2;
    bad[300] = NAN;
    CHECK(f0v_check_create(true, bad.data(), 1, 1, err, sizeof(err)) == -1 && strstr(err, "log2 table"));
    bad = L2;
    bad[480] = INFINITY;
    CHECK(!f0v_table_ok(bad.data()));
    bad = L2;
    bad[10] = bad[9] - 1e-9;
    CHECK(!f0v_table_ok(bad.data()) && f0v_table_ok(L2.data()));
  }
  CHECK(f0v_check_track(true, 1, 16, err, sizeof(err)) == 0 && f0v_check_track(true, 16, 16, err, sizeof(err)) == 0);
  CHECK(f0v_check_track(false, 1, 16, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(f0v_check_track(true, 0, 16, err, sizeof(err)) == -1 && f0v_check_track(true, 17, 16, err, sizeof(err)) == -1 && strstr(err, "17 clips (1 .. 16)"));

  // the recursion
  int state[8];
  double cost = -1.0;
  {  // F = 1: the end state is the lowest local cost, no step is taken
    Tables T(1);
    T.set(0, 0, 100, 0.05);
    T.set(0, 1, 200, 0.02);
    CHECK(f0v_viterbi_host(1, T.lag.data(), T.dp.data(), 48, L2.data(), def, state, &cost));
    CHECK(state[0] == 1 && cost == 0.02 + 0.01 * (L2[200] - L2[48]) && cost < 0.05 + 0.01 * (L2[100] - L2[48]) && cost < 0.30);
    T.set(0, 1, 200, 0.5);  // a poor dip: unvoiced is cheaper than either
    T.set(0, 0, 100, 0.4);
    CHECK(f0v_viterbi_host(1, T.lag.data(), T.dp.data(), 48, L2.data(), def, state, &cost) && state[0] == 7 && cost == 0.30);
    CHECK(!f0v_viterbi_host(0, T.lag.data(), T.dp.data(), 48, L2.data(), def, state, &cost) && cost == 0.30);
    CHECK(!f0v_viterbi_host(1, nullptr, T.dp.data(), 48, L2.data(), def, state, &cost));
  }
  {  // every state absent but 7: the path is unvoiced and costs F uv (0.25: exact)
    Tables T(4);
    CHECK(f0v_viterbi_host(4, T.lag.data(), T.dp.data(), 48, L2.data(), F0vCost{0.01, 0.35, 0.14, 0.25}, state, &cost));
    CHECK(state[0] == 7 && state[1] == 7 && state[2] == 7 && state[3] == 7 && cost == 1.0);
  }
  {  // a tie at every step (every cost 0): the smallest source wins, the smallest end state wins
    Tables T(5);
    for (int t = 0; t < 5; ++t) T.set(t, 0, 100, 0.0), T.set(t, 1, 200, 0.0), T.set(t, 2, 300, 0.0);
    CHECK(f0v_viterbi_host(5, T.lag.data(), T.dp.data(), 48, L2.data(), zero, state, &cost) && cost == 0.0);
    for (int t = 0; t < 5; ++t) CHECK(state[t] == 0);
    T.set(1, 0, 0, 0.0);  // state 0 absent in frames 1 and 3: the path goes through the next one there and comes back
    T.set(3, 0, 0, 0.0);
    CHECK(f0v_viterbi_host(5, T.lag.data(), T.dp.data(), 48, L2.data(), zero, state, &cost) && cost == 0.0);
    CHECK(state[0] == 0 && state[1] == 1 && state[2] == 0 && state[3] == 1 && state[4] == 0);
    T.set(4, 0, 0, 0.0);  // ... and absent in the last frame: the end state is 1
    T.set(4, 1, 0, 0.0);
    CHECK(f0v_viterbi_host(5, T.lag.data(), T.dp.data(), 48, L2.data(), zero, state, &cost) && state[4] == 2 && state[3] == 1 && state[2] == 0);
  }
  {  // an octave slip in the middle frame is pulled back: the frame's own lowest dip is the octave above, the path stays
    Tables T(3);
    T.set(0, 0, 80, 0.05), T.set(0, 1, 160, 0.02);
    T.set(1, 0, 80, 0.01), T.set(1, 1, 160, 0.03);
    T.set(2, 0, 80, 0.05), T.set(2, 1, 160, 0.02);
    CHECK(f0v_viterbi_host(3, T.lag.data(), T.dp.data(), 48, L2.data(), def, state, &cost));
    CHECK(state[0] == 1 && state[1] == 1 && state[2] == 1);
    const double l = 0.01 * (L2[160] - L2[48]);
    CHECK(cost == (0.02 + l) + ((0.03 + l) + (0.02 + l)));  // a[t] = local + (a[t-1] + 0)
    CHECK(f0v_viterbi_host(3, T.lag.data(), T.dp.data(), 48, L2.data(), F0vCost{0.01, 0.0, 0.14, 0.30}, state, &cost));  // no jump cost: it slips
    CHECK(state[0] == 1 && state[1] == 0 && state[2] == 1);
  }

  {  // a lag outside 1 .. T is an absent state, as on the device: never read as an index of the table
    CHECK(f0v_present(1) && f0v_present(TT_F0_LAG_MAX) && !f0v_present(0) && !f0v_present(-1) && !f0v_present(TT_F0_LAG_MAX + 1) && !f0v_present(INT_MAX));
    Tables T(2);
    T.set(0, 0, TT_F0_LAG_MAX + 1, 0.0), T.set(0, 1, 100, 0.05), T.set(1, 0, -5, 0.0), T.set(1, 1, INT_MAX, 0.0), T.set(1, 2, 100, 0.05);
    CHECK(f0v_viterbi_host(2, T.lag.data(), T.dp.data(), 48, L2.data(), def, state, &cost) && state[0] == 1 && state[1] == 2);
  }

  printf("f0v_host_check: ok\n");
  return 0;
}
