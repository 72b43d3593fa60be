// Stand-alone check of the F0 tracker's host code (f0_host.h): the frame count at every border, the lag range of every integer frequency of
// 50 .. 1000 Hz against exact integer arithmetic, every refusal of a clip's parameters, offsets and slices, and the argument checks - no
// device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all f0_host_check.cpp -o f0_host_check && ./f0_host_check
// Exit status 0 and "f0_host_check: ok" when everything holds.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "../f0_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

int main() {
  char err[256];

  // frames: ceil(n / 240) at every border of the first hops, of a frame group of 4 or 8, and of the longest clip
  CHECK(f0_frames(1) == 1 && f0_frames(239) == 1 && f0_frames(240) == 1 && f0_frames(241) == 2);
  CHECK(f0_frames(719) == 3 && f0_frames(720) == 3 && f0_frames(721) == 4);
  CHECK(f0_frames(4 * 240 - 1) == 4 && f0_frames(4 * 240) == 4 && f0_frames(4 * 240 + 1) == 5);
  CHECK(f0_frames(8 * 240 - 1) == 8 && f0_frames(8 * 240) == 8 && f0_frames(8 * 240 + 1) == 9);
  CHECK(f0_frames(TT_F0_MAX_SAMPLES) == 34953 && f0_frames(TT_F0_MAX_SAMPLES - 127) == 34953 && f0_frames(TT_F0_MAX_SAMPLES - 128) == 34952);
  long frames = 0;
  for (int n = 1; n <= 100000; ++n) {
    const int F = f0_frames(n);
    CHECK((long long)(F - 1) * TT_F0_HOP < n && n <= (long long)F * TT_F0_HOP);  // the last frame stands inside the clip
    ++frames;
  }

  // lags of every integer frequency: lo = ceil(24000 / fmax), hi = floor(24000 / fmin), against integer division
  long ranges = 0;
  for (int fmax = 50; fmax <= 1000; ++fmax)
    for (int fmin : {50, 60, fmax / 2 > 50 ? fmax / 2 : 50, fmax}) {
      int lo = -7, hi = -7;
      const int want_lo = (TT_F0_SAMPLE_RATE + fmax - 1) / fmax, want_hi = TT_F0_SAMPLE_RATE / fmin;
      if (fmin > fmax) {
        CHECK(!f0_lag_from_hz(fmin, fmax, &lo, &hi) && lo == -7 && hi == -7);
        continue;
      }
      if (want_lo > want_hi) {  // (no whole lag between the two: e.g. 999 .. 999 Hz)
        CHECK(!f0_lag_from_hz(fmin, fmax, &lo, &hi) && lo == -7 && hi == -7);
        continue;
      }
      CHECK(f0_lag_from_hz(fmin, fmax, &lo, &hi) && lo == want_lo && hi == want_hi && f0_lags_ok(lo, hi));
      ++ranges;
    }
  {
    int lo = -7, hi = -7;
    CHECK(f0_lag_from_hz(50, 1000, &lo, &hi) && lo == TT_F0_LAG_MIN && hi == TT_F0_LAG_MAX);
    CHECK(f0_lag_from_hz(60, 500, &lo, &hi) && lo == 48 && hi == 400);
    CHECK(f0_lag_from_hz(62.5, 490.0, &lo, &hi) && lo == 49 && hi == 384);
    lo = hi = -7;
    CHECK(!f0_lag_from_hz(49.999, 500, &lo, &hi) && !f0_lag_from_hz(60, 1000.001, &lo, &hi) && !f0_lag_from_hz(500, 60, &lo, &hi));
    CHECK(!f0_lag_from_hz(NAN, 500, &lo, &hi) && !f0_lag_from_hz(60, NAN, &lo, &hi) && !f0_lag_from_hz(-INFINITY, INFINITY, &lo, &hi));
    CHECK(!f0_lag_from_hz(60, 500, nullptr, &hi) && !f0_lag_from_hz(60, 500, &lo, nullptr) && lo == -7 && hi == -7);
  }

  // the parameter rules
  CHECK(f0_lags_ok(24, 480) && f0_lags_ok(24, 24) && f0_lags_ok(480, 480) && f0_lags_ok(48, 400));
  CHECK(!f0_lags_ok(23, 480) && !f0_lags_ok(24, 481) && !f0_lags_ok(100, 99) && !f0_lags_ok(INT_MIN, INT_MAX) && !f0_lags_ok(0, 0) && !f0_lags_ok(-1, 24));
  CHECK(f0_thr_ok(0.0, 0.0) && f0_thr_ok(2.0, 1e300) && f0_thr_ok(0.15, 0.0096));
  CHECK(!f0_thr_ok(-1e-300, 0.0) && !f0_thr_ok(2.0000001, 0.0) && !f0_thr_ok(NAN, 0.0) && !f0_thr_ok(INFINITY, 0.0));
  CHECK(!f0_thr_ok(0.15, -1e-300) && !f0_thr_ok(0.15, NAN) && !f0_thr_ok(0.15, INFINITY) && !f0_thr_ok(0.15, -INFINITY));

  // a clip's status from its numbers
  const int M = 12000;
  auto st = [&](int i0, int i1, int lo, int hi, double thr, double fl, int f0_, int f1) { return f0_clip_status(i0, i1, M, lo, hi, thr, fl, f0_, f1); };
  CHECK(st(0, 12000, 48, 400, 0.15, 0.01, 0, 50) == TT_F0_OK && st(5, 6, 24, 480, 0.0, 0.0, 7, 8) == TT_F0_OK);
  CHECK(st(100, 100, 48, 400, 0.15, 0.01, 0, 0) == TT_F0_EMPTY && st(100, 100, 0, 0, -1.0, -1.0, 0, 0) == TT_F0_EMPTY);  // (nothing else is looked at)
  CHECK(st(0, 12001, 48, 400, 0.15, 0.01, 0, 51) == TT_F0_REFUSED);                                   // over max_samples
  CHECK(st(-1, 100, 48, 400, 0.15, 0.01, 0, 50) == TT_F0_REFUSED && st(100, 99, 48, 400, 0.15, 0.01, 0, 50) == TT_F0_REFUSED);
  CHECK(st(INT_MIN, INT_MAX, 48, 400, 0.15, 0.01, 0, 50) == TT_F0_REFUSED && st(0, INT_MAX, 48, 400, 0.15, 0.01, 0, INT_MAX) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 23, 400, 0.15, 0.01, 0, 50) == TT_F0_REFUSED && st(0, 12000, 48, 481, 0.15, 0.01, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 400, 48, 0.15, 0.01, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 48, 400, -0.1, 0.01, 0, 50) == TT_F0_REFUSED && st(0, 12000, 48, 400, 2.1, 0.01, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 48, 400, NAN, 0.01, 0, 50) == TT_F0_REFUSED && st(0, 12000, 48, 400, 0.15, -0.01, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 48, 400, 0.15, NAN, 0, 50) == TT_F0_REFUSED && st(0, 12000, 48, 400, 0.15, INFINITY, 0, 50) == TT_F0_REFUSED);
  CHECK(st(0, 12000, 48, 400, 0.15, 0.01, 0, 49) == TT_F0_REFUSED && st(0, 12000, 48, 400, 0.15, 0.01, -1, 50) == TT_F0_REFUSED);  // the frame slice
  CHECK(st(0, 12000, 48, 400, 0.15, 0.01, INT_MAX, INT_MIN) == TT_F0_REFUSED && st(0, 12000, 48, 400, 0.15, 0.01, 10, 60) == TT_F0_OK);
  CHECK(st(0, 12000, 48, 400, 0.15, 0.01, 0, INT_MAX) == TT_F0_OK);

  // the handle's and the call's arguments
  CHECK(f0_check_create(true, 1, 1, err, sizeof(err)) == 0 && f0_check_create(true, TT_F0_MAX_SAMPLES, TT_F0_MAX_CLIPS, err, sizeof(err)) == 0);
  CHECK(f0_check_create(false, 1, 1, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(f0_check_create(true, 0, 1, err, sizeof(err)) == -1 && strstr(err, "max_samples 0 (1 .. 8388608)"));
  CHECK(f0_check_create(true, TT_F0_MAX_SAMPLES + 1, 1, err, sizeof(err)) == -1 && f0_check_create(true, 1, 0, err, sizeof(err)) == -1 && strstr(err, "max_clips 0"));
  CHECK(f0_check_create(true, 1, 65, err, sizeof(err)) == -1 && strstr(err, "max_clips 65 (1 .. 64)"));
  CHECK(f0_check_track(true, 1, 16, err, sizeof(err)) == 0 && f0_check_track(true, 16, 16, err, sizeof(err)) == 0);
  CHECK(f0_check_track(false, 1, 16, err, sizeof(err)) == -1 && strstr(err, "null argument"));
  CHECK(f0_check_track(true, 0, 16, err, sizeof(err)) == -1 && f0_check_track(true, 17, 16, err, sizeof(err)) == -1 && strstr(err, "17 clips (1 .. 16)"));

  printf("f0_host_check: ok (%ld clip lengths, %ld frequency ranges)\n", frames, ranges);
  return 0;
}
