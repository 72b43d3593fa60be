// Stand-alone check of the sampler's pure functions (the first part of sample_steps.h): Philox4x32-10 against the Random123 known answers,
// the float <-> key maps, the (0, 1) mapping of a Philox word, and the score (repetition penalty, temperature, zero fold) against a
// restatement - no device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all sample_host_check.cpp -o sample_host_check && ./sample_host_check
// Exit status 0 and "sample_host_check: ok" when everything holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../sample_steps.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}
static float from_bits(unsigned u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct Scalars { float rep_penalty, temperature; };

// RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, one zero
static float score_restated(float raw, bool seen, float penalty, float temperature) {
  if (seen && penalty != 1.0f) raw = raw < 0.f ? raw * penalty : raw / penalty;
  if (temperature != 1.0f) raw = raw / temperature;
  return raw == 0.f ? 0.f : raw;
}

int main() {
  {  // Random123 kat_vectors, philox4x32 10 rounds
    const unsigned kat[3][10] = {
        {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (const auto& v : kat) {
      unsigned out[4];
      philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5], out);
      CHECK(out[0] == v[6] && out[1] == v[7] && out[2] == v[8] && out[3] == v[9]);
    }
  }
  long keys = 0;
  {  // key2f(f2key(x)) == x bitwise; key order == float order (both zeros after the fold: one key)
    std::vector<float> xs = {-INFINITY, -3.4028235e38f, -1.f, -1.17549435e-38f, from_bits(0x807fffffu), from_bits(0x80000001u), -0.f, 0.f,
                             from_bits(0x00000001u), from_bits(0x007fffffu), 1.17549435e-38f, 1.f, 3.4028235e38f, INFINITY};
    unsigned seed = 2463534242u;
    for (int i = 0; i < 200000; ++i) {
      seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5;
      const float f = from_bits(seed);
      if (f == f) xs.push_back(f);
    }
    for (unsigned e = 0; e < 255; ++e)
      for (unsigned s = 0; s < 2; ++s)
        for (unsigned m : {0u, 1u, 0x400000u, 0x7fffffu}) xs.push_back(from_bits((s << 31) | (e << 23) | m));
    for (float x : xs) CHECK(bits(key2f(f2key(x))) == bits(x));
    const Scalars unit = {1.f, 1.f};
    for (float& x : xs) x = sample_score(x, false, unit);  // the fold alone
    for (size_t i = 0; i < xs.size(); ++i) {
      CHECK(bits(xs[i]) != 0x80000000u);
      const size_t j = (i * 7919u + 13u) % xs.size();
      for (size_t o : {j, i + 1 < xs.size() ? i + 1 : 0}) {
        const unsigned ka = f2key(xs[i]), kb = f2key(xs[o]);
        CHECK((xs[i] < xs[o]) == (ka < kb) && (xs[i] == xs[o]) == (ka == kb));
        ++keys;
      }
    }
    CHECK(f2key(-INFINITY) == 0x007fffffu);  // (the kernels pad with key 0, below every score)
  }
  {  // u in (0, 1) at both ends of the word, and every value in between by monotonicity
    const float lo = philox_u(0u), hi = philox_u(0xffffffffu);
    CHECK(lo > 0.f && lo < 1.f && hi > 0.f && hi < 1.f && lo < hi);
    CHECK(philox_u(0xffu) == lo && philox_u(0x100u) > lo);
  }
  long scores = 0;
  for (float penalty : {1.f, 2.f})
    for (float temperature : {1.f, 0.8f})
      for (int seen = 0; seen < 2; ++seen)
        for (float raw : {-7.25f, -1e-3f, -0.f, 0.f, 1e-3f, 0.3f, 7.25f, -INFINITY, -1e-45f, 1e-45f}) {
          const Scalars sc = {penalty, temperature};
          const float got = sample_score(raw, seen != 0, sc), want = score_restated(raw, seen != 0, penalty, temperature);
          CHECK(bits(got) == bits(want));
          CHECK(bits(sample_penalty(raw, seen != 0, penalty)) == bits(seen && penalty != 1.f ? (raw < 0.f ? raw * penalty : raw / penalty) : raw));
          ++scores;
        }
  printf("sample_host_check: ok (3 Philox vectors, %ld key comparisons, %ld scores)\n", keys, scores);
  return 0;
}
