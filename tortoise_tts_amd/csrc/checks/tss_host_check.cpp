// Stand-alone check of the streaming time-stretch's host code (tsm_stream_host.h): the frames done and the outputs ready against brute
// force, the two safety inequalities, the reach of every push into the history, and the slot bookkeeping with every refusal - no device, no
// library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tss_host_check.cpp -o tss_host_check && ./tss_host_check
// Exit status 0 and "tss_host_check: ok" when everything holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../tsm_stream_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// the frames k >= 1 whose whole region x[a_k - 256 .. a_k + 1407) lies below n
static int brute_done(int n, int rq) {
  int k = 0;
  while (tsm_nominal(k + 1, rq) - kTsmS + kTsmRegion <= n) ++k;
  return k;
}

static bool same(const TssBook& a, const TssBook& b) {
  if (a.slots.size() != b.slots.size()) return false;
  for (size_t i = 0; i < a.slots.size(); ++i)
    if (memcmp(&a.slots[i], &b.slots[i], sizeof(TssSlot)) != 0) return false;
  return true;
}

int main() {
  const int rates[] = {32768, 32769, 40000, 52429, 65535, 65536, 65537, 81920, 100000, 131071, 131072};
  char err[256];
  unsigned seed = 12345;
  auto rnd = [&](int k) {
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (unsigned)k);
  };

  // done(n) is brute force; a_k does not decrease
  for (int rq : rates) {
    CHECK(tsm_rate_ok(rq));
    for (int k = 1; k < 400; ++k) CHECK(tsm_nominal(k + 1, rq) >= tsm_nominal(k, rq));
    for (int n = 0; n < 6000; ++n) CHECK(tsm_frames_done(n, rq) == brute_done(n, rq));
    CHECK(tsm_frames_done(kTsmLook - 1, rq) == 0 && tsm_frames_done(kTsmLook, rq) == 1);
  }
  // nothing is emitted early that the whole-clip call would not produce: for every final length N >= n, done(n) <= K(N) - 1 and
  // done(n) Hs <= n_out(N).  Both right-hand sides do not decrease in N, so N = n is the case to check.  The frames left at a flush: at most 8.
  int worst_left = 0;
  for (int rq : rates)
    for (int n = 1; n <= 100001; ++n) {
      const int done = tsm_frames_done(n, rq), n_out = tsm_out_samples(n, rq), K = tsm_frames(n_out);
      CHECK(done <= K - 1 && (long long)done * kTsmHs <= n_out);
      CHECK(tsm_out_samples(n + 1, rq) >= n_out);
      worst_left = std::max(worst_left, K - 1 - done);
    }
  CHECK(worst_left == 8);

  // streams: every push's plan against brute force, its reach into the history, the totals at the flush
  const int lengths[] = {1, 300, 1406, 1407, 1408, 1663, 5000, 9001, 40000};
  const int sizes[] = {0, 1, 2, 5, 383, 384, 385, 1406, 1407, 1408, 1663, 1664, 4096, 20000};
  long pushes = 0;
  int worst = 0;
  for (int rq : rates) {
    TssBook book;
    book.init(4);
    for (int n : lengths)
      for (int round = 0; round < 4; ++round) {
        CHECK(book.check_open(1, rq, err, sizeof(err)) == 0);
        book.commit_open(1, rq);
        int left = n, total_out = 0, total_frames = 0, total_offsets = 0;
        while (true) {
          const int c = left > 0 ? std::min(round == 0 ? 1 + rnd(3) * 700 : sizes[rnd(14)], left) : 0;
          const int flush = left - c == 0 && rnd(2);
          const int ids[1] = {1}, nc[1] = {c}, fl[1] = {flush};
          std::vector<TssItem> items;
          CHECK(book.plan(1, ids, nc, fl, &items, err, sizeof(err)) == 0 && items.size() == 1);
          const TssItem& it = items[0];
          const int want_frames = flush ? tsm_frames(tsm_out_samples(it.n_end, rq)) - 1 : brute_done(it.n_end, rq);
          const int want_out = flush ? tsm_out_samples(it.n_end, rq) : want_frames * kTsmHs;
          CHECK(it.k0 == total_frames + 1 && it.k1 == want_frames && it.k1 >= it.k0 - 1 && it.m0 == total_out && it.m1 == want_out && it.m1 >= it.m0);
          CHECK(it.n_prev == n - left && it.n_end == it.n_prev + c && it.rq == rq && it.in_off == 0 && it.out_off == 0 && it.off_off == 0);
          CHECK(it.m1 - it.m0 == tss_ready(it.n_prev, c, rq, flush) && it.m0 == (it.k0 - 1) * kTsmHs);
          CHECK(it.m1 <= it.k1 * kTsmHs && (it.k1 < it.k0 || it.m1 > (it.k1 - 1) * kTsmHs));  // every frame run writes into the push's outputs
          for (int k = it.k0; k <= it.k1; ++k) {  // the frames of the push: inside history + chunk, and below n_end unless flushed
            const int first = std::max(tsm_nominal(k, rq) - kTsmS, 0);
            const int reach = it.n_prev - first;
            CHECK(reach <= kTsmRegion - 1 && reach <= TT_TSS_HIST);
            worst = std::max(worst, reach);
            CHECK(flush || tsm_nominal(k, rq) + kTsmLook <= it.n_end);
          }
          book.commit(items, fl);
          ++pushes;
          total_out = it.m1;
          total_frames = it.k1;
          total_offsets += TssBook::offsets_of(it.k0, it.k1);
          left -= c;
          // the next frame reaches back at most 1662 samples from here
          CHECK(it.n_end - std::max(tsm_nominal(it.k1 + 1, rq) - kTsmS, 0) <= kTsmRegion - 1);
          if (flush) break;
        }
        CHECK(total_out == tsm_out_samples(n, rq) && total_offsets == tsm_frames(total_out) && book.slots[1].state == kTssFinished);
        CHECK(book.slots[1].n_in == n && book.slots[1].frames == total_frames && book.slots[1].m_out == total_out);
      }
  }
  CHECK(worst <= 1662 && worst >= 1600);

  // refusals change nothing
  TssBook book;
  book.init(3);
  book.commit_open(0, 65536);
  book.commit_open(2, 131072);
  {
    const int ids[2] = {0, 2}, nc[2] = {3000, 40}, fl[2] = {0, 1};
    std::vector<TssItem> items;
    CHECK(book.plan(2, ids, nc, fl, &items, err, sizeof(err)) == 0);
    CHECK(items[0].k0 == 1 && items[0].k1 == 5 && items[0].m1 == 5 * kTsmHs);
    CHECK(items[1].in_off == 3000 && items[1].out_off == 5 * kTsmHs && items[1].off_off == 6 && items[1].m1 == 20 && items[1].k1 == 1);
    book.commit(items, fl);
    CHECK(book.slots[0].parity == 1 && book.slots[2].parity == 1 && book.slots[2].state == kTssFinished);
  }
  const TssBook before = book;
  struct Bad { int n; int ids[3]; int nc[3]; int fl[3]; const char* what; };
  const Bad bad[] = {
      {0, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},  {4, {0, 1, 2}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},
      {1, {3, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot 3"},            {1, {-1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot -1"},
      {2, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "named twice"},       {1, {1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "is closed"},
      {2, {0, 2, 0}, {1, 1, 1}, {0, 0, 0}, "is finished"},       {1, {0, 0, 0}, {-5, 1, 1}, {0, 0, 0}, "a chunk of -5"},
      {1, {0, 0, 0}, {TT_TSM_MAX_SAMPLES - 2999, 1, 1}, {1, 0, 0}, "exceed a stream's"},
  };
  for (const Bad& b : bad) {
    std::vector<TssItem> items;
    CHECK(book.plan(b.n, b.ids, b.nc, b.fl, &items, err, sizeof(err)) == -1 && strstr(err, b.what) && same(book, before));
  }
  {
    std::vector<TssItem> items;
    const int one[1] = {0};
    CHECK(book.plan(1, nullptr, one, one, &items, err, sizeof(err)) == -1 && strstr(err, "null argument"));
    CHECK(book.plan(1, one, nullptr, one, &items, err, sizeof(err)) == -1 && book.plan(1, one, one, nullptr, &items, err, sizeof(err)) == -1);
    const int nc[1] = {TT_TSM_MAX_SAMPLES - 3000}, fl[1] = {1};  // up to the limit exactly is fine
    CHECK(book.plan(1, one, nc, fl, &items, err, sizeof(err)) == 0 && items[0].m1 == TT_TSM_MAX_SAMPLES && same(book, before));
  }
  for (int rq : {0, -1, 32767, 131073, 1 << 30})
    CHECK(book.check_open(1, rq, err, sizeof(err)) == -1 && strstr(err, "rate") && tss_ready(0, 10, rq, 0) == -1 && same(book, before));
  CHECK(book.check_open(3, 65536, err, sizeof(err)) == -1 && book.check_open(-1, 65536, err, sizeof(err)) == -1 && same(book, before));
  CHECK(book.close(3, err, sizeof(err)) == -1 && book.close(-1, err, sizeof(err)) == -1 && same(book, before));
  CHECK(tss_ready(TT_TSM_MAX_SAMPLES - 5, 6, 65536, 0) == -1 && tss_ready(-1, 6, 65536, 0) == -1 && tss_ready(0, -1, 65536, 0) == -1);
  CHECK(tss_ready(0, 0, 65536, 1) == 0 && tss_ready(0, 1406, 65536, 0) == 0 && tss_ready(0, 1407, 65536, 0) == kTsmHs && tss_ready(0, 1, 65536, 1) == 1);
  CHECK(tss_ready(TT_TSM_MAX_SAMPLES - 5, 5, 32768, 1) > 0);
  // a flush of nothing finishes the stream and emits nothing
  {
    TssBook b2;
    b2.init(1);
    b2.commit_open(0, 40000);
    const int ids[1] = {0}, nc[1] = {0}, fl[1] = {1};
    std::vector<TssItem> items;
    CHECK(b2.plan(1, ids, nc, fl, &items, err, sizeof(err)) == 0 && items[0].k1 == 0 && items[0].m1 == 0 && TssBook::offsets_of(items[0].k0, items[0].k1) == 0);
    b2.commit(items, fl);
    CHECK(b2.slots[0].state == kTssFinished);
  }
  // reopening a finished slot resets it; closing frees it
  CHECK(book.check_open(2, 40000, err, sizeof(err)) == 0);
  book.commit_open(2, 40000);
  CHECK(book.slots[2].state == kTssOpen && book.slots[2].n_in == 0 && book.slots[2].m_out == 0 && book.slots[2].frames == 0 && book.slots[2].parity == 0);
  CHECK(book.close(2, err, sizeof(err)) == 0 && book.slots[2].state == kTssClosed);
  printf("tss_host_check: ok (%ld pushes, worst reach into the history %d of %d, at most %d frames left at a flush)\n", pushes, worst, TT_TSS_HIST,
         worst_left);
  return 0;
}
