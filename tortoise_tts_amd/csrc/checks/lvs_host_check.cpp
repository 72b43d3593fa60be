// Stand-alone check of the streaming leveler's host code (loudness_stream_host.h): what is ready against brute force from the formulas'
// reach, the reach of every push into the history, and the slot bookkeeping with every refusal - no device, no library.  Meant for the
// host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all lvs_host_check.cpp -o lvs_host_check && ./lvs_host_check
// Exit status 0 and "lvs_host_check: ok" when everything holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../loudness_stream_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

constexpr int Lh = TT_LOUD_LOOKAHEAD, H = TT_LOUD_HOP;

// the last input sample y[n] reads: s[n] <- m[n +- Lh] <- r[n +- 2 Lh] <- P[.. n + 2 Lh] <- x[.. n + 2 Lh + 8]
static int reach_forward(int n) { return n + Lh + Lh + 8; }
static int reach_back(int n) { return n - Lh - Lh - 1 - 7; }
// the samples ready with n in: every input they read is there
static int brute_ready(int n, int limit) {
  if (limit == TT_LVS_NONE) return n;
  int r = 0;
  while (reach_forward(r) <= n - 1) ++r;
  return r;
}

static bool same(const LvsBook& a, const LvsBook& b) {
  if (a.slots.size() != b.slots.size() || a.max_hops != b.max_hops) return false;
  for (size_t i = 0; i < a.slots.size(); ++i)
    if (memcmp(&a.slots[i], &b.slots[i], sizeof(LvsSlot)) != 0) return false;
  return true;
}

int main() {
  char err[256];
  unsigned seed = 4321;
  auto rnd = [&](int k) {
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (unsigned)k);
  };
  CHECK(TT_LVS_DELAY == reach_forward(0) && reach_back(0) == -TT_LVS_DELAY);
  for (int n = 0; n < 3000; ++n)
    for (int limit : {TT_LVS_NONE, TT_LVS_LOOKAHEAD}) {
      CHECK(lvs_ready_total(n, limit, false) == brute_ready(n, limit) && lvs_ready_total(n, limit, true) == n);
      CHECK(lvs_ready_total(n + 1, limit, false) >= lvs_ready_total(n, limit, false));
    }

  // streams: every push's plan, its reach into the history, the gain's hop, the totals at the flush
  const int lengths[] = {0, 1, 149, 150, 151, 247, 248, 249, 496, 497, 2399, 2400, 2401, 9600, 40000};
  const int sizes[] = {0, 1, 2, 149, 150, 151, 247, 248, 249, 511, 512, 513, 1024, 2400, 20000};
  long pushes = 0;
  int worst = 0;
  for (int limit : {TT_LVS_NONE, TT_LVS_LOOKAHEAD}) {
    LvsBook book;
    book.init(4, 20);
    for (int n : lengths)
      for (int round = 0; round < 4; ++round) {
        CHECK(book.check_open(1, TT_LVS_ADAPT, limit, 1.f, -23.f, 0.9f, 12.f, 24.f, 3.f, 12.f, err, sizeof(err)) == 0);
        book.commit_open(1, TT_LVS_ADAPT, limit, 1.f, -23.f, 0.9f, 12.f, 24.f, 3.f, 12.f);
        int left = n, total_out = 0;
        bool first = true;
        while (true) {
          const int c = left > 0 ? std::min(round == 0 ? 1 + rnd(3) * 300 : sizes[rnd(15)], left) : 0;
          const int flush = left - c == 0 && rnd(2);
          const int ids[1] = {1}, nc[1] = {c}, fl[1] = {flush};
          std::vector<LvsItem> items;
          int most = -1;
          CHECK(book.plan(1, ids, nc, fl, &items, &most, err, sizeof(err)) == 0 && items.size() == 1);
          const LvsItem& it = items[0];
          const int ready = flush ? it.n_end : brute_ready(it.n_end, limit);
          CHECK(it.n_prev == n - left && it.n_end == it.n_prev + c && it.in_off == 0 && it.out_off == 0 && it.slot == 1);
          CHECK(lvs_first(it) == first && lvs_flush(it) == (flush != 0) && lvs_limit(it) == limit && lvs_steer(it) == TT_LVS_ADAPT);
          CHECK(most == ready - total_out && most == lvs_ready(it.n_prev, c, limit, flush) && most >= 0);
          CHECK(lvs_ready_total(it.n_prev, limit, false) == total_out);  // what the kernel derives n_out from
          if (most > 0) {
            // the first output of the push reaches back into the history by at most TT_LVS_HIST, and so does the running segment
            const int back = it.n_prev - std::max(limit == TT_LVS_LOOKAHEAD ? reach_back(total_out) : total_out, 0);
            CHECK(back <= TT_LVS_HIST);
            worst = std::max(worst, back);
            // every input an output reads is in, unless flushed; the gain of every r it reads is measured
            if (!flush && limit == TT_LVS_LOOKAHEAD) CHECK(reach_forward(ready - 1) <= it.n_end - 1);
            const int last_r = std::min(limit == TT_LVS_LOOKAHEAD ? ready - 1 + 2 * Lh : ready - 1, it.n_end - 1);
            CHECK(last_r / H <= it.n_end / H && last_r / H <= book.max_hops);
          }
          const int seg_back = it.n_prev - (it.n_prev / TT_LOUD_SEGMENT * TT_LOUD_SEGMENT - 2);
          CHECK(seg_back <= TT_LOUD_SEGMENT + 1 && seg_back <= TT_LVS_HIST);
          book.commit(items);
          ++pushes;
          first = false;
          total_out = ready;
          left -= c;
          CHECK(book.slots[1].n_in == it.n_end && book.slots[1].n_out == total_out && book.slots[1].hops == it.n_end / H);
          if (flush) break;
        }
        CHECK(total_out == n && book.slots[1].state == kLvsFinished);
      }
  }
  CHECK(worst <= 2 * TT_LVS_DELAY && worst >= TT_LVS_DELAY);

  // refusals change nothing
  LvsBook book;
  book.init(3, 4);
  book.commit_open(0, TT_LVS_ADAPT, TT_LVS_LOOKAHEAD, 1.f, -23.f, 0.9f, 12.f, 24.f, 3.f, 12.f);
  book.commit_open(2, TT_LVS_FIXED, TT_LVS_NONE, 2.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f);
  {
    const int ids[2] = {0, 2}, nc[2] = {3000, 40}, fl[2] = {0, 1};
    std::vector<LvsItem> items;
    int most = 0;
    CHECK(book.plan(2, ids, nc, fl, &items, &most, err, sizeof(err)) == 0 && most == 3000 - TT_LVS_DELAY);
    CHECK(items[1].in_off == 3000 && items[1].out_off == 3000 - TT_LVS_DELAY && lvs_steer(items[1]) == TT_LVS_FIXED && items[1].gain0 == 2.f);
    book.commit(items);
    CHECK(book.slots[0].parity == 1 && book.slots[0].hops == 1 && book.slots[2].state == kLvsFinished && book.slots[2].n_out == 40);
  }
  const LvsBook before = book;
  struct Bad { int n; int ids[3]; int nc[3]; int fl[3]; const char* what; };
  const Bad bad[] = {
      {0, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},  {4, {0, 1, 2}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},
      {1, {3, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot 3"},            {1, {-1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot -1"},
      {2, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "named twice"},       {1, {1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "is closed"},
      {2, {0, 2, 0}, {1, 1, 1}, {0, 0, 0}, "is finished"},       {1, {0, 0, 0}, {-5, 1, 1}, {0, 0, 0}, "a chunk of -5"},
      {1, {0, 0, 0}, {4 * H - 3000 + H, 1, 1}, {1, 0, 0}, "pass the handle's 4 hops"},
  };
  for (const Bad& b : bad) {
    std::vector<LvsItem> items;
    int most = 0;
    CHECK(book.plan(b.n, b.ids, b.nc, b.fl, &items, &most, err, sizeof(err)) == -1 && strstr(err, b.what) && same(book, before));
  }
  {
    std::vector<LvsItem> items;
    int most = 0;
    const int one[1] = {0};
    CHECK(book.plan(1, nullptr, one, one, &items, &most, err, sizeof(err)) == -1 && strstr(err, "null argument"));
    CHECK(book.plan(1, one, nullptr, one, &items, &most, err, sizeof(err)) == -1 && book.plan(1, one, one, nullptr, &items, &most, err, sizeof(err)) == -1);
    const int nc[1] = {4 * H - 3000 + H - 1}, fl[1] = {1};  // up to the last sample of the partial hop behind max_hops is fine
    CHECK(book.plan(1, one, nc, fl, &items, &most, err, sizeof(err)) == 0 && items[0].n_end == 5 * H - 1 && same(book, before));
  }
  const float nan = nanf(""), inf = HUGE_VALF;
  struct BadOpen { int slot, steer, limit; float g0, T, c, boost, cut, rise, fall; const char* what; };
  const BadOpen bo[] = {
      {3, 0, 0, 1, -23, 1, 1, 1, 1, 1, "slot 3"},        {-1, 0, 0, 1, -23, 1, 1, 1, 1, 1, "slot -1"},
      {1, 2, 0, 1, -23, 1, 1, 1, 1, 1, "steering"},      {1, 0, 2, 1, -23, 1, 1, 1, 1, 1, "limiting"},
      {1, 0, 0, 0, -23, 1, 1, 1, 1, 1, "gain0"},         {1, 0, 0, nan, -23, 1, 1, 1, 1, 1, "gain0"},
      {1, 0, 0, inf, -23, 1, 1, 1, 1, 1, "gain0"},       {1, 0, 0, 1, nan, 1, 1, 1, 1, 1, "target"},
      {1, 0, 0, 1, -inf, 1, 1, 1, 1, 1, "target"},       {1, 0, 1, 1, -23, 0, 1, 1, 1, 1, "ceiling"},
      {1, 0, 1, 1, -23, -1, 1, 1, 1, 1, "ceiling"},      {1, 0, 1, 1, -23, nan, 1, 1, 1, 1, "ceiling"},
      {1, 0, 0, 1, -23, 1, -1, 1, 1, 1, "boost and cut"}, {1, 0, 0, 1, -23, 1, 1, nan, 1, 1, "boost and cut"},
      {1, 0, 0, 1, -23, 1, 1, 1, -0.5f, 1, "rates"},     {1, 0, 0, 1, -23, 1, 1, 1, 1, -1, "rates"},
      {1, 0, 0, 1, -23, 1, 1, 1, inf, 1, "rates"},
  };
  for (const BadOpen& b : bo)
    CHECK(book.check_open(b.slot, b.steer, b.limit, b.g0, b.T, b.c, b.boost, b.cut, b.rise, b.fall, err, sizeof(err)) == -1 && strstr(err, b.what) &&
          same(book, before));
  CHECK(book.close(3, err, sizeof(err)) == -1 && book.close(-1, err, sizeof(err)) == -1 && same(book, before));
  CHECK(lvs_ready(-1, 6, 0, 0) == -1 && lvs_ready(0, -1, 0, 0) == -1 && lvs_ready(0, 5, 2, 0) == -1 && lvs_ready(0, 5, -1, 0) == -1);
  CHECK(lvs_ready((int)kLvsMaxSamples - 5, 6, 1, 0) == -1 && lvs_ready((int)kLvsMaxSamples - 5, 5, 1, 1) == 5 + TT_LVS_DELAY);
  CHECK(lvs_ready(0, 0, 1, 1) == 0 && lvs_ready(0, 248, 1, 0) == 0 && lvs_ready(0, 249, 1, 0) == 1 && lvs_ready(0, 7, 0, 0) == 7 && lvs_ready(100, 1, 1, 1) == 101);
  // a flush of nothing finishes the stream and emits nothing; reopening resets; closing frees
  {
    const int ids[1] = {0}, nc[1] = {0}, fl[1] = {1};
    std::vector<LvsItem> items;
    int most = -1;
    CHECK(book.plan(1, ids, nc, fl, &items, &most, err, sizeof(err)) == 0 && most == TT_LVS_DELAY && !lvs_first(items[0]));
    book.commit(items);
    CHECK(book.slots[0].state == kLvsFinished && book.slots[0].n_out == 3000);
  }
  book.commit_open(0, TT_LVS_FIXED, TT_LVS_NONE, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f);
  CHECK(book.slots[0].state == kLvsOpen && book.slots[0].n_in == 0 && book.slots[0].n_out == 0 && book.slots[0].pushes == 0 && book.slots[0].parity == 0);
  CHECK(book.close(0, err, sizeof(err)) == 0 && book.slots[0].state == kLvsClosed);
  printf("lvs_host_check: ok (%ld pushes, worst reach into the history %d of %d)\n", pushes, worst, TT_LVS_HIST);
  return 0;
}
