// Stand-alone check of the streaming resampler's host code (resample_stream_host.h): the emission counts against brute force, the reach of
// every push into the history, and the slot bookkeeping with every refusal - no device, no library.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all rss_host_check.cpp -o rss_host_check && ./rss_host_check
// Exit status 0 and "rss_host_check: ok" when everything holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../resample_stream_host.h"

using namespace tt;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static int brute_ready(int n, int P, int Q, int H) {
  int m = 0;
  while ((long long)m * P / Q + H + 1 <= (long long)n - 1) ++m;
  return m;
}

static bool same(const RssBook& a, const RssBook& b) {
  if (a.slots.size() != b.slots.size()) return false;
  for (size_t i = 0; i < a.slots.size(); ++i)
    if (memcmp(&a.slots[i], &b.slots[i], sizeof(RssSlot)) != 0) return false;
  return true;
}

int main() {
  const int ratios[][2] = {{1, 2}, {80, 147}, {3, 2}, {3, 1}, {77936, 65536}, {55109, 65536}, {8, 1}, {1, 8}, {147, 160}, {160, 147}, {320, 147}, {3, 4}};
  const int lengths[] = {1, 2, 37, 300, 1000, 5000};
  const int tile_out[3] = {1, 1024, 256};
  char err[256];
  unsigned seed = 12345;
  auto rnd = [&](int k) {
    seed = seed * 1664525u + 1013904223u;
    return (int)((seed >> 8) % (unsigned)k);
  };
  long pushes = 0;
  int worst = 0;
  for (const auto& pq : ratios) {
    const int P = pq[0], Q = pq[1];
    CHECK(rs_ratio_ok(P, Q));
    const int H = rs_half_width(rs_cq(P, Q));
    const int sizes[] = {0, 1, 2, 5, 37, H, H + 1, 2 * H + 1, 2 * H + 2, 1023, 1025, 4000};
    for (int form : {TT_RSS_AUTO, TT_RSS_TABLE, TT_RSS_BANK}) {
      RssBook book;
      book.init(4, form);
      if (book.form_for(P, Q) < 0) {
        CHECK(form == TT_RSS_BANK && !rss_bank_fits(P, Q) && book.check_open(1, P, Q, err, sizeof(err)) == -1 && strstr(err, "does not fit"));
        continue;
      }
      for (int n : lengths)
        for (int round = 0; round < 3; ++round) {
          CHECK(book.check_open(1, P, Q, err, sizeof(err)) == 0);
          book.commit_open(1, P, Q);
          int left = n, total_out = 0;
          while (true) {
            const int c = left > 0 ? std::min(sizes[rnd(12)], left) : 0;
            const int flush = left - c == 0 && rnd(2);
            const int ids[1] = {1}, nc[1] = {c}, fl[1] = {flush};
            std::vector<RssItem> items;
            int tiles[3];
            CHECK(book.plan(1, ids, nc, fl, tile_out, &items, tiles, err, sizeof(err)) == 0 && items.size() == 1);
            const RssItem& it = items[0];
            const int want = flush ? rs_out_samples(it.n_end, P, Q) : brute_ready(it.n_end, P, Q, H);
            CHECK(it.m1 == want && it.m1 >= it.m0 && it.m0 == total_out && it.n_prev == n - left && it.form == book.slots[1].form);
            CHECK(it.m1 - it.m0 == rss_ready(it.n_prev, c, P, Q, flush));
            CHECK(tiles[it.form] == std::max(1, (it.m1 - it.m0 + tile_out[it.form] - 1) / tile_out[it.form]) && tiles[3 - it.form] == 0);
            if (it.m1 > it.m0) {  // the earliest tap of the push: inside the history
              const int reach = it.n_prev - ((int)((long long)it.m0 * P / Q) - H);
              CHECK(reach <= 2 * H + 1 && reach <= TT_RSS_HIST);
              worst = std::max(worst, reach);
            }
            book.commit(items, fl);
            ++pushes;
            total_out = it.m1;
            left -= c;
            if (flush) break;
          }
          CHECK(total_out == rs_out_samples(n, P, Q) && book.slots[1].state == kRssFinished && book.slots[1].n_in == n);
        }
    }
  }
  CHECK(worst <= 571);

  // refusals change nothing
  RssBook book;
  book.init(3, TT_RSS_AUTO);
  book.commit_open(0, 3, 1);
  book.commit_open(2, 1, 2);
  CHECK(book.slots[0].form == TT_RSS_BANK && book.slots[2].form == TT_RSS_BANK);
  {
    const int ids[2] = {0, 2}, nc[2] = {500, 40}, fl[2] = {0, 1};
    std::vector<RssItem> items;
    int tiles[3];
    CHECK(book.plan(2, ids, nc, fl, tile_out, &items, tiles, err, sizeof(err)) == 0);
    CHECK(items[1].in_off == 500 && items[1].out_off == items[0].m1 - items[0].m0 && items[1].first == std::max(1, (items[0].m1 + 255) / 256));
    book.commit(items, fl);
  }
  const RssBook before = book;
  struct Bad { int n; int ids[3]; int nc[3]; int fl[3]; const char* what; };
  const Bad bad[] = {
      {0, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},  {4, {0, 1, 2}, {1, 1, 1}, {0, 0, 0}, "streams (1 .. 3)"},
      {1, {3, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot 3"},            {1, {-1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "slot -1"},
      {2, {0, 0, 0}, {1, 1, 1}, {0, 0, 0}, "named twice"},       {1, {1, 0, 0}, {1, 1, 1}, {0, 0, 0}, "is closed"},
      {2, {0, 2, 0}, {1, 1, 1}, {0, 0, 0}, "is finished"},       {1, {0, 0, 0}, {-5, 1, 1}, {0, 0, 0}, "a chunk of -5"},
      {1, {0, 0, 0}, {TT_RS_MAX_SAMPLES - 499, 1, 1}, {1, 0, 0}, "exceed a stream's"},
  };
  for (const Bad& b : bad) {
    std::vector<RssItem> items;
    int tiles[3];
    CHECK(book.plan(b.n, b.ids, b.nc, b.fl, tile_out, &items, tiles, err, sizeof(err)) == -1 && strstr(err, b.what) && same(book, before));
  }
  {
    std::vector<RssItem> items;
    int tiles[3];
    const int one[1] = {0};
    CHECK(book.plan(1, nullptr, one, one, tile_out, &items, tiles, err, sizeof(err)) == -1 && strstr(err, "null argument"));
    const int nc[1] = {TT_RS_MAX_SAMPLES - 500}, fl[1] = {1};  // up to the limit exactly is fine
    CHECK(book.plan(1, one, nc, fl, tile_out, &items, tiles, err, sizeof(err)) == 0 && items[0].m1 == rs_out_samples(TT_RS_MAX_SAMPLES, 3, 1));
  }
  for (const auto& pq : {std::pair<int, int>{9, 1}, {1, 9}, {6, 4}, {0, 1}, {1, 0}, {-3, 2}, {(1 << 20) + 1, 1 << 20}})
    CHECK(book.check_open(1, pq.first, pq.second, err, sizeof(err)) == -1 && strstr(err, "ratio") && rss_ready(0, 10, pq.first, pq.second, 0) == -1);
  CHECK(book.check_open(3, 3, 1, err, sizeof(err)) == -1 && book.check_open(-1, 3, 1, err, sizeof(err)) == -1 && same(book, before));
  CHECK(book.close(3, err, sizeof(err)) == -1 && same(book, before));
  CHECK(rss_ready(TT_RS_MAX_SAMPLES - 5, 6, 3, 1, 0) == -1 && rss_ready(-1, 6, 3, 1, 0) == -1 && rss_ready(0, -1, 3, 1, 0) == -1);
  CHECK(rss_ready(0, 0, 3, 1, 1) == 0 && rss_ready(0, 108, 3, 1, 0) == 0 && rss_ready(0, 109, 3, 1, 0) == 1 && rss_ready(0, 1, 3, 1, 1) == 1);
  // reopening a finished slot resets it; closing frees it
  CHECK(book.check_open(2, 80, 147, err, sizeof(err)) == 0);
  book.commit_open(2, 80, 147);
  CHECK(book.slots[2].state == kRssOpen && book.slots[2].n_in == 0 && book.slots[2].m_out == 0 && book.slots[2].parity == 0 && book.slots[2].form == TT_RSS_TABLE);
  CHECK(book.close(2, err, sizeof(err)) == 0 && book.slots[2].state == kRssClosed);
  // forms: the few-phase rates take the bank under AUTO, 147 phases take the table there but have a bank when asked
  RssBook bank;
  bank.init(1, TT_RSS_BANK);
  CHECK(bank.form_for(80, 147) == TT_RSS_BANK && bank.form_for(320, 147) == -1 && bank.form_for(77936, 65536) == -1 && book.form_for(320, 147) == TT_RSS_TABLE);
  printf("rss_host_check: ok (%ld pushes, worst reach into the history %d of %d)\n", pushes, worst, TT_RSS_HIST);
  return 0;
}
