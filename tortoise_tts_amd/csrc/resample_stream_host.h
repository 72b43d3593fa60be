// Host bookkeeping of the streaming resampler (include/tortoise_mi355x_rss.h): the emission counts, the slots' counters and every
// argument check of tt_rss_open / tt_rss_push.  Plain C++ with no device part, so that csrc/checks/rss_host_check.cpp can run it under the
// host sanitizers.  A check either fails and changes nothing, or yields a plan that commit() applies after the launch was issued.
#pragma once
#include <stdio.h>
#include <vector>
#include "../../include/tortoise_mi355x_rss.h"
#include "resample_steps.h"

namespace tt {

static_assert(TT_RSS_HIST >= 2 * kRsHMax + 1 && TT_RSS_HIST % 64 == 0, "the history covers the widest filter's reach");

// ready(n): outputs whose last tap exists once n samples are in (flush: once the stream has ended at n)
static inline int rss_ready_total(int n, int P, int Q, int H, bool flush) {
  const long long have = flush ? n : (long long)n - H - 1;
  return have > 0 ? (int)((have * Q + P - 1) / P) : 0;
}

static inline int rss_ready(int n_before, int n_chunk, int P, int Q, int flush) {
  if (!rs_ratio_ok(P, Q) || n_before < 0 || n_chunk < 0 || (long long)n_before + n_chunk > TT_RS_MAX_SAMPLES) return -1;
  const int H = rs_half_width(rs_cq(P, Q));
  return rss_ready_total(n_before + n_chunk, P, Q, H, flush != 0) - rss_ready_total(n_before, P, Q, H, false);
}

// whether the bank of (P, Q) fits a slot
static inline bool rss_bank_fits(int P, int Q) { return (long long)Q * (2 * rs_half_width(rs_cq(P, Q)) + 2) <= TT_RSS_BANK_MAX; }

enum { kRssClosed = 0, kRssOpen = 1, kRssFinished = 2 };

struct RssSlot {
  int state = kRssClosed;
  int P = 0, Q = 0, H = 0;
  int form = TT_RSS_TABLE;  // TT_RSS_TABLE or TT_RSS_BANK
  int n_in = 0, m_out = 0;
  int parity = 0;           // which copy of the history is current
};

// What one pushed slot's part of the launch needs (the kernels take these by value).
struct RssItem {
  int slot, P, Q, H;
  int n_prev, n_end;    // samples before and after the push: inputs at and beyond n_end read 0
  int in_off, out_off;  // where the chunk starts in `audio` and the outputs in `out`
  int m0, m1;           // the outputs emitted: m0 .. m1 - 1
  int parity;           // the history copy to read; the other one is written
  int form;             // TT_RSS_TABLE or TT_RSS_BANK: the kernel that serves the slot
  int first;            // the slot's first work item among those of its form (it has max(1, tiles) of them)
};

struct RssBook {
  int form = TT_RSS_AUTO;
  std::vector<RssSlot> slots;

  void init(int max_streams, int form_) {
    slots.assign((size_t)max_streams, RssSlot());
    form = form_;
  }
  int max_streams() const { return (int)slots.size(); }

  // the form a slot at (P, Q) takes, or -1 where a TT_RSS_BANK handle cannot serve it
  int form_for(int P, int Q) const {
    const bool fits = rss_bank_fits(P, Q);
    if (form == TT_RSS_TABLE) return TT_RSS_TABLE;
    if (form == TT_RSS_BANK) return fits ? TT_RSS_BANK : -1;
    return fits && Q <= TT_RSS_AUTO_MAX_Q ? TT_RSS_BANK : TT_RSS_TABLE;
  }

  // 0, or -1 with a message in err
  int check_open(int slot, int P, int Q, char* err, size_t n) const {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_rss_open: slot %d (0 .. %d)", slot, max_streams() - 1);
    if (!rs_ratio_ok(P, Q)) {
      snprintf(err, n, "tt_rss_open: ratio %d/%d (terms 1 .. %d, 1/%d .. %d, reduced unless Q = %d)", P, Q, TT_RS_MAX_TERM, TT_RS_MAX_RATIO,
               TT_RS_MAX_RATIO, TT_RS_PITCH_ONE);
      return -1;
    }
    if (form_for(P, Q) < 0) {
      snprintf(err, n, "tt_rss_open: the phase bank of ratio %d/%d does not fit (Q (2 H + 2) <= %d)", P, Q, TT_RSS_BANK_MAX);
      return -1;
    }
    return 0;
  }
  void commit_open(int slot, int P, int Q) {
    RssSlot& s = slots[(size_t)slot];
    s = RssSlot();
    s.state = kRssOpen;
    s.P = P; s.Q = Q; s.H = rs_half_width(rs_cq(P, Q));
    s.form = form_for(P, Q);
  }
  int close(int slot, char* err, size_t n) {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_rss_close: slot %d (0 .. %d)", slot, max_streams() - 1);
    slots[(size_t)slot] = RssSlot();
    return 0;
  }

  // The plan of a push: items[i] for pushed slot i, the work items of each form in tiles[form] (tile_out[form] outputs per tile).
  // 0, or -1 with a message in err; nothing changes either way.
  int plan(int n_push, const int* ids, const int* n_chunk, const int* flush, const int tile_out[3], std::vector<RssItem>* items, int tiles[3],
           char* err, size_t n) const {
    if (!ids || !n_chunk || !flush) return fail(err, n, "tt_rss_push: null argument", 0, 0);
    if (n_push < 1 || n_push > max_streams()) return fail(err, n, "tt_rss_push: %d streams (1 .. %d)", n_push, max_streams());
    items->clear();
    tiles[0] = tiles[1] = tiles[2] = 0;
    long long in_off = 0, out_off = 0;
    for (int i = 0; i < n_push; ++i) {
      const int id = ids[i];
      if (id < 0 || id >= max_streams()) return fail(err, n, "tt_rss_push: slot %d (0 .. %d)", id, max_streams() - 1);
      for (int k = 0; k < i; ++k)
        if (ids[k] == id) return fail(err, n, "tt_rss_push: slot %d is named twice", id, 0);
      const RssSlot& s = slots[(size_t)id];
      if (s.state == kRssClosed) return fail(err, n, "tt_rss_push: slot %d is closed", id, 0);
      if (s.state == kRssFinished) return fail(err, n, "tt_rss_push: slot %d is finished (flushed): open it again", id, 0);
      if (n_chunk[i] < 0) return fail(err, n, "tt_rss_push: slot %d: a chunk of %d samples", id, n_chunk[i]);
      if ((long long)s.n_in + n_chunk[i] > TT_RS_MAX_SAMPLES) {
        snprintf(err, n, "tt_rss_push: slot %d: %d + %d samples exceed a stream's %d", id, s.n_in, n_chunk[i], TT_RS_MAX_SAMPLES);
        return -1;
      }
      RssItem it;
      it.slot = id; it.P = s.P; it.Q = s.Q; it.H = s.H;
      it.n_prev = s.n_in; it.n_end = s.n_in + n_chunk[i];
      it.m0 = s.m_out; it.m1 = rss_ready_total(it.n_end, s.P, s.Q, s.H, flush[i] != 0);
      it.parity = s.parity; it.form = s.form;
      it.in_off = (int)in_off; it.out_off = (int)out_off;
      it.first = tiles[s.form];
      const int t = (it.m1 - it.m0 + tile_out[s.form] - 1) / tile_out[s.form];
      tiles[s.form] += t > 1 ? t : 1;  // a push that emits nothing still advances the history
      in_off += n_chunk[i];
      out_off += it.m1 - it.m0;
      if (in_off > 0x7fffffffll - TT_RS_MAX_SAMPLES || out_off > 0x7fffffffll - (long long)TT_RS_MAX_RATIO * TT_RS_MAX_SAMPLES)
        return fail(err, n, "tt_rss_push: the packed chunks or outputs of %d streams exceed 32-bit offsets", n_push, 0);
      items->push_back(it);
    }
    return 0;
  }
  void commit(const std::vector<RssItem>& items, const int* flush) {
    for (size_t i = 0; i < items.size(); ++i) {
      RssSlot& s = slots[(size_t)items[i].slot];
      s.n_in = items[i].n_end;
      s.m_out = items[i].m1;
      s.parity ^= 1;
      if (flush[i]) s.state = kRssFinished;
    }
  }

 private:
  static int fail(char* err, size_t n, const char* fmt, int a, int b) {
    snprintf(err, n, fmt, a, b);
    return -1;
  }
};

}  // namespace tt
