// Host bookkeeping of the streaming time-stretch (include/tortoise_mi355x_tss.h): the frames done, the emission counts, the slots' counters
// and every argument check of tt_tss_open / tt_tss_push.  Plain C++ with no device part, so that csrc/checks/tss_host_check.cpp can run it
// under the host sanitizers.  A check either fails and changes nothing, or yields a plan that commit() applies after the launch was issued.
#pragma once
#include <stdio.h>
#include <vector>
#include "../../include/tortoise_mi355x_tss.h"
#include "tsm_steps.h"

namespace tt {

static_assert(TT_TSS_LOOK == kTsmLook && TT_TSS_HIST >= kTsmRegion - 1 && TT_TSS_HIST % 64 == 0, "the history covers the next frame's reach");

// the frames 1 .. f have run once n samples are in (flush: once the stream has ended at n)
static inline int tss_frames_total(int n, int rq, bool flush) {
  if (!flush) return tsm_frames_done(n, rq);
  return n >= 1 ? tsm_frames(tsm_out_samples(n, rq)) - 1 : 0;
}
// the outputs that exist then
static inline int tss_ready_total(int n, int rq, bool flush) {
  if (!flush) return tsm_frames_done(n, rq) * kTsmHs;
  return n >= 1 ? tsm_out_samples(n, rq) : 0;
}

static inline bool tss_count_ok(int n_before, int n_chunk, int rq) {
  return tsm_rate_ok(rq) && n_before >= 0 && n_chunk >= 0 && (long long)n_before + n_chunk <= TT_TSM_MAX_SAMPLES;
}
static inline int tss_ready(int n_before, int n_chunk, int rq, int flush) {
  if (!tss_count_ok(n_before, n_chunk, rq)) return -1;
  return tss_ready_total(n_before + n_chunk, rq, flush != 0) - tss_ready_total(n_before, rq, false);
}

enum { kTssClosed = 0, kTssOpen = 1, kTssFinished = 2 };

struct TssSlot {
  int state = kTssClosed;
  int rq = 0;
  int n_in = 0, m_out = 0, frames = 0;
  int parity = 0;  // which copy of the history is current
};

// What one pushed slot's workgroup needs (the kernel takes these by value).
struct TssItem {
  int slot, parity;    // the history copy to read; the other one is written
  int n_prev, n_end;   // samples before and after the push: inputs at and beyond n_end read 0 (only a flush has frames that reach them)
  int k0, k1;          // the frames the push runs: k0 .. k1 (none when k1 < k0)
  int m0, m1;          // the outputs emitted: m0 = (k0 - 1) Hs .. m1 - 1; m1 = k1 Hs, or n_out on a flush
  int in_off, out_off; // where the chunk starts in `audio` and the outputs in `out`
  int off_off;         // where the slot's entries start in `offsets`
  int rq;
};

struct TssBook {
  std::vector<TssSlot> slots;

  void init(int max_streams) { slots.assign((size_t)max_streams, TssSlot()); }
  int max_streams() const { return (int)slots.size(); }

  // 0, or -1 with a message in err
  int check_open(int slot, int rq, char* err, size_t n) const {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_tss_open: slot %d (0 .. %d)", slot, max_streams() - 1);
    if (!tsm_rate_ok(rq)) return fail(err, n, "tt_tss_open: rate %d / 65536 is outside %d .. 131072", rq, TT_TSM_RATE_MIN);
    return 0;
  }
  void commit_open(int slot, int rq) {
    TssSlot& s = slots[(size_t)slot];
    s = TssSlot();
    s.state = kTssOpen;
    s.rq = rq;
  }
  int close(int slot, char* err, size_t n) {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_tss_close: slot %d (0 .. %d)", slot, max_streams() - 1);
    slots[(size_t)slot] = TssSlot();
    return 0;
  }

  // offsets entries of a push that runs frames k0 .. k1
  static int offsets_of(int k0, int k1) { return k1 >= k0 ? k1 - k0 + 1 + (k0 == 1) : 0; }

  // The plan of a push: items[i] for pushed slot i.  0, or -1 with a message in err; nothing changes either way.
  int plan(int n_push, const int* ids, const int* n_chunk, const int* flush, std::vector<TssItem>* items, char* err, size_t n) const {
    if (!ids || !n_chunk || !flush) return fail(err, n, "tt_tss_push: null argument", 0, 0);
    if (n_push < 1 || n_push > max_streams()) return fail(err, n, "tt_tss_push: %d streams (1 .. %d)", n_push, max_streams());
    items->clear();
    long long in_off = 0, out_off = 0, off_off = 0;
    for (int i = 0; i < n_push; ++i) {
      const int id = ids[i];
      if (id < 0 || id >= max_streams()) return fail(err, n, "tt_tss_push: slot %d (0 .. %d)", id, max_streams() - 1);
      for (int k = 0; k < i; ++k)
        if (ids[k] == id) return fail(err, n, "tt_tss_push: slot %d is named twice", id, 0);
      const TssSlot& s = slots[(size_t)id];
      if (s.state == kTssClosed) return fail(err, n, "tt_tss_push: slot %d is closed", id, 0);
      if (s.state == kTssFinished) return fail(err, n, "tt_tss_push: slot %d is finished (flushed): open it again", id, 0);
      if (n_chunk[i] < 0) return fail(err, n, "tt_tss_push: slot %d: a chunk of %d samples", id, n_chunk[i]);
      if ((long long)s.n_in + n_chunk[i] > TT_TSM_MAX_SAMPLES) {
        snprintf(err, n, "tt_tss_push: slot %d: %d + %d samples exceed a stream's %d", id, s.n_in, n_chunk[i], TT_TSM_MAX_SAMPLES);
        return -1;
      }
      TssItem it;
      it.slot = id; it.parity = s.parity; it.rq = s.rq;
      it.n_prev = s.n_in; it.n_end = s.n_in + n_chunk[i];
      it.k0 = s.frames + 1; it.k1 = tss_frames_total(it.n_end, s.rq, flush[i] != 0);
      it.m0 = s.m_out; it.m1 = tss_ready_total(it.n_end, s.rq, flush[i] != 0);
      it.in_off = (int)in_off; it.out_off = (int)out_off; it.off_off = (int)off_off;
      in_off += n_chunk[i];
      out_off += it.m1 - it.m0;
      off_off += offsets_of(it.k0, it.k1);
      if (in_off > 0x7fffffffll - TT_TSM_MAX_SAMPLES || out_off > 0x7fffffffll - 2ll * TT_TSM_MAX_SAMPLES)
        return fail(err, n, "tt_tss_push: the packed chunks or outputs of %d streams exceed 32-bit offsets", n_push, 0);
      items->push_back(it);
    }
    return 0;
  }
  void commit(const std::vector<TssItem>& items, const int* flush) {
    for (size_t i = 0; i < items.size(); ++i) {
      TssSlot& s = slots[(size_t)items[i].slot];
      s.n_in = items[i].n_end;
      s.m_out = items[i].m1;
      s.frames = items[i].k1;
      s.parity ^= 1;
      if (flush[i]) s.state = kTssFinished;
    }
  }

 private:
  static int fail(char* err, size_t n, const char* fmt, int a, int b) {
    snprintf(err, n, fmt, a, b);
    return -1;
  }
};

}  // namespace tt
