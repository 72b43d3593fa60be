// Host bookkeeping of the streaming leveler (include/tortoise_mi355x_lvs.h): what is ready, the slots' counters and settings, and every
// argument check of tt_lvs_open / tt_lvs_push.  Plain C++ with no device part, so that csrc/checks/lvs_host_check.cpp can run it under the
// host sanitizers.  A check either fails and changes nothing, or yields a plan that commit() applies after the launches were issued.
#pragma once
#include <math.h>
#include <stdio.h>
#include <vector>
#include "../../include/tortoise_mi355x_lvs.h"

#ifdef __HIPCC__
#define TT_LVS_HD __host__ __device__  // the kernels derive the counts from the items with the same functions
#else
#define TT_LVS_HD
#endif

namespace tt {

static_assert(TT_LVS_DELAY == 2 * TT_LOUD_LOOKAHEAD + 8, "the limiter's reach: r 2 Lh, P's neighbour and the oversampler 8 more");
static_assert(TT_LVS_HIST >= 2 * TT_LVS_DELAY && TT_LVS_HIST >= TT_LOUD_SEGMENT + 1 && TT_LVS_HIST % 64 == 0, "the history covers both readers");

constexpr long long kLvsMaxSamples = (long long)TT_LVS_MAX_HOPS * TT_LOUD_HOP;  // 2 073 600 000 < 2^31

// the outputs that exist once n samples are in (flush: once the stream has ended at n)
TT_LVS_HD static inline int lvs_ready_total(int n, int limit, bool flush) {
  if (flush || limit == TT_LVS_NONE) return n;
  return n > TT_LVS_DELAY ? n - TT_LVS_DELAY : 0;
}
static inline bool lvs_count_ok(int n_before, int n_chunk, int limit) {
  return (limit == TT_LVS_NONE || limit == TT_LVS_LOOKAHEAD) && n_before >= 0 && n_chunk >= 0 && (long long)n_before + n_chunk <= kLvsMaxSamples;
}
static inline int lvs_ready(int n_before, int n_chunk, int limit, int flush) {
  if (!lvs_count_ok(n_before, n_chunk, limit)) return -1;
  return lvs_ready_total(n_before + n_chunk, limit, flush != 0) - lvs_ready_total(n_before, limit, false);
}

enum { kLvsClosed = 0, kLvsOpen = 1, kLvsFinished = 2 };

struct LvsSlot {
  int state = kLvsClosed;
  int steer = 0, limit = 0;
  float gain0 = 1.f, target = 0.f, ceiling = 1.f, boost = 0.f, cut = 0.f, rise = 0.f, fall = 0.f;
  int n_in = 0, n_out = 0, hops = 0;
  int parity = 0;  // which copy of the history is current
  int pushes = 0;  // launches issued since the slot was opened: the first one sets the slot's device state
};

// What one pushed slot's workgroups need (the kernels take these by value): 13 words.
struct LvsItem {
  int slot, bits;          // bits: parity | steer << 1 | limit << 2 | flush << 3 | first << 4
  int n_prev, n_end;       // samples before and after the push
  int in_off, out_off;     // where the chunk starts in `audio` and the outputs in `out`
  float gain0, target, ceiling, boost, cut, rise, fall;
};
TT_LVS_HD static inline int lvs_parity(const LvsItem& it) { return it.bits & 1; }
TT_LVS_HD static inline int lvs_steer(const LvsItem& it) { return it.bits >> 1 & 1; }
TT_LVS_HD static inline int lvs_limit(const LvsItem& it) { return it.bits >> 2 & 1; }
TT_LVS_HD static inline bool lvs_flush(const LvsItem& it) { return (it.bits >> 3 & 1) != 0; }
TT_LVS_HD static inline bool lvs_first(const LvsItem& it) { return (it.bits >> 4 & 1) != 0; }

struct LvsBook {
  std::vector<LvsSlot> slots;
  int max_hops = 0;

  void init(int max_streams, int hops) {
    slots.assign((size_t)max_streams, LvsSlot());
    max_hops = hops;
  }
  int max_streams() const { return (int)slots.size(); }

  // 0, or -1 with a message in err
  int check_open(int slot, int steer, int limit, float gain0, float target, float ceiling, float boost, float cut, float rise, float fall, char* err,
                 size_t n) const {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_lvs_open: slot %d (0 .. %d)", slot, max_streams() - 1);
    if (steer != TT_LVS_ADAPT && steer != TT_LVS_FIXED) return fail(err, n, "tt_lvs_open: steering mode %d (0 .. 1)", steer, 0);
    if (limit != TT_LVS_NONE && limit != TT_LVS_LOOKAHEAD) return fail(err, n, "tt_lvs_open: limiting mode %d (0 .. 1)", limit, 0);
    if (!(gain0 > 0.f && gain0 <= 1e30f)) return fail(err, n, "tt_lvs_open: slot %d: gain0 is not a positive finite number", slot, 0);
    if (!(fabsf(target) <= 1e30f)) return fail(err, n, "tt_lvs_open: slot %d: the target is not finite", slot, 0);
    if (!(ceiling > 0.f && ceiling <= 1e30f)) return fail(err, n, "tt_lvs_open: slot %d: the ceiling is not a positive finite number", slot, 0);
    if (!(boost >= 0.f && boost <= 1e30f) || !(cut >= 0.f && cut <= 1e30f))
      return fail(err, n, "tt_lvs_open: slot %d: boost and cut are dB >= 0", slot, 0);
    if (!(rise >= 0.f && rise <= 1e30f) || !(fall >= 0.f && fall <= 1e30f))
      return fail(err, n, "tt_lvs_open: slot %d: negative or non-finite rates (rise and fall are dB per second >= 0)", slot, 0);
    return 0;
  }
  void commit_open(int slot, int steer, int limit, float gain0, float target, float ceiling, float boost, float cut, float rise, float fall) {
    LvsSlot& s = slots[(size_t)slot];
    s = LvsSlot();
    s.state = kLvsOpen;
    s.steer = steer; s.limit = limit;
    s.gain0 = gain0; s.target = target; s.ceiling = ceiling; s.boost = boost; s.cut = cut; s.rise = rise; s.fall = fall;
  }
  int close(int slot, char* err, size_t n) {
    if (slot < 0 || slot >= max_streams()) return fail(err, n, "tt_lvs_close: slot %d (0 .. %d)", slot, max_streams() - 1);
    slots[(size_t)slot] = LvsSlot();
    return 0;
  }

  // The plan of a push: items[i] for pushed slot i and the most outputs any slot emits.  0, or -1 with a message in err; nothing changes.
  int plan(int n_push, const int* ids, const int* n_chunk, const int* flush, std::vector<LvsItem>* items, int* most_out, char* err, size_t n) const {
    if (!ids || !n_chunk || !flush) return fail(err, n, "tt_lvs_push: null argument", 0, 0);
    if (n_push < 1 || n_push > max_streams()) return fail(err, n, "tt_lvs_push: %d streams (1 .. %d)", n_push, max_streams());
    items->clear();
    long long in_off = 0, out_off = 0;
    int most = 0;
    for (int i = 0; i < n_push; ++i) {
      const int id = ids[i];
      if (id < 0 || id >= max_streams()) return fail(err, n, "tt_lvs_push: slot %d (0 .. %d)", id, max_streams() - 1);
      for (int k = 0; k < i; ++k)
        if (ids[k] == id) return fail(err, n, "tt_lvs_push: slot %d is named twice", id, 0);
      const LvsSlot& s = slots[(size_t)id];
      if (s.state == kLvsClosed) return fail(err, n, "tt_lvs_push: slot %d is closed", id, 0);
      if (s.state == kLvsFinished) return fail(err, n, "tt_lvs_push: slot %d is finished (flushed): open it again", id, 0);
      if (n_chunk[i] < 0) return fail(err, n, "tt_lvs_push: slot %d: a chunk of %d samples", id, n_chunk[i]);
      if (((long long)s.n_in + n_chunk[i]) / TT_LOUD_HOP > max_hops) {
        snprintf(err, n, "tt_lvs_push: slot %d: %d + %d samples pass the handle's %d hops", id, s.n_in, n_chunk[i], max_hops);
        return -1;
      }
      LvsItem it;
      it.slot = id;
      it.bits = s.parity | s.steer << 1 | s.limit << 2 | (flush[i] != 0) << 3 | (s.pushes == 0) << 4;
      it.n_prev = s.n_in; it.n_end = s.n_in + n_chunk[i];
      it.in_off = (int)in_off; it.out_off = (int)out_off;
      it.gain0 = s.gain0; it.target = s.target; it.ceiling = s.ceiling; it.boost = s.boost; it.cut = s.cut; it.rise = s.rise; it.fall = s.fall;
      const int emits = lvs_ready_total(it.n_end, s.limit, flush[i] != 0) - s.n_out;
      in_off += n_chunk[i];
      out_off += emits;
      if (emits > most) most = emits;
      if (in_off > 0x7fffffffll - TT_LVS_HIST || out_off > 0x7fffffffll - TT_LVS_HIST)
        return fail(err, n, "tt_lvs_push: the packed chunks or outputs of %d streams exceed 32-bit offsets", n_push, 0);
      items->push_back(it);
    }
    *most_out = most;
    return 0;
  }
  void commit(const std::vector<LvsItem>& items) {
    for (size_t i = 0; i < items.size(); ++i) {
      LvsSlot& s = slots[(size_t)items[i].slot];
      s.n_in = items[i].n_end;
      s.n_out = lvs_ready_total(s.n_in, s.limit, lvs_flush(items[i]));
      s.hops = s.n_in / TT_LOUD_HOP;
      s.parity ^= 1;
      s.pushes += 1;
      if (lvs_flush(items[i])) s.state = kLvsFinished;
    }
  }

 private:
  static int fail(char* err, size_t n, const char* fmt, int a, int b) {
    snprintf(err, n, fmt, a, b);
    return -1;
  }
};

}  // namespace tt
