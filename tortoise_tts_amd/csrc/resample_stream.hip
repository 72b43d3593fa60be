// The resampler fed in chunks (include/tortoise_mi355x_rss.h): a stream at another sample rate, bit for bit the whole-clip result of
// resample.hip.  The counters and every argument check are host code (resample_stream_host.h); a push hands the kernels one RssItem per
// pushed slot BY VALUE (no upload, no copy back) and is one launch per form among the pushed slots - one launch where they share a form.
//
//   work item            (pushed slot, tile of its outputs): a slot has max(1, tiles) of them, workgroup b takes item b.  Item 0 of a slot
//                        also advances the slot's history: it reads the current copy (positions n_prev - 576 .. n_prev - 1) and the chunk
//                        and writes the OTHER copy (n_end - 576 .. n_end - 1), which no workgroup of this launch reads.  The next push is
//                        ordered behind this one on the handle's stream and reads that copy.
//   span                 the inputs a tile touches, x[i(first) - H .. i(last) + H + 1], staged in LDS once: position j comes from the history
//                        for j < n_prev, from the chunk up to n_end, and is 0 before sample 0 and from n_end on (only a flush has taps
//                        there).  This loader is the one difference to rs_resample_kernel's tile.
//   rss_table_kernel     any ratio: rs_resample_kernel's tile (1024 outputs, one per thread, the 16385-value table in LDS) around rs_output.
//   rss_bank_kernel      a slot whose bank[r][d] = h_j (Q rows of W = 2 H + 2 weights, built once at open by rss_bank_build_kernel with
//                        rs_tap_weight, i.e. the table form's values to the bit) fits 16384 floats: a tile of kRssBankTile = 256 outputs, one
//                        per thread; the bank and the span sit in LDS and an output is W x (two LDS reads, one FMA) in ascending tap
//                        order - no table gather, no blend, no index walk.  Lanes hold neighbouring outputs: their span reads are P / Q
//                        dwords apart, and their bank reads hit different rows at the same column, so the row stride in LDS is W + 1
//                        (odd: rows r and r' fall on the same bank only when r = r' mod 64; lanes on the same row read one address, a
//                        broadcast).  256-output tiles because pieces are short: a 40 960-sample piece to 8 kHz is 54 workgroups
//                        instead of 14.
#include <vector>
#include "runtime.h"
#include "resample_stream_host.h"

namespace tt {

constexpr int kRssTableTile = 1024;  // outputs (= threads) of a table-form tile: rs_resample_kernel's
constexpr int kRssBankTile = 256;    // outputs (= threads) of a bank-form tile
static_assert(kRssTableTile == 1024 && kRssBankTile == 256, "the tiles the tests and DESIGN.md 5.29 name");
constexpr int kRssTableSpan = ((kRssTableTile - 1) * TT_RS_MAX_RATIO + 1 + 2 * kRsHMax + 1 + 15) / 16 * 16;
constexpr int kRssBankSpan = ((kRssBankTile - 1) * TT_RS_MAX_RATIO + 1 + 2 * kRsHMax + 1 + 15) / 16 * 16;
constexpr size_t kRssTableLds = (size_t)(TT_RS_TABLE + 3 + kRssTableSpan) * sizeof(float);
constexpr int kRssBankLdsMax = TT_RSS_BANK_MAX + TT_RSS_BANK_MAX / 2;  // Q (W + 1) <= Q W (1 + 1 / W), W >= 2
static_assert(kRssTableLds <= 160 * 1024 && (size_t)(kRssBankLdsMax + kRssBankSpan) * sizeof(float) <= 160 * 1024, "the kernels' LDS plans");

struct RssArgs {
  int n;
  RssItem it[TT_RSS_MAX_STREAMS];
};
static_assert(sizeof(RssArgs) + 4 * sizeof(void*) <= 4096, "the items travel as kernel arguments");

// the item and the tile of workgroup b among the items of `form`.  false: no such item.
__device__ static inline bool rss_find(const RssArgs& a, int form, int b, int tile_out, RssItem* it, int* tile) {
  for (int i = 0; i < a.n; ++i) {
    if (a.it[i].form != form) continue;
    const int t = (a.it[i].m1 - a.it[i].m0 + tile_out - 1) / tile_out;
    const int items = t > 1 ? t : 1;
    if (b >= a.it[i].first && b < a.it[i].first + items) {
      *it = a.it[i];
      *tile = b - a.it[i].first;
      return true;
    }
  }
  return false;
}

// position j of the slot's stream during this push
__device__ static inline float rss_sample(const RssItem& it, const float* __restrict__ hist, const float* __restrict__ chunk, int j) {
  if (j < 0 || j >= it.n_end) return 0.f;
  if (j >= it.n_prev) return chunk[j - it.n_prev];
  const int e = j - it.n_prev + TT_RSS_HIST;
  return e >= 0 ? hist[e] : 0.f;  // (e < 0 is beyond any tap's reach: resample_stream_host.h, tortoise_mi355x_rss.h)
}

// the slot's first work item writes the other copy of the history
template <int kThreads>
__device__ static inline void rss_advance_history(const RssItem& it, float* __restrict__ hist_all, const float* __restrict__ chunk) {
  const float* cur = hist_all + ((size_t)it.slot * 2 + it.parity) * TT_RSS_HIST;
  float* next = hist_all + ((size_t)it.slot * 2 + (it.parity ^ 1)) * TT_RSS_HIST;
  for (int e = threadIdx.x; e < TT_RSS_HIST; e += kThreads) next[e] = rss_sample(it, cur, chunk, it.n_end - TT_RSS_HIST + e);
}

__global__ __launch_bounds__(kRssTableTile) void rss_table_kernel(RssArgs a, const float* __restrict__ audio,
                                                                  const float* __restrict__ table, float* __restrict__ hist_all,
                                                                  float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rss_lds[];
  float* tab_s = rss_lds;                     // [TT_RS_TABLE]
  float* span_s = rss_lds + TT_RS_TABLE + 3;  // [kRssTableSpan]
  RssItem it;
  int tile;
  if (!rss_find(a, TT_RSS_TABLE, blockIdx.x, kRssTableTile, &it, &tile)) return;  // (uniform over the workgroup)
  const int t = threadIdx.x;
  const float* chunk = audio + it.in_off;
  if (tile == 0) rss_advance_history<kRssTableTile>(it, hist_all, chunk);
  const int m0 = it.m0 + tile * kRssTableTile, m1 = min(m0 + kRssTableTile, it.m1);
  if (m0 >= m1) return;  // the push emits nothing
  const float* hist = hist_all + ((size_t)it.slot * 2 + it.parity) * TT_RSS_HIST;
  const int P = it.P, Q = it.Q, H = it.H;
  const unsigned cq = rs_cq(P, Q);
  const float c32 = rs_c32(P, Q);
  for (int e = t; e < TT_RS_TABLE; e += kRssTableTile) tab_s[e] = table[e];
  const int j0 = (int)((long long)m0 * P / Q) - H;  // the first input the tile touches
  const int span = (int)((long long)(m1 - 1) * P / Q) + H + 1 - j0 + 1;
  for (int e = t; e < span; e += kRssTableTile) span_s[e] = rss_sample(it, hist, chunk, j0 + e);
  __syncthreads();
  const int m = m0 + t;
  if (m < m1) {
    const long long num = (long long)m * P;
    const int i = (int)(num / Q), r = (int)(num % Q);
    out[(size_t)it.out_off + (m - it.m0)] = rs_output(tab_s, span_s + (i - H - j0), H, cq, Q, r, c32);
  }
}

__global__ __launch_bounds__(kRssBankTile) void rss_bank_kernel(RssArgs a, const float* __restrict__ audio,
                                                                const float* __restrict__ banks, float* __restrict__ hist_all,
                                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rss_lds[];
  float* span_s = rss_lds;                 // [kRssBankSpan]
  float* bank_s = rss_lds + kRssBankSpan;  // [Q][W + 1]
  RssItem it;
  int tile;
  if (!rss_find(a, TT_RSS_BANK, blockIdx.x, kRssBankTile, &it, &tile)) return;  // (uniform over the workgroup)
  const int t = threadIdx.x;
  const float* chunk = audio + it.in_off;
  if (tile == 0) rss_advance_history<kRssBankTile>(it, hist_all, chunk);
  const int m0 = it.m0 + tile * kRssBankTile, m1 = min(m0 + kRssBankTile, it.m1);
  if (m0 >= m1) return;  // the push emits nothing
  const float* hist = hist_all + ((size_t)it.slot * 2 + it.parity) * TT_RSS_HIST;
  const float* bank = banks + (size_t)it.slot * TT_RSS_BANK_MAX;
  const int P = it.P, Q = it.Q, H = it.H, W = 2 * H + 2, S = W + 1;
  for (int e = t; e < Q * W; e += kRssBankTile) bank_s[(e / W) * S + e % W] = bank[e];
  const int j0 = (int)((long long)m0 * P / Q) - H;  // the first input the tile touches
  const int span = (int)((long long)(m1 - 1) * P / Q) + H + 1 - j0 + 1;
  for (int e = t; e < span; e += kRssBankTile) span_s[e] = rss_sample(it, hist, chunk, j0 + e);
  __syncthreads();
  const int m = m0 + t;
  if (m < m1) {
    const long long num = (long long)m * P;
    const int i = (int)(num / Q), r = (int)(num % Q);
    const float* xs = span_s + (i - H - j0);  // x[i - H ..]
    const float* row = bank_s + r * S;
    float acc = 0.f;
    for (int d = 0; d < W; ++d) acc = fmaf(row[d], xs[d], acc);
    out[(size_t)it.out_off + (m - it.m0)] = acc;
  }
}

// bank[r][d + H] = h_j of phase r and tap d = -H .. H + 1: rs_output's u and rs_tap_weight, from the table in global memory
__global__ __launch_bounds__(256) void rss_bank_build_kernel(int P, int Q, const float* __restrict__ table, float* __restrict__ bank) {
  const unsigned cq = rs_cq(P, Q);
  const int H = rs_half_width(cq), W = 2 * H + 2;
  const float c32 = rs_c32(P, Q);
  for (int e = blockIdx.x * 256 + threadIdx.x; e < Q * W; e += gridDim.x * 256) {
    const int r = e / W, d = e % W - H;
    unsigned f, g_up;
    rs_phase(r, cq, Q, &f, &g_up);
    bank[e] = rs_tap_weight(table, rs_tap_u(d, cq, f, g_up), c32);
  }
}

}  // namespace tt

using namespace tt;

struct tt_rss : EngineHandle {
  RssBook book;
  float* table = nullptr;  // [TT_RS_TABLE] the prototype, as tt_rs has it
  float* hist = nullptr;   // [max_streams][2][TT_RSS_HIST]
  float* banks = nullptr;  // [max_streams][TT_RSS_BANK_MAX] (not for a TT_RSS_TABLE handle)
};

static const int kRssTileOut[3] = {1, kRssTableTile, kRssBankTile};  // by form (TT_RSS_AUTO is no slot's form)

extern "C" {

int tt_rss_abi_version(void) { return 1; }  // ABI changes

int tt_rss_ready(int n_in_before, int n_chunk, int P, int Q, int flush) { return rss_ready(n_in_before, n_chunk, P, Q, flush); }

int tt_rss_create(int max_streams, int form, tt_rss** out) {
  TT_REQUIRE(out, "tt_rss_create: null argument");
  TT_REQUIRE(max_streams >= 1 && max_streams <= TT_RSS_MAX_STREAMS, "tt_rss_create: max_streams %d (1 .. %d)", max_streams, TT_RSS_MAX_STREAMS);
  TT_REQUIRE(form == TT_RSS_AUTO || form == TT_RSS_TABLE || form == TT_RSS_BANK, "tt_rss_create: form %d (TT_RSS_AUTO, _TABLE, _BANK)", form);
  tt_rss* e = new tt_rss();
  e->book.init(max_streams, form);
  int rc = e->open("tt_rss_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->table, TT_RS_TABLE, false);
  if (!rc) rc = e->arena.alloc_t(&e->hist, (size_t)max_streams * 2 * TT_RSS_HIST, true);
  if (!rc && form != TT_RSS_TABLE) rc = e->arena.alloc_t(&e->banks, (size_t)max_streams * TT_RSS_BANK_MAX, true);
  if (!rc) {
    std::vector<float> tab(TT_RS_TABLE);
    rs_fill_table(tab.data());
    if (hipMemcpy(e->table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipFuncSetAttribute((const void*)rss_table_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRssTableLds) != hipSuccess ||
        hipFuncSetAttribute((const void*)rss_bank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((kRssBankLdsMax + kRssBankSpan) * sizeof(float))) != hipSuccess) {
      set_error("tt_rss_create: the table upload or the kernels' LDS setting failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_rss_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_rss_destroy(tt_rss* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_rss_open(tt_rss* e, int slot, int P, int Q, void* stream) {
  TT_REQUIRE(e, "tt_rss_open: null argument");
  char err[256];
  if (e->book.check_open(slot, P, Q, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  const int form = e->book.form_for(P, Q);
  const int rc = e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    if (form == TT_RSS_BANK) {
      const int W = 2 * rs_half_width(rs_cq(P, Q)) + 2;
      rss_bank_build_kernel<<<(Q * W + 255) / 256, 256, 0, s>>>(P, Q, e->table, e->banks + (size_t)slot * TT_RSS_BANK_MAX);
      TT_CHECK_HIP(hipGetLastError());
    }
    return 0;
  });
  if (rc) return rc;
  e->book.commit_open(slot, P, Q);
  return 0;
}

int tt_rss_close(tt_rss* e, int slot) {
  TT_REQUIRE(e, "tt_rss_close: null argument");
  char err[256];
  if (e->book.close(slot, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  return 0;
}

int tt_rss_state(tt_rss* e, int slot, int* n_in, int* m_out, int* finished, int* form) {
  TT_REQUIRE(e, "tt_rss_state: null argument");
  TT_REQUIRE(slot >= 0 && slot < e->book.max_streams(), "tt_rss_state: slot %d (0 .. %d)", slot, e->book.max_streams() - 1);
  const RssSlot& s = e->book.slots[(size_t)slot];
  TT_REQUIRE(s.state != kRssClosed, "tt_rss_state: slot %d is closed", slot);
  if (n_in) *n_in = s.n_in;
  if (m_out) *m_out = s.m_out;
  if (finished) *finished = s.state == kRssFinished;
  if (form) *form = s.form;
  return 0;
}

int tt_rss_push(tt_rss* e, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, void* stream) {
  TT_REQUIRE(e && audio && out, "tt_rss_push: null argument");
  char err[256];
  std::vector<RssItem> items;
  int tiles[3];
  if (e->book.plan(n_push, slots, n_chunk, flush, kRssTileOut, &items, tiles, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  RssArgs a;
  a.n = n_push;
  size_t bank_floats = 0;  // the largest staged bank among the pushed slots
  for (int i = 0; i < n_push; ++i) {
    a.it[i] = items[(size_t)i];
    if (e->book.slots[(size_t)items[(size_t)i].slot].form == TT_RSS_BANK) {
      const size_t W = 2 * (size_t)items[(size_t)i].H + 2;
      bank_floats = std::max(bank_floats, (size_t)items[(size_t)i].Q * (W + 1));
    }
  }
  const int rc = e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    if (tiles[TT_RSS_BANK]) {
      rss_bank_kernel<<<tiles[TT_RSS_BANK], kRssBankTile, (kRssBankSpan + bank_floats) * sizeof(float), s>>>(a, audio, e->banks, e->hist,
                                                                                                             out);
      TT_CHECK_HIP(hipGetLastError());
    }
    if (tiles[TT_RSS_TABLE]) {
      rss_table_kernel<<<tiles[TT_RSS_TABLE], kRssTableTile, kRssTableLds, s>>>(a, audio, e->table, e->hist, out);
      TT_CHECK_HIP(hipGetLastError());
    }
    return 0;
  });
  if (rc) return rc;
  e->book.commit(items, flush);
  return 0;
}

}  // extern "C"
