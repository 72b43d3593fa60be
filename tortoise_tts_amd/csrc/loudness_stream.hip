// The streaming leveler (include/tortoise_mi355x_lvs.h): causal BS.1770 loudness, a slew-limited gain and the look-ahead limiter, fed in
// chunks.  The counters and every argument check are host code (loudness_stream_host.h); a push hands the kernels one LvsItem per pushed
// slot BY VALUE (no upload, no copy back) and is TWO launches, built from loudness_steps.h - the whole-clip kernels' arithmetic.
//
//   lvs_measure_kernel   ONE WORKGROUP PER PUSHED SLOT, 256 threads.
//     history            two copies and a parity, as tt_rss / tt_tss have them: both launches of a push read the current copy and the
//                        chunk, this one writes the OTHER copy (the last TT_LVS_HIST inputs after the push).
//     segments           the segments the push completes, 256 at a time, one THREAD per segment: the zero-state run, the carry from the
//                        slot's saved state (every thread runs the chain, thread i keeps the state in front of segment i), the second
//                        run into the segment's sum.  The samples are staged through LDS 30 per segment at a time (rows of 31 words: the
//                        lanes' reads fall into different banks), so 256 segments take 31 KB.
//     hops               thread 0 adds the segments' sums to the running hop's partial sum in ascending order and stores q_h where a hop
//                        ends.
//     gates              for each hop the push completes, loud_gate_kernel's sums over the prefix's blocks (the same 256-thread strides
//                        and tree) and the G_h step: a chain of a few hops per piece.
//   lvs_apply_kernel     a grid over (tile of TT_LVS_TILE outputs, pushed slot), 256 threads: the tile's inputs with a halo of D on either
//                        side from the history and the chunk into LDS, then P, r (with g[n] from the slot's gl), the sliding minimum, the
//                        Hann sum and the store; the readings by integer atomics (a maximum of the bits of non-negative floats, a count).
//   Nothing a slot computes depends on which other slots are pushed with it, or on the chunking.
#include <vector>
#include "runtime.h"
#include "loudness_steps.h"
#include "loudness_stream_host.h"

namespace tt {

constexpr int kLvSub = 30;   // samples of a segment staged at a time
constexpr int kLvTile = TT_LVS_TILE, kLvD = TT_LVS_DELAY;
static_assert(kLdS % kLvSub == 0 && kLvD == 2 * kLdLh + 8, "loudness_stream.hip's staging and halo");

struct LvsArgs {
  int n;
  LvsItem it[TT_LVS_MAX_STREAMS];
};

// the handle's device memory: per slot, and per slot and hop
struct LvsDev {
  float* hist;      // [slots][2][TT_LVS_HIST]
  double* st;       // [slots][8] carried state (4), the running hop's partial sum, G of the last hop
  unsigned* ist;    // [slots][4] bits of max P, bits of max |y|, samples limited
  double *q, *L, *G;            // [slots][max_hops]
  int *status, *babs, *brel;    // [slots][max_hops]
  float* gl;                    // [slots][max_hops + 2]: gl_-2, gl_-1, gl_0, ...
  int max_hops;
};
static_assert(sizeof(LvsArgs) + sizeof(LvsDev) + sizeof(LoudCoef) + 4 * sizeof(void*) <= 4096, "the items travel as kernel arguments");

// position j of the stream: the history below n_prev, the chunk up to n_end, 0 before sample 0 and from n_end on
struct LvsReader {
  const float* chunk;
  const float* hist;
  int n_prev, n_end;
  __device__ __forceinline__ float operator()(int j) const {
    if (j < 0 || j >= n_end) return 0.f;
    if (j >= n_prev) return chunk[j - n_prev];
    const int e = j - n_prev + TT_LVS_HIST;  // (e < 0 is beyond either reader's reach: loudness_stream_host.h)
    return e >= 0 ? hist[e] : 0.f;
  }
};

__device__ __forceinline__ LvsReader lvs_reader(const LvsItem& it, const LvsDev& d, const float* audio) {
  return {audio + it.in_off, d.hist + ((size_t)it.slot * 2 + lvs_parity(it)) * TT_LVS_HIST, it.n_prev, it.n_end};
}

// the segments base .. base + cnt - 1, one per thread, kLvSub samples at a time through xs
template <int PASS>
__device__ __forceinline__ void lvs_run(const LoudCoef& k, const LvsReader& rd, float* xs, int base, int cnt, LoudMem& m, double& e) {
  const int t = threadIdx.x;
  for (int sub = 0; sub < kLdS / kLvSub; ++sub) {
    for (int i = t; i < cnt * kLvSub; i += kLdThreads) {
      const int row = i / kLvSub, c = i - row * kLvSub;
      xs[row * (kLvSub + 1) + c] = rd((base + row) * kLdS + sub * kLvSub + c);
    }
    __syncthreads();
    if (t < cnt) loud_segment<PASS>(k, [&](int j) { return (double)xs[t * (kLvSub + 1) + j]; }, kLvSub, m, e);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLdThreads) void lvs_measure_kernel(LvsArgs a, LoudCoef k, LvsDev d, const float* __restrict__ audio) {
  __shared__ float xs[kLdThreads * (kLvSub + 1)];
  __shared__ double zs[kLdThreads][4];
  __shared__ double se[kLdThreads];
  __shared__ double red[kLdThreads];
  if ((int)blockIdx.x >= a.n) return;  // (uniform over the workgroup)
  const LvsItem it = a.it[blockIdx.x];
  const int t = threadIdx.x;
  const LvsReader rd = lvs_reader(it, d, audio);
  {  // the history after this push, into the other copy
    float* next = d.hist + ((size_t)it.slot * 2 + (lvs_parity(it) ^ 1)) * TT_LVS_HIST;
    for (int i = t; i < TT_LVS_HIST; i += kLdThreads) next[i] = rd(it.n_end - TT_LVS_HIST + i);
  }
  double* st = d.st + (size_t)it.slot * 8;
  const size_t row = (size_t)it.slot * (size_t)d.max_hops;
  double* q = d.q + row;
  float* gl = d.gl + row + 2 * (size_t)it.slot;
  double S[4] = {0.0, 0.0, 0.0, 0.0}, partial = 0.0, Gprev;  // (S and Gprev the same in every thread; the partial sum is thread 0's)
  if (lvs_first(it)) {
    Gprev = 20.0 * log10((double)it.gain0);
    if (t == 0) {
      gl[0] = it.gain0; gl[1] = it.gain0;
      unsigned* ist = d.ist + (size_t)it.slot * 4;
      ist[0] = 0u; ist[1] = 0u; ist[2] = 0u;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) S[r] = st[r];
    partial = st[4];
    Gprev = st[5];
  }
  const int seg0 = it.n_prev / kLdS, seg1 = it.n_end / kLdS;
  for (int base = seg0; base < seg1; base += kLdThreads) {
    const int cnt = min(kLdThreads, seg1 - base);
    const int first = (base + t) * kLdS;  // (unused beyond cnt)
    const double x1 = t < cnt ? (double)rd(first - 1) : 0.0, x2 = t < cnt ? (double)rd(first - 2) : 0.0;
    LoudMem m = {x1, x2, 0.0, 0.0, 0.0, 0.0};
    double e = 0.0;
    lvs_run<0>(k, rd, xs, base, cnt, m, e);
    zs[t][0] = m.v1; zs[t][1] = m.v2; zs[t][2] = m.y1; zs[t][3] = m.y2;
    __syncthreads();
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < cnt; ++i) {
      if (t == i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[r] = S[r];
      }
      loud_carry_step(k, zs[i], S);
    }
    m = {x1, x2, mine[0], mine[1], mine[2], mine[3]};
    lvs_run<1>(k, rd, xs, base, cnt, m, e);
    se[t] = e;
    __syncthreads();
    if (t == 0) {
      constexpr int per = kLdH / kLdS;
      for (int i = 0; i < cnt; ++i) {
        partial += se[i];
        if ((base + i) % per == per - 1) {
          q[(base + i) / per] = partial;
          partial = 0.0;
        }
      }
    }
    __syncthreads();  // (zs and se are written again)
  }
  __threadfence();  // (the hop energies are read back below by other threads of the workgroup)
  __syncthreads();
  const int hop0 = it.n_prev / kLdH, hop1 = it.n_end / kLdH;
  const double T = (double)it.target, boost = (double)it.boost, cut = (double)it.cut, rise = (double)it.rise, fall = (double)it.fall;
  for (int h = hop0; h < hop1; ++h) {
    const LoudGates gt = loud_gates(q, h >= 3 ? h - 2 : 0, k.z_abs, red);
    double G = Gprev;
    float glh = it.gain0;
    if (lvs_steer(it) == TT_LVS_ADAPT) {
      double D = Gprev;
      if (gt.st == TT_LOUD_OK) D = fmin(fmax(T - gt.L, -cut), boost);
      const double down = -(0.1 * fall), up = 0.1 * rise;
      const double step = fmin(fmax(D - Gprev, down), up);
      G = Gprev + step;
      glh = loud_gain_of_db(G);
    }
    if (t == 0) {
      d.L[row + h] = gt.L; d.G[row + h] = G;
      d.status[row + h] = gt.st; d.babs[row + h] = (int)gt.na; d.brel[row + h] = (int)gt.nr;
      gl[h + 2] = glh;
    }
    Gprev = G;
  }
  if (t == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) st[r] = S[r];
    st[4] = partial;
    st[5] = Gprev;
  }
}

__global__ __launch_bounds__(kLdThreads) void lvs_apply_kernel(LvsArgs a, LvsDev d, const float* __restrict__ table, const float* __restrict__ audio,
                                                               float* __restrict__ out) {
  __shared__ float xs[kLvTile + 2 * kLvD];       // x[t0 - 248 ..]
  __shared__ float Ps[kLvTile + 4 * kLdLh + 1];  // P[t0 - 241 ..]
  __shared__ float rs[kLvTile + 4 * kLdLh];      // r[t0 - 240 ..]
  __shared__ float ds[kLvTile + 2 * kLdLh];      // 1 - m[t0 - 120 ..]
  __shared__ float tab[kLdTable];
  const LvsItem it = a.it[blockIdx.y];
  const int t = threadIdx.x;
  const int limit = lvs_limit(it);
  const int n_out = lvs_ready_total(it.n_prev, limit, false), ready = lvs_ready_total(it.n_end, limit, lvs_flush(it));
  const int t0 = n_out + (int)blockIdx.x * kLvTile;
  if (t0 >= ready) return;  // (uniform over the workgroup)
  const int cnt = min(kLvTile, ready - t0);
  const LvsReader rd = lvs_reader(it, d, audio);
  const float* gl = d.gl + (size_t)it.slot * ((size_t)d.max_hops + 2);
  float* y = out + it.out_off + (t0 - n_out);
  auto gain = [&](int n) {  // g[n], n below n_end: the hop before n's is measured
    const int h = n / kLdH;
    const float tt = (float)(n - h * kLdH) / 2400.f, g0 = gl[h], g1 = gl[h + 1];
    return fmaf(tt, g1 - g0, g0);
  };
  if (limit == TT_LVS_NONE) {
    float mx = 0.f;
    for (int i = t; i < cnt; i += kLdThreads) {
      const float v = gain(t0 + i) * rd(t0 + i);
      y[i] = v;
      mx = fmaxf(mx, fabsf(v));
    }
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if ((t & 63) == 0) atomicMax(d.ist + (size_t)it.slot * 4 + 1, __float_as_uint(mx));  // (non-negative floats order as their bits)
    return;
  }
  for (int i = t; i < kLdTable; i += kLdThreads) tab[i] = table[i];
  for (int i = t; i < kLvTile + 2 * kLvD; i += kLdThreads) xs[i] = rd(t0 - kLvD + i);
  __syncthreads();
  for (int i = t; i < kLvTile + 4 * kLdLh + 1; i += kLdThreads) {
    const int s = t0 - (2 * kLdLh + 1) + i;  // xs index of x[s - 7] is i
    Ps[i] = s >= 0 && s < it.n_end ? loud_peak_at(xs + i, tab) : 0.f;
  }
  __syncthreads();
  for (int i = t; i < kLvTile + 4 * kLdLh; i += kLdThreads) {
    const int s = t0 - 2 * kLdLh + i;
    rs[i] = s >= 0 && s < it.n_end ? loud_ratio(it.ceiling, gain(s), Ps[i], Ps[i + 1]) : 1.f;
  }
  __syncthreads();
  for (int i = t; i < cnt + 2 * kLdLh; i += kLdThreads) ds[i] = loud_slide(rs + i);
  __syncthreads();
  const float* wn = tab + 3 * kLdTaps;
  float mp = 0.f, my = 0.f;
  int lim = 0;
  for (int i = t; i < cnt; i += kLdThreads) {
    const float s = loud_smooth(wn, ds + i, rs[i + 2 * kLdLh]);
    const float v = (gain(t0 + i) * xs[i + kLvD]) * s;
    y[i] = v;
    mp = fmaxf(mp, Ps[i + 2 * kLdLh + 1]);
    my = fmaxf(my, fabsf(v));
    lim += s < 1.f;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    mp = fmaxf(mp, __shfl_xor(mp, m));
    my = fmaxf(my, __shfl_xor(my, m));
    lim += __shfl_xor(lim, m);
  }
  if ((t & 63) == 0) {
    unsigned* ist = d.ist + (size_t)it.slot * 4;
    atomicMax(ist, __float_as_uint(mp));
    atomicMax(ist + 1, __float_as_uint(my));
    if (lim) atomicAdd(ist + 2, (unsigned)lim);
  }
}

}  // namespace tt

using namespace tt;

struct tt_lvs : EngineHandle {
  LvsBook book;
  LoudCoef coef;
  LvsDev dev = {};
  float* table = nullptr;  // [kLdTable] as tt_loud has it
};

extern "C" {

int tt_lvs_abi_version(void) { return 1; }  // ABI changes

int tt_lvs_ready(int n_in_before, int n_chunk, int limit, int flush) { return lvs_ready(n_in_before, n_chunk, limit, flush); }

int tt_lvs_create(int max_streams, int max_hops, tt_lvs** out) {
  TT_REQUIRE(out, "tt_lvs_create: null argument");
  TT_REQUIRE(max_streams >= 1 && max_streams <= TT_LVS_MAX_STREAMS, "tt_lvs_create: max_streams %d (1 .. %d)", max_streams, TT_LVS_MAX_STREAMS);
  TT_REQUIRE(max_hops >= 0 && max_hops <= TT_LVS_MAX_HOPS, "tt_lvs_create: max_hops %d (1 .. %d, 0 for %d)", max_hops, TT_LVS_MAX_HOPS,
             TT_LVS_DEFAULT_HOPS);
  if (max_hops == 0) max_hops = TT_LVS_DEFAULT_HOPS;
  tt_lvs* e = new tt_lvs();
  e->book.init(max_streams, max_hops);
  loud_design(&e->coef);
  LvsDev& d = e->dev;
  d.max_hops = max_hops;
  const size_t n = (size_t)max_streams, nh = n * (size_t)max_hops;
  int rc = e->open("tt_lvs_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->table, kLdTable, false);
  if (!rc) rc = e->arena.alloc_t(&d.hist, n * 2 * TT_LVS_HIST, true);
  if (!rc) rc = e->arena.alloc_t(&d.st, n * 8, true);
  if (!rc) rc = e->arena.alloc_t(&d.ist, n * 4, true);
  if (!rc) rc = e->arena.alloc_t(&d.q, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.L, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.G, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.status, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.babs, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.brel, nh, true);
  if (!rc) rc = e->arena.alloc_t(&d.gl, nh + 2 * n, true);
  if (!rc) {
    float tab[kLdTable];
    loud_table(tab);
    if (hipMemcpy(e->table, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("tt_lvs_create: the table upload failed");
      rc = -2;
    }
  }
  if (rc) {
    tt_lvs_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_lvs_destroy(tt_lvs* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_lvs_open(tt_lvs* e, int slot, int steer, int limit, float gain0, float target, float ceiling, float boost, float cut, float rise,
                float fall) {
  TT_REQUIRE(e, "tt_lvs_open: null argument");
  char err[256];
  if (e->book.check_open(slot, steer, limit, gain0, target, ceiling, boost, cut, rise, fall, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  e->book.commit_open(slot, steer, limit, gain0, target, ceiling, boost, cut, rise, fall);
  return 0;
}

int tt_lvs_close(tt_lvs* e, int slot) {
  TT_REQUIRE(e, "tt_lvs_close: null argument");
  char err[256];
  if (e->book.close(slot, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  return 0;
}

int tt_lvs_state(tt_lvs* e, int slot, int* n_in, int* n_out, int* hops_done, int* finished) {
  TT_REQUIRE(e, "tt_lvs_state: null argument");
  TT_REQUIRE(slot >= 0 && slot < e->book.max_streams(), "tt_lvs_state: slot %d (0 .. %d)", slot, e->book.max_streams() - 1);
  const LvsSlot& s = e->book.slots[(size_t)slot];
  TT_REQUIRE(s.state != kLvsClosed, "tt_lvs_state: slot %d is closed", slot);
  if (n_in) *n_in = s.n_in;
  if (n_out) *n_out = s.n_out;
  if (hops_done) *hops_done = s.hops;
  if (finished) *finished = s.state == kLvsFinished;
  return 0;
}

int tt_lvs_push(tt_lvs* e, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, void* stream) {
  TT_REQUIRE(e && audio && out, "tt_lvs_push: null argument");
  char err[256];
  std::vector<LvsItem> items;
  int most = 0;
  if (e->book.plan(n_push, slots, n_chunk, flush, &items, &most, err, sizeof(err))) {
    set_error("%s", err);
    return -1;
  }
  LvsArgs a;
  a.n = n_push;
  for (int i = 0; i < n_push; ++i) a.it[i] = items[(size_t)i];
  const int tiles = (most + kLvTile - 1) / kLvTile;
  const int rc = e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    lvs_measure_kernel<<<n_push, kLdThreads, 0, s>>>(a, e->coef, e->dev, audio);
    if (tiles > 0) lvs_apply_kernel<<<dim3((unsigned)tiles, (unsigned)n_push), kLdThreads, 0, s>>>(a, e->dev, e->table, audio, out);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  e->book.commit(items);
  return 0;
}

int tt_lvs_read(tt_lvs* e, int slot, double* lufs, int* status, int* blocks_abs, int* blocks_rel, double* gain_db, float* gain, float* peak,
                float* out_peak, int* limited, void* stream) {
  TT_REQUIRE(e, "tt_lvs_read: null argument");
  TT_REQUIRE(slot >= 0 && slot < e->book.max_streams(), "tt_lvs_read: slot %d (0 .. %d)", slot, e->book.max_streams() - 1);
  const LvsSlot& s = e->book.slots[(size_t)slot];
  TT_REQUIRE(s.state != kLvsClosed, "tt_lvs_read: slot %d is closed", slot);
  double L = -HUGE_VAL, G = 20.0 * log10((double)s.gain0);
  int st = TT_LOUD_SHORT, ba = 0, br = 0;
  float g = s.gain0;
  unsigned ist[4] = {0u, 0u, 0u, 0u};
  if (s.pushes > 0) {
    const LvsDev& d = e->dev;
    const size_t at = (size_t)slot * (size_t)d.max_hops + (size_t)(s.hops > 0 ? s.hops - 1 : 0);
    const int rc = e->sb.run((hipStream_t)stream, [&](hipStream_t q) -> int {
      TT_CHECK_HIP(hipMemcpyAsync(ist, d.ist + (size_t)slot * 4, sizeof(ist), hipMemcpyDeviceToHost, q));
      if (s.hops > 0) {
        TT_CHECK_HIP(hipMemcpyAsync(&L, d.L + at, sizeof(double), hipMemcpyDeviceToHost, q));
        TT_CHECK_HIP(hipMemcpyAsync(&G, d.G + at, sizeof(double), hipMemcpyDeviceToHost, q));
        TT_CHECK_HIP(hipMemcpyAsync(&st, d.status + at, sizeof(int), hipMemcpyDeviceToHost, q));
        TT_CHECK_HIP(hipMemcpyAsync(&ba, d.babs + at, sizeof(int), hipMemcpyDeviceToHost, q));
        TT_CHECK_HIP(hipMemcpyAsync(&br, d.brel + at, sizeof(int), hipMemcpyDeviceToHost, q));
        TT_CHECK_HIP(hipMemcpyAsync(&g, d.gl + at + 2 * (size_t)slot + 2, sizeof(float), hipMemcpyDeviceToHost, q));
      }
      TT_CHECK_HIP(hipStreamSynchronize(q));
      return 0;
    });
    if (rc) return rc;
  }
  if (lufs) *lufs = L;
  if (status) *status = st;
  if (blocks_abs) *blocks_abs = ba;
  if (blocks_rel) *blocks_rel = br;
  if (gain_db) *gain_db = G;
  if (gain) *gain = g;
  if (peak) memcpy(peak, &ist[0], sizeof(float));
  if (out_peak) memcpy(out_peak, &ist[1], sizeof(float));
  if (limited) *limited = (int)ist[2];
  return 0;
}

int tt_lvs_trace(tt_lvs* e, int slot, int first_hop, int count, double* q, double* lufs, double* gain_db, int* status, int* blocks_abs,
                 int* blocks_rel, void* stream) {
  TT_REQUIRE(e, "tt_lvs_trace: null argument");
  TT_REQUIRE(slot >= 0 && slot < e->book.max_streams(), "tt_lvs_trace: slot %d (0 .. %d)", slot, e->book.max_streams() - 1);
  const LvsSlot& s = e->book.slots[(size_t)slot];
  TT_REQUIRE(s.state != kLvsClosed, "tt_lvs_trace: slot %d is closed", slot);
  TT_REQUIRE(first_hop >= 0 && count >= 0 && (long long)first_hop + count <= s.hops, "tt_lvs_trace: hops %d + %d of the %d measured", first_hop,
             count, s.hops);
  if (count == 0) return 0;
  const LvsDev& d = e->dev;
  const size_t at = (size_t)slot * (size_t)d.max_hops + (size_t)first_hop, c = (size_t)count;
  return e->sb.run((hipStream_t)stream, [&](hipStream_t sq) -> int {
    if (q) TT_CHECK_HIP(hipMemcpyAsync(q, d.q + at, c * sizeof(double), hipMemcpyDeviceToHost, sq));
    if (lufs) TT_CHECK_HIP(hipMemcpyAsync(lufs, d.L + at, c * sizeof(double), hipMemcpyDeviceToHost, sq));
    if (gain_db) TT_CHECK_HIP(hipMemcpyAsync(gain_db, d.G + at, c * sizeof(double), hipMemcpyDeviceToHost, sq));
    if (status) TT_CHECK_HIP(hipMemcpyAsync(status, d.status + at, c * sizeof(int), hipMemcpyDeviceToHost, sq));
    if (blocks_abs) TT_CHECK_HIP(hipMemcpyAsync(blocks_abs, d.babs + at, c * sizeof(int), hipMemcpyDeviceToHost, sq));
    if (blocks_rel) TT_CHECK_HIP(hipMemcpyAsync(blocks_rel, d.brel + at, c * sizeof(int), hipMemcpyDeviceToHost, sq));
    TT_CHECK_HIP(hipStreamSynchronize(sq));
    return 0;
  });
}

}  // extern "C"
