// Band-limited resampling along a pitch map (include/tortoise_mi355x_rsw.h): the resampler of resample.hip with a pitch ratio that changes
// inside the clip.
//
//   rsw_prepare_kernel   one workgroup: every clip's status (the table is checked here, row by row with rsw_row_ok and rsw_tail of
//                        resample_warp_host.h, the code the host plans and checks with), and a zero in `peak` for the clips that will be
//                        resampled.
//   rsw_resample_kernel  rs_resample_kernel's decomposition: the work is (clip, tile of kRswTile = 1024 consecutive outputs), workgroup b
//                        takes tiles b, b + grid, ... of the list clip 0's tiles, clip 1's tiles, ..., which every workgroup derives from
//                        the offsets and the tables (rsw_clips, the prepare kernel's own verdict, so a refused clip has no tiles and
//                        nothing of it is written).  Nothing about an output depends on where its clip stands in the batch or on
//                        which workgroup computes it.
//     table              the 16385 prototype values in LDS, loaded once per workgroup and kept over its tiles, as in resample.hip.
//     segments           the clip's table (at most 64 x 4 integers) sits in LDS beside the cq, H and c32 of every segment (rs_cq,
//                        rs_half_width, rs_c32 of resample_steps.h, computed once per segment by thread i and not per output); reloaded
//                        when a workgroup's next tile belongs to another clip.
//     search             the segments of a tile's first and last output (lo, hi) are found by a uniform scan; an output then starts at lo
//                        and steps forward while the next border is not beyond it.  A tile inside one segment - all but S - 1 of a clip's
//                        tiles - steps zero times.
//     span               x[i(first) - Hmax .. i(last) + Hmax + 1], Hmax the widest H of the segments lo .. hi, staged once with zeros
//                        outside the clip.  The position is monotone across borders, so first and last output bound every index; with
//                        P <= 2 * 65536 and H <= 72 that is at most 1023 * 2 + 1 + 2 * 72 + 2 = 2193 samples, a quarter of resample.hip's
//                        8756, and the LDS of a workgroup is 75 KB: TWO workgroups of 1024 threads fit a CU (kRswPerCu).
//     thread             one output: pos = t_i + (m - m_i) P_i in 64 bits, index pos >> 16, phase pos & 65535, then rs_output of
//                        resample_steps.h with Q = 65536 as a constant (rs_phase's division is a shift; its result is the same integer).
//                        Lanes of a wave on two sides of a border run different H, cq and c32: the tap loops diverge for that wave only.
//     peak               as in resample.hip: wave, workgroup, then ONE vector atomic max per tile.
#include <math.h>
#include <vector>
#include "runtime.h"
#include "resample_steps.h"
#include "resample_warp_host.h"

namespace tt {

#ifndef TT_RSW_PER_CU
#define TT_RSW_PER_CU 2  // workgroups per CU the grid is sized for (the LDS allows two); -D for an A/B build (build.py variants), profiles/r26_pitchmap.txt
#endif
constexpr int kRswThreads = 1024, kRswTile = kRswThreads, kRswPerCu = TT_RSW_PER_CU;
constexpr unsigned kRswCqMin = (unsigned)(kRsCqNum * TT_RS_PITCH_ONE / ((long long)TT_RS_RHO_DEN * TT_RSW_P_MAX));  // cq at P = 2 * 65536
constexpr int kRswHMax = (int)((kRsOne + kRswCqMin - 1) / kRswCqMin);                                            // 72
constexpr int kRswSpan = ((kRswTile - 1) * (TT_RSW_P_MAX / TT_RS_PITCH_ONE) + 1 + 2 * kRswHMax + 2 + 15) / 16 * 16;  // samples of LDS for a tile's inputs
constexpr size_t kRswLds = (size_t)(TT_RS_TABLE + 3 + kRswSpan) * sizeof(float);
static_assert(kRswHMax == 72 && TT_RSW_P_MAX == 2 * TT_RS_PITCH_ONE && kRswThreads >= TT_RS_MAX_CLIPS && kRswThreads >= 4 * TT_RSW_MAX_SEGMENTS &&
              kRswThreads % TT_RSW_MAX_SEGMENTS == 0,
              "the widest filter of the pitch range, and one thread per clip and per table entry");
static_assert(kRswPerCu * (kRswLds + 4096) <= 160 * 1024, "rsw_resample_kernel's LDS plan (4 KB: its static arrays, rounded up)");

// Every clip's verdict, by all kRswThreads threads of a workgroup alike: st_s[c] the status, len_s[c] and nout_s[c] the length and output
// length of an OK clip (0 otherwise).  Thread c takes clip c's sizes; then the rows are checked side by side, thread 64 k + i row i of clip
// 16 j + k in pass j (rsw_row_ok of resample_warp_host.h: a row's rules involve its successor alone), so that a table of 64 segments costs
// what one of 1 costs - as first built, one thread walked its clip's rows in turn, 64 dependent trips to memory ahead of every workgroup's
// first tile (profiles/r26_pitchmap.txt); then thread c takes the table's end and the slice of out.
__device__ static inline void rsw_clips(int n_clips, const int* __restrict__ in_off, const int* __restrict__ seg, const int* __restrict__ seg_off,
                                        const int* __restrict__ out_off, int max_samples, int max_segments, int* st_s, int* len_s, int* nout_s,
                                        int* bad_s, int t) {
  if (t < TT_RS_MAX_CLIPS) {
    int st = TT_RSW_REFUSED, n = 0;
    if (t < n_clips) {
      const int i0 = in_off[t], s0 = seg_off[t], S = seg_off[t + 1] - s0;
      n = in_off[t + 1] - i0;
      if (i0 < 0 || n < 0) st = TT_RSW_REFUSED;
      else if (n == 0) st = TT_RSW_EMPTY;
      else if (n > max_samples || s0 < 0 || S < 1 || S > max_segments || !rsw_sizes_ok(n, S)) st = TT_RSW_REFUSED;
      else st = TT_RSW_OK;
    }
    st_s[t] = st;
    len_s[t] = st == TT_RSW_OK ? n : 0;
    nout_s[t] = 0;
    bad_s[t] = 0;
  }
  __syncthreads();
  for (int base = 0; base < n_clips; base += kRswThreads / TT_RSW_MAX_SEGMENTS) {
    const int c = base + t / TT_RSW_MAX_SEGMENTS, i = t % TT_RSW_MAX_SEGMENTS;
    if (c < n_clips && st_s[c] == TT_RSW_OK) {
      const int s0 = seg_off[c], S = seg_off[c + 1] - s0;
      if (i < S && !rsw_row_ok(S, seg + 4 * (long long)s0, i)) bad_s[c] = 1;  // (every writer writes 1)
    }
  }
  __syncthreads();
  if (t < n_clips && st_s[t] == TT_RSW_OK) {
    const int s0 = seg_off[t], S = seg_off[t + 1] - s0, o0 = out_off[t];
    const int n_out = bad_s[t] ? 0 : rsw_tail(len_s[t], S, seg + 4 * (long long)s0);  // 0: the table breaks a rule
    if (n_out == 0 || o0 < 0 || out_off[t + 1] - o0 != n_out) {  // nothing is written outside the clip's own slice
      st_s[t] = TT_RSW_REFUSED;
      len_s[t] = 0;
    } else {
      nout_s[t] = n_out;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kRswThreads) void rsw_prepare_kernel(int n_clips, const int* __restrict__ in_off, const int* __restrict__ seg,
                                                                  const int* __restrict__ seg_off, const int* __restrict__ out_off,
                                                                  int max_samples, int max_segments, float* __restrict__ peak,
                                                                  int* __restrict__ status) {
  __shared__ int st_s[TT_RS_MAX_CLIPS], len_s[TT_RS_MAX_CLIPS], nout_s[TT_RS_MAX_CLIPS], bad_s[TT_RS_MAX_CLIPS];
  const int c = threadIdx.x;
  rsw_clips(n_clips, in_off, seg, seg_off, out_off, max_samples, max_segments, st_s, len_s, nout_s, bad_s, c);
  if (c >= n_clips) return;
  status[c] = st_s[c];
  if (st_s[c] == TT_RSW_OK && peak) peak[c] = 0.f;
}

__global__ __launch_bounds__(kRswThreads) void rsw_resample_kernel(int n_clips, const float* __restrict__ audio, const int* __restrict__ in_off,
                                                                   const int* __restrict__ seg, const int* __restrict__ seg_off,
                                                                   const float* __restrict__ table, int max_samples, int max_segments,
                                                                   float* __restrict__ out, const int* __restrict__ out_off,
                                                                   float* __restrict__ peak) {
  extern __shared__ __attribute__((aligned(16))) float rsw_lds[];
  float* tab_s = rsw_lds;                     // [TT_RS_TABLE]
  float* span_s = rsw_lds + TT_RS_TABLE + 3;  // [kRswSpan]
  __shared__ int st_s[TT_RS_MAX_CLIPS], len_s[TT_RS_MAX_CLIPS], nout_s[TT_RS_MAX_CLIPS], bad_s[TT_RS_MAX_CLIPS];
  __shared__ int seg_s[4 * TT_RSW_MAX_SEGMENTS], h_s[TT_RSW_MAX_SEGMENTS];
  __shared__ unsigned cq_s[TT_RSW_MAX_SEGMENTS];
  __shared__ float c32_s[TT_RSW_MAX_SEGMENTS];
  __shared__ float peak_s[kRswThreads / 64];
  const int t = threadIdx.x;
  rsw_clips(n_clips, in_off, seg, seg_off, out_off, max_samples, max_segments, st_s, len_s, nout_s, bad_s, t);  // nout_s 0: not resampled
  int total = 0;
  for (int c = 0; c < n_clips; ++c) total += (nout_s[c] + kRswTile - 1) / kRswTile;
  if ((int)blockIdx.x >= total) return;  // (uniform over the workgroup)
  for (int e = t; e < TT_RS_TABLE; e += kRswThreads) tab_s[e] = table[e];
  int have = -1;  // the clip whose segments are in LDS
  for (int g = blockIdx.x; g < total; g += gridDim.x) {
    int c = 0, first = 0;  // tile g is tile (g - first) of clip c
    for (;; ++c) {
      const int tiles = (nout_s[c] + kRswTile - 1) / kRswTile;
      if (g < first + tiles) break;
      first += tiles;
    }
    const int n = len_s[c], n_out = nout_s[c], S = seg_off[c + 1] - seg_off[c];
    const float* x = audio + in_off[c];
    float* y = out + out_off[c];
    __syncthreads();  // the previous tile's reads of span_s and of the segments are done
    if (c != have) {  // (uniform)
      const int* tb = seg + 4 * (long long)seg_off[c];
      if (t < 4 * S) seg_s[t] = tb[t];
      if (t < S) {
        const int P = tb[4 * t + 3];
        const unsigned cq = rs_cq(P, TT_RS_PITCH_ONE);
        cq_s[t] = cq;
        h_s[t] = rs_half_width(cq);
        c32_s[t] = rs_c32(P, TT_RS_PITCH_ONE);
      }
      have = c;
      __syncthreads();
    }
    const int m0 = (g - first) * kRswTile, m1 = min(m0 + kRswTile, n_out);  // this tile's outputs
    int lo = 0;
    while (lo + 1 < S && rsw_m(seg_s, lo + 1) <= m0) ++lo;
    int hi = lo, Hm = h_s[lo];
    while (hi + 1 < S && rsw_m(seg_s, hi + 1) <= m1 - 1) Hm = max(Hm, h_s[++hi]);
    const int j0 = (int)(rsw_position(m0, rsw_m(seg_s, lo), rsw_t(seg_s, lo), rsw_p(seg_s, lo)) >> 16) - Hm;  // the first input it touches
    const int span = (int)(rsw_position(m1 - 1, rsw_m(seg_s, hi), rsw_t(seg_s, hi), rsw_p(seg_s, hi)) >> 16) + Hm + 1 - j0 + 1;
    for (int e = t; e < span; e += kRswThreads) {
      const int j = j0 + e;
      span_s[e] = j >= 0 && j < n ? x[j] : 0.f;
    }
    __syncthreads();  // (also: the table is in place)
    float pk = 0.f;
    const int m = m0 + t;
    if (m < m1) {
      int i = lo;
      while (i < hi && rsw_m(seg_s, i + 1) <= m) ++i;
      const long long pos = rsw_position(m, rsw_m(seg_s, i), rsw_t(seg_s, i), rsw_p(seg_s, i));
      const int H = h_s[i];
      const float acc = rs_output(tab_s, span_s + ((int)(pos >> 16) - H - j0), H, cq_s[i], TT_RS_PITCH_ONE, (int)(pos & 65535), c32_s[i]);
      y[m] = acc;
      pk = fabsf(acc);
    }
    if (peak) {
      for (int s = 32; s >= 1; s >>= 1) pk = fmaxf(pk, __shfl_xor(pk, s));
      if ((t & 63) == 0) peak_s[t >> 6] = pk;
      __syncthreads();
      if (t == 0) {
#pragma unroll
        for (int w = 1; w < kRswThreads / 64; ++w) pk = fmaxf(pk, peak_s[w]);
        atomicMax((unsigned*)peak + c, __float_as_uint(pk));  // (non-negative floats order as their bits)
      }
    }
  }
}

}  // namespace tt

using namespace tt;

struct tt_rsw : EngineHandle {
  int max_samples = 0, max_clips = 0, max_segments = 0, grid = 0;
  float* table = nullptr;  // [TT_RS_TABLE] the prototype, fp64 values rounded to f32 (tt_rs_create's)
};

extern "C" {

int tt_rsw_abi_version(void) { return 1; }  // ABI changes

int tt_rsw_plan(int n, int n_segments, const int* starts, const int* ps, int* table_out) {
  char err[256];
  if (rsw_plan(n, n_segments, starts, ps, table_out, err, sizeof(err)) != 0) {
    set_error("%s", err);
    return -1;
  }
  return 0;
}

int tt_rsw_out_samples(int n, int n_segments, const int* table) { return table ? rsw_out_samples(n, n_segments, table) : 0; }

int tt_rsw_create(int max_samples, int max_clips, int max_segments, tt_rsw** out) {
  char err[256];
  TT_REQUIRE(out, "tt_rsw_create: null argument");
  TT_REQUIRE(rsw_check_create(max_samples, max_clips, max_segments, err, sizeof(err)) == 0, "%s", err);
  tt_rsw* e = new tt_rsw();
  e->max_samples = max_samples; e->max_clips = max_clips; e->max_segments = max_segments;
  int rc = e->open("tt_rsw_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->table, TT_RS_TABLE, false);
  if (!rc) {
    std::vector<float> tab(TT_RS_TABLE);
    rs_fill_table(tab.data());
    int dev = 0, cus = 0;
    if (hipMemcpy(e->table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
        hipFuncSetAttribute((const void*)rsw_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRswLds) != hipSuccess) {
      set_error("tt_rsw_create: the table upload or the kernel's LDS setting failed");
      rc = -2;
    }
    e->grid = cus * kRswPerCu;
  }
  if (rc) {
    tt_rsw_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_rsw_destroy(tt_rsw* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_rsw_resample(tt_rsw* e, int n_clips, const float* audio, const int* in_off, const int* seg, const int* seg_off, float* out,
                    const int* out_off, float* peak, int* status, void* stream) {
  char err[256];
  TT_REQUIRE(rsw_check_resample(e && audio && in_off && seg && seg_off && out && out_off && status, n_clips, e ? e->max_clips : 0, err,
                                sizeof(err)) == 0, "%s", err);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    rsw_prepare_kernel<<<1, kRswThreads, 0, s>>>(n_clips, in_off, seg, seg_off, out_off, e->max_samples, e->max_segments, peak, status);
    TT_CHECK_HIP(hipGetLastError());
    rsw_resample_kernel<<<e->grid, kRswThreads, kRswLds, s>>>(n_clips, audio, in_off, seg, seg_off, e->table, e->max_samples, e->max_segments,
                                                              out, out_off, peak);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
