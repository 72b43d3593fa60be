// Fundamental frequency (include/tortoise_mi355x_f0.h): a YIN tracker over ragged batches of finished clips.
//
//   f0_track_kernel   blockIdx = (group of kF0G = 4 consecutive frames, clip), 256 threads, one launch for the difference function, the scan
//                     and the pick, nothing in between in HBM.  Frames overlap: with slot sums S(s, tau) = sum_{j in slot s} (x[j] - x[j+tau])^2
//                     over slots of 240 samples, d_f(tau) is the sum of four slots' values, so the group computes kF0G + 3 = 7 slots' sums
//                     once - 1.75 times what the clip needs, against 4 times frame by frame.
//                       stage     the group's span, (kF0G + 3) 240 + 480 = 2160 floats, into LDS, zero outside the clip.
//                       slots     the register tiling of tsm_search: thread (u, h), u < 120, owns the four adjacent lags 4u + 1 .. 4u + 4
//                                 and half h of every slot (120 samples, ascending).  Per four samples one broadcast ds_read_b128 of
//                                 x[j ..] and one new aligned ds_read_b128 of x[j + 4u ..], consecutive over the lanes; the eight values
//                                 held feed all 16 (sample, lag) terms.  A term is one v_sub_f32 and one v_fma_f32.  After slot s >= 3 the
//                                 thread adds its last four slot sums, oldest first, ((S_s-3 + S_s-2) + S_s-1) + S_s: its half of d of
//                                 frame s - 3, to LDS.  d = half 0 + half 1.  At most 120 + 3 + 1 + 1 rounded operations on a path.
//                       scan      wave w takes frame w (and w + 4, ... of a larger group).  Lane l holds lags 8l + 1 .. 8l + 8: a local f64 running sum, a shuffle
//                                 scan of the lanes' totals, c = (sum of the lanes before) + local; d' in f64 to the wave's LDS table.
//                       pick      lane l looks at lags l, l + 64, ...: both searches are min-index reductions over the wave, the argmin a
//                                 (value, index) reduction.  No lane walks the table.  P is 15 samples a lane and a butterfly.
//                     Nothing about a frame depends on where its clip stands in the batch: the order of every sum is fixed by the frame's
//                     index in its own clip.
//   f0_count_kernel   one workgroup per clip: the status of every clip, and n_voiced (the frames with f0 > 0) of the clips that were read.
//
// No atomics.  Plain vector stores only.
#include <math.h>
#include "runtime.h"
#include "f0_host.h"
#include "../../include/tortoise_mi355x_test.h"

namespace tt {

constexpr int kF0H = TT_F0_HOP, kF0W = TT_F0_WINDOW, kF0T = TT_F0_LAG_MAX, kF0Lead = TT_F0_LEAD;
#ifndef TT_F0_G
#define TT_F0_G 4  // a multiple of 4, at most 8 (the LDS plan below).  4: 39 KB of LDS, four workgroups a CU, one round of scan and pick; 8: 0.79 of
#endif             // the terms, 59 KB, two a CU, two rounds - and the slower of the two as measured (profiles/r27_f0.txt)
constexpr int kF0G = TT_F0_G;                             // frames of a workgroup
constexpr int kF0Threads = 256;
constexpr int kF0Slots = kF0G + kF0W / kF0H - 1;          // 7 slots of kF0H samples
constexpr int kF0Span = kF0Slots * kF0H + kF0T;           // 2160 floats
constexpr int kF0Quads = kF0T / 4;                        // 120 threads of a half own the lags
constexpr int kF0Half = kF0H / 2;                         // samples of a thread's part of a slot
constexpr int kF0Row = kF0T + 4;                          // doubles of a wave's d' table (entries 0 .. T)
constexpr int kF0PerLane = 8;                             // lags of a lane in the scan
constexpr int kF0None = 0x7fffffff;
static_assert(kF0W == 4 * kF0H && kF0Lead == kF0W - kF0H && kF0T % 4 == 0 && kF0Half % 4 == 0 && kF0Span % 4 == 0, "a frame is four slots");
static_assert(2 * 128 == kF0Threads && kF0Quads <= 128 && kF0G % (kF0Threads / 64) == 0 && 64 * kF0PerLane >= kF0T && kF0W % 64 == 0, "thread plan");
static_assert((kF0Span + kF0G * 2 * kF0T) * sizeof(float) + (kF0Threads / 64) * kF0Row * sizeof(double) <= 64 * 1024, "LDS plan");

typedef float f0_f4 __attribute__((ext_vector_type(4)));

struct F0Args {
  int n_clips, max_samples;
  const float* audio;
  const int* in_off;
  const int* par;
  const double* thr;
  const int* frm_off;
};

// the status of clip c before its audio is read; *n_p its samples when it is TT_F0_OK
__device__ static inline int f0_clip(const F0Args& a, int c, int* n_p) {
  const int i0 = a.in_off[c], i1 = a.in_off[c + 1];
  const int st = f0_clip_status(i0, i1, a.max_samples, a.par[2 * c], a.par[2 * c + 1], a.thr[2 * c], a.thr[2 * c + 1], a.frm_off[c], a.frm_off[c + 1]);
  *n_p = st == TT_F0_OK ? i1 - i0 : 0;
  return st;
}

__device__ static inline int f0_wave_min(int v) {
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

__global__ __launch_bounds__(kF0Threads) void f0_track_kernel(F0Args a, int* __restrict__ lag_out, float* __restrict__ f0_out,
                                                              float* __restrict__ aper_out, double* __restrict__ dprime_out) {
  __shared__ __attribute__((aligned(16))) float x_s[kF0Span];
  __shared__ __attribute__((aligned(16))) float part_s[kF0G * 2 * kF0T];  // [frame][half][lag - 1]
  __shared__ double dp_s[(kF0Threads / 64) * kF0Row];
  const int c = blockIdx.y, t = threadIdx.x;
  int n;
  if (f0_clip(a, c, &n) != TT_F0_OK) return;  // (uniform)
  const int F = f0_frames(n), fg = blockIdx.x * kF0G;
  if (fg >= F) return;  // (uniform)
  const int nf = min(kF0G, F - fg), ns = nf + 3;
  const float* x = a.audio + a.in_off[c];

  // stage
  const int b0 = fg * kF0H - kF0Lead, span = ns * kF0H + kF0T;
  for (int e = t; e < span; e += kF0Threads) {
    const int i = b0 + e;
    x_s[e] = i >= 0 && i < n ? x[i] : 0.f;
  }
  __syncthreads();

  // slots
  const int u = t & 127, h = t >> 7;
  if (u < kF0Quads) {
    const f0_f4* x4 = (const f0_f4*)x_s;
    float p0[4] = {0.f, 0.f, 0.f, 0.f}, p1[4] = {0.f, 0.f, 0.f, 0.f}, p2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ns; ++s) {
      const f0_f4* xa = x4 + s * (kF0H / 4) + h * (kF0Half / 4);  // (the last read below: float4 (ns - 1) 60 + 30 + 29 + 1 + 119 < span / 4)
      const f0_f4* xb = xa + u;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      f0_f4 B0 = xb[0];
#pragma unroll 2
      for (int q = 0; q < kF0Half / 4; ++q) {
        const f0_f4 A = xa[q], B1 = xb[q + 1];
        const float av[4] = {A.x, A.y, A.z, A.w};
        const float y[8] = {B0.x, B0.y, B0.z, B0.w, B1.x, B1.y, B1.z, B1.w};  // x[j0 + 4u ..], j0 = the first of these four samples
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float e = av[i] - y[i + 1 + k];  // x[j] - x[j + tau], tau = 4u + 1 + k
            acc[k] = fmaf(e, e, acc[k]);
          }
        }
        B0 = B1;
      }
      if (s >= 3) {
        f0_f4 d;
        d.x = ((p0[0] + p1[0]) + p2[0]) + acc[0];
        d.y = ((p0[1] + p1[1]) + p2[1]) + acc[1];
        d.z = ((p0[2] + p1[2]) + p2[2]) + acc[2];
        d.w = ((p0[3] + p1[3]) + p2[3]) + acc[3];
        *(f0_f4*)(part_s + ((s - 3) * 2 + h) * kF0T + 4 * u) = d;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p0[k] = p1[k];
        p1[k] = p2[k];
        p2[k] = acc[k];
      }
    }
  }
  __syncthreads();

  // scan and pick: wave w, frames w, w + 4, ... (every wave runs every round: the barriers are uniform)
  const int lane = t & 63, w = t >> 6;
  double* dp = dp_s + w * kF0Row;
  const int lo = a.par[2 * c], hi = a.par[2 * c + 1];
  const double thr = a.thr[2 * c], floor_e = a.thr[2 * c + 1];
  const size_t fo = (size_t)a.frm_off[c];
  for (int round = 0; round < kF0G / (kF0Threads / 64); ++round) {
    const int i = round * (kF0Threads / 64) + w;
    const bool live = i < nf;  // (uniform over the wave)
    if (live) {
      const float* pa = part_s + (i * 2) * kF0T + lane * kF0PerLane;
      float dv[kF0PerLane];
      double loc[kF0PerLane];
      double run = 0.0;
#pragma unroll
      for (int k = 0; k < kF0PerLane; ++k) {
        const bool in = lane * kF0PerLane + k < kF0T;
        dv[k] = in ? pa[k] + pa[kF0T + k] : 0.f;
        run += (double)dv[k];
        loc[k] = run;
      }
      double tot = run;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(tot, d);
        if (lane >= d) tot = o + tot;
      }
      double before = __shfl_up(tot, 1);
      if (lane == 0) before = 0.0;
#pragma unroll
      for (int k = 0; k < kF0PerLane; ++k) {
        const int tau = lane * kF0PerLane + k + 1;
        if (tau <= kF0T) {
          const double cs = before + loc[k];
          dp[tau] = cs > 0.0 ? ((double)dv[k] * (double)tau) / cs : 1.0;
        }
      }
      if (lane == 0) dp[0] = 1.0;
    }
    __syncthreads();  // the table is written
    if (live) {
      const int f = fg + i;
      // P
      double P = 0.0;
      const float* xf = x_s + i * kF0H + lane * (kF0W / 64);
#pragma unroll
      for (int k = 0; k < kF0W / 64; ++k) {
        const double v = (double)xf[k];
        P = fma(v, v, P);
      }
      for (int m = 32; m >= 1; m >>= 1) P += __shfl_xor(P, m);
      // t0
      int t0 = kF0None;
      for (int tau = lane; tau <= hi; tau += 64)
        if (tau >= lo && dp[tau] < thr) t0 = min(t0, tau);
      t0 = f0_wave_min(t0);
      int th;
      if (t0 != kF0None) {  // (uniform) the end of the descent from t0
        th = kF0None;
        for (int tau = lane; tau <= hi; tau += 64)
          if (tau >= t0 && (tau == hi || dp[tau + 1] >= dp[tau])) th = min(th, tau);
        th = f0_wave_min(th);
      } else {  // the first argmin over [lo, hi]
        double bv = 0.0;
        int bi = kF0None;
        for (int tau = lane; tau <= hi; tau += 64)
          if (tau >= lo && (bi == kF0None || dp[tau] < bv)) bv = dp[tau], bi = tau;
        for (int m = 32; m >= 1; m >>= 1) {
          const double ov = __shfl_xor(bv, m);
          const int oi = __shfl_xor(bi, m);
          if (oi != kF0None && (bi == kF0None || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        }
        th = bi;
      }
      const bool voiced = t0 != kF0None && P >= floor_e;
      const double bq = dp[th];
      double delta = 0.0;
      if (th >= 2 && th <= kF0T - 1) {
        const double aq = dp[th - 1], cq = dp[th + 1];
        const double den = (aq - 2.0 * bq) + cq;
        if (den > 0.0) delta = fmin(1.0, fmax(-1.0, 0.5 * (aq - cq) / den));
      }
      if (lane == 0) {
        lag_out[fo + f] = th;
        f0_out[fo + f] = voiced ? (float)((double)TT_F0_SAMPLE_RATE / ((double)th + delta)) : 0.f;
        aper_out[fo + f] = (float)bq;
      }
      if (dprime_out) {
        double* row = dprime_out + (fo + f) * (size_t)(kF0T + 1);
        for (int tau = lane; tau <= kF0T; tau += 64) row[tau] = dp[tau];
      }
    }
    __syncthreads();  // the table is read
  }
}

__global__ __launch_bounds__(kF0Threads) void f0_count_kernel(F0Args a, const float* __restrict__ f0_out, int* __restrict__ n_voiced,
                                                              int* __restrict__ status) {
  __shared__ int cnt_s[kF0Threads / 64];
  const int c = blockIdx.x, t = threadIdx.x;
  int n;
  const int st = f0_clip(a, c, &n);
  if (st != TT_F0_OK) {  // (uniform)
    if (t == 0) status[c] = st;
    return;
  }
  const int F = f0_frames(n);
  const float* f0 = f0_out + a.frm_off[c];
  int cnt = 0;
  for (int f = t; f < F; f += kF0Threads) cnt += f0[f] > 0.f ? 1 : 0;
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
  if ((t & 63) == 0) cnt_s[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    int all = 0;
    for (int w = 0; w < kF0Threads / 64; ++w) all += cnt_s[w];
    n_voiced[c] = all;
    status[c] = TT_F0_OK;
  }
}

}  // namespace tt

using namespace tt;

struct tt_f0 : EngineHandle {
  int max_samples = 0, max_clips = 0, groups = 0;
};

static int f0_run(tt_f0* e, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off, int* lag,
                  float* f0, float* aper, int* n_voiced, int* status, double* dprime, void* stream) {
  char err[160];
  TT_REQUIRE(f0_check_track(e && audio && in_off && par && thr && frm_off && lag && f0 && aper && n_voiced && status, n_clips,
                            e ? e->max_clips : 0, err, sizeof(err)) == 0, "%s", err);
  const F0Args a{n_clips, e->max_samples, audio, in_off, par, thr, frm_off};
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    f0_track_kernel<<<dim3(e->groups, n_clips), kF0Threads, 0, s>>>(a, lag, f0, aper, dprime);
    TT_CHECK_HIP(hipGetLastError());
    f0_count_kernel<<<n_clips, kF0Threads, 0, s>>>(a, f0, n_voiced, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

extern "C" {

int tt_f0_abi_version(void) { return 1; }  // ABI changes

int tt_f0_frames(int n) { return n >= 1 && n <= TT_F0_MAX_SAMPLES ? f0_frames(n) : 0; }

int tt_f0_lags(double fmin, double fmax, int* lag_lo, int* lag_hi) {
  TT_REQUIRE(lag_lo && lag_hi, "tt_f0_lags: null argument");
  TT_REQUIRE(f0_lag_from_hz(fmin, fmax, lag_lo, lag_hi), "tt_f0_lags: %g .. %g Hz (%d .. %d Hz, with a whole lag inside)", fmin, fmax,
             TT_F0_SAMPLE_RATE / TT_F0_LAG_MAX, TT_F0_SAMPLE_RATE / TT_F0_LAG_MIN);
  return 0;
}

int tt_f0_create(int max_samples, int max_clips, tt_f0** out) {
  char err[160];
  TT_REQUIRE(f0_check_create(out != nullptr, max_samples, max_clips, err, sizeof(err)) == 0, "%s", err);
  tt_f0* e = new tt_f0();
  e->max_samples = max_samples; e->max_clips = max_clips;
  e->groups = (f0_frames(max_samples) + kF0G - 1) / kF0G;
  const int rc = e->open("tt_f0_create", false);
  if (rc) {
    tt_f0_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_f0_destroy(tt_f0* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_f0_track(tt_f0* e, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off, int* lag,
                float* f0, float* aper, int* n_voiced, int* status, void* stream) {
  return f0_run(e, n_clips, audio, in_off, par, thr, frm_off, lag, f0, aper, n_voiced, status, nullptr, stream);
}

int tt_op_f0_track(void* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off, int* lag,
                   float* f0, float* aper, int* n_voiced, int* status, double* dprime, void* stream) {
  TT_REQUIRE(dprime, "tt_op_f0_track: null argument");
  return f0_run((tt_f0*)h, n_clips, audio, in_off, par, thr, frm_off, lag, f0, aper, n_voiced, status, dprime, stream);
}

int tt_op_f0_group(void) { return kF0G; }

}  // extern "C"
