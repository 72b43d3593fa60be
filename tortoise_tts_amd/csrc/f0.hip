// Fundamental frequency (include/tortoise_mi355x_f0.h): a YIN tracker over ragged batches of finished clips.
//
//   f0_track_kernel   built from the steps of f0_steps.h (which f0_viterbi.hip shares).
//                     blockIdx = (group of kF0G = 4 consecutive frames, clip), 256 threads, one launch for the difference function, the scan
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
#include "f0_steps.h"
#include "../../include/tortoise_mi355x_test.h"

namespace tt {

__global__ __launch_bounds__(kF0Threads) void f0_track_kernel(F0Args a, int* __restrict__ lag_out, float* __restrict__ f0_out,
                                                              float* __restrict__ aper_out, double* __restrict__ dprime_out) {
  __shared__ __attribute__((aligned(16))) float x_s[kF0Span];
  __shared__ __attribute__((aligned(16))) float part_s[kF0G * 2 * kF0T];  // [frame][half][lag - 1]
  __shared__ double dp_s[kF0Waves * kF0Row];
  const int c = blockIdx.y, t = threadIdx.x;
  int n;
  if (f0_clip(a, c, &n) != TT_F0_OK) return;  // (uniform)
  const int F = f0_frames(n), fg = blockIdx.x * kF0G;
  if (fg >= F) return;  // (uniform)
  const int nf = min(kF0G, F - fg), ns = nf + 3;
  f0_stage(x_s, a.audio + a.in_off[c], n, fg, ns, t);
  __syncthreads();
  f0_slots(x_s, part_s, ns, t);
  __syncthreads();

  // scan and pick: wave w, frames w, w + 4, ... (every wave runs every round: the barriers are uniform)
  const int lane = t & 63, w = t >> 6;
  double* dp = dp_s + w * kF0Row;
  const int lo = a.par[2 * c], hi = a.par[2 * c + 1];
  const double thr = a.thr[2 * c], floor_e = a.thr[2 * c + 1];
  const size_t fo = (size_t)a.frm_off[c];
  for (int round = 0; round < kF0G / kF0Waves; ++round) {
    const int i = round * kF0Waves + w;
    const bool live = i < nf;  // (uniform over the wave)
    if (live) f0_scan(part_s, dp, i, lane);
    __syncthreads();  // the table is written
    if (live) {
      const int f = fg + i;
      const double P = f0_power(x_s, i, lane);
      bool has_t0;
      const int th = f0_pick(dp, lo, hi, thr, lane, &has_t0);
      const bool voiced = has_t0 && P >= floor_e;
      const double delta = f0_parabola(dp, th);
      if (lane == 0) {
        lag_out[fo + f] = th;
        f0_out[fo + f] = voiced ? (float)((double)TT_F0_SAMPLE_RATE / ((double)th + delta)) : 0.f;
        aper_out[fo + f] = (float)dp[th];
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
