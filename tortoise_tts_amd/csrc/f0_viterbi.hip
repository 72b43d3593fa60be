// Octave-robust F0 (include/tortoise_mi355x_f0v.h): YIN candidates of every frame, then a Viterbi path through them.  Two launches.
//
//   f0v_candidates_kernel  f0_track_kernel's geometry - blockIdx = (group of kF0G frames, clip), 256 threads - and its steps up to the d' table
//                          (f0_steps.h: stage, slots, scan; the bits of d' are tt_f0_track's).  Then the wave of a frame finds the candidates:
//                            dips     lane l looks at lags l, l + 64, ...: eight table entries and a dip flag each, in registers.
//                            lowest   seven (value, lag) min-reductions over the wave; the lane that owns a winner clears its flag.
//                            ranks    lane r < 7 holds winner r; its state is the number of winners with a smaller lag.
//                            parabola lane r refines its own winner (f0_parabola) and writes its slot.
//                          No lane walks the table.  Slot 7 takes tt_f0_track's own pick (f0_pick), for the rows the path leaves unvoiced.
//                          8 x (i32 lag, f64 dp, f32 f0) a frame, to the handle's workspace (or the caller's arrays: tt_op_f0v_candidates).
//   f0v_path_kernel        one wave per clip, 64 lanes = 8 destination states s x 8 source states j, lane = 8 s + j.  Lane (s, j) holds
//                          a[t-1][j] and forms a[t-1][j] + trans(j -> s); three (value, index) exchange steps over the 8 lanes of a
//                          destination (DPP: quad_perm twice, row_half_mirror) give the min and its smallest-j argmin on all eight;
//                          a[t][s] = local + min; one cross-lane read hands a[t][j] to lane (s, j).  The chain a frame is those steps and two
//                          f64 additions; everything else (the candidates of the next eight frames - one coalesced load a lane -, L2 of the
//                          lags out of LDS, local and trans) does not depend on a and runs ahead of it.  Backpointers: 8 x 3 bits in one
//                          i32 a frame (three ballots: bit plane b holds bit b of every state's argmin), kept in the register of lane
//                          t mod 64 and stored 64 frames at a time.  After the last frame the wave walks back 64 frames at a time - the
//                          words of a chunk in registers, one readlane a frame -, every lane keeps the state of its own frame and writes
//                          that frame's outputs: the parallel pass.
//                          A frame's arithmetic depends only on its index in its own clip: a ragged batch is bit-identical to solo calls.
//
// Costs are f0v_host.h's f0v_local / f0v_trans (single rounded f64 operations, never contracted).  No atomics.  Plain vector stores only.
#include <math.h>
#include <string.h>
#include "f0_steps.h"
#include "f0v_host.h"
#include "../../include/tortoise_mi355x_test.h"

namespace tt {

#ifndef TT_F0V_DPP
#define TT_F0V_DPP 1  // 1: the three exchange steps of the path are DPP moves; 0: ds_bpermute shuffles (the same values)
#endif

struct F0vArgs {
  F0Args f;
  const double* cost;  // f64 [n_clips, 4]; null: no costs to check (tt_op_f0v_candidates)
  const int* frames;   // null: a clip's frames come from its samples; else F of every clip (tt_op_f0v_path: no audio)
  int max_frames;      // of the handle
  int own_tables;      // 1: clip c's candidate tables begin at frame c max_frames of the handle's workspace; 0: at frm_off[c] of the caller's
};

__device__ static inline F0vCost f0v_cost(const F0vArgs& a, int c) {
  return a.cost ? F0vCost{a.cost[4 * c], a.cost[4 * c + 1], a.cost[4 * c + 2], a.cost[4 * c + 3]} : F0vCost{0.0, 0.0, 0.0, 0.0};
}

// the status of clip c; *F_p its frames and *n_p its samples (0 without audio) when it is TT_F0_OK
__device__ static inline int f0v_clip(const F0vArgs& a, int c, int* F_p, int* n_p) {
  const F0vCost k = f0v_cost(a, c);
  int st, F = 0, n = 0;
  if (a.frames) {
    F = a.frames[c];
    st = f0v_path_status(F, a.max_frames, a.f.par[2 * c], a.f.par[2 * c + 1], k, a.f.frm_off[c], a.f.frm_off[c + 1]);
  } else {
    const int i0 = a.f.in_off[c], i1 = a.f.in_off[c + 1];
    st = f0v_clip_status(i0, i1, a.f.max_samples, a.f.par[2 * c], a.f.par[2 * c + 1], a.f.thr[2 * c], a.f.thr[2 * c + 1], k, a.f.frm_off[c],
                         a.f.frm_off[c + 1]);
    if (st == TT_F0_OK) n = i1 - i0, F = f0_frames(n);
  }
  *F_p = st == TT_F0_OK ? F : 0;
  *n_p = n;
  return st;
}

__device__ static inline size_t f0v_table_base(const F0vArgs& a, int c) {
  return (a.own_tables ? (size_t)c * (size_t)a.max_frames : (size_t)a.f.frm_off[c]) * kF0vS;
}

__global__ __launch_bounds__(kF0Threads) void f0v_candidates_kernel(F0vArgs a, int* __restrict__ c_lag, double* __restrict__ c_dp,
                                                                    float* __restrict__ c_f0, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) float x_s[kF0Span];
  __shared__ __attribute__((aligned(16))) float part_s[kF0G * 2 * kF0T];  // [frame][half][lag - 1]
  __shared__ double dp_s[kF0Waves * kF0Row];
  const int c = blockIdx.y, t = threadIdx.x;
  int n, F;
  const int st = f0v_clip(a, c, &F, &n);
  if (status && blockIdx.x == 0 && t == 0) status[c] = st;
  if (st != TT_F0_OK) return;  // (uniform)
  const int fg = blockIdx.x * kF0G;
  if (fg >= F) return;  // (uniform)
  const int nf = min(kF0G, F - fg), ns = nf + 3;
  f0_stage(x_s, a.f.audio + a.f.in_off[c], n, fg, ns, t);
  __syncthreads();
  f0_slots(x_s, part_s, ns, t);
  __syncthreads();

  const int lane = t & 63, w = t >> 6;
  double* dp = dp_s + w * kF0Row;
  const int lo = a.f.par[2 * c], hi = a.f.par[2 * c + 1];
  const double thr = a.f.thr[2 * c], floor_e = a.f.thr[2 * c + 1];
  const size_t base = f0v_table_base(a, c);
  for (int round = 0; round < kF0G / kF0Waves; ++round) {
    const int i = round * kF0Waves + w;
    const bool live = i < nf;  // (uniform over the wave)
    if (live) f0_scan(part_s, dp, i, lane);
    __syncthreads();  // the table is written
    if (live) {
      const double P = f0_power(x_s, i, lane);
      bool has_t0;
      const int th = f0_pick(dp, lo, hi, thr, lane, &has_t0);
      // dips: the lane's lags lane, lane + 64, ... of [lo, hi]
      double v[kF0PerLane];
      unsigned dips = 0;
#pragma unroll
      for (int k = 0; k < kF0PerLane; ++k) {
        const int tau = lane + 64 * k;
        v[k] = 0.0;
        if (tau >= lo && tau <= hi) {  // (tau - 1 >= 23, tau + 1 <= T where it is read)
          const double x = dp[tau];
          v[k] = x;
          if (x < dp[tau - 1] && (tau == kF0T || dp[tau + 1] >= x)) dips |= 1u << k;
        }
      }
      if (P < floor_e) dips = 0;  // every voiced state of the frame is absent
      // the seven lowest, lowest first; ties to the smaller lag
      int my = kF0None;  // lane r < 7: winner r
      double myv = 0.0;
      int win[kF0vU];
#pragma unroll
      for (int r = 0; r < kF0vU; ++r) {
        double bv = 0.0;
        int bi = kF0None;
#pragma unroll
        for (int k = 0; k < kF0PerLane; ++k)
          if ((dips >> k & 1u) && (bi == kF0None || v[k] < bv)) bv = v[k], bi = lane + 64 * k;
        for (int m = 32; m >= 1; m >>= 1) {
          const double ov = __shfl_xor(bv, m);
          const int oi = __shfl_xor(bi, m);
          if (oi != kF0None && (bi == kF0None || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        }
        win[r] = bi;
        if (lane == r) my = bi, myv = bv;
        if (bi != kF0None && (bi & 63) == lane) dips &= ~(1u << (bi >> 6));
      }
      if (lane < kF0vS) {
        int slot = lane, lag = 0;
        double d = 0.0;
        float f0 = 0.f;
        if (lane == kF0vU) {  // tt_f0_track's own pick
          lag = th;
          d = dp[th];
        } else if (my != kF0None) {
          slot = 0;
#pragma unroll
          for (int r = 0; r < kF0vU; ++r) slot += win[r] < my ? 1 : 0;  // (an absent winner is kF0None: never below)
          lag = my;
          d = myv;
          f0 = (float)((double)TT_F0_SAMPLE_RATE / ((double)my + f0_parabola(dp, my)));
        }  // (else: winner `lane` is absent, and so is state `lane` - the present ones rank below the number of winners)
        const size_t o = base + (size_t)(fg + i) * kF0vS + slot;
        c_lag[o] = lag;
        c_dp[o] = d;
        c_f0[o] = f0;
      }
    }
    __syncthreads();  // the table is read
  }
}

#if TT_F0V_DPP
template <int CTRL>
__device__ static inline int f0v_move(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
#define F0V_X1 0xB1   // quad_perm [1, 0, 3, 2]: lane ^ 1
#define F0V_X2 0x4E   // quad_perm [2, 3, 0, 1]: lane ^ 2
#define F0V_X4 0x141  // row_half_mirror: lane l of eight <-> 7 - l, the other quad
#else
template <int M>
__device__ static inline int f0v_move(int v) {
  return __shfl_xor(v, M);
}
#define F0V_X1 1
#define F0V_X2 2
#define F0V_X4 4
#endif

// one exchange step of the (value, index) minimum over the eight lanes of a destination: the smaller value, the smaller index on a tie
template <int X>
__device__ static inline void f0v_exchange(double& v, int& idx) {
  const double ov = __hiloint2double(f0v_move<X>(__double2hiint(v)), f0v_move<X>(__double2loint(v)));
  const int oi = f0v_move<X>(idx);
  if (ov < v || (ov == v && oi < idx)) v = ov, idx = oi;
}

__device__ static inline int f0v_gather8(unsigned long long m) {  // bits 0, 8, .., 56 of m -> bits 0 .. 7
  return (int)(((m & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}
__device__ __host__ static inline int f0v_back(int word, int s) {
  return (word >> s & 1) | (word >> (8 + s) & 1) << 1 | (word >> (16 + s) & 1) << 2;
}

__global__ __launch_bounds__(64) void f0v_path_kernel(F0vArgs a, const double* __restrict__ L2g, const int* __restrict__ c_lag,
                                                      const double* __restrict__ c_dp, const float* __restrict__ c_f0, int* bp_ws,
                                                      int* __restrict__ lag_out, float* __restrict__ f0_out, float* __restrict__ aper_out,
                                                      int* __restrict__ state_out, int* __restrict__ n_voiced, double* __restrict__ path_cost,
                                                      int* __restrict__ status) {
  __shared__ double L2[TT_F0V_TABLE];
  const int c = blockIdx.x, lane = threadIdx.x;
  int F, n;
  const int st = f0v_clip(a, c, &F, &n);
  if (st != TT_F0_OK) {  // (uniform)
    if (lane == 0) status[c] = st;
    return;
  }
  for (int i = lane; i < TT_F0V_TABLE; i += 64) L2[i] = i ? L2g[i] : 0.0;
  __syncthreads();
  const F0vCost k = f0v_cost(a, c);
  const double l2lo = L2[a.f.par[2 * c]];
  const size_t base = f0v_table_base(a, c), bpb = (size_t)c * (size_t)a.max_frames, fo = (size_t)a.f.frm_off[c];
  const int s = lane >> 3, j = lane & 7;
  const double inf = INFINITY;

  // the candidates of eight frames: lane 8 i + q holds state q of frame t0 + i
  int lgN = 0;
  double dN = 0.0;
  if (s < F) lgN = c_lag[base + lane], dN = c_dp[base + lane];
  double a_src = inf, l2j = 0.0;  // a[t-1][j], and L2 of state j's lag in frame t - 1
  bool pj = false;                // state j of frame t - 1 is present
  int bpreg = 0;
  for (int t0 = 0; t0 < F; t0 += 8) {
    const int lgC = lgN;
    const double dC = dN;
    lgN = 0, dN = 0.0;
    if (t0 + 8 + s < F) {
      const size_t o = base + (size_t)(t0 + 8) * kF0vS + lane;
      lgN = c_lag[o], dN = c_dp[o];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = t0 + i;
      if (t >= F) break;  // (uniform)
      const int lag_s = __shfl(lgC, 8 * i + s);
      const double dp_s = __shfl(dC, 8 * i + s);
      const bool ps = s == kF0vU || f0v_present(lag_s);
      const double l2s = s != kF0vU && ps ? L2[lag_s] : 0.0;
      const double loc = f0v_local(s, dp_s, l2s, l2lo, k);
      double a_new;
      int word = 0;
      if (t == 0) {  // (uniform)
        a_new = ps ? loc : inf;
      } else {
        const bool ju = j == kF0vU, su = s == kF0vU;
        const double tr = ju && su ? 0.0 : ju || su ? k.vuv : f0v_mul(k.jump, fabs(f0v_add(l2s, -l2j)));
        double v = pj ? f0v_add(a_src, tr) : inf;
        int idx = j;
        f0v_exchange<F0V_X1>(v, idx);
        f0v_exchange<F0V_X2>(v, idx);
        f0v_exchange<F0V_X4>(v, idx);
        a_new = ps ? f0v_add(loc, v) : inf;
        word = f0v_gather8(__ballot(idx & 1)) | f0v_gather8(__ballot(idx & 2)) << 8 | f0v_gather8(__ballot(idx & 4)) << 16;
      }
      if ((t & 63) == lane) bpreg = word;
      if ((t & 63) == 63 || t == F - 1) {  // (uniform)
        if (lane <= (t & 63)) bp_ws[bpb + (size_t)(t & ~63) + lane] = bpreg;
      }
      a_src = __shfl(a_new, 8 * j);
      l2j = __shfl(l2s, 8 * j);
      pj = __shfl((int)ps, 8 * j) != 0;
    }
  }
  // the end state: the smallest s with minimal a[F-1][s] (lane (s, j) holds a[F-1][j])
  double cost = a_src;
  int end = j;
  f0v_exchange<F0V_X1>(cost, end);
  f0v_exchange<F0V_X2>(cost, end);
  f0v_exchange<F0V_X4>(cost, end);
  end = __shfl(end, 0);
  cost = __shfl(cost, 0);

  // backtrace and outputs, 64 frames at a time from the end; lane i of a chunk owns frame t0 + i
  int cur = end, cnt = 0;
  for (int t0 = (F - 1) & ~63; t0 >= 0; t0 -= 64) {
    const int mine = t0 + lane;
    const int wd = mine < F ? bp_ws[bpb + (size_t)mine] : 0;  // (the lane that stored it)
    int state = 0;
#pragma unroll
    for (int i = 63; i >= 0; --i) {
      const int t = t0 + i;
      if (t < F) {  // (uniform)
        if (lane == i) state = cur;
        if (t >= 1) cur = f0v_back(__shfl(wd, i), cur);
      }
    }
    if (mine < F) {
      const size_t o = base + (size_t)mine * kF0vS + state;
      lag_out[fo + mine] = c_lag[o];
      f0_out[fo + mine] = state == kF0vU ? 0.f : c_f0[o];
      aper_out[fo + mine] = (float)c_dp[o];
      state_out[fo + mine] = state;
      cnt += state != kF0vU ? 1 : 0;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
  if (lane == 0) {
    n_voiced[c] = cnt;
    path_cost[c] = cost;
    status[c] = TT_F0_OK;
  }
}

}  // namespace tt

using namespace tt;

struct tt_f0v : EngineHandle {
  int max_samples = 0, max_clips = 0, max_frames = 0, groups = 0;
  double* L2 = nullptr;
  int *c_lag = nullptr, *bp = nullptr;
  double* c_dp = nullptr;
  float* c_f0 = nullptr;
};

static F0vArgs f0v_args(const tt_f0v* e, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const double* cost,
                        const int* frames, const int* frm_off, int own_tables) {
  return F0vArgs{F0Args{n_clips, e->max_samples, audio, in_off, par, thr, frm_off}, cost, frames, e->max_frames, own_tables};
}

extern "C" {

int tt_f0v_abi_version(void) { return 1; }  // ABI changes

int tt_f0v_create(int max_samples, int max_clips, const double* log2_table, tt_f0v** out) {
  char err[160];
  TT_REQUIRE(f0v_check_create(out != nullptr, log2_table, max_samples, max_clips, err, sizeof(err)) == 0, "%s", err);
  tt_f0v* e = new tt_f0v();
  e->max_samples = max_samples; e->max_clips = max_clips;
  e->max_frames = f0_frames(max_samples);
  e->groups = (e->max_frames + kF0G - 1) / kF0G;
  int rc = e->open("tt_f0v_create", false);
  const size_t slots = (size_t)max_clips * (size_t)e->max_frames * kF0vS;
  if (!rc) rc = e->arena.alloc((void**)&e->L2, TT_F0V_TABLE * sizeof(double));
  if (!rc) rc = e->arena.alloc((void**)&e->c_lag, slots * sizeof(int));
  if (!rc) rc = e->arena.alloc((void**)&e->c_dp, slots * sizeof(double));
  if (!rc) rc = e->arena.alloc((void**)&e->c_f0, slots * sizeof(float));
  if (!rc) rc = e->arena.alloc((void**)&e->bp, (size_t)max_clips * (size_t)e->max_frames * sizeof(int));
  if (!rc && hipMemcpy(e->L2, log2_table, TT_F0V_TABLE * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("tt_f0v_create: the log2 table could not be copied to the device");
    rc = -2;
  }
  if (rc) {
    tt_f0v_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_f0v_destroy(tt_f0v* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_f0v_track(tt_f0v* e, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const double* cost,
                 const int* frm_off, int* lag, float* f0, float* aper, int* state, int* n_voiced, double* path_cost, int* status, void* stream) {
  char err[160];
  TT_REQUIRE(f0v_check_track(e && audio && in_off && par && thr && cost && frm_off && lag && f0 && aper && state && n_voiced && path_cost && status,
                             n_clips, e ? e->max_clips : 0, err, sizeof(err)) == 0, "%s", err);
  const F0vArgs a = f0v_args(e, n_clips, audio, in_off, par, thr, cost, nullptr, frm_off, 1);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    f0v_candidates_kernel<<<dim3(e->groups, n_clips), kF0Threads, 0, s>>>(a, e->c_lag, e->c_dp, e->c_f0, nullptr);
    TT_CHECK_HIP(hipGetLastError());
    f0v_path_kernel<<<n_clips, 64, 0, s>>>(a, e->L2, e->c_lag, e->c_dp, e->c_f0, e->bp, lag, f0, aper, state, n_voiced, path_cost, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int tt_op_f0v_candidates(void* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off,
                         int* c_lag, double* c_dp, float* c_f0, int* status, void* stream) {
  tt_f0v* e = (tt_f0v*)h;
  char err[160];
  TT_REQUIRE(f0v_check_track(e && audio && in_off && par && thr && frm_off && c_lag && c_dp && c_f0 && status, n_clips, e ? e->max_clips : 0, err,
                             sizeof(err)) == 0, "%s", err);
  const F0vArgs a = f0v_args(e, n_clips, audio, in_off, par, thr, nullptr, nullptr, frm_off, 0);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    f0v_candidates_kernel<<<dim3(e->groups, n_clips), kF0Threads, 0, s>>>(a, c_lag, c_dp, c_f0, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int tt_op_f0v_path(void* h, int n_clips, const int* frames, const int* par, const double* cost, const int* frm_off, const int* c_lag,
                   const double* c_dp, const float* c_f0, int* lag, float* f0, float* aper, int* state, int* n_voiced, double* path_cost,
                   int* status, void* stream) {
  tt_f0v* e = (tt_f0v*)h;
  char err[160];
  TT_REQUIRE(f0v_check_track(e && frames && par && cost && frm_off && c_lag && c_dp && c_f0 && lag && f0 && aper && state && n_voiced && path_cost &&
                                 status, n_clips, e ? e->max_clips : 0, err, sizeof(err)) == 0, "%s", err);
  const F0vArgs a = f0v_args(e, n_clips, nullptr, nullptr, par, nullptr, cost, frames, frm_off, 0);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    f0v_path_kernel<<<n_clips, 64, 0, s>>>(a, e->L2, c_lag, c_dp, c_f0, e->bp, lag, f0, aper, state, n_voiced, path_cost, status);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
