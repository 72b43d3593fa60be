// Row norms (LayerNorm / x-transformers RMSNorm) fused with the residual-stream update, and
// token-major GroupNorm (stats + apply) for DiffusionTts.  All statistics are fp32 (GroupNorm's
// cross-chunk combine is fp64); normalised activations are emitted directly in the GEMM operand
// type so no separate cast pass exists anywhere in the engine.
#include <type_traits>
#include "norm_steps.h"

namespace tt {

thread_local RowNormRan g_rownorm_ran = {-1, -1, 0, 0};
thread_local GroupNormRan g_groupnorm_ran = {0, -1, 0, 0};

// ------------------------------------------------------------------------------- row norm
// D <= 4096, D % 4 == 0.  One body for the two run-time forms: a row shared by a span of threads (norm_steps.h), four quads per thread,
// the run-time slab count one round trip per slab; RMSNorm, or LayerNorm (two-pass variance in registers) optionally followed by a
// second LayerNorm and an activation.  SLOTS: the f32 copy can be filed under a device-side counter.
template <typename T, class Span, bool SLOTS>
__device__ __forceinline__ void rownorm_row(const RowNormArgs& a, int row, Span sp) {
  constexpr int J = 4;
  float4 v[J];
  float* xr = a.x + (size_t)row * a.ldx;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = span_col(sp, j);
    if (c < a.D) {
      RowQuad<-1, -1> q;
      row_request(a, row, xr, c, q);
      v[j] = row_update(a, row, xr, c, true, q);
      sum += quad_sum(v[j]);
    } else {
      v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  if (a.mode == NORM_NONE) return;
  if (a.mode == NORM_RMS) {
    const float inv = rms_inv(v, sp, a.D, a.eps1, a.guard);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = span_col(sp, j);
      if (c < a.D) v[j] = rms_scale(v[j], inv, *(const float4*)(a.g1 + c));
    }
  } else {
    const float* gs[2] = {a.g1, a.g2};
    const float* bs[2] = {a.b1, a.b2};
    const float epss[2] = {a.eps1, a.eps2};
    const int nln = a.g2 ? 2 : 1;
    for (int l = 0; l < nln; ++l) {
      if (l > 0) sum = row_sum(v, sp, a.D);
      const LnStats st = ln_stats(v, sum, sp, a.D, epss[l], l == 0 ? a.guard : nullptr);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = span_col(sp, j);
        if (c < a.D) v[j] = ln_affine(v[j], st, *(const float4*)(gs[l] + c), *(const float4*)(bs[l] + c));
      }
    }
    if (a.act != ACT_NONE) {
#pragma unroll
      for (int j = 0; j < J; ++j)
        v[j] = make_float4(apply_act(v[j].x, a.act, 0.f), apply_act(v[j].y, a.act, 0.f), apply_act(v[j].z, a.act, 0.f), apply_act(v[j].w, a.act, 0.f));
    }
  }
  float* o32 = SLOTS ? row_f32_block(a, row) : a.out_f32;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = span_col(sp, j);
    if (c < a.D) row_emit<T>(a, o32, row, c, v[j]);
  }
}

// Generic form: one 256-thread block per row; the only one with the f32 slots.
template <typename T>
__global__ __launch_bounds__(256) void rownorm_kernel(RowNormArgs a) {
  __shared__ float red[4];
  rownorm_row<T, BlockSpan, true>(a, blockIdx.x, BlockSpan{red});
}

// Wave-per-row form for D <= 1024: no block barriers, four rows per 256-thread block.  Same arithmetic order per row as the block form
// is NOT required (tests compare to fp64).
template <typename T>
__global__ __launch_bounds__(256) void rownorm_wave_kernel(RowNormArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  rownorm_row<T, WaveSpan, false>(a, row, WaveSpan{});
}

// Narrow rows (D <= 1024): one float4 per thread and every operand the row needs - input, bias, split-K slabs, affine
// parameters - requested before the first use, so the row costs one memory round trip instead of three (input, slabs,
// affine).  NSLAB / BIAS / RMS are compile-time so no branch sits between the requests.  Same arithmetic order as the
// generic kernel: bias, slabs in order, two-pass variance.
template <typename T, int NSLAB, bool BIAS, bool RMS>
__global__ __launch_bounds__(256) void rownorm_narrow_kernel(RowNormArgs a) {
  __shared__ float red[8];
  FreshBlockSpan sp{red};
  const int row = blockIdx.x, tid = threadIdx.x;
  const bool live = tid * 4 < a.D;
  const int c = min(tid * 4, a.D - 4);  // idle lanes re-read the last quad (no branch), masked below
  float* xr = a.x + (size_t)row * a.ldx;
  RowQuad<NSLAB, BIAS ? 1 : 0> q;
  row_request(a, row, xr, c, q);
  const float4 g = *(const float4*)(a.g1 + c);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (!RMS) b = *(const float4*)(a.b1 + c);
  __builtin_amdgcn_sched_barrier(0);

  float4 v[1] = {row_update(a, row, xr, c, live, q)};
  if (!live) v[0] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 y;
  if constexpr (RMS) y = rms_scale(v[0], rms_inv(v, sp, a.D, a.eps1, a.guard), g);
  else y = ln_affine(v[0], ln_stats(v, quad_sum(v[0]), sp, a.D, a.eps1, a.guard), g, b);
  if (live) row_emit<T>(a, a.out_f32, row, c, y);
}

// f(std::integral_constant) for a run-time bool / one of the listed ints (false: v is none of them)
template <class F> static void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
template <int... Vs, class F> static bool dispatch_int(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

template <typename T>
static bool rownorm_narrow_launch(const ProfScope& ps, const RowNormArgs& a, hipStream_t stream) {
  if (a.D > 1024 || a.mode == NORM_NONE || a.g2 != nullptr || a.f32_slot != nullptr || a.f32_row_slot != nullptr || a.act != ACT_NONE) return false;
  const bool bias = a.add_bias != nullptr, rms = a.mode == NORM_RMS;
  return dispatch_int<0, 1, 2, 4, 8>(a.nslab, [&](auto ns) {
    dispatch_bool(bias, [&](auto bi) {
      dispatch_bool(rms, [&](auto rm) {
        g_rownorm_ran = RowNormRan{1, decltype(ns)::value, bias ? 1 : 0, rms ? 1 : 0};
        launch_timed(ps, rownorm_narrow_kernel<T, decltype(ns)::value, decltype(bi)::value, decltype(rm)::value>, dim3(a.M), dim3(256), 0, stream, a);
      });
    });
  });
}

int rownorm_launch(int dtype, const RowNormArgs& a, hipStream_t stream) {
  TT_REQUIRE(a.M > 0 && a.D > 0 && a.D % 4 == 0 && a.D <= 4096, "rownorm: bad shape M=%d D=%d", a.M, a.D);
  TT_REQUIRE(a.ldx % 4 == 0, "rownorm: ldx must be a multiple of 4");
  TT_REQUIRE(a.act == ACT_NONE || a.mode == NORM_LAYER, "rownorm: a post-norm activation needs the LayerNorm mode");
  ProfScope ps(PROF_ROWNORM, stream, 0.0, (double)a.M * a.D * (4.0 * (1 + a.nslab + (a.write_x ? 1 : 0)) + (a.out_t ? 2.0 : 0.0) + (a.out_f32 ? 4.0 : 0.0)), true);
  // few rows (decode): one block per row keeps 4x more loads in flight; many rows: wave per row, no barriers (that kernel has no
  // f32 slots: a problem that files its f32 copy under a counter stays on the generic kernel)
  g_rownorm_ran = RowNormRan{0, -1, a.add_bias ? 1 : 0, a.mode == NORM_RMS ? 1 : 0};
  if (a.D <= 1024 && a.M >= 1024 && !a.row_blocks && !a.f32_slot && !a.f32_row_slot) {
    g_rownorm_ran.kernel = 2;
    TT_DISPATCH_T(dtype, T, launch_timed(ps, rownorm_wave_kernel<T>, dim3(cdiv(a.M, 4)), dim3(256), 0, stream, a));
  } else {
    bool narrow = false;
    TT_DISPATCH_T(dtype, T, narrow = rownorm_narrow_launch<T>(ps, a, stream));
    if (!narrow) TT_DISPATCH_T(dtype, T, launch_timed(ps, rownorm_kernel<T>, dim3(a.M), dim3(256), 0, stream, a));
  }
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------- group norm
// x: [B][S][C] f32 token-major, 32 groups of cpg = C/32 channels (cpg % 4 == 0), C/4 a power of
// two <= 256 or C == 1024*k.  Stage 1 writes per-(batch, row-chunk, group) (sum, sumsq).
constexpr int GN_ROWS = 16;
constexpr int GN_MAX_CHUNKS = 64;  // the apply kernel's finalize prologue reduces <= 8 partials per thread
static inline int gn_rows_per_chunk(int S) { return std::max(GN_ROWS, cdiv(S, GN_MAX_CHUNKS)); }

// (vl: valid rows of sample b in a padded batch, see GroupNormArgs::vlen; a chunk past them contributes zeros)
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, int S, int C, float* __restrict__ partial, int rows_per_chunk,
                                                       GroupNormArgs va) {
  __shared__ float ls[256][2];
  const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
  const int vl = va.vperiod > 0 ? va.vlen[b % va.vperiod] : S;
  const int tid = threadIdx.x;
  const int c4n = C >> 2;                       // float4 columns per row
  const int CL = c4n < 256 ? c4n : 256;         // column lanes
  const int RL = 256 / CL;                      // row lanes
  const int cl = tid % CL, rl = tid / CL;
  const int cpg4 = (C / 32) >> 2;               // float4 columns per group
  const int r0 = chunk * rows_per_chunk;
  const int r1 = min(vl, r0 + rows_per_chunk);
  // With C > 1024 a thread owns several columns in different groups: handle one column set per pass.
  for (int cb = 0; cb < c4n; cb += 256) {
    float s = 0.f, q = 0.f;
    const int c4 = cb + cl;
    if (c4 < c4n) {
#pragma unroll 8
      for (int r = r0 + rl; r < r1; r += RL) {
        const float4 t = *(const float4*)(x + ((size_t)b * S + r) * C + c4 * 4);
        s += t.x + t.y + t.z + t.w;
        q += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
      }
    }
    __syncthreads();
    ls[tid][0] = s;
    ls[tid][1] = q;
    __syncthreads();
    // groups covered by this pass: columns [cb, cb+CL) -> groups (cb/cpg4) .. ; one thread per group
    const int ngrp = CL / cpg4;
    if (tid < ngrp) {
      float ts = 0.f, tq = 0.f;
      for (int r = 0; r < RL; ++r)
        for (int c = 0; c < cpg4; ++c) {
          ts += ls[r * CL + tid * cpg4 + c][0];
          tq += ls[r * CL + tid * cpg4 + c][1];
        }
      const int g = cb / cpg4 + tid;
      float* p = partial + (((size_t)b * nchunk + chunk) * 32 + g) * 2;
      p[0] = ts;
      p[1] = tq;
    }
  }
}

// Per-(batch, group) mean / rstd from partial sums, fp64 combine in a fixed order.  Two sources:
//   a.gemm_part == nullptr : partial[b][chunk][32][2] from gn_stats_kernel
//   a.gemm_part != nullptr : [row_tile][slot][C/16][2] written by the producing GEMM's epilogue (norm_steps.h gn_partial_item)
// The first GN_HEAD fused partials of every thread can be requested ahead of the activation rows (gn_partial_head) so the
// statistics round trip overlaps the row loads; gn_finalize then sums head + remainder in the same fixed order: thread (part, g) takes
// items part, part + 8, ... of group g, and the 8 parts are combined in part order.
constexpr int GN_HEAD = 8;

template <int SPG_SHIFT>
__device__ __forceinline__ void gn_partial_head(const GroupNormArgs& a, int b, int tid, float2 (&head)[GN_HEAD]) {
  const int g = tid & 31, part = tid >> 5;
  const int r_shift = 31 - __builtin_clz(a.part_rows), nc16 = a.C >> 4;
  const GnItems it = gn_items<SPG_SHIFT>(b, a.S, r_shift);
#pragma unroll
  for (int k = 0; k < GN_HEAD; ++k) head[k] = gn_partial_item<SPG_SHIFT>(a.gemm_part, a.S, b, g, part + 8 * k, it, nc16, r_shift);
}

template <int SPG_SHIFT>
__device__ __forceinline__ void gn_finalize(const GroupNormArgs& a, int b, int tid, int nchunk, float* mean_s, float* rstd_s,
                                            double (*part_s)[32], double (*part_q)[32], const float2* head = nullptr) {
  const int g = tid & 31, part = tid >> 5;
  double s = 0.0, q = 0.0;
  if (a.gemm_part) {
    const int r_shift = 31 - __builtin_clz(a.part_rows), nc16 = a.C >> 4;
    const GnItems it = gn_items<SPG_SHIFT>(b, a.S, r_shift);
    int e = part;
    if (head) {
#pragma unroll
      for (int k = 0; k < GN_HEAD; ++k, e += 8) {
        if (e < it.n) {
          s += (double)head[k].x;
          q += (double)head[k].y;
        }
      }
    }
#pragma unroll 4
    for (; e < it.n; e += 8) {
      const float2 v = gn_partial_item<SPG_SHIFT>(a.gemm_part, a.S, b, g, e, it, nc16, r_shift);
      s += (double)v.x;
      q += (double)v.y;
    }
  } else {
    float2 pv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // nchunk <= 64: at most 8 independent loads per thread
      const int i = part + 8 * k;
      pv[k] = i < nchunk ? *(const float2*)(a.partial + (((size_t)b * nchunk + i) * 32 + g) * 2) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s += (double)pv[k].x;
      q += (double)pv[k].y;
    }
  }
  part_s[part][g] = s;
  part_q[part][g] = q;
  __syncthreads();
  if (tid < 32) {
    const GnSums t = gn_combine(part_s, part_q, tid);
    // 1 / (S * C / 32), set by groupnorm_launch; a padded batch counts the sample's valid rows only
    const double inv_n = a.vperiod > 0 ? 1.0 / ((double)a.vlen[b % a.vperiod] * (double)(a.C / 32)) : a.inv_count;
    gn_mean_rstd(t, inv_n, a, mean_s[tid], rstd_s[tid]);
  }
  __syncthreads();
}

__device__ __forceinline__ const float* gn_ss_block(const GroupNormArgs& a, int b) {
  return a.scale_shift + (size_t)(b / (a.ss_batch_div > 0 ? a.ss_batch_div : 1)) * a.ss_batch_stride;
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(GroupNormArgs a, int nchunk, int rows_per_block) {
  __shared__ float mean_s[32], rstd_s[32];
  __shared__ double part_s[8][32], part_q[8][32];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x;
  const int C = a.C, S = a.S;
  {
    const int spg = (a.C / 32) >> 4;  // strips per group: 1, 2 or 4 (C = 512, 1024, 2048)
    if (spg == 4) gn_finalize<2>(a, b, tid, nchunk, mean_s, rstd_s, part_s, part_q);
    else if (spg == 2) gn_finalize<1>(a, b, tid, nchunk, mean_s, rstd_s, part_s, part_q);
    else gn_finalize<0>(a, b, tid, nchunk, mean_s, rstd_s, part_s, part_q);
  }
  const int c4n = C >> 2;
  const int cpg = C / 32;
  const int r0 = chunk * rows_per_block;
  const int r1 = min(S, r0 + rows_per_block);
  const int total = (r1 - r0) * c4n;
  const int vl = a.vperiod > 0 ? a.vlen[b % a.vperiod] : S;
  for (int f = tid; f < total; f += 256) {
    const int r = r0 + f / c4n;
    const int c = (f % c4n) * 4;
    const int g = c / cpg;
    const size_t off = ((size_t)b * S + r);
    const float4 t = *(const float4*)(a.x + off * C + c);
    const float4 gm = *(const float4*)(a.gamma + c);
    const float4 bt = *(const float4*)(a.beta + c);
    float4 y = gn_affine(t, mean_s[g], rstd_s[g], gm, bt);
    if (a.scale_shift) {
      const float* ss = gn_ss_block(a, b);
      y = gn_scale_shift(y, *(const float4*)(ss + c), *(const float4*)(ss + C + c));
    }
    gn_emit<T>(a, off, c, gn_act_pad(y, a.act, r >= vl));
  }
}

// C == 1024 fast path: thread t owns channels 4t..4t+3 (group t/8) of ROWS consecutive rows.  The x rows are requested BEFORE the
// statistics are finalised, so the streaming loads overlap the (latency-bound) prologue.
// ROWS per block: 4 in general (two blocks per CU overlap each other's statistics prologue); 2 for passes of <= 4096 rows (the
// denoiser alone, 1740 rows: 870 blocks instead of 435 - in-situ A/B -1.7 % on the sampler iteration; 1 row and 8 rows are slower)
constexpr int GN_APPLY_ROWS = 4;
template <typename T, bool FUSED, bool SS, int ROWS>
__global__ __launch_bounds__(256) void gn_apply_c1024_kernel(GroupNormArgs a, int nchunk) {
  __shared__ float mean_s[32], rstd_s[32];
  __shared__ double part_s[8][32], part_q[8][32];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int S = a.S;
  constexpr int C = 1024;
  const int r0 = blockIdx.x * ROWS;
  const int c = tid * 4;
  // request order = need order: statistics partials, then the rows and the affine parameters
  float2 head[GN_HEAD];
  if constexpr (FUSED) gn_partial_head<1>(a, b, tid, head);  // FUSED <=> a.gemm_part != nullptr (compile time: no branch to sink consumers into)
  float4 xr[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = min(r0 + i, S - 1);
    xr[i] = *(const float4*)(a.x + ((size_t)b * S + r) * C + c);
  }
  const float4 gm = *(const float4*)(a.gamma + c);
  const float4 bt = *(const float4*)(a.beta + c);
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sh = sc;
  if constexpr (SS) {  // SS <=> a.scale_shift != nullptr
    const float* ss = gn_ss_block(a, b);
    sc = *(const float4*)(ss + c);
    sh = *(const float4*)(ss + C + c);
  }
  __builtin_amdgcn_sched_barrier(0);  // keep every request above in flight before the first consumer waits
  gn_finalize<1>(a, b, tid, nchunk, mean_s, rstd_s, part_s, part_q, FUSED ? head : nullptr);
  const float mu = mean_s[tid >> 3], rs = rstd_s[tid >> 3];
  const int vl = a.vperiod > 0 ? a.vlen[b % a.vperiod] : S;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = r0 + i;
    if (r >= S) break;
    float4 y = gn_affine(xr[i], mu, rs, gm, bt);
    if constexpr (SS) y = gn_scale_shift(y, sc, sh);
    gn_emit<T>(a, (size_t)b * S + r, c, gn_act_pad(y, a.act, r >= vl));
  }
}

int groupnorm_launch(int dtype, const GroupNormArgs& a0, hipStream_t stream) {
  GroupNormArgs a = a0;
  a.inv_count = 1.0 / ((double)a.S * (double)(a.C / 32));
  const int c4n = a.C / 4;
  TT_REQUIRE(a.C % 128 == 0 && ((c4n <= 256 && (c4n & (c4n - 1)) == 0) || c4n % 256 == 0), "groupnorm: unsupported C=%d", a.C);
  TT_REQUIRE(a.B > 0 && a.S > 0 && a.partial != nullptr, "groupnorm: bad arguments");
  const int rpc = gn_rows_per_chunk(a.S);
  const int nchunk = cdiv(a.S, rpc);
  dim3 grid(nchunk, a.B);
  // (dispatch-timed when the statistics come from the producing GEMM: then the apply kernel is the only launch of this scope)
  ProfScope ps(PROF_GROUPNORM, stream, 0.0, (double)a.B * a.S * a.C * ((a.gemm_part ? 4.0 : 8.0) + (a.out_t ? 2.0 : 0.0) + (a.out_f32 ? 4.0 : 0.0)), a.gemm_part != nullptr);
  if (a.gemm_part) {
    const int spg = (a.C / 32) / 16;
    TT_REQUIRE((a.C / 32) % 16 == 0 && (spg == 1 || spg == 2 || spg == 4) && a.part_rows > 0 && (a.part_rows & (a.part_rows - 1)) == 0 && a.S >= a.part_rows,
               "groupnorm: fused statistics need 16 / 32 / 64 channels per group, a power-of-two row tile and S >= the row tile");
  } else {
    gn_stats_kernel<<<grid, 256, 0, stream>>>(a.x, a.S, a.C, a.partial, rpc, a);
    TT_CHECK_HIP(hipGetLastError());
  }
  const bool few = a.C == 1024 && (long)a.B * a.S <= 4096;
  const int rpb = few ? 2 : GN_APPLY_ROWS;  // apply is pure streaming: many small blocks
  dim3 grid2(cdiv(a.S, rpb), a.B);
  g_groupnorm_ran = GroupNormRan{a.gemm_part ? 0 : 1, a.C == 1024 ? 1 : 0, rpb, a.C == 1024 && a.gemm_part ? 1 : 0};
  if (a.C == 1024) {  // (T = float: the fp32 verification mode)
    TT_DISPATCH_T(dtype, T, dispatch_bool(a.gemm_part != nullptr, [&](auto fused) {
      dispatch_bool(a.scale_shift != nullptr, [&](auto ss) {
        dispatch_int<2, GN_APPLY_ROWS>(rpb, [&](auto rows) {
          launch_timed(ps, gn_apply_c1024_kernel<T, decltype(fused)::value, decltype(ss)::value, decltype(rows)::value>, grid2, dim3(256), 0, stream, a, nchunk);
        });
      });
    }));
  } else {
    TT_DISPATCH_T(dtype, T, launch_timed(ps, gn_apply_kernel<T>, grid2, dim3(256), 0, stream, a, nchunk, rpb));
  }
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

size_t groupnorm_partial_floats(int B, int S) { return (size_t)B * cdiv(S, gn_rows_per_chunk(S)) * 32 * 2; }
// The workspace of any batch whose samples total at most `rows` rows, whatever its split into samples: a sample of S rows has
// cdiv(S, max(GN_ROWS, ..)) <= S / GN_ROWS + 1 chunks; summed over the samples that is <= rows / GN_ROWS + one per sample, and there are at most
// `rows` samples (one-row samples): <= rows / GN_ROWS + rows chunks of [32 groups][sum, sumsq].  64 chunks of slack on top.
size_t groupnorm_partial_floats_rows(size_t rows) { return (rows / GN_ROWS + rows + 64) * 32 * 2; }

}  // namespace tt
