// GEMV-shaped decode GEMMs for handles that decode at most 4 sequences at a time (round 6; the streaming path, tortoise/api_fast.py:389-420,
// pulls ONE sequence token by token through tortoise/models/autoregressive.py:150-163).
//
// At one row the row tile of an MFMA kernel is padding: the 32 x 16 tile still moves 64 KB of activation rows (31 of 32 of them copies of
// row 0) next to 32 KB of weights per workgroup and pays the LDS ring's fill and barriers for 16 MFMA-steps of work.  Here a workgroup of 4
// waves owns 16 output columns, a wave 4 of them: it requests the W rows of its columns in full (K / 512 sixteen-byte loads per lane per
// row, ALL of them before the first use - one HBM round trip for the whole launch), holds the M <= 4 activation rows in registers, multiplies
// on the packed-pair dot instruction (v_dot2_f32_bf16 / v_dot2_f32_f16, f32 accumulation) and finishes every (row, column) with one
// cross-lane sum.  No LDS, no barrier, no split-K: the projections add bias + product onto the residual row in place, so the LayerNorm behind
// them has no slabs to fold.  The summation order is fixed (lane-local over k, then the DPP tree): deterministic, and a handle either always
// or never runs these kernels (the choice is the handle's max_batch, not the batch of a call), so chunked == one-shot decoding stays
// bit-exact.  They are NOT the bits of the MFMA path - a sharded job (per-rank batches of >= 16) never sees them.
// The two GEMVs behind a LayerNorm (QKV, c_fc) compute the norm themselves (template flag LN): five launches per layer, not seven.
// In situ (bench.py --workload stream, profiles/r06_ab_stream_gemv.txt): first chunk 62.5 ms (MFMA tiles) -> 56.0 (GEMV) -> 46.7 ms (norms inside).
// Measured against the product's skinny MFMA tile at M = 1 (scripts/kbench.py gemv, cold weights): QKV 5.04 -> 3.31 us, c_fc 5.15 -> 3.72,
// lm_head 6.83 -> 5.39; at M = 4 the two are equal, at M = 8 the MFMA tile wins - hence the <= 4 rule.
// Wide session handles (TT_AR_OPT_SESSIONS = 2) decode 5 .. 16 rows here anyway: a session's bits must equal its bits alone on a
// max_batch = 1 handle, which the MFMA tiles do not give.  gemv_rows_kernel keeps the weight registers and walks the rows past them in
// groups (four rows, two at K = 4096), every row with exactly the arithmetic of the <= 4-row kernel; no scratch in any instantiation
// (VGPRs / waves per SIMD: K = 1024 112 - 122 / 4, its LayerNorm forms 208 - 215 / 2; K = 2048 208 - 218 / 2; K = 4096 254 - 256 plus
// 16 - 32 AGPRs / 1).
#include "ops.h"

namespace tt {

__device__ __forceinline__ float gv_dot8(Vec<bf16>::x8 a, Vec<bf16>::x8 b, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 4, 5), __builtin_shufflevector(b, b, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a, a, 6, 7), __builtin_shufflevector(b, b, 6, 7), acc, false);
  return acc;
}
__device__ __forceinline__ float gv_dot8(Vec<f16>::x8 a, Vec<f16>::x8 b, float acc) {
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 4, 5), __builtin_shufflevector(b, b, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(a, a, 6, 7), __builtin_shufflevector(b, b, 6, 7), acc, false);
  return acc;
}

// EPI: GEMV_F32 out_f32 = acc + bias (lm_head) | GEMV_RES x += acc + bias in place (projections) | GEMV_GELU_T out_t = gelu_tanh(acc + bias) (c_fc)
//      | GEMV_QKV q * scale -> qbuf, K / V appended to the per-sequence cache at the device-side step (EpiQkvDecode's layout) - on a session
//        handle at every row's own slot (row_slot)
// LN: the activation rows are LayerNorm(ln_x rows) computed here (K == 1024: a lane's sixteen channels of each f32 residual row, two-pass variance
//     over the wave, affine, rounded to T like the row-norm kernel's output) while the weight rows are in flight - every workgroup repeats the
//     4 KB row's norm instead of a launch of its own doing it once.
// The pieces below are shared by the two kernels: gemv_kernel (M <= 4, every row in registers) and gemv_rows_kernel (5 .. 16 rows in groups
// against the same weight registers).  A row's arithmetic is the same in both and does not depend on the other rows of the launch.

// this wave's W rows (columns n0 .. n0 + 3), all requested before the first use
template <typename T, int KC>
__device__ __forceinline__ void gv_load_w(const GemvArgs& a, int n0, int lane, typename Vec<T>::x8 (&w)[4][KC]) {
  const T* W = (const T*)a.W;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const T* wr = W + (size_t)(n0 + c) * a.ldw + lane * 8;
#pragma unroll
    for (int k = 0; k < KC; ++k) w[c][k] = *(const typename Vec<T>::x8*)(wr + k * 512);
  }
}
// activation rows r0 .. r0 + RG - 1 (rows beyond M repeat the last row: never stored)
template <typename T, int RG, int KC>
__device__ __forceinline__ void gv_load_rows(const GemvArgs& a, int r0, int lane, typename Vec<T>::x8 (&x)[RG][KC]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    const T* ar = (const T*)a.A + (size_t)min(r0 + r, a.M - 1) * a.lda + lane * 8;
#pragma unroll
    for (int k = 0; k < KC; ++k) x[r][k] = *(const typename Vec<T>::x8*)(ar + k * 512);
  }
}
// the f32 residual rows r0 .. r0 + RG - 1 in front of a fused LayerNorm: a lane's sixteen channels of each
template <int RG>
__device__ __forceinline__ void gv_load_ln_rows(const GemvArgs& a, int r0, int lane, float4 (&f)[RG][4]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    const float* xr = a.ln_x + (size_t)min(r0 + r, a.M - 1) * a.ldx + lane * 8;
    f[r][0] = *(const float4*)xr; f[r][1] = *(const float4*)(xr + 4); f[r][2] = *(const float4*)(xr + 512); f[r][3] = *(const float4*)(xr + 516);
  }
}
__device__ __forceinline__ void gv_load_ln_affine(const GemvArgs& a, int lane, float4 (&g)[4], float4 (&b)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane * 8 + (j >> 1) * 512 + (j & 1) * 4;
    g[j] = *(const float4*)(a.ln_g + c);
    b[j] = *(const float4*)(a.ln_b + c);
  }
}
// LayerNorm of rows r0 .. r0 + RG - 1 (two-pass variance over the wave, affine, rounded to T); f is overwritten
template <typename T, int RG>
__device__ __forceinline__ void gv_norm_rows(const GemvArgs& a, int r0, float4 (&f)[RG][4], const float4 (&g)[4], const float4 (&b)[4],
                                             typename Vec<T>::x8 (&x)[RG][2]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += f[r][j].x + f[r][j].y + f[r][j].z + f[r][j].w;
    const float mean = wave_sum(sum) * (1.0f / 1024.0f);
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[r][j].x -= mean; f[r][j].y -= mean; f[r][j].z -= mean; f[r][j].w -= mean;
      sq += f[r][j].x * f[r][j].x + f[r][j].y * f[r][j].y + f[r][j].z * f[r][j].z + f[r][j].w * f[r][j].w;
    }
    const float var = wave_sum(sq) * (1.0f / 1024.0f);
    if (a.guard && blockIdx.x == 0 && threadIdx.x == 0 && r0 + r < a.M && !(var < INFINITY)) atomicAdd(a.guard, 1);  // NaN / inf in the row (norm.hip's guard)
    const float rstd = rsqrtf(var + a.ln_eps);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 lo = f[r][2 * k], hi = f[r][2 * k + 1];
      const typename Vec<T>::x4 p = pack4<T>(lo.x * rstd * g[2 * k].x + b[2 * k].x, lo.y * rstd * g[2 * k].y + b[2 * k].y, lo.z * rstd * g[2 * k].z + b[2 * k].z,
                                             lo.w * rstd * g[2 * k].w + b[2 * k].w);
      const typename Vec<T>::x4 q = pack4<T>(hi.x * rstd * g[2 * k + 1].x + b[2 * k + 1].x, hi.y * rstd * g[2 * k + 1].y + b[2 * k + 1].y,
                                             hi.z * rstd * g[2 * k + 1].z + b[2 * k + 1].z, hi.w * rstd * g[2 * k + 1].w + b[2 * k + 1].w);
      x[r][k] = __builtin_shufflevector(p, q, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }
}
// rows r0 .. r0 + RG - 1 against the wave's four columns: lane-local dot over k, one cross-lane sum per (row, column), lane 0 stores the
// rows below M.  trow[r]: row r0 + r's KV slot (GEMV_QKV)
template <typename T, int RG, int KC, int EPI>
__device__ __forceinline__ void gv_rows(const GemvArgs& a, int r0, int n0, int lane, const typename Vec<T>::x8 (&w)[4][KC],
                                        const typename Vec<T>::x8 (&x)[RG][KC], float4 bv, const int (&trow)[RG]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < KC; ++k) acc = gv_dot8(x[r][k], w[c][k], acc);
      v[c] = wave_sum(acc);
    }
    const int row = r0 + r;
    if (lane != 0 || row >= a.M) continue;
    v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
    if (EPI == GEMV_F32) {
      *(float4*)(a.out_f32 + (size_t)row * a.ldo32 + n0) = make_float4(v[0], v[1], v[2], v[3]);
    } else if (EPI == GEMV_RES) {
      float4* xr = (float4*)(a.out_f32 + (size_t)row * a.ldo32 + n0);
      const float4 o = *xr;
      *xr = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]);
    } else if (EPI == GEMV_GELU_T) {
      *(typename Vec<T>::x4*)((T*)a.out_t + (size_t)row * a.ldot + n0) = pack4<T>(gelu_tanh(v[0]), gelu_tanh(v[1]), gelu_tanh(v[2]), gelu_tanh(v[3]));
    } else {  // GEMV_QKV: column n0 = part * dmodel + h * 64 + d, d a multiple of 4 (gemm_impl.h EpiQkvDecode::store)
      const int t = trow[r];
      if (a.row_slot && t < 0) continue;
      const int part = n0 / a.dmodel, cc = n0 - part * a.dmodel;
      const int h = cc >> 6, d = cc & 63;
      const size_t bh = (size_t)row * a.heads + h;
      if (part == 0) {
        *(typename Vec<T>::x4*)((T*)a.qbuf + (size_t)row * a.dmodel + cc) = pack4<T>(v[0] * a.q_scale, v[1] * a.q_scale, v[2] * a.q_scale, v[3] * a.q_scale);
      } else if (part == 1) {
        *(typename Vec<T>::x4*)((T*)a.kc + ((bh * 8 + (d >> 3)) * a.tmax + t) * 8 + (d & 7)) = pack4<T>(v[0], v[1], v[2], v[3]);
      } else {
        *(typename Vec<T>::x4*)((T*)a.vc + (bh * a.tmax + t) * 64 + d) = pack4<T>(v[0], v[1], v[2], v[3]);
      }
    }
  }
}
// KV slot of rows r0 .. r0 + RG - 1 (GEMV_QKV): the device-side step, or on a session handle every row's own
template <int RG, int EPI>
__device__ __forceinline__ void gv_slots(const GemvArgs& a, int r0, int t, int (&trow)[RG]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) trow[r] = (EPI == GEMV_QKV && a.row_slot) ? a.row_slot[min(r0 + r, a.M - 1)] : t;
}

template <typename T, int MR, int KC, int EPI, bool LN>
__global__ __launch_bounds__(256) void gemv_kernel(GemvArgs a) {
  typedef typename Vec<T>::x8 x8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16 + wave * 4;  // this wave's four columns (N % 4 == 0: whole quads, never ragged inside a wave)
  if (n0 >= a.N) return;
  x8 w[4][KC];
  gv_load_w<T, KC>(a, n0, lane, w);
  x8 x[MR][KC];
  if constexpr (LN) {
    static_assert(!LN || KC == 2, "the fused LayerNorm is the trunk's 1024-channel norm");
    float4 f[MR][4], g[4], b[4];
    gv_load_ln_rows<MR>(a, 0, lane, f);
    gv_load_ln_affine(a, lane, g, b);
    gv_norm_rows<T, MR>(a, 0, f, g, b, x);
  } else {
    gv_load_rows<T, MR, KC>(a, 0, lane, x);
  }
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) bv = *(const float4*)(a.bias + n0);
  int t = 0;
  int trow[MR];  // session handle: every row's own slot, requested with the bias (off the tail of the stores); < 0: that row stores nothing
  if (EPI == GEMV_QKV && !a.row_slot) t = *a.step;
  gv_slots<MR, EPI>(a, 0, t, trow);
  gv_rows<T, MR, KC, EPI>(a, 0, n0, lane, w, x, bv, trow);
}

// 5 .. 16 rows (wide session handles): the wave's weight rows are loaded once and the activation rows walk past them in groups of RG,
// the next group's rows in flight while the current one is multiplied (K = 4096: two rows a group, so that the 128 weight registers,
// the group and its successor fit the 256 VGPRs without spilling).  Groups whose rows all have row_live < 0 (free session slots) are
// skipped: no loads, no products, no stores.
template <int KC> struct GvRowGroup { static constexpr int RG = KC == 8 ? 2 : 4; };
template <typename T, int KC, int EPI, bool LN>
__global__ __launch_bounds__(256) void gemv_rows_kernel(GemvArgs a) {
  typedef typename Vec<T>::x8 x8;
  constexpr int RG = GvRowGroup<KC>::RG;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16 + wave * 4;
  if (n0 >= a.N) return;
  const int ng = (a.M + RG - 1) / RG;
  unsigned live = (1u << ng) - 1u;  // bit g: group g (rows g * RG ..) is computed
  if (a.row_live) {
    live = 0u;
    for (int r = 0; r < a.M; ++r)
      if (a.row_live[r] >= 0) live |= 1u << (r / RG);
  }
  if (!live) return;
  x8 w[4][KC];
  gv_load_w<T, KC>(a, n0, lane, w);
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) bv = *(const float4*)(a.bias + n0);
  int t = 0;
  if (EPI == GEMV_QKV && !a.row_slot) t = *a.step;
  int gi = __builtin_ctz(live);
  if constexpr (LN) {
    static_assert(!LN || KC == 2, "the fused LayerNorm is the trunk's 1024-channel norm");
    float4 g[4], b[4], f[RG][4];
    gv_load_ln_rows<RG>(a, gi * RG, lane, f);
    gv_load_ln_affine(a, lane, g, b);
    for (;;) {
      x8 x[RG][KC];
      gv_norm_rows<T, RG>(a, gi * RG, f, g, b, x);
      live &= live - 1u;
      const int gn = live ? __builtin_ctz(live) : -1;
      if (gn >= 0) gv_load_ln_rows<RG>(a, gn * RG, lane, f);
      int trow[RG];
      gv_slots<RG, EPI>(a, gi * RG, t, trow);
      gv_rows<T, RG, KC, EPI>(a, gi * RG, n0, lane, w, x, bv, trow);
      if (gn < 0) break;
      gi = gn;
    }
  } else {
    x8 xn[RG][KC];
    gv_load_rows<T, RG, KC>(a, gi * RG, lane, xn);
    for (;;) {
      x8 x[RG][KC];
#pragma unroll
      for (int r = 0; r < RG; ++r)
#pragma unroll
        for (int k = 0; k < KC; ++k) x[r][k] = xn[r][k];
      live &= live - 1u;
      const int gn = live ? __builtin_ctz(live) : -1;
      if (gn >= 0) gv_load_rows<T, RG, KC>(a, gn * RG, lane, xn);
      int trow[RG];
      gv_slots<RG, EPI>(a, gi * RG, t, trow);
      gv_rows<T, RG, KC, EPI>(a, gi * RG, n0, lane, w, x, bv, trow);
      if (gn < 0) break;
      gi = gn;
    }
  }
}

bool gemv_supported(int dtype, const GemvArgs& a) {
  const bool rows_ok = a.ln_x ? (a.K == 1024 && (a.ldx & 3) == 0 && ((size_t)a.ln_x & 15) == 0 && a.ln_g && a.ln_b && ((size_t)a.ln_g & 15) == 0 && ((size_t)a.ln_b & 15) == 0 &&
                                 (a.epi == GEMV_QKV || a.epi == GEMV_GELU_T))
                              : (a.A && (a.lda & 7) == 0 && ((size_t)a.A & 15) == 0);
  return (dtype == DT_BF16 || dtype == DT_F16) && a.M >= 1 && a.M <= 16 && (a.K == 1024 || a.K == 2048 || a.K == 4096) && (a.N & 3) == 0 && rows_ok &&
         (a.ldw & 7) == 0 && ((size_t)a.W & 15) == 0 && (!a.bias || ((size_t)a.bias & 15) == 0) &&
         (a.epi == GEMV_QKV ? ((a.step || a.row_slot) && a.qbuf && a.kc && a.vc && a.dmodel % 64 == 0 && a.N == 3 * a.dmodel && a.heads * 64 == a.dmodel)
          : a.epi == GEMV_GELU_T ? (a.out_t && ((size_t)a.out_t & 7) == 0 && (a.ldot & 3) == 0)
                                 : (a.out_f32 && ((size_t)a.out_f32 & 15) == 0 && (a.ldo32 & 3) == 0));
}

template <typename T, int MR, int KC, int EPI, bool LN>
static void gemv_go(const ProfScope& ps, const GemvArgs& a, hipStream_t s) {
  const dim3 grid(cdiv(a.N, 16));
  if constexpr (MR > 4) launch_timed(ps, gemv_rows_kernel<T, KC, EPI, LN>, grid, dim3(256), 0, s, a);
  else launch_timed(ps, gemv_kernel<T, MR, KC, EPI, LN>, grid, dim3(256), 0, s, a);
}
template <typename T, int MR, int KC>
static void gemv_dispatch_epi(const ProfScope& ps, const GemvArgs& a, hipStream_t s) {
  if constexpr (KC == 2) {
    if (a.ln_x) {  // the two GEMVs behind a LayerNorm (gemv_supported)
      if (a.epi == GEMV_GELU_T) gemv_go<T, MR, KC, GEMV_GELU_T, true>(ps, a, s);
      else gemv_go<T, MR, KC, GEMV_QKV, true>(ps, a, s);
      return;
    }
  }
  switch (a.epi) {
    case GEMV_F32: gemv_go<T, MR, KC, GEMV_F32, false>(ps, a, s); break;
    case GEMV_RES: gemv_go<T, MR, KC, GEMV_RES, false>(ps, a, s); break;
    case GEMV_GELU_T: gemv_go<T, MR, KC, GEMV_GELU_T, false>(ps, a, s); break;
    default: gemv_go<T, MR, KC, GEMV_QKV, false>(ps, a, s); break;
  }
}
template <typename T, int MR>
static void gemv_dispatch_k(const ProfScope& ps, const GemvArgs& a, hipStream_t s) {
  if (a.K == 1024) gemv_dispatch_epi<T, MR, 2>(ps, a, s);
  else if (a.K == 2048) gemv_dispatch_epi<T, MR, 4>(ps, a, s);
  else gemv_dispatch_epi<T, MR, 8>(ps, a, s);
}
template <typename T>
static void gemv_dispatch_m(const ProfScope& ps, const GemvArgs& a, hipStream_t s) {
  if (a.M == 1) gemv_dispatch_k<T, 1>(ps, a, s);
  else if (a.M == 2) gemv_dispatch_k<T, 2>(ps, a, s);
  else if (a.M <= 4) gemv_dispatch_k<T, 4>(ps, a, s);
  else gemv_dispatch_k<T, 16>(ps, a, s);  // gemv_rows_kernel
}

int gemv_launch(int dtype, const GemvArgs& a, hipStream_t stream) {
  TT_REQUIRE(gemv_supported(dtype, a), "gemv: unsupported problem (M=%d N=%d K=%d epi=%d dtype=%d): M <= 16, K in {1024, 2048, 4096}, N %% 4 == 0, aligned operands", a.M, a.N, a.K,
             a.epi, dtype);
  // algorithmic work: the weights once, the rows in and out
  ProfScope ps(PROF_GEMV, stream, 2.0 * a.M * a.N * a.K, 2.0 * a.N * a.K + 2.0 * a.M * a.K + 4.0 * a.M * a.N, true);
  if (dtype == DT_BF16) gemv_dispatch_m<bf16>(ps, a, stream);
  else gemv_dispatch_m<f16>(ps, a, stream);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace tt
