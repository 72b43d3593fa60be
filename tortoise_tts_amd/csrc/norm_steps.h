// The steps that the row-norm and GroupNorm kernels share (norm.hip: rownorm_kernel, rownorm_narrow_kernel, rownorm_wave_kernel,
// gn_apply_kernel, gn_apply_c1024_kernel; gemm_gna.h: the statistics prologue of gemm_gna_kernel).  Each kernel keeps its own schedule -
// which operand is requested when - and takes the arithmetic from here.  Every floating-point expression is whole inside one step: the
// build contracts per expression (-ffp-contract=on), so an expression cut at a function boundary would round differently.
#pragma once
#include "ops.h"

namespace tt {

// ------------------------------------------------------------------------------- row norm
// A row lives in registers as float4 quads.  A span is the set of threads that share one row: thread t of N holds quad j at
// column (t + N j) * 4, and sum() adds one float per thread over the span.
struct BlockSpan {  // one 256-thread workgroup per row; red: 4 floats of LDS, recycled behind a barrier
  static constexpr int N = 256;
  float* red;
  __device__ __forceinline__ int t() const { return threadIdx.x; }
  __device__ __forceinline__ float sum(float v) { return block_sum_256(v, red); }
};
struct FreshBlockSpan {  // the same with one 4-float array per reduction: no barrier is needed to recycle it
  static constexpr int N = 256;
  float* red;
  __device__ __forceinline__ int t() const { return threadIdx.x; }
  __device__ __forceinline__ float sum(float v) {
    float* r = red;
    red += 4;
    return block_sum_256_fresh(v, r);
  }
};
struct WaveSpan {  // one wave per row: the reductions are register shuffles only
  static constexpr int N = 64;
  __device__ __forceinline__ int t() const { return threadIdx.x & 63; }
  __device__ __forceinline__ float sum(float v) { return wave_sum(v); }
};
template <class Span> __device__ __forceinline__ int span_col(const Span& sp, int j) { return (sp.t() + Span::N * j) * 4; }

__device__ __forceinline__ void quad_add(float4& t, const float4 p) { t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w; }
__device__ __forceinline__ float quad_sum(const float4 t) { return t.x + t.y + t.z + t.w; }
__device__ __forceinline__ float quad_sumsq(const float4 t) { return t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w; }
__device__ __forceinline__ float quad_centred_sumsq(const float4 t, float mean) {
  const float dx = t.x - mean, dy = t.y - mean, dz = t.z - mean, dw = t.w - mean;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}

// Row update, one quad (xr: the row of x): source row (x_in, else x) + bias + split-K slabs in slab order, written back to x when write_x.  Two halves so
// that a kernel can put further requests between them: row_request issues the loads whose number is known at compile time, row_update
// adds in order.  NSLAB < 0: a.nslab slabs, one round trip per slab; BIAS < 0: whether a.add_bias is set.
template <int NSLAB, int BIAS> struct RowQuad { float4 t, bias, slab[NSLAB > 0 ? NSLAB : 1]; };
__device__ __forceinline__ const float* row_slab(const RowNormArgs& a, int row, int c, int s) { return a.add_slabs + (size_t)s * a.slab_stride + (size_t)row * a.ldslab + c; }

template <int NSLAB, int BIAS>
__device__ __forceinline__ void row_request(const RowNormArgs& a, int row, const float* xr, int c, RowQuad<NSLAB, BIAS>& q) {
  const float* src = a.x_in ? a.x_in + (size_t)row * a.ldxin : xr;
  q.t = *(const float4*)(src + c);
  if (BIAS > 0 || (BIAS < 0 && a.add_bias)) q.bias = *(const float4*)(a.add_bias + c);
#pragma unroll
  for (int s = 0; s < NSLAB; ++s) q.slab[s] = *(const float4*)row_slab(a, row, c, s);
}
template <int NSLAB, int BIAS>
__device__ __forceinline__ float4 row_update(const RowNormArgs& a, int row, float* xr, int c, bool live, const RowQuad<NSLAB, BIAS>& q) {
  float4 t = q.t;
  if (BIAS > 0 || (BIAS < 0 && a.add_bias)) quad_add(t, q.bias);
  if constexpr (NSLAB >= 0) {
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) quad_add(t, q.slab[s]);
  } else {
    for (int s = 0; s < a.nslab; ++s) quad_add(t, *(const float4*)row_slab(a, row, c, s));
  }
  if (a.write_x && live) *(float4*)(xr + c) = t;
  return t;
}

// the thread's share of the row sum: its live quads in j order
template <int J, class Span>
__device__ __forceinline__ float row_sum(const float4 (&v)[J], const Span& sp, int D) {
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (span_col(sp, j) < D) sum += quad_sum(v[j]);
  return sum;
}

// NaN / inf in the row: an operand overflowed upstream.  One count per row, from the span's first thread.
template <class Span> __device__ __forceinline__ void row_guard(int* guard, const Span& sp, float stat) {
  if (guard && sp.t() == 0 && !(stat < INFINITY)) atomicAdd(guard, 1);
}

// x-transformers RMSNorm: x / max(||x|| * D^-0.5, eps) * g.  Quads beyond the row are zero.
template <int J, class Span>
__device__ __forceinline__ float rms_inv(const float4 (&v)[J], Span& sp, int D, float eps, int* guard) {
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) sq += quad_sumsq(v[j]);
  sq = sp.sum(sq);
  row_guard(guard, sp, sq);
  const float nrm = sqrtf(sq) * rsqrtf((float)D);
  return 1.0f / fmaxf(nrm, eps);
}
__device__ __forceinline__ float4 rms_scale(const float4 v, float inv, const float4 g) {
  return make_float4(v.x * inv * g.x, v.y * inv * g.y, v.z * inv * g.z, v.w * inv * g.w);
}

// One LayerNorm pass over a register row: mean from the threads' sums, two-pass (centred) variance in registers, then the affine per quad.
struct LnStats { float mean, rstd; };
template <int J, class Span>
__device__ __forceinline__ LnStats ln_stats(const float4 (&v)[J], float sum, Span& sp, int D, float eps, int* guard) {
  LnStats st;
  st.mean = sp.sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (span_col(sp, j) < D) sq += quad_centred_sumsq(v[j], st.mean);
  const float var = sp.sum(sq) / (float)D;
  row_guard(guard, sp, var);
  st.rstd = rsqrtf(var + eps);
  return st;
}
__device__ __forceinline__ float4 ln_affine(const float4 v, const LnStats st, const float4 g, const float4 b) {
  return make_float4((v.x - st.mean) * st.rstd * g.x + b.x, (v.y - st.mean) * st.rstd * g.y + b.y, (v.z - st.mean) * st.rstd * g.z + b.z,
                     (v.w - st.mean) * st.rstd * g.w + b.w);
}

// Emit one quad of the normalised row: the GEMM operand type and / or the f32 copy (o32: out_f32, or the block row_f32_block chose).
template <typename T>
__device__ __forceinline__ void row_emit(const RowNormArgs& a, float* o32, int row, int c, const float4 y) {
  if (a.out_t) *(typename Vec<T>::x4*)((T*)a.out_t + (size_t)row * a.ldot + c) = pack4<T>(y.x, y.y, y.z, y.w);
  if (o32) *(float4*)(o32 + (size_t)row * a.ldo32 + c) = y;
}
// the f32 copy's block under a step counter (f32_slot) or the row's own counter (f32_row_slot; negative: this row files nothing)
__device__ __forceinline__ float* row_f32_block(const RowNormArgs& a, int row) {
  float* o32 = a.out_f32;
  if (o32 && a.f32_slot) o32 += (size_t)(*a.f32_slot + a.f32_slot_base) * a.f32_slot_stride;
  if (o32 && a.f32_row_slot) {
    const int sl = a.f32_row_slot[row];
    o32 = sl < 0 ? nullptr : o32 + (size_t)(sl + a.f32_slot_base) * a.f32_slot_stride;
  }
  return o32;
}

// ------------------------------------------------------------------------------- group norm
// Per-quad transform in three steps (a kernel may request the scale / shift quads between the first two): the affine on the group's
// statistics; (1 + scale) / shift; activation and exact zeros for a padding row (the next conv's zero padding).
__device__ __forceinline__ float4 gn_affine(const float4 t, float mu, float rs, const float4 gm, const float4 bt) {
  return make_float4((t.x - mu) * rs * gm.x + bt.x, (t.y - mu) * rs * gm.y + bt.y, (t.z - mu) * rs * gm.z + bt.z, (t.w - mu) * rs * gm.w + bt.w);
}
__device__ __forceinline__ float4 gn_scale_shift(const float4 y, const float4 sc, const float4 sh) {
  return make_float4(y.x * (1.f + sc.x) + sh.x, y.y * (1.f + sc.y) + sh.y, y.z * (1.f + sc.z) + sh.z, y.w * (1.f + sc.w) + sh.w);
}
__device__ __forceinline__ float4 gn_act_pad(const float4 y, int act, bool pad_row) {
  float v[4] = {y.x, y.y, y.z, y.w};
  if (act != ACT_NONE) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = apply_act(v[i], act, 0.f);
  }
  if (pad_row) v[0] = v[1] = v[2] = v[3] = 0.f;
  return make_float4(v[0], v[1], v[2], v[3]);
}
template <typename T>
__device__ __forceinline__ void gn_emit(const GroupNormArgs& a, size_t off, int c, const float4 y) {
  if (a.out_t) *(typename Vec<T>::x4*)((T*)a.out_t + off * a.ldot + c) = pack4<T>(y.x, y.y, y.z, y.w);
  if (a.out_f32) *(float4*)(a.out_f32 + off * a.ldo32 + c) = y;
}

// Statistics partials of a producing GEMM's epilogue, [row_tile][slot][C / 16][2]: sample b's items are (row tile, 16-column strip of the
// group) pairs, 1 << SPG_SHIFT strips per group.  All index arithmetic is shifts and compares: the tile height is a power of two
// (r_shift its log2) and the strips per group a compile-time one, because this code sits in front of every activation load of its
// kernel (integer divisions by run-time values cost ~30 instructions each, 3 per item).
struct GnItems { int t0, n; };  // first row tile, number of items
template <int SPG_SHIFT> __device__ __forceinline__ GnItems gn_items(int b, int S, int r_shift) {
  const int t0 = (b * S) >> r_shift, t1 = ((b + 1) * S - 1) >> r_shift;
  return GnItems{t0, (t1 - t0 + 1) << SPG_SHIFT};
}
template <int SPG_SHIFT>
__device__ __forceinline__ float2 gn_partial_item(const float* gemm_part, int S, int b, int g, int e, const GnItems it, int nc16, int r_shift) {
  const int ec = min(e, it.n - 1);  // clamped, unconditional load; out-of-range items are left out by the caller
  const int t = it.t0 + (ec >> SPG_SHIFT), strip = (g << SPG_SHIFT) + (ec & ((1 << SPG_SHIFT) - 1));
  // a row tile's slot 0 holds the rows of the sequence its FIRST row belongs to, slot 1 those of the next sequence: tile t of
  // sample b starts inside sample b unless it is the first tile and straddles in from sample b - 1
  const int slot = ((t << r_shift) < b * S) ? 1 : 0;
  return *(const float2*)(gemm_part + (((size_t)t * 2 + slot) * nc16 + strip) * 2);
}

// Group g's (sum, sum of squares) from the 8 per-part fp64 sums in LDS, in part order, and its mean / rstd from them.  The sums are
// combined in fp64 (E[x^2] - E[x]^2 cancels in fp32); the reciprocal square root of the O(1) result is an fp32 instruction, not an fp64
// divide + square root (hundreds of cycles on the one wave every workgroup waits for).  inv_n = 1 / (rows * C / 32).
struct GnSums { double s, q; };
__device__ __forceinline__ GnSums gn_combine(const double (*part_s)[32], const double (*part_q)[32], int g) {
  GnSums t{0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    t.s += part_s[p][g];
    t.q += part_q[p][g];
  }
  return t;
}
template <class Args>  // GroupNormArgs / GnaArgs: eps and the guard counter
__device__ __forceinline__ void gn_mean_rstd(const GnSums t, double inv_n, const Args& a, float& mean, float& rstd) {
  const double m = t.s * inv_n;
  double var = t.q * inv_n - m * m;
  if (a.guard && !(var < 1.0e300)) atomicAdd(a.guard, 1);  // NaN / inf statistics: an operand overflowed upstream
  if (var < 0.0) var = 0.0;
  mean = (float)m;
  rstd = rsqrtf((float)var + a.eps);
}

}  // namespace tt
