// The steps that the sampling kernels share (sampling.hip: sample_kernel, sample_wide_kernel, typical_mask_kernel and the ar_* bookkeeping
// kernels).  Each kernel keeps its own schedule and LDS plan and takes the arithmetic from here: one definition of the score, the draw,
// the (value, token) argmax and the sequential top-p sums, so that the restatement of the reference's sampling loop cannot drift between
// the kernels.  Every floating-point expression is whole inside one step (-ffp-contract=on works per expression).
// The first part is plain C++: checks/sample_host_check.cpp compiles it without HIP and runs it under the host sanitizers.
#pragma once
#ifdef __HIPCC__
#include "ops.h"
#define TT_PURE __host__ __device__ __forceinline__
#else
#define TT_PURE inline
#endif

namespace tt {

// ------------------------------------------------------------------------------- pure functions
// order-preserving map float -> unsigned (key order == float order once -0.0 is folded into +0.0: sample_score) and back
TT_PURE unsigned f2key(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
TT_PURE float key2f(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

TT_PURE void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// a Philox word -> u in (0, 1).  The sum rounds to even from 2^23 on, so r >> 8 == 0xFFFFFF alone would give 2^24, u == 1, q == -log u == -0.0
// and p / q == -inf: a token that could never be drawn where its q should be the SMALLEST there is.  That one value in 2^24 takes the largest
// float below 1 instead (q = 6e-8; sample_host_check.cpp checks both ends).  A deliberate difference from the kernels before sample_steps.h.
TT_PURE float philox_u(unsigned r) {
  const float u = ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f);
  return u < 1.0f ? u : 0.99999994f;
}

// RepetitionPenaltyLogitsProcessor on one score (the typical mask takes this piece alone), then temperature; -0.0 ties with +0.0 in
// the reference's float comparisons: one zero, so that key order == float order
TT_PURE float sample_penalty(float s, bool seen_bit, float rep_penalty) {
  if (rep_penalty != 1.0f && seen_bit) s = s < 0.f ? s * rep_penalty : s / rep_penalty;
  return s;
}
template <class Scalars> TT_PURE float sample_score(float raw, bool seen_bit, const Scalars& sc) {
  float s = sample_penalty(raw, seen_bit, sc.rep_penalty);
  if (sc.temperature != 1.0f) s = s / sc.temperature;
  if (__builtin_bit_cast(unsigned, s) == 0x80000000u) s = 0.f;
  return s;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------- the row
// the row's sampling scalars: its own entry on a session handle with per-row scalars (block-uniform, read once), else the argument block
__device__ __forceinline__ SampleScalars sample_scalars(const SampleArgs& a, int b) {
  if (a.rows) return a.rows[b];
  SampleScalars sc;
  sc.rep_penalty = a.rep_penalty; sc.temperature = a.temperature; sc.top_p = a.top_p; sc.top_k = a.top_k; sc.typical_mass = a.typical_mass;
  return sc;
}
__device__ __forceinline__ int sample_step(const SampleArgs& a, int b) { return a.sess ? a.sess[SESS_N * a.B + b] : a.state[0]; }
__device__ __forceinline__ const float* sample_logits(const SampleArgs& a, int b, int grp, int step) {
  if (a.sess) return (step == 0 && a.pre_logits ? a.pre_logits : a.logits) + (size_t)b * a.ldl;  // token 0: the row's admission prefill
  return a.logits + (a.ldl ? (size_t)b * a.ldl : (size_t)grp * (a.ldg ? a.ldg : a.V));
}
// Everything block-uniform that a sampler knows about its row b, read once
struct SampleRow {
  int b, step, grp;        // step: Philox counter and codes column; grp: utterance of this row
  int row_offset;          // global candidate index of row 0 (its load is awaited by the first Philox draw only: see cand())
  unsigned long long key;  // Philox key of the row's utterance
  const float* lg;
  unsigned* seen;
  // global index of the candidate within its utterance (the draw does not depend on the batching); a session row is candidate 0
  __device__ __forceinline__ int cand(const SampleArgs& a) const { return a.sess ? 0 : row_offset + (a.ngroups > 1 ? b - grp * a.group_size : b); }
};
__device__ __forceinline__ SampleRow sample_row(const SampleArgs& a, const SampleScalars& sc, int b) {
  SampleRow r;
  r.b = b;
  r.step = sample_step(a, b);
  r.grp = a.ngroups > 1 ? b / a.group_size : 0;
  // the key comes from device memory when the caller replays a cached step graph (the seed of a call is then data, not a baked-in kernel
  // argument), else from the argument block; a session row has its own key.  row_offset likewise.
  r.key = a.keys_dev ? a.keys_dev[a.sess ? b : r.grp] : (a.ngroups > 1 ? a.group_seeds[r.grp] : a.seed);
  r.row_offset = a.row_offset_dev ? *a.row_offset_dev : a.row_offset;
  // per-row scalars: a typical row reads the mask's output row, the others their own source (sample_launch switches `logits` for the
  // whole launch otherwise)
  r.lg = a.rows && sc.typical_mass != 0.f ? a.typical_out + (size_t)b * a.ldl : sample_logits(a, b, r.grp, r.step);
  r.seen = a.seen + (size_t)b * ((a.V + 31) / 32);
  return r;
}

// ------------------------------------------------------------------------------- the draw
// multinomial(p, 1) == argmax(p / q), q ~ Exp(1): this is the only place that reads exp_noise or runs Philox.  `id` must be a token (< V).
__device__ __forceinline__ float sample_draw(const SampleArgs& a, const SampleRow& r, int id, float p) {
  float q;
  if (a.exp_noise) {
    q = a.exp_noise[((size_t)r.step * a.B + r.b) * a.V + id];
  } else {
    unsigned o[4];
    philox4x32_10((unsigned)id, (unsigned)r.step, (unsigned)r.cand(a), 0u, (unsigned)r.key, (unsigned)(r.key >> 32), o);
    q = -__logf(philox_u(o[0]));
  }
  return p / q;
}

// ------------------------------------------------------------------------------- the best (value, token) pair
// order: value descending, token ascending.  The initial pair loses to every real one; a row of non-finite scores keeps it (sample_commit).
struct Best {
  float v = -1.f;
  int i = 0x7fffffff;
  __device__ __forceinline__ void take(float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
};
__device__ __forceinline__ Best best_wave(Best b) {  // every lane gets the wave's best
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b.take(__shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64));
  return b;
}
// NW waves; thread 0 gets the block's best (one barrier; red_v / red_i: NW slots of LDS)
template <int NW> __device__ __forceinline__ Best best_block(Best b, float* red_v, int* red_i, int tid) {
  b = best_wave(b);
  if ((tid & 63) == 0) {
    red_v[tid >> 6] = b.v;
    red_i[tid >> 6] = b.i;
  }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < NW; ++w) b.take(red_v[w], red_i[w]);
  return b;
}

// ------------------------------------------------------------------------------- softmax and top-p in the oracle's arithmetic
// The total, the ascending cumulative cut and the kept total are strictly sequential sums in index order: the kept set is decided with
// exactly the additions and divisions the oracle's cumulative sum makes.  Every lane of ONE wave computes them redundantly; values are
// handed round with v_readlane (a few cycles each) instead of one dependent LDS round trip (~100 cycles) per element.
__device__ __forceinline__ float softmax_e(float s, float smax) { return __expf(s - smax); }
__device__ __forceinline__ float lane_value(float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); }
// v of lanes 0 .. 63 added left to right, fully unrolled (lanes beyond the data hold +0.0, which changes no partial sum)
__device__ __forceinline__ float seq_sum_wave(float v) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 64; ++j) acc += lane_value(v, j);
  return acc;
}
// x[0 .. n) in LDS, 64 at a time through seq_sum_wave's chain (acc carried on): same additions in the same order as `for (i) acc += x[i]`.
// UNROLL = 64 spells the chain out (the full-sort sampler, n up to the vocabulary: generate at top_k = 0 110 -> 84 ms for 16 x 64 tokens);
// UNROLL = 1 keeps it a loop: sample_kernel's rare plateau tail, where the 3 x 64 spelled-out links cost every launch 0.9 us (the
// kernel's code grew by 600 instructions; profiles/sampler_refactor_bench.txt)
template <int UNROLL> __device__ __forceinline__ float seq_sum_lds(const float* x, int n, int lane) {
  float acc = 0.f;
  for (int base = 0; base < n; base += 64) {
    const float v = base + lane < n ? x[base + lane] : 0.f;
#pragma unroll UNROLL
    for (int j = 0; j < 64; ++j) acc += lane_value(v, j);
  }
  return acc;
}
// TopPLogitsWarper over e[0 .. n) in LDS (descending): the ascending cumulative probability of element r is the sum of e[i] / total over
// i = n-1 .. r; elements whose sum stays <= 1 - top_p go, at least one stays.  Returns the number kept.  The divisions happen on load,
// 64 at a time (the same IEEE division a serial walk makes); the partial sums never decrease, so the first element of a chunk whose sum
// exceeds the cut is known from HOW MANY of the chunk's 64 sums do: no branch per element.
template <int UNROLL> __device__ __forceinline__ int top_p_keep_lds(const float* e, int n, float total, float top_p, int lane) {
  if (!(top_p < 1.0f)) return n;
  const float thr = 1.0f - top_p;
  float tail = 0.f;
  for (int hi = n - 1; hi >= 1; hi -= 64) {  // elements hi, hi - 1, ... in chunks of 64 (lane j holds element hi - j; +0.0 below element 1)
    const int r_l = hi - lane;
    const float v = r_l >= 1 ? e[r_l] / total : 0.f;
    int over = 0;
#pragma unroll UNROLL
    for (int j = 0; j < 64; ++j) {
      tail += lane_value(v, j);
      over += tail > thr ? 1 : 0;
    }
    if (over) return hi - (64 - over) + 1;
  }
  return 1;
}

// ------------------------------------------------------------------------------- embedding rows and step bookkeeping
// whole block: x[:] = tok_row[:] + pos_row[:] (mel_embedding[token] + mel_pos_embedding[position]), D a multiple of 4
__device__ __forceinline__ void embed_row(float* x, const float* tok_row, const float* pos_row, int D, int tid, int nthreads) {
  for (int c = tid * 4; c < D; c += nthreads * 4) {
    const float4 e = *(const float4*)(tok_row + c);
    const float4 p = *(const float4*)(pos_row + c);
    *(float4*)(x + c) = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
  }
}
// whole block: the input row of a row that does not decode, so that the rows the batch carries along stay finite
__device__ __forceinline__ void zero_row(float* x, int D, int tid, int nthreads) {
  for (int c = tid * 4; c < D; c += nthreads * 4) *(float4*)(x + c) = make_float4(0.f, 0.f, 0.f, 0.f);
}
// one thread, last kernel of a step: state[0] = tokens sampled so far, state[1] = slot / index of the newest token (the one the next
// decode step feeds), state[2] = index of the first token after which every row had stopped (-1: none yet).  With `progress` (pinned host
// memory) the two host-visible words are published with system-scope stores: the host paces and ends its launch loop on them without
// draining the queue (tt_ar_generate).
__device__ __forceinline__ void ar_publish_step(int* state, const int* unfinished_count, int* progress) {
  const int step = state[0];  // index of the token the sampler just produced
  state[0] = step + 1;
  state[1] = step;
  if (progress) {
    if (unfinished_count && unfinished_count[step] == 0 && state[2] < 0) {
      state[2] = step;
      __hip_atomic_store(progress + 1, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(progress, step + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// word w of a fresh row's seen mask: fake_inputs = [1] * P + [start_mel_token] (autoregressive.py:546-548), ids 1 and start are "seen"
__device__ __forceinline__ unsigned seen_init_word(int w, int start_token) {
  unsigned v = 0u;
  if (w == 0) v |= 1u << 1;
  if (w == (start_token >> 5)) v |= 1u << (start_token & 31);
  return v;
}
#endif  // __HIPCC__

}  // namespace tt
