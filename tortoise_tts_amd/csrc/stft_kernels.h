// The kernel bodies of the analysis / synthesis chain that csrc/formant.hip and csrc/denoise.hip share, built from stft_steps.h.  Each is the
// whole text of one kernel for ONE clip (the caller's __global__ picks the clip from blockIdx.y and its own clip table) with the part that
// differs between the two chains as a functor, inlined:
//
//   stft_tile_body     re, im of 32 frames x 32 bins per wave (the virtual frame operand staged once per workgroup in LDS); the epilogue
//                      gets the two accumulators as they stand: epi(re, im, t0, T, column, h), lane (column, h), register r = frame
//                      t0 + mfma_row(r, h) - registers 4 g .. 4 g + 3 are the four consecutive frames t0 + 8 g + 4 h ..
//   stft_inverse_body  y[t][k] = Z[t] . inverse[:, k], Z = (re, im) * mult(g) formed in the A operand's registers: mult maps the float2 of
//                      the two bins' gains to their two multipliers (formant: exp, denoise: the gains themselves)
//   stft_ola_body      out[j] = sum_t y[t][j + n_fft / 2 - t hop] / sum_t window^2, increasing t, one thread per sample, no atomics
//
// A frame's summation order over k depends on nothing but k, so a clip's bits do not depend on the batch it is in.
#pragma once
#include "stft_steps.h"

namespace tt {

// x: the clip (n samples, T = 1 + n / hop frames); blockIdx.x: the tile of 32 frames, blockIdx.z: bins_per_block bins, 32 per wave; xs: the
// workgroup's dynamic LDS (stft_lds_bytes); nt: the workgroup's threads
template <class Epi>
__device__ __forceinline__ void stft_tile_body(const float* __restrict__ x, int n, int T, const float* __restrict__ basis, int n_fft, int hop,
                                               int bins_pad, int bins_per_block, int nt, float* xs, const Epi& epi) {
  const int t0 = blockIdx.x * kStftTile;
  if (t0 >= T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  stft_stage(x, n, t0, n_fft, hop, xs, tid, nt);
  __syncthreads();
  const int b0 = blockIdx.z * bins_per_block + wave * 32;
  if (b0 >= bins_pad) return;
  const int i = lane & 31, h = lane >> 5;
  f32x16 re, im;
#pragma unroll
  for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
  stft_mfma(xs, basis, n_fft, hop, bins_pad, b0, lane, re, im);
  epi(re, im, t0, T, b0 + i, h);
}

// spec [T][2 bins_pad], gains [T][bins_pad] and y [T][n_fft] of the clip; waves: the 32-sample column tiles of one workgroup
template <class Mult>
__device__ __forceinline__ void stft_inverse_body(const float* __restrict__ spec, const float* __restrict__ gains, int T,
                                                  const float* __restrict__ inverse, int n_fft, int bins_pad, int waves, float* __restrict__ y,
                                                  const Mult& mult) {
  const int t0 = blockIdx.x * kStftTile;
  if (t0 >= T) return;
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int n0 = (blockIdx.z * waves + (threadIdx.x >> 6)) * 32;
  if (n0 >= n_fft) return;
  const size_t row = (size_t)min(t0 + i, T - 1);
  const float* sp = spec + row * 2 * bins_pad + 4 * h;
  const float* gp = gains + row * bins_pad + 2 * h;
  const float* ib = inverse + (size_t)(4 * h) * n_fft + n0 + i;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < 2 * bins_pad; k += 8) {  // (re, im) of two bins per lane and trip
    float4 z = *(const float4*)(sp + k);
    const float2 g = *(const float2*)(gp + k / 2);
    const float* b = ib + (size_t)k * n_fft;  // rows_mfma8's four loads and four MFMAs, the loads pinned ahead of the gain's arithmetic:
    float b0 = b[0], b1 = b[n_fft], b2 = b[2 * (size_t)n_fft], b3 = b[3 * (size_t)n_fft];
    asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));  // left to itself the compiler issues them one by one, each waited for
    const float2 e = mult(g);
    z.x *= e.x; z.y *= e.x; z.z *= e.y; z.w *= e.y;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.x, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.y, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.z, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(z.w, b3, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + mfma_row(r, h);
    if (t < T) y[(size_t)t * n_fft + n0 + i] = acc[r];
  }
}

// y [T][n_fft] of the clip, out its n samples; one thread per sample, nt of them per workgroup
__device__ __forceinline__ void stft_ola_body(const float* __restrict__ y, int n, int T, const float* __restrict__ basis, int n_fft, int hop,
                                              int bins_pad, int nt, float* __restrict__ out) {
  const int j = blockIdx.x * nt + threadIdx.x;
  if (j >= n) return;
  const int p = j + n_fft / 2;  // position in the padded clip: frame t covers t hop .. t hop + n_fft - 1
  const int tlo = p >= n_fft ? (p - n_fft) / hop + 1 : 0, thi = min(p / hop, T - 1);
  float num = 0.f, den = 0.f;
  for (int t = tlo; t <= thi; ++t) {
    const int k = p - t * hop;
    const float w = basis[(size_t)k * 2 * bins_pad];  // column 0: window[k] cos(0)
    num += y[(size_t)t * n_fft + k];
    den += w * w;
  }
  out[j] = num / den;
}

}  // namespace tt
