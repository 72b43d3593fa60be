// The wave-level steps of the f32 STFT family on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation), as csrc/melfront.hip
// first wrote them inline in mel_stft_kernel / mel_project_kernel; csrc/formant.hip builds its kernels from them.  melfront.hip keeps its
// own inline text (its binary is the measured one), so a change to a step here must be weighed against it by hand.
//
//   stft_stage        a workgroup stages the one contiguous stretch of the clip its 32 centred frames cover (31 * hop + n_fft samples,
//                     reflected once) in LDS, one pad word per hop samples: the 32 lanes of an A read (stride hop) hit 32 banks
//   stft_mfma         frames (rows) x 32 bins (columns): A is virtual (frame i, column k = staged sample i * hop + k), B the cos / -sin
//                     pair of a bin from the table [n_fft][2 * bins_pad]; re and im of a bin end in the same lane and register
//   rows_mfma8        eight k of a row-major A (one float4 per lane: lane (i, h) holds k + 4 h .. k + 4 h + 3 of row i) against a table
//                     B[k][col]: MFMA j multiplies the pairs (k + j, k + 4 + j), a fixed order whatever the batch
//   mfma_row          D lane l, register r = D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]
#pragma once
#include "common.h"

namespace tt {

constexpr int kStftTile = 32;  // frames of one MFMA block

__device__ __forceinline__ int stft_pos(int p, int hop) { return p + p / hop; }
static inline size_t stft_lds_bytes(int n_fft, int hop) {
  const int span = (kStftTile - 1) * hop + n_fft;
  return sizeof(float) * ((size_t)span + span / hop + 1);
}

__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// x: the clip (n samples); frames t0 .. t0 + 31; tid / nt: this thread and the workgroup's size.  The caller synchronises.
__device__ __forceinline__ void stft_stage(const float* __restrict__ x, int n, int t0, int n_fft, int hop, float* xs, int tid, int nt) {
  const int span = (kStftTile - 1) * hop + n_fft;
  const int q0 = t0 * hop - n_fft / 2;
  for (int p = tid; p < span; p += nt) {
    int q = q0 + p;
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    xs[stft_pos(p, hop)] = q >= 0 && q < n ? x[q] : 0.f;  // (beyond the reflection: only frames >= T read it, and those are not written)
  }
}

// re / im += frames . basis[:, b0 + i] over all n_fft samples.  hop divides n_fft and is a multiple of 8: a group of four k pairs lies
// in one chunk, whose pad offset is kc / hop.  b0 + 31 < bins_pad.
__device__ __forceinline__ void stft_mfma(const float* xs, const float* __restrict__ basis, int n_fft, int hop, int bins_pad, int b0, int lane,
                                          f32x16& re, f32x16& im) {
  const int i = lane & 31, h = lane >> 5;
  const float* bp = basis + 2 * (size_t)(b0 + i);
  const size_t ldb = 2 * (size_t)bins_pad;
  const int arow = i * (hop + 1);
  for (int kc = 0; kc < n_fft; kc += hop) {
    const float* xa = xs + arow + kc + kc / hop + h;
    const float* bk = bp + (size_t)(kc + h) * ldb;
    for (int k0 = 0; k0 < hop; k0 += 8) {  // four k pairs per trip, their loads issued ahead of the eight MFMAs
      float a[4];
      float2 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = xa[k0 + 2 * j];
        w[j] = *(const float2*)(bk + (size_t)(k0 + 2 * j) * ldb);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[j].x, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[j].y, im, 0, 0, 0);
      }
    }
  }
}

// acc += A[:, k .. k + 7] . B[k .. k + 7][:]: a = this lane's four A values (k + 4 h ..), b -> B[k + 4 h][this lane's column], ldb B's row length
__device__ __forceinline__ void rows_mfma8(const float4 a, const float* __restrict__ b, size_t ldb, f32x16& acc) {
  const float b0 = b[0], b1 = b[ldb], b2 = b[2 * ldb], b3 = b[3 * ldb];
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, acc, 0, 0, 0);
}

}  // namespace tt
