// Band-limited resampling at an arbitrary ratio (include/tortoise_mi355x_rs.h): pitch and output sample rate of finished clips.
//
//   rs_prepare_kernel    one workgroup: every clip's status, and a zero in `peak` for the clips that will be resampled.
//   rs_resample_kernel   outputs are independent, so the work is (clip, tile of kRsTile = 1024 consecutive outputs).  The grid is one
//                        workgroup of 1024 threads per CU (the LDS below allows one), and workgroup b takes tiles b, b + grid, ... of the list
//                        clip 0's tiles, clip 1's tiles, ...: every workgroup derives that list from the offsets and the ratios (at most 64
//                        clips, a uniform loop), so nothing about an output depends on where its clip stands in the batch or on which
//                        workgroup computes it.  A workgroup beyond the last tile leaves before it loads anything.
//     table              the 16385 prototype values sit in LDS (64 KB + 4 bytes, hence dynamic LDS above the 64 KiB default), loaded once
//                        per workgroup and kept over its tiles.
//     span               the inputs a tile can touch, x[i(first) - H .. i(last) + H + 1] (at most 8756 samples: 1023 * 8 + 1 + 2 * 285 + 1),
//                        are staged in LDS once, zeros outside the clip: no tap tests a bound.
//     thread             owns kRsPer consecutive outputs: ONE in the product (1024 threads, four waves per SIMD, whose other waves cover a
//                        wave's wait for its gather), four in the form built first (256 threads, one wave per SIMD: 2 .. 2.7 times as slow,
//                        profiles/r20_resample.txt).  (i, r) of the first come from one 64-bit division, further ones by adding
//                        (P / Q, P % Q) with carry.  The output itself is rs_output of resample_steps.h, which the streaming kernels
//                        (resample_stream.hip) share.  The header's per-tap division is not executed: with f = floor(r cq / Q) and
//                        g = ceil(r cq / Q) (one 64-bit division per output), u = |d| cq + f for d = j - i <= 0 and u = d cq - g for
//                        d >= 1, exactly, so u walks down and up again by cq.
//     gather             a tap reads tab[k] and tab[k + 1] (neighbours: one ds_read2_b32) and one span value.  Lanes hold neighbouring outputs,
//                        so their span reads are P / Q dwords apart and their k differ by the phase: the table reads of a wave fall on the 64
//                        banks as the phases do, without a layout that would spread them (a bank-swizzled or phase-major table is the
//                        next form, not built).  Small-Q ratios recompute their few distinct phases per output rather than reuse them.
//     peak               thread -> wave (shuffles) -> workgroup (LDS) maximum of |y|, then ONE vector atomic max per tile on the bits of the
//                        non-negative float.
#include <math.h>
#include <vector>
#include "runtime.h"
#include "resample_steps.h"

namespace tt {

#ifndef TT_RS_THREADS
#define TT_RS_THREADS 1024  // threads of a workgroup and consecutive outputs of a thread: 1024 x 1 (16 waves on the CU hide the gather's LDS latency)
#define TT_RS_PER 1         // against 256 x 4 (one wave per SIMD), measured in profiles/r20_resample.txt; -D both for an A/B build (build.py variants)
#endif
constexpr int kRsThreads = TT_RS_THREADS, kRsPer = TT_RS_PER, kRsTile = kRsThreads * kRsPer;
static_assert(kRsTile == 1024 && kRsThreads % 64 == 0 && kRsThreads >= TT_RS_MAX_CLIPS, "a tile is 1024 outputs");
constexpr int kRsSpan = ((kRsTile - 1) * TT_RS_MAX_RATIO + 1 + 2 * kRsHMax + 1 + 15) / 16 * 16;     // samples of LDS for a tile's inputs
constexpr size_t kRsLds = (size_t)(TT_RS_TABLE + 3 + kRsSpan) * sizeof(float);                      // (the table padded to 16388 floats)
static_assert(kRsLds <= 160 * 1024, "rs_resample_kernel's LDS plan");

// the status of clip c, and for an OK clip its length and output length
__device__ static inline int rs_clip(const int* __restrict__ in_off, const int* __restrict__ Ps, const int* __restrict__ Qs,
                                     const int* __restrict__ out_off, int max_samples, int c, int* n_p, int* n_out_p) {
  const int i0 = in_off[c], n = in_off[c + 1] - i0, o0 = out_off[c];
  *n_p = 0;
  *n_out_p = 0;
  if (i0 < 0 || n < 0) return TT_RS_REFUSED;
  if (n == 0) return TT_RS_EMPTY;
  const int P = Ps[c], Q = Qs[c];
  if (n > max_samples || !rs_ratio_ok(P, Q)) return TT_RS_REFUSED;
  const int n_out = rs_out_samples(n, P, Q);
  if (o0 < 0 || out_off[c + 1] - o0 != n_out) return TT_RS_REFUSED;  // nothing is written outside the clip's own slice
  *n_p = n;
  *n_out_p = n_out;
  return TT_RS_OK;
}

__global__ __launch_bounds__(TT_RS_MAX_CLIPS) void rs_prepare_kernel(int n_clips, const int* __restrict__ in_off, const int* __restrict__ Ps,
                                                                     const int* __restrict__ Qs, const int* __restrict__ out_off,
                                                                     int max_samples, float* __restrict__ peak, int* __restrict__ status) {
  const int c = threadIdx.x;
  if (c >= n_clips) return;
  int n, n_out;
  const int st = rs_clip(in_off, Ps, Qs, out_off, max_samples, c, &n, &n_out);
  status[c] = st;
  if (st == TT_RS_OK && peak) peak[c] = 0.f;
}

__global__ __launch_bounds__(kRsThreads) void rs_resample_kernel(int n_clips, const float* __restrict__ audio, const int* __restrict__ in_off,
                                                                 const int* __restrict__ Ps, const int* __restrict__ Qs,
                                                                 const float* __restrict__ table, int max_samples, float* __restrict__ out,
                                                                 const int* __restrict__ out_off, float* __restrict__ peak) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  float* tab_s = rs_lds;                     // [TT_RS_TABLE]
  float* span_s = rs_lds + TT_RS_TABLE + 3;  // [kRsSpan]
  __shared__ int len_s[TT_RS_MAX_CLIPS], nout_s[TT_RS_MAX_CLIPS];
  __shared__ float peak_s[kRsThreads / 64];
  const int t = threadIdx.x;
  if (t < TT_RS_MAX_CLIPS) {
    int n = 0, n_out = 0;
    if (t < n_clips) rs_clip(in_off, Ps, Qs, out_off, max_samples, t, &n, &n_out);
    len_s[t] = n;
    nout_s[t] = n_out;  // 0: not resampled
  }
  __syncthreads();
  int total = 0;
  for (int c = 0; c < n_clips; ++c) total += (nout_s[c] + kRsTile - 1) / kRsTile;
  if ((int)blockIdx.x >= total) return;  // (uniform over the workgroup)
  for (int e = t; e < TT_RS_TABLE; e += kRsThreads) tab_s[e] = table[e];
  for (int g = blockIdx.x; g < total; g += gridDim.x) {
    int c = 0, first = 0;  // tile g is tile (g - first) of clip c
    for (;; ++c) {
      const int tiles = (nout_s[c] + kRsTile - 1) / kRsTile;
      if (g < first + tiles) break;
      first += tiles;
    }
    const int n = len_s[c], n_out = nout_s[c], P = Ps[c], Q = Qs[c];
    const float* x = audio + in_off[c];
    float* y = out + out_off[c];
    const unsigned cq = rs_cq(P, Q);
    const int H = rs_half_width(cq);
    const float c32 = rs_c32(P, Q);
    const int m0 = (g - first) * kRsTile, m1 = min(m0 + kRsTile, n_out);  // this tile's outputs
    const int j0 = (int)((long long)m0 * P / Q) - H;                      // the first input it touches
    const int span = (int)((long long)(m1 - 1) * P / Q) + H + 1 - j0 + 1;
    __syncthreads();  // the previous tile's reads of span_s are done
    for (int e = t; e < span; e += kRsThreads) {
      const int j = j0 + e;
      span_s[e] = j >= 0 && j < n ? x[j] : 0.f;
    }
    __syncthreads();  // (also: the table is in place)
    float pk = 0.f;
    int m = m0 + t * kRsPer;
    if (m < m1) {
      const long long num = (long long)m * P;
      int i = (int)(num / Q), r = (int)(num % Q);
      const int di = P / Q, dr = P % Q;
#pragma unroll 1
      for (int e = 0; e < kRsPer && m < m1; ++e, ++m) {
        const float acc = rs_output(tab_s, span_s + (i - H - j0), H, cq, Q, r, c32);  // x[i - H ..]: the steps of resample_steps.h
        y[m] = acc;
        pk = fmaxf(pk, fabsf(acc));
        i += di;
        r += dr;
        if (r >= Q) {
          r -= Q;
          ++i;
        }
      }
    }
    if (peak) {
      for (int s = 32; s >= 1; s >>= 1) pk = fmaxf(pk, __shfl_xor(pk, s));
      if ((t & 63) == 0) peak_s[t >> 6] = pk;
      __syncthreads();
      if (t == 0) {
#pragma unroll
        for (int w = 1; w < kRsThreads / 64; ++w) pk = fmaxf(pk, peak_s[w]);
        atomicMax((unsigned*)peak + c, __float_as_uint(pk));  // (non-negative floats order as their bits)
      }
    }
  }
}

}  // namespace tt

using namespace tt;

struct tt_rs : EngineHandle {
  int max_samples = 0, max_clips = 0, grid = 0;
  float* table = nullptr;  // [TT_RS_TABLE] the prototype, fp64 values rounded to f32
};

extern "C" {

int tt_rs_abi_version(void) { return 1; }  // ABI changes

int tt_rs_out_samples(int n, int P, int Q) { return n >= 1 && n <= TT_RS_MAX_SAMPLES && rs_ratio_ok(P, Q) ? rs_out_samples(n, P, Q) : 0; }

int tt_rs_create(int max_samples, int max_clips, tt_rs** out) {
  TT_REQUIRE(out, "tt_rs_create: null argument");
  TT_REQUIRE(max_samples >= 1 && max_samples <= TT_RS_MAX_SAMPLES, "tt_rs_create: max_samples %d (1 .. %d)", max_samples, TT_RS_MAX_SAMPLES);
  TT_REQUIRE(max_clips >= 1 && max_clips <= TT_RS_MAX_CLIPS, "tt_rs_create: max_clips %d (1 .. %d)", max_clips, TT_RS_MAX_CLIPS);
  tt_rs* e = new tt_rs();
  e->max_samples = max_samples; e->max_clips = max_clips;
  int rc = e->open("tt_rs_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->table, TT_RS_TABLE, false);
  if (!rc) {
    std::vector<float> tab(TT_RS_TABLE);
    rs_fill_table(tab.data());
    int dev = 0, cus = 0;
    if (hipMemcpy(e->table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
        hipFuncSetAttribute((const void*)rs_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLds) != hipSuccess) {
      set_error("tt_rs_create: the table upload or the kernel's LDS setting failed");
      rc = -2;
    }
    e->grid = cus;
  }
  if (rc) {
    tt_rs_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_rs_destroy(tt_rs* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_rs_resample(tt_rs* e, int n_clips, const float* audio, const int* in_off, const int* P, const int* Q, float* out, const int* out_off,
                   float* peak, int* status, void* stream) {
  TT_REQUIRE(e && audio && in_off && P && Q && out && out_off && status, "tt_rs_resample: null argument");
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->max_clips, "tt_rs_resample: %d clips (1 .. %d)", n_clips, e->max_clips);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    rs_prepare_kernel<<<1, TT_RS_MAX_CLIPS, 0, s>>>(n_clips, in_off, P, Q, out_off, e->max_samples, peak, status);
    TT_CHECK_HIP(hipGetLastError());
    rs_resample_kernel<<<e->grid, kRsThreads, kRsLds, s>>>(n_clips, audio, in_off, P, Q, e->table, e->max_samples, out, out_off, peak);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
