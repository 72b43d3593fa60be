// Formant-preserving pitch: cepstral envelope correction (include/tortoise_mi355x_fmt.h).  Five launches, every sum on
// v_mfma_f32_32x32x2_f32 (exact f32 products: the log of a quiet bin magnifies any operand rounding), built from csrc/stft_steps.h.  The
// STFT, inverse and overlap-add kernels are the bodies of csrc/stft_kernels.h, shared with csrc/denoise.hip, with this chain's epilogue
// (the log) and gain (exp) put in:
//
//   fmt_stft_kernel      re, im of 32 frames x 64 bins per workgroup (melfront's STFT: virtual frame operand staged once in LDS), written
//                        interleaved, with the log epilogue L = 0.5 log(re^2 + im^2 + 1e-10) beside them
//   fmt_cepstrum_kernel  c[t][q] = L[t] . A[:, q]         one wave per 32 frames x 32 coefficients, K = bins_pad
//   fmt_gain_kernel      g[t][b] = clamp(c[t] . D[:, b])   one wave per 32 frames x 32 bins, K = 64, D chosen by the clip's warp index
//   fmt_inverse_kernel   y[t][k] = Z[t] . inverse[:, k], Z = (re, im) exp(g) formed in the A operand's registers; four waves per workgroup,
//                        each 32 frames x 32 samples, K = 2 bins_pad
//   fmt_ola_kernel       out[j] = sum_t y[t][j + n_fft / 2 - t hop] / sum_t window^2, increasing t, one thread per sample, no atomics
//
// Ragged batches: blockIdx.y is the clip.  A tile never holds frames of two clips and a frame's summation order over k depends on nothing
// but k, so every clip's output is bit-identical to running it alone.  Intermediates live in the handle (one slot per clip of a call).
#include <limits.h>
#include "runtime.h"
#include "stft_kernels.h"
#include "../../include/tortoise_mi355x_fmt.h"
#include "../../include/tortoise_mi355x_test.h"

namespace tt {

constexpr int kFmtBinsPerBlock = 64;     // two waves of 32 bins (fmt_stft_kernel)
constexpr int kFmtInvWaves = 4;          // 32-sample column tiles of one fmt_inverse_kernel workgroup
constexpr int kFmtMaxSamples = 1 << 24;  // keeps every 32-bit sample / frame index far from overflow
constexpr size_t kFmtMaxLds = 64 * 1024;
constexpr float kFmtDelta = 1e-10f;

struct FmtClips {  // by value in the kernel arguments: nothing to copy to the device, nothing to keep alive
  long long in_off[TT_FMT_MAX_CLIPS];
  long long out_off[TT_FMT_MAX_CLIPS];
  long long st_off[TT_FMT_MAX_CLIPS];  // of the clip's log magnitudes / gains [T][bins_pad]; its spectrum [T][2 bins_pad] starts at twice that
  int len[TT_FMT_MAX_CLIPS];
  int warp[TT_FMT_MAX_CLIPS];
};

struct FmtLogEpilogue {  // the spectrum interleaved, the log magnitude beside it
  float* sp;
  float* lm;
  int bins_pad;
  __device__ __forceinline__ void operator()(const f32x16& re, const f32x16& im, int t0, int T, int col, int h) const {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = t0 + mfma_row(r, h);
      if (t < T) {
        const size_t e = (size_t)t * bins_pad + col;
        *(float2*)(sp + 2 * e) = make_float2(re[r], im[r]);
        lm[e] = 0.5f * logf(re[r] * re[r] + im[r] * im[r] + kFmtDelta);
      }
    }
  }
};

__global__ __launch_bounds__(128) void fmt_stft_kernel(const float* __restrict__ wav, FmtClips clips, const float* __restrict__ basis, int n_fft,
                                                       int hop, int bins_pad, float* __restrict__ spec, float* __restrict__ logmag) {
  extern __shared__ float xs[];
  const int c = blockIdx.y, n = clips.len[c], T = 1 + n / hop;
  stft_tile_body(wav + clips.in_off[c], n, T, basis, n_fft, hop, bins_pad, kFmtBinsPerBlock, 128, xs,
                 FmtLogEpilogue{spec + 2 * clips.st_off[c], logmag + clips.st_off[c], bins_pad});
}

// cep: [slot][t][64], slot stride cep_clip elements
__global__ __launch_bounds__(64) void fmt_cepstrum_kernel(const float* __restrict__ logmag, FmtClips clips, const float* __restrict__ A, int hop,
                                                          int bins_pad, float* __restrict__ cep, size_t cep_clip) {
  const int c = blockIdx.y, T = 1 + clips.len[c] / hop;
  const int t0 = blockIdx.x * kStftTile, q0 = blockIdx.z * 32;
  if (t0 >= T) return;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const float* l = logmag + clips.st_off[c] + (size_t)min(t0 + i, T - 1) * bins_pad + 4 * h;
  const float* a = A + (size_t)(4 * h) * TT_FMT_Q_PAD + q0 + i;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < bins_pad; k += 8) rows_mfma8(*(const float4*)(l + k), a + (size_t)k * TT_FMT_Q_PAD, TT_FMT_Q_PAD, acc);
  float* o = cep + (size_t)c * cep_clip;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + mfma_row(r, h);
    if (t < T) o[(size_t)t * TT_FMT_Q_PAD + q0 + i] = acc[r];
  }
}

__global__ __launch_bounds__(64) void fmt_gain_kernel(const float* __restrict__ cep, size_t cep_clip, FmtClips clips, const float* __restrict__ warps,
                                                      int hop, int bins_pad, float limit, float* __restrict__ gains) {
  const int c = blockIdx.y, T = 1 + clips.len[c] / hop;
  const int t0 = blockIdx.x * kStftTile, b0 = blockIdx.z * 32;
  if (t0 >= T) return;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const float* cr = cep + (size_t)c * cep_clip + (size_t)min(t0 + i, T - 1) * TT_FMT_Q_PAD + 4 * h;
  const float* d = warps + ((size_t)clips.warp[c] * TT_FMT_Q_PAD + 4 * h) * bins_pad + b0 + i;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int k = 0; k < TT_FMT_Q_PAD; k += 8) rows_mfma8(*(const float4*)(cr + k), d + (size_t)k * bins_pad, bins_pad, acc);
  float* o = gains + clips.st_off[c];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + mfma_row(r, h);
    if (t < T) {
      float g = acc[r];
      if (limit > 0.f) g = fminf(fmaxf(g, -limit), limit);
      o[(size_t)t * bins_pad + b0 + i] = g;
    }
  }
}

struct FmtExpGain {  // log gains -> multipliers
  __device__ __forceinline__ float2 operator()(const float2 g) const { return make_float2(expf(g.x), expf(g.y)); }
};

// y: [slot][t][n_fft], slot stride y_clip elements
__global__ __launch_bounds__(64 * kFmtInvWaves) void fmt_inverse_kernel(const float* __restrict__ spec, const float* __restrict__ gains, FmtClips clips,
                                                                        const float* __restrict__ inverse, int n_fft, int hop, int bins_pad,
                                                                        float* __restrict__ y, size_t y_clip) {
  const int c = blockIdx.y, T = 1 + clips.len[c] / hop;
  stft_inverse_body(spec + 2 * clips.st_off[c], gains + clips.st_off[c], T, inverse, n_fft, bins_pad, kFmtInvWaves, y + (size_t)c * y_clip,
                    FmtExpGain{});
}

__global__ __launch_bounds__(256) void fmt_ola_kernel(const float* __restrict__ y, size_t y_clip, FmtClips clips, const float* __restrict__ basis,
                                                      int n_fft, int hop, int bins_pad, float* __restrict__ out) {
  const int c = blockIdx.y, n = clips.len[c], T = 1 + n / hop;
  stft_ola_body(y + (size_t)c * y_clip, n, T, basis, n_fft, hop, bins_pad, 256, out + clips.out_off[c]);
}

}  // namespace tt

using namespace tt;

struct tt_fmt : EngineHandle {
  tt_fmt_config cfg;
  tt_fmt_tables tab;
  float *spec = nullptr, *logmag = nullptr, *cep = nullptr, *gains = nullptr, *y = nullptr;  // one slot per clip of a call
  size_t frames_max = 0;  // frames of a clip of max_samples
  size_t stft_lds = 0;
  float limit = 0.f;      // ln(10) G / 20
};

static int fmt_check_clips(const tt_fmt* e, const char* who, const int* clip_lengths, int n_clips, const float* out, const long long* out_offsets,
                           FmtClips* in) {
  TT_REQUIRE(e && clip_lengths && out && out_offsets, "%s: null argument", who);
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->cfg.max_clips, "%s: %d clips (1 .. %d)", who, n_clips, e->cfg.max_clips);
  memset(in, 0, sizeof(*in));
  for (int c = 0; c < n_clips; ++c) {
    TT_REQUIRE(clip_lengths[c] >= e->cfg.n_fft / 2 + 1, "%s: clip %d has %d samples; reflect padding needs at least n_fft / 2 + 1 = %d", who, c,
               clip_lengths[c], e->cfg.n_fft / 2 + 1);
    TT_REQUIRE(clip_lengths[c] <= e->cfg.max_samples, "%s: clip %d has %d samples, the handle takes %d", who, c, clip_lengths[c], e->cfg.max_samples);
    TT_REQUIRE(out_offsets[c] >= 0, "%s: negative offset of clip %d", who, c);
    in->out_off[c] = out_offsets[c];
    in->len[c] = clip_lengths[c];
    in->st_off[c] = (long long)((size_t)c * e->frames_max * e->cfg.bins_pad);
  }
  return 0;
}

static int fmt_check_run(const tt_fmt* e, const char* who, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* warp_index,
                         int n_clips, const float* out, const long long* out_offsets, FmtClips* in) {
  TT_REQUIRE(wav && clip_offsets && warp_index, "%s: null argument", who);
  TT_TRY(fmt_check_clips(e, who, clip_lengths, n_clips, out, out_offsets, in));
  for (int c = 0; c < n_clips; ++c) {
    TT_REQUIRE(clip_offsets[c] >= 0, "%s: negative offset of clip %d", who, c);
    TT_REQUIRE(warp_index[c] >= 0 && warp_index[c] < e->cfg.n_warps, "%s: clip %d asks for warp %d, the handle has %d", who, c, warp_index[c],
               e->cfg.n_warps);
    in->in_off[c] = clip_offsets[c];
    in->warp[c] = warp_index[c];
  }
  return 0;
}

static int fmt_tiles(const tt_fmt* e, const FmtClips& in, int n_clips) {
  int tmax = 0;
  for (int k = 0; k < n_clips; ++k) tmax = std::max(tmax, 1 + in.len[k] / e->cfg.hop);
  return cdiv(tmax, kStftTile);
}

// steps 1 to 4 into the handle's slots
static int fmt_analyse(tt_fmt* e, const float* wav, const FmtClips& in, int n_clips, hipStream_t s) {
  const tt_fmt_config& c = e->cfg;
  const int tiles = fmt_tiles(e, in, n_clips);
  const size_t cep_clip = e->frames_max * TT_FMT_Q_PAD;
  fmt_stft_kernel<<<dim3(tiles, n_clips, cdiv(c.bins_pad, kFmtBinsPerBlock)), 128, e->stft_lds, s>>>(wav, in, e->tab.basis, c.n_fft, c.hop, c.bins_pad,
                                                                                                   e->spec, e->logmag);
  TT_CHECK_HIP(hipGetLastError());
  fmt_cepstrum_kernel<<<dim3(tiles, n_clips, TT_FMT_Q_PAD / 32), 64, 0, s>>>(e->logmag, in, e->tab.cepstrum, c.hop, c.bins_pad, e->cep, cep_clip);
  TT_CHECK_HIP(hipGetLastError());
  fmt_gain_kernel<<<dim3(tiles, n_clips, c.bins_pad / 32), 64, 0, s>>>(e->cep, cep_clip, in, e->tab.warps, c.hop, c.bins_pad, e->limit, e->gains);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

// steps 5 to 7 from spectrum / gains at in.st_off
static int fmt_synthesise(tt_fmt* e, const float* spec, const float* gains, const FmtClips& in, int n_clips, float* out, hipStream_t s) {
  const tt_fmt_config& c = e->cfg;
  const int tiles = fmt_tiles(e, in, n_clips);
  const size_t y_clip = e->frames_max * c.n_fft;
  int nmax = 0;
  for (int k = 0; k < n_clips; ++k) nmax = std::max(nmax, in.len[k]);
  fmt_inverse_kernel<<<dim3(tiles, n_clips, cdiv(c.n_fft / 32, kFmtInvWaves)), 64 * kFmtInvWaves, 0, s>>>(spec, gains, in, e->tab.inverse, c.n_fft, c.hop,
                                                                                                         c.bins_pad, e->y, y_clip);
  TT_CHECK_HIP(hipGetLastError());
  fmt_ola_kernel<<<dim3(cdiv(nmax, 256), n_clips), 256, 0, s>>>(e->y, y_clip, in, e->tab.basis, c.n_fft, c.hop, c.bins_pad, out);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int tt_fmt_abi_version(void) { return 1; }  // ABI changes

size_t tt_fmt_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_fmt_config);
    case 1: return sizeof(tt_fmt_tables);
    default: return 0;
  }
}

int tt_fmt_create(const tt_fmt_config* cfg, const tt_fmt_tables* tables, tt_fmt** out) {
  TT_REQUIRE(cfg && tables && out, "tt_fmt_create: null argument");
  const tt_fmt_config& c = *cfg;
  TT_REQUIRE(c.hop >= 8 && c.hop % 8 == 0 && c.n_fft >= 64 && c.n_fft % 64 == 0 && c.n_fft % c.hop == 0,
             "tt_fmt_create: n_fft %d / hop %d (n_fft a multiple of 64 and of hop, hop a multiple of 8)", c.n_fft, c.hop);
  TT_REQUIRE(c.bins_pad >= c.n_fft / 2 + 1 && c.bins_pad % 32 == 0, "tt_fmt_create: bins_pad %d (a multiple of 32, at least n_fft / 2 + 1 = %d)",
             c.bins_pad, c.n_fft / 2 + 1);
  TT_REQUIRE(c.q >= 1 && c.q <= TT_FMT_Q_PAD, "tt_fmt_create: q %d (1 .. %d)", c.q, TT_FMT_Q_PAD);
  TT_REQUIRE(c.max_gain_db >= 0.f && c.max_gain_db <= 200.f, "tt_fmt_create: max_gain_db %g (0: no clamp, up to 200)", (double)c.max_gain_db);
  TT_REQUIRE(c.max_samples >= c.n_fft / 2 + 1 && c.max_samples <= kFmtMaxSamples, "tt_fmt_create: max_samples %d (%d .. %d)", c.max_samples,
             c.n_fft / 2 + 1, kFmtMaxSamples);
  TT_REQUIRE(c.max_clips >= 1 && c.max_clips <= TT_FMT_MAX_CLIPS, "tt_fmt_create: max_clips %d (1 .. %d)", c.max_clips, TT_FMT_MAX_CLIPS);
  TT_REQUIRE(c.n_warps >= 1 && c.n_warps <= TT_FMT_MAX_WARPS, "tt_fmt_create: n_warps %d (1 .. %d)", c.n_warps, TT_FMT_MAX_WARPS);
  TT_REQUIRE(tables->basis && tables->inverse && tables->cepstrum && tables->warps, "tt_fmt_create: null table");
  const size_t lds = stft_lds_bytes(c.n_fft, c.hop);
  TT_REQUIRE(lds <= kFmtMaxLds, "tt_fmt_create: 32 frames of n_fft %d at hop %d need %zu bytes of LDS (at most %zu)", c.n_fft, c.hop, lds, kFmtMaxLds);
  tt_fmt* e = new tt_fmt();
  e->cfg = c;
  e->tab = *tables;
  e->stft_lds = lds;
  e->limit = (float)(log(10.0) * (double)c.max_gain_db / 20.0);
  e->frames_max = (size_t)(1 + c.max_samples / c.hop);
  const size_t fr = e->frames_max * c.max_clips;
  int rc = e->open("tt_fmt_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->spec, fr * 2 * c.bins_pad, false);
  if (!rc) rc = e->arena.alloc_t(&e->logmag, fr * c.bins_pad, false);
  if (!rc) rc = e->arena.alloc_t(&e->cep, fr * TT_FMT_Q_PAD, false);
  if (!rc) rc = e->arena.alloc_t(&e->gains, fr * c.bins_pad, false);
  if (!rc) rc = e->arena.alloc_t(&e->y, fr * c.n_fft, false);
  if (rc) {
    tt_fmt_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_fmt_destroy(tt_fmt* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_fmt_frames(const tt_fmt* e, int n) {
  if (!e || n < 0) return -1;
  return 1 + n / e->cfg.hop;
}

int tt_fmt_run(tt_fmt* e, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* warp_index, int n_clips, float* out,
               const long long* out_offsets, void* stream) {
  FmtClips in;
  TT_TRY(fmt_check_run(e, "tt_fmt_run", wav, clip_offsets, clip_lengths, warp_index, n_clips, out, out_offsets, &in));
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(fmt_analyse(e, wav, in, n_clips, s));
    return fmt_synthesise(e, e->spec, e->gains, in, n_clips, out, s);
  });
}

int tt_op_fmt_run(void* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* warp_index, int n_clips, float* out,
                  const long long* out_offsets, float* spectrum, float* logmag, float* gains, const long long* stage_offsets, void* stream) {
  tt_fmt* e = (tt_fmt*)h;
  FmtClips in;
  TT_TRY(fmt_check_run(e, "tt_op_fmt_run", wav, clip_offsets, clip_lengths, warp_index, n_clips, out, out_offsets, &in));
  const bool staged = spectrum || logmag || gains;
  TT_REQUIRE(!staged || stage_offsets, "tt_op_fmt_run: staged outputs without stage_offsets");
  for (int c = 0; staged && c < n_clips; ++c) TT_REQUIRE(stage_offsets[c] >= 0, "tt_op_fmt_run: negative stage offset of clip %d", c);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(fmt_analyse(e, wav, in, n_clips, s));
    TT_TRY(fmt_synthesise(e, e->spec, e->gains, in, n_clips, out, s));
    for (int c = 0; staged && c < n_clips; ++c) {
      const size_t el = (size_t)(1 + in.len[c] / e->cfg.hop) * e->cfg.bins_pad, so = (size_t)stage_offsets[c], ho = (size_t)in.st_off[c];
      if (spectrum) TT_CHECK_HIP(hipMemcpyAsync(spectrum + 2 * so, e->spec + 2 * ho, 2 * el * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (logmag) TT_CHECK_HIP(hipMemcpyAsync(logmag + so, e->logmag + ho, el * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (gains) TT_CHECK_HIP(hipMemcpyAsync(gains + so, e->gains + ho, el * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return 0;
  });
}

int tt_op_fmt_synth(void* h, const float* spectrum, const float* gains, const long long* stage_offsets, const int* clip_lengths, int n_clips, float* out,
                    const long long* out_offsets, void* stream) {
  tt_fmt* e = (tt_fmt*)h;
  FmtClips in;
  TT_REQUIRE(spectrum && gains && stage_offsets, "tt_op_fmt_synth: null argument");
  TT_TRY(fmt_check_clips(e, "tt_op_fmt_synth", clip_lengths, n_clips, out, out_offsets, &in));
  for (int c = 0; c < n_clips; ++c) {
    TT_REQUIRE(stage_offsets[c] >= 0 && stage_offsets[c] % 4 == 0, "tt_op_fmt_synth: stage offset of clip %d must be a non-negative multiple of 4", c);
    in.st_off[c] = stage_offsets[c];
  }
  TT_REQUIRE(((uintptr_t)spectrum | (uintptr_t)gains) % 16 == 0, "tt_op_fmt_synth: spectrum and gains must be 16-byte aligned");
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int { return fmt_synthesise(e, spectrum, gains, in, n_clips, out, s); });
}

}  // extern "C"
