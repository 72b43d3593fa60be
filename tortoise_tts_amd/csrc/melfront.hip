// Mel front-end of the voice_samples path (include/tortoise_mi355x_mel.h): resampler, STFT and mel projection as three f32 GEMMs on
// v_mfma_f32_32x32x2_f32 (exact f32 products: the log of a quiet mel bin magnifies any operand rounding, so no 16-bit operands here).
//
//   mel_stft_kernel      spec[t][b] = |frames[t] . basis[:, b]|^power.  The A operand is virtual: frame t, column k is
//                        x[reflect(t * hop + k - n_fft / 2)].  A workgroup stages the one contiguous stretch of the clip its 32 frames
//                        cover (31 * hop + n_fft samples, reflected and clamped once) in LDS; each of its two waves owns 32 bins, re and im
//                        of a bin in the same lane and register, so the epilogue has both in reach.
//   mel_project_kernel   mel[m][t] = log(max(fb[m] . spec[t], floor)) * scale[m], one wave per 32 mels x 32 frames, written channels-first.
//   mel_resample_kernel  out[n * new + p] = taps[p] . xpad[n * orig ..], again with a virtual A operand (zero outside the clip).
//
// Ragged batches: blockIdx.y is the clip.  A tile never holds frames of two clips and a frame's summation order over k depends on
// nothing but k, so every clip's output is bit-identical to running it alone.
#include <limits.h>
#include "runtime.h"
#include "../../include/tortoise_mi355x_mel.h"

namespace tt {

constexpr int kMelTile = 32;             // frames per workgroup (STFT) / per wave (projection): one MFMA block
constexpr int kStftBinsPerBlock = 64;    // two waves of 32 bins
constexpr int kMelMaxSamples = 1 << 26;  // keeps every 32-bit sample / frame index far from overflow
constexpr size_t kStftMaxLds = 64 * 1024;

struct MelClips {  // by value in the kernel arguments: nothing to copy to the device, nothing to keep alive
  long long in_off[TT_MEL_MAX_CLIPS];
  long long out_off[TT_MEL_MAX_CLIPS];
  int len[TT_MEL_MAX_CLIPS];
};

// LDS position of staged sample p: one pad word per hop samples, so that the 32 lanes of an A read (stride hop) hit 32 banks
__device__ __forceinline__ int stft_lds_pos(int p, int hop) { return p + p / hop; }

__global__ __launch_bounds__(128) void mel_stft_kernel(const float* __restrict__ wav, MelClips clips, const float* __restrict__ basis, int n_fft,
                                                       int hop, int bins_pad, int power, int clamp, float* __restrict__ spec) {
  extern __shared__ float xs[];
  const int c = blockIdx.y, n = clips.len[c], T = 1 + n / hop;
  const int t0 = blockIdx.x * kMelTile;
  if (t0 >= T) return;
  const float* x = wav + clips.in_off[c];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int span = (kMelTile - 1) * hop + n_fft;
  const int q0 = t0 * hop - n_fft / 2;
  for (int p = tid; p < span; p += 128) {
    int q = q0 + p;
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    float v = 0.f;  // (beyond the reflection: only frames >= T read it, and those are not written)
    if (q >= 0 && q < n) {
      v = x[q];
      if (clamp) v = fminf(fmaxf(v, -1.f), 1.f);
    }
    xs[stft_lds_pos(p, hop)] = v;
  }
  __syncthreads();
  const int b0 = blockIdx.z * kStftBinsPerBlock + wave * 32;
  if (b0 >= bins_pad) return;
  const int i = lane & 31, h = lane >> 5;
  f32x16 re, im;
#pragma unroll
  for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
  // A[row = frame i][k]: lane (i, h) holds k = k0 + h.  B[k][col = bin i]: the cos / -sin pair of bin b0 + i in row k0 + h of the table.
  const float* bp = basis + 2 * (size_t)(b0 + i);
  const size_t ldb = 2 * (size_t)bins_pad;
  const int arow = i * (hop + 1);
  for (int kc = 0; kc < n_fft; kc += hop) {  // (hop divides n_fft and is a multiple of 8: a group of four k pairs lies in one chunk, whose pad offset is kc / hop)
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
  // D lane l reg r = D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]
  float* o = spec + clips.out_off[c];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (t < T) {
      const float p2 = re[r] * re[r] + im[r] * im[r];
      o[(size_t)t * bins_pad + b0 + i] = power == 2 ? p2 : sqrtf(p2);
    }
  }
}

// One wave: mels m0 .. m0 + 31 (rows) x frames t0 .. t0 + 31 (columns).  Each lane reads four consecutive k of its fb row and of its
// spectrum row at once; MFMA j of a group of eight k multiplies the pairs (k + j, k + 4 + j): a fixed order, whatever the batch.
__global__ __launch_bounds__(64) void mel_project_kernel(const float* __restrict__ spec, MelClips clips, MelClips outs, const float* __restrict__ fb,
                                                         const float* __restrict__ scale, int hop, int n_mels, int bins_pad, float floor_,
                                                         float* __restrict__ out) {
  const int c = blockIdx.y, T = 1 + clips.len[c] / hop;
  const int t0 = blockIdx.x * kMelTile, m0 = blockIdx.z * 32;
  if (t0 >= T) return;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const float* s = spec + clips.out_off[c] + (size_t)min(t0 + i, T - 1) * bins_pad + 4 * h;
  const float* f = fb + (size_t)min(m0 + i, n_mels - 1) * bins_pad + 4 * h;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < bins_pad; k += 16) {  // (bins_pad is a multiple of 32) two groups of eight k per trip, loads ahead of the MFMAs
    const float4 a0 = *(const float4*)(f + k), a1 = *(const float4*)(f + k + 8);
    const float4 b0 = *(const float4*)(s + k), b1 = *(const float4*)(s + k + 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc, 0, 0, 0);
  }
  const int t = t0 + i;
  if (t >= T) return;
  float* o = out + outs.out_off[c];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (m < n_mels) {
      float v = logf(fmaxf(acc[r], floor_));
      if (scale) v *= scale[m];
      o[(size_t)m * T + t] = v;
    }
  }
}

// One wave: input frames n0 .. n0 + 31 (rows) x output phases p0 .. p0 + 31 (columns), k over the 2 * width + orig taps.
__global__ __launch_bounds__(64) void mel_resample_kernel(const float* __restrict__ x, int n, const float* __restrict__ taps, int orig, int new_rate,
                                                          int width, int n_out, float* __restrict__ out) {
  const int L = 2 * width + orig;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
  const long long base = (long long)(n0 + i) * orig - width;  // x index of tap 0 of this lane's frame
  const int p = min(p0 + i, new_rate - 1);
  const float* w = taps + (size_t)p * L;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < L; k0 += 2) {
    const int k = k0 + h;
    const long long q = base + k;
    const bool ok = k < L;
    const float a = ok && q >= 0 && q < n ? x[q] : 0.f;
    const float b = ok ? w[k] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (p0 + i >= new_rate) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long idx = (long long)(n0 + (r & 3) + 8 * (r >> 2) + 4 * h) * new_rate + p0 + i;
    if (idx < n_out) out[idx] = acc[r];
  }
}

}  // namespace tt

using namespace tt;

struct tt_mel : EngineHandle {
  tt_mel_config cfg;
  tt_mel_tables tab;
  float* spec = nullptr;     // [max_clips][frames(max_samples)][bins_pad]
  size_t spec_clip = 0;      // elements of one clip's slot
  size_t stft_lds = 0;
};

struct tt_mel_resampler : EngineHandle {
  const float* taps = nullptr;
  int orig = 0, new_rate = 0, width = 0, max_samples = 0;
};

static int mel_check_clips(const tt_mel* e, const char* who, const float* wav, const long long* clip_offsets, const int* clip_lengths, int n_clips,
                           float* out, const long long* out_offsets, MelClips* in) {
  TT_REQUIRE(e && wav && clip_offsets && clip_lengths && out && out_offsets, "%s: null argument", who);
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->cfg.max_clips, "%s: %d clips (1 .. %d)", who, n_clips, e->cfg.max_clips);
  memset(in, 0, sizeof(*in));
  for (int c = 0; c < n_clips; ++c) {
    TT_REQUIRE(clip_lengths[c] >= e->cfg.n_fft / 2 + 1, "%s: clip %d has %d samples; reflect padding needs at least n_fft / 2 + 1 = %d", who, c,
               clip_lengths[c], e->cfg.n_fft / 2 + 1);
    TT_REQUIRE(clip_lengths[c] <= e->cfg.max_samples, "%s: clip %d has %d samples, the handle takes %d", who, c, clip_lengths[c], e->cfg.max_samples);
    TT_REQUIRE(clip_offsets[c] >= 0 && out_offsets[c] >= 0, "%s: negative offset of clip %d", who, c);
    in->in_off[c] = clip_offsets[c];
    in->out_off[c] = out_offsets[c];
    in->len[c] = clip_lengths[c];
  }
  return 0;
}

// spec_out: the caller's spectrum buffer with the caller's offsets (tt_mel_spectrum), or NULL: the handle's own slots
static int mel_stft_launch(tt_mel* e, const float* wav, MelClips in, int n_clips, float* spec_out, hipStream_t s) {
  const tt_mel_config& c = e->cfg;
  int tmax = 0;
  for (int k = 0; k < n_clips; ++k) tmax = std::max(tmax, 1 + in.len[k] / c.hop);
  if (!spec_out) {
    for (int k = 0; k < n_clips; ++k) in.out_off[k] = (long long)(k * e->spec_clip);
    spec_out = e->spec;
  }
  dim3 grid(cdiv(tmax, kMelTile), n_clips, cdiv(c.bins_pad, kStftBinsPerBlock));
  mel_stft_kernel<<<grid, 128, e->stft_lds, s>>>(wav, in, e->tab.basis, c.n_fft, c.hop, c.bins_pad, c.power, c.clamp_input, spec_out);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

static int mel_project_launch(tt_mel* e, const MelClips& in, int n_clips, float* out, hipStream_t s) {
  const tt_mel_config& c = e->cfg;
  MelClips sp = in;
  int tmax = 0;
  for (int k = 0; k < n_clips; ++k) {
    tmax = std::max(tmax, 1 + in.len[k] / c.hop);
    sp.out_off[k] = (long long)(k * e->spec_clip);
  }
  dim3 grid(cdiv(tmax, kMelTile), n_clips, cdiv(c.n_mels, 32));
  mel_project_kernel<<<grid, 64, 0, s>>>(e->spec, sp, in, e->tab.fb, e->tab.scale, c.hop, c.n_mels, c.bins_pad, c.floor, out);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int tt_mel_abi_version(void) { return 1; }  // ABI changes

size_t tt_mel_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_mel_config);
    case 1: return sizeof(tt_mel_tables);
    default: return 0;
  }
}

int tt_mel_create(const tt_mel_config* cfg, const tt_mel_tables* tables, tt_mel** out) {
  TT_REQUIRE(cfg && tables && out, "tt_mel_create: null argument");
  const tt_mel_config& c = *cfg;
  TT_REQUIRE(c.hop >= 8 && c.hop % 8 == 0 && c.n_fft >= 64 && c.n_fft % 64 == 0 && c.n_fft % c.hop == 0,
             "tt_mel_create: n_fft %d / hop %d (n_fft a multiple of 64 and of hop, hop a multiple of 8)", c.n_fft, c.hop);
  TT_REQUIRE(c.n_mels >= 1 && c.n_mels <= 128, "tt_mel_create: n_mels %d (1 .. 128)", c.n_mels);
  TT_REQUIRE(c.bins_pad >= c.n_fft / 2 + 1 && c.bins_pad % 32 == 0, "tt_mel_create: bins_pad %d (a multiple of 32, at least n_fft / 2 + 1 = %d)",
             c.bins_pad, c.n_fft / 2 + 1);
  TT_REQUIRE(c.power == 1 || c.power == 2, "tt_mel_create: power %d (1: magnitude, 2: power)", c.power);
  TT_REQUIRE(c.floor > 0.f, "tt_mel_create: floor must be positive");
  TT_REQUIRE(c.max_samples >= c.n_fft / 2 + 1 && c.max_samples <= kMelMaxSamples, "tt_mel_create: max_samples %d (%d .. %d)", c.max_samples,
             c.n_fft / 2 + 1, kMelMaxSamples);
  TT_REQUIRE(c.max_clips >= 1 && c.max_clips <= TT_MEL_MAX_CLIPS, "tt_mel_create: max_clips %d (1 .. %d)", c.max_clips, TT_MEL_MAX_CLIPS);
  TT_REQUIRE(tables->basis && tables->fb, "tt_mel_create: null table");
  const int span = (kMelTile - 1) * c.hop + c.n_fft;
  const size_t lds = sizeof(float) * ((size_t)span + span / c.hop + 1);
  TT_REQUIRE(lds <= kStftMaxLds, "tt_mel_create: 32 frames of n_fft %d at hop %d need %zu bytes of LDS (at most %zu)", c.n_fft, c.hop, lds, kStftMaxLds);
  tt_mel* e = new tt_mel();
  e->cfg = c;
  e->tab = *tables;
  e->stft_lds = lds;
  e->spec_clip = (size_t)(1 + c.max_samples / c.hop) * c.bins_pad;
  int rc = e->open("tt_mel_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->spec, e->spec_clip * c.max_clips, false);
  if (rc) {
    tt_mel_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_mel_destroy(tt_mel* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_mel_frames(const tt_mel* e, int n) {
  if (!e || n < 0) return -1;
  return 1 + n / e->cfg.hop;
}

int tt_mel_run(tt_mel* e, const float* wav, const long long* clip_offsets, const int* clip_lengths, int n_clips, float* out,
               const long long* out_offsets, void* stream) {
  MelClips in;
  TT_TRY(mel_check_clips(e, "tt_mel_run", wav, clip_offsets, clip_lengths, n_clips, out, out_offsets, &in));
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(mel_stft_launch(e, wav, in, n_clips, nullptr, s));
    return mel_project_launch(e, in, n_clips, out, s);
  });
}

int tt_mel_spectrum(tt_mel* e, const float* wav, const long long* clip_offsets, const int* clip_lengths, int n_clips, float* out,
                    const long long* out_offsets, void* stream) {
  MelClips in;
  TT_TRY(mel_check_clips(e, "tt_mel_spectrum", wav, clip_offsets, clip_lengths, n_clips, out, out_offsets, &in));
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int { return mel_stft_launch(e, wav, in, n_clips, out, s); });
}

int tt_mel_resampler_create(const float* taps, int orig, int new_rate, int width, int max_samples, tt_mel_resampler** out) {
  TT_REQUIRE(taps && out, "tt_mel_resampler_create: null argument");
  TT_REQUIRE(orig >= 1 && new_rate >= 1 && orig != new_rate && orig <= 4096 && new_rate <= 4096, "tt_mel_resampler_create: %d -> %d (1 .. 4096, different)",
             orig, new_rate);
  TT_REQUIRE(width >= 0 && width <= 4096, "tt_mel_resampler_create: width %d (0 .. 4096)", width);
  TT_REQUIRE(max_samples >= 1 && max_samples <= kMelMaxSamples && cdiv64((int64_t)max_samples * new_rate, orig) <= INT_MAX / 2,
             "tt_mel_resampler_create: max_samples %d", max_samples);
  tt_mel_resampler* e = new tt_mel_resampler();
  e->taps = taps;
  e->orig = orig; e->new_rate = new_rate; e->width = width; e->max_samples = max_samples;
  const int rc = e->open("tt_mel_resampler_create", false);
  if (rc) {
    tt_mel_resampler_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_mel_resampler_destroy(tt_mel_resampler* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_mel_resampled_length(const tt_mel_resampler* e, int n) {
  if (!e || n < 0) return -1;
  return (int)cdiv64((int64_t)e->new_rate * n, e->orig);
}

int tt_mel_resample(tt_mel_resampler* e, const float* in, int n, float* out, void* stream) {
  TT_REQUIRE(e && in && out, "tt_mel_resample: null argument");
  TT_REQUIRE(n >= 1 && n <= e->max_samples, "tt_mel_resample: %d samples (1 .. %d)", n, e->max_samples);
  const int n_out = tt_mel_resampled_length(e, n);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    dim3 grid(cdiv(cdiv(n_out, e->new_rate), 32), cdiv(e->new_rate, 32));
    mel_resample_kernel<<<grid, 64, 0, s>>>(in, n, e->taps, e->orig, e->new_rate, e->width, n_out, out);
    TT_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
