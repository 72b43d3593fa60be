// Stationary-noise reduction by spectral subtraction (include/tortoise_mi355x_nr.h).  Five launches; the transforms are the
// bodies of csrc/stft_kernels.h that csrc/formant.hip runs as well (v_mfma_f32_32x32x2_f32: exact f32 products):
//
//   nr_stft_kernel     re, im of 32 frames x 64 bins per workgroup, interleaved [t][bins_pad], and the power P = re^2 + im^2 TRANSPOSED,
//                      [bin][t_pad]: a lane of the MFMA's D holds four consecutive frames of one bin per register group, one 16-byte store
//   nr_floor_kernel    S[b]: one wave per bin reads its row of P coalesced.  auto: the exact k-th smallest by bisection of the 32-bit
//                      pattern, most significant bit first - ans |= bit while fewer than k + 1 values lie below it; the count of a round is
//                      integer (ballots + popcounts), so the result does not depend on the order anything is read in.  T <= 1024: the row
//                      sits in 16 registers a lane; longer: every round reads the row again (it stays in L2).  region: lane-strided f32
//                      partial sums, a butterfly, one division
//   nr_gain_kernel     Pbar over (2 Rt + 1) x (2 Rb + 1) cells from a tile of P with its halo in LDS (read along t, used along b), the gain
//                      G [t][bins_pad], the layout the inverse's A operand reads as a float2 per lane
//   nr_inverse_kernel  y[t][k] = (G (re, im))[t] . inverse[:, k]
//   nr_ola_kernel      out[j] = sum_t y[t][j + n_fft / 2 - t hop] / sum_t window^2
//
// Ragged batches: blockIdx.y is the clip; no tile, no select and no sum spans two clips, and nothing depends on the batch: every clip's
// samples and floor are bit-identical to running it alone.  What is decided from the lengths (status, rank, region checks) is host code
// (denoise_host.h).  Intermediates live in the handle (one slot per clip of a call).
#include <limits.h>
#include "runtime.h"
#include "stft_kernels.h"
#include "denoise_host.h"
#include "../../include/tortoise_mi355x_test.h"

namespace tt {

bool g_nr_select_long = false;  // ttx_kernel_variant(TTX_NR_SELECT_LONG): 1 = the select re-reads the row every round whatever T (tests, A/B runs)

constexpr int kNrBinsPerBlock = 64;  // two waves of 32 bins (nr_stft_kernel)
constexpr int kNrInvWaves = 4;       // 32-sample column tiles of one nr_inverse_kernel workgroup
constexpr size_t kNrMaxLds = 64 * 1024;
constexpr int kNrRegVals = TT_NR_REG_FRAMES / 64;  // values a lane holds in the select's register form
constexpr int kNrFloorWaves = 4;                   // bins of one nr_floor_kernel workgroup
constexpr int kNrTile = 32;                        // frames and bins of one nr_gain_kernel workgroup
constexpr int kNrHalo = TT_NR_MAX_SMOOTH;
constexpr int kNrTileW = kNrTile + 2 * kNrHalo;

struct NrClips {  // by value in the kernel arguments
  long long in_off[TT_NR_MAX_CLIPS];
  long long out_off[TT_NR_MAX_CLIPS];
  int len[TT_NR_MAX_CLIPS];
  int skip[TT_NR_MAX_CLIPS];   // TT_NR_SHORT: copied, no kernel touches it
  int rank[TT_NR_MAX_CLIPS];   // k of the order statistic (auto)
  int first[TT_NR_MAX_CLIPS];  // region: first frame
  int nf[TT_NR_MAX_CLIPS];     // region: frames; 0 = auto
};

struct NrSlots {  // element strides of one clip's slot
  size_t spec, pt, gains, y;
  int t_pad;  // row length of the transposed power
};

struct NrGain {
  float beta, g_min, w;
  int rt, rb;
};

struct NrPowerEpilogue {  // the spectrum interleaved [t][bins_pad]; the power [bin][t_pad], four frames a store
  float* sp;
  float* pt;
  int bins_pad, t_pad;
  __device__ __forceinline__ void operator()(const f32x16& re, const f32x16& im, int t0, int T, int col, int h) const {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 4 * g + q, t = t0 + 8 * g + 4 * h + q;  // = t0 + mfma_row(r, h)
        if (t < T) *(float2*)(sp + 2 * ((size_t)t * bins_pad + col)) = make_float2(re[r], im[r]);
        p[q] = __fadd_rn(__fmul_rn(re[r], re[r]), __fmul_rn(im[r], im[r]));  // as written: no contraction
      }
      // frames from T on are within the row (t_pad is a whole number of tiles) and nobody reads them
      *(float4*)(pt + (size_t)col * t_pad + t0 + 8 * g + 4 * h) = make_float4(p[0], p[1], p[2], p[3]);
    }
  }
};

struct NrLinearGain {
  __device__ __forceinline__ float2 operator()(const float2 g) const { return g; }
};

__global__ __launch_bounds__(128) void nr_stft_kernel(const float* __restrict__ wav, NrClips clips, NrSlots sl, const float* __restrict__ basis,
                                                      int n_fft, int hop, int bins_pad, float* __restrict__ spec, float* __restrict__ pt) {
  extern __shared__ float xs[];
  const int c = blockIdx.y, n = clips.len[c], T = 1 + n / hop;
  if (clips.skip[c]) return;
  stft_tile_body(wav + clips.in_off[c], n, T, basis, n_fft, hop, bins_pad, kNrBinsPerBlock, 128, xs,
                 NrPowerEpilogue{spec + (size_t)c * sl.spec, pt + (size_t)c * sl.pt, bins_pad, sl.t_pad});
}

__global__ __launch_bounds__(64 * kNrFloorWaves) void nr_floor_kernel(const float* __restrict__ pt, NrClips clips, NrSlots sl, int hop, int bins,
                                                                      int bins_pad, float scale, int force_long, float* __restrict__ floor_out) {
  const int c = blockIdx.y;
  if (clips.skip[c]) return;
  const int T = 1 + clips.len[c] / hop;
  const int lane = threadIdx.x & 63, b = blockIdx.x * kNrFloorWaves + (threadIdx.x >> 6);
  if (b >= bins_pad) return;
  float* fo = floor_out + (size_t)c * bins_pad + b;
  if (b >= bins) {  // padding
    if (lane == 0) *fo = 0.f;
    return;
  }
  const float* rowf = pt + (size_t)c * sl.pt + (size_t)b * sl.t_pad;
  const int nf = clips.nf[c];
  if (nf > 0) {  // region: the mean, in an order that depends on (first, nf) alone
    const int t0 = clips.first[c];
    float s = 0.f;
    for (int t = t0 + lane; t < t0 + nf; t += 64) s = __fadd_rn(s, rowf[t]);
#pragma unroll
    for (int off = 32; off; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off));
    if (lane == 0) *fo = __fdiv_rn(s, (float)nf);
    return;
  }
  // auto: the largest x with #{P < x} <= k is the k-th smallest (nr_bisect, denoise_host.h); only the count differs between the forms
  const unsigned* row = (const unsigned*)rowf;
  const int k = clips.rank[c];
  unsigned ans;
  if (T <= TT_NR_REG_FRAMES && !force_long) {
    unsigned v[kNrRegVals];
#pragma unroll
    for (int j = 0; j < kNrRegVals; ++j) {
      const int t = j * 64 + lane;
      v[j] = t < T ? row[t] : 0xFFFFFFFFu;  // never below a candidate
    }
    ans = nr_bisect(k, [&](unsigned cand) {
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < kNrRegVals; ++j) cnt += __popcll(__ballot(v[j] < cand));
      return cnt;
    });
  } else {
    ans = nr_bisect(k, [&](unsigned cand) {
      int cnt = 0;
      for (int t = lane; t < T; t += 64) cnt += row[t] < cand ? 1 : 0;
#pragma unroll
      for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
      return cnt;
    });
  }
  if (lane == 0) *fo = __fmul_rn(__uint_as_float(ans), scale);
}

__global__ __launch_bounds__(256) void nr_gain_kernel(const float* __restrict__ pt, NrClips clips, NrSlots sl, int hop, int bins, int bins_pad,
                                                      const float* __restrict__ floor, NrGain p, float* __restrict__ gains) {
  __shared__ float ps[kNrTileW][kNrTileW + 1];  // [frame][bin]; filled along t, read along b
  const int c = blockIdx.y;
  if (clips.skip[c]) return;
  const int T = 1 + clips.len[c] / hop;
  const int t0 = blockIdx.x * kNrTile, b0 = blockIdx.z * kNrTile;
  if (t0 >= T) return;
  const int tid = threadIdx.x;
  const float* pc = pt + (size_t)c * sl.pt;
  for (int e = tid; e < kNrTileW * kNrTileW; e += 256) {
    const int bb = e / kNrTileW, tt = e % kNrTileW;
    const int b = min(max(b0 + bb - kNrHalo, 0), bins - 1), t = min(max(t0 + tt - kNrHalo, 0), T - 1);
    ps[tt][bb] = pc[(size_t)b * sl.t_pad + t];
  }
  __syncthreads();
  const int bl = tid & 31, b = b0 + bl;
  const float bs = __fmul_rn(p.beta, floor[(size_t)c * bins_pad + b]);
  float* g_out = gains + (size_t)c * sl.gains;
  for (int tl = tid >> 5; tl < kNrTile && t0 + tl < T; tl += 8) {
    float s = 0.f;
    for (int dt = -p.rt; dt <= p.rt; ++dt)
      for (int db = -p.rb; db <= p.rb; ++db) s = __fadd_rn(s, ps[tl + kNrHalo + dt][bl + kNrHalo + db]);
    const float pbar = __fmul_rn(s, p.w);
    float g = 0.f;
    if (b < bins) g = pbar > bs ? fmaxf(p.g_min, __fsub_rn(1.f, __fdiv_rn(bs, pbar))) : p.g_min;
    g_out[(size_t)(t0 + tl) * bins_pad + b] = g;
  }
}

__global__ __launch_bounds__(64 * kNrInvWaves) void nr_inverse_kernel(const float* __restrict__ spec, const float* __restrict__ gains, NrClips clips,
                                                                      NrSlots sl, const float* __restrict__ inverse, int n_fft, int hop, int bins_pad,
                                                                      float* __restrict__ y) {
  const int c = blockIdx.y, T = 1 + clips.len[c] / hop;
  if (clips.skip[c]) return;
  stft_inverse_body(spec + (size_t)c * sl.spec, gains + (size_t)c * sl.gains, T, inverse, n_fft, bins_pad, kNrInvWaves, y + (size_t)c * sl.y,
                    NrLinearGain{});
}

__global__ __launch_bounds__(256) void nr_ola_kernel(const float* __restrict__ y, NrClips clips, NrSlots sl, const float* __restrict__ basis, int n_fft,
                                                     int hop, int bins_pad, float* __restrict__ out) {
  const int c = blockIdx.y, n = clips.len[c], T = 1 + n / hop;
  if (clips.skip[c]) return;
  stft_ola_body(y + (size_t)c * sl.y, n, T, basis, n_fft, hop, bins_pad, 256, out + clips.out_off[c]);
}

}  // namespace tt

using namespace tt;

struct tt_nr : EngineHandle {
  tt_nr_config cfg;
  tt_nr_tables tab;
  float *spec = nullptr, *pt = nullptr, *gains = nullptr, *y = nullptr;  // one slot per clip of a call
  NrSlots sl;
  size_t frames_max = 0;  // frames of a clip of max_samples
  size_t stft_lds = 0;
};

static int nr_check_run(const tt_nr* e, const char* who, const float* wav, const long long* clip_offsets, const int* clip_lengths,
                        const int* noise_first_frame, const int* noise_frames, const tt_nr_params* params, int n_clips, const float* out,
                        const long long* out_offsets, const float* floor_out, const int* status_out, NrClips* in) {
  TT_REQUIRE(e && wav && clip_offsets && clip_lengths && noise_first_frame && noise_frames && params && out && out_offsets && floor_out && status_out,
             "%s: null argument", who);
  TT_REQUIRE(n_clips >= 1 && n_clips <= e->cfg.max_clips, "%s: %d clips (1 .. %d)", who, n_clips, e->cfg.max_clips);
  const char* why = nr_params_fault(*params);
  TT_REQUIRE(!why, "%s: %s", who, why);
  memset(in, 0, sizeof(*in));
  for (int c = 0; c < n_clips; ++c) {
    TT_REQUIRE(clip_lengths[c] >= e->cfg.n_fft / 2 + 1, "%s: clip %d has %d samples; reflect padding needs at least n_fft / 2 + 1 = %d", who, c,
               clip_lengths[c], e->cfg.n_fft / 2 + 1);
    TT_REQUIRE(clip_lengths[c] <= e->cfg.max_samples, "%s: clip %d has %d samples, the handle takes %d", who, c, clip_lengths[c], e->cfg.max_samples);
    TT_REQUIRE(clip_offsets[c] >= 0 && out_offsets[c] >= 0, "%s: negative offset of clip %d", who, c);
    const int T = 1 + clip_lengths[c] / e->cfg.hop;
    TT_REQUIRE(noise_frames[c] >= 0, "%s: clip %d has a noise region of %d frames", who, c, noise_frames[c]);
    why = nr_region_fault(noise_first_frame[c], noise_frames[c], T);
    TT_REQUIRE(!why, "%s: clip %d (%d frames), noise region %d .. + %d: %s", who, c, T, noise_first_frame[c], noise_frames[c], why);
    in->in_off[c] = clip_offsets[c];
    in->out_off[c] = out_offsets[c];
    in->len[c] = clip_lengths[c];
    in->skip[c] = nr_status(T, noise_frames[c]) == TT_NR_SHORT;
    in->rank[c] = nr_rank(params->quantile_num, T);
    in->first[c] = noise_frames[c] ? noise_first_frame[c] : 0;
    in->nf[c] = noise_frames[c];
  }
  return 0;
}

// all five launches and the copies of the short clips
static int nr_launch(tt_nr* e, const float* wav, const NrClips& in, const tt_nr_params& p, int n_clips, float* out, float* floor_out, hipStream_t s) {
  const tt_nr_config& c = e->cfg;
  int tmax = 0, nmax = 0;
  for (int k = 0; k < n_clips; ++k) {
    if (in.skip[k]) {
      TT_CHECK_HIP(hipMemcpyAsync(out + in.out_off[k], wav + in.in_off[k], (size_t)in.len[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
      TT_CHECK_HIP(hipMemsetAsync(floor_out + (size_t)k * c.bins_pad, 0, (size_t)c.bins_pad * sizeof(float), s));
      continue;
    }
    tmax = std::max(tmax, 1 + in.len[k] / c.hop);
    nmax = std::max(nmax, in.len[k]);
  }
  if (!tmax) return 0;
  const int tiles = cdiv(tmax, kStftTile), bins = c.n_fft / 2 + 1;
  NrGain g;
  g.beta = p.beta; g.g_min = p.g_min; g.rt = p.smooth_frames; g.rb = p.smooth_bins;
  g.w = (float)(1.0 / (double)((2 * g.rt + 1) * (2 * g.rb + 1)));
  nr_stft_kernel<<<dim3(tiles, n_clips, cdiv(c.bins_pad, kNrBinsPerBlock)), 128, e->stft_lds, s>>>(wav, in, e->sl, e->tab.basis, c.n_fft, c.hop, c.bins_pad,
                                                                                                 e->spec, e->pt);
  TT_CHECK_HIP(hipGetLastError());
  nr_floor_kernel<<<dim3(cdiv(c.bins_pad, kNrFloorWaves), n_clips), 64 * kNrFloorWaves, 0, s>>>(e->pt, in, e->sl, c.hop, bins, c.bins_pad, p.quantile_scale,
                                                                                              g_nr_select_long ? 1 : 0, floor_out);
  TT_CHECK_HIP(hipGetLastError());
  nr_gain_kernel<<<dim3(cdiv(tmax, kNrTile), n_clips, c.bins_pad / kNrTile), 256, 0, s>>>(e->pt, in, e->sl, c.hop, bins, c.bins_pad, floor_out, g, e->gains);
  TT_CHECK_HIP(hipGetLastError());
  nr_inverse_kernel<<<dim3(tiles, n_clips, cdiv(c.n_fft / 32, kNrInvWaves)), 64 * kNrInvWaves, 0, s>>>(e->spec, e->gains, in, e->sl, e->tab.inverse, c.n_fft,
                                                                                                      c.hop, c.bins_pad, e->y);
  TT_CHECK_HIP(hipGetLastError());
  nr_ola_kernel<<<dim3(cdiv(nmax, 256), n_clips), 256, 0, s>>>(e->y, in, e->sl, e->tab.basis, c.n_fft, c.hop, c.bins_pad, out);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int tt_nr_abi_version(void) { return 1; }  // ABI changes

size_t tt_nr_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_nr_config);
    case 1: return sizeof(tt_nr_tables);
    case 2: return sizeof(tt_nr_params);
    default: return 0;
  }
}

int tt_nr_rank(int quantile_num, int frames) { return nr_rank(quantile_num, frames); }

int tt_nr_region(long long start, long long end, int hop, int frames, int* first, int* count) { return nr_region(start, end, hop, frames, first, count); }

int tt_nr_create(const tt_nr_config* cfg, const tt_nr_tables* tables, tt_nr** out) {
  TT_REQUIRE(cfg && tables && out, "tt_nr_create: null argument");
  const tt_nr_config& c = *cfg;
  TT_REQUIRE(c.hop >= 8 && c.hop % 8 == 0 && c.n_fft >= 64 && c.n_fft % 64 == 0 && c.n_fft % c.hop == 0,
             "tt_nr_create: n_fft %d / hop %d (n_fft a multiple of 64 and of hop, hop a multiple of 8)", c.n_fft, c.hop);
  TT_REQUIRE(c.bins_pad >= c.n_fft / 2 + 1 && c.bins_pad % 32 == 0, "tt_nr_create: bins_pad %d (a multiple of 32, at least n_fft / 2 + 1 = %d)",
             c.bins_pad, c.n_fft / 2 + 1);
  TT_REQUIRE(c.max_samples >= c.n_fft / 2 + 1 && c.max_samples <= TT_NR_MAX_SAMPLES, "tt_nr_create: max_samples %d (%d .. %d)", c.max_samples,
             c.n_fft / 2 + 1, TT_NR_MAX_SAMPLES);
  TT_REQUIRE(c.max_clips >= 1 && c.max_clips <= TT_NR_MAX_CLIPS, "tt_nr_create: max_clips %d (1 .. %d)", c.max_clips, TT_NR_MAX_CLIPS);
  TT_REQUIRE(tables->basis && tables->inverse, "tt_nr_create: null table");
  const size_t lds = stft_lds_bytes(c.n_fft, c.hop);
  TT_REQUIRE(lds <= kNrMaxLds, "tt_nr_create: 32 frames of n_fft %d at hop %d need %zu bytes of LDS (at most %zu)", c.n_fft, c.hop, lds, kNrMaxLds);
  tt_nr* e = new tt_nr();
  e->cfg = c;
  e->tab = *tables;
  e->stft_lds = lds;
  e->frames_max = (size_t)(1 + c.max_samples / c.hop);
  e->sl.t_pad = (int)(cdiv((int)e->frames_max, kStftTile) * kStftTile);  // a tile's four-frame stores stay inside the row
  e->sl.spec = e->frames_max * 2 * c.bins_pad;
  e->sl.pt = (size_t)c.bins_pad * e->sl.t_pad;
  e->sl.gains = e->frames_max * c.bins_pad;
  e->sl.y = e->frames_max * c.n_fft;
  int rc = e->open("tt_nr_create", false);
  if (!rc) rc = e->arena.alloc_t(&e->spec, e->sl.spec * c.max_clips, false);
  if (!rc) rc = e->arena.alloc_t(&e->pt, e->sl.pt * c.max_clips, false);
  if (!rc) rc = e->arena.alloc_t(&e->gains, e->sl.gains * c.max_clips, false);
  if (!rc) rc = e->arena.alloc_t(&e->y, e->sl.y * c.max_clips, false);
  if (rc) {
    tt_nr_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_nr_destroy(tt_nr* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_nr_frames(const tt_nr* e, int n) {
  if (!e || n < 0) return -1;
  return 1 + n / e->cfg.hop;
}

int tt_nr_run(tt_nr* e, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* noise_first_frame, const int* noise_frames,
              const tt_nr_params* params, int n_clips, float* out, const long long* out_offsets, float* floor_out, int* status_out, void* stream) {
  NrClips in;
  TT_TRY(nr_check_run(e, "tt_nr_run", wav, clip_offsets, clip_lengths, noise_first_frame, noise_frames, params, n_clips, out, out_offsets, floor_out,
                      status_out, &in));
  for (int c = 0; c < n_clips; ++c) status_out[c] = in.skip[c] ? TT_NR_SHORT : TT_NR_OK;
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int { return nr_launch(e, wav, in, *params, n_clips, out, floor_out, s); });
}

int tt_op_nr_run(void* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* noise_first_frame, const int* noise_frames,
                 const tt_nr_params* params, int n_clips, float* out, const long long* out_offsets, float* floor_out, int* status_out, float* spectrum,
                 float* power, float* gains, const long long* stage_offsets, void* stream) {
  tt_nr* e = (tt_nr*)h;
  NrClips in;
  TT_TRY(nr_check_run(e, "tt_op_nr_run", wav, clip_offsets, clip_lengths, noise_first_frame, noise_frames, params, n_clips, out, out_offsets, floor_out,
                      status_out, &in));
  const bool staged = spectrum || power || gains;
  TT_REQUIRE(!staged || stage_offsets, "tt_op_nr_run: staged outputs without stage_offsets");
  for (int c = 0; staged && c < n_clips; ++c) TT_REQUIRE(stage_offsets[c] >= 0, "tt_op_nr_run: negative stage offset of clip %d", c);
  for (int c = 0; c < n_clips; ++c) status_out[c] = in.skip[c] ? TT_NR_SHORT : TT_NR_OK;
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(nr_launch(e, wav, in, *params, n_clips, out, floor_out, s));
    for (int c = 0; staged && c < n_clips; ++c) {
      if (in.skip[c]) continue;  // nothing was computed for a copied clip
      const size_t T = (size_t)(1 + in.len[c] / e->cfg.hop), el = T * e->cfg.bins_pad, so = (size_t)stage_offsets[c];
      if (spectrum) TT_CHECK_HIP(hipMemcpyAsync(spectrum + 2 * so, e->spec + (size_t)c * e->sl.spec, 2 * el * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (power)  // [bins_pad][T]: the rows of the transposed power without their padding
        TT_CHECK_HIP(hipMemcpy2DAsync(power + so, T * sizeof(float), e->pt + (size_t)c * e->sl.pt, (size_t)e->sl.t_pad * sizeof(float), T * sizeof(float),
                                      (size_t)e->cfg.bins_pad, hipMemcpyDeviceToDevice, s));
      if (gains) TT_CHECK_HIP(hipMemcpyAsync(gains + so, e->gains + (size_t)c * e->sl.gains, el * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return 0;
  });
}

}  // extern "C"
