// HiFi-GAN decoder of the streaming path: GPT latents -> waveform without CLVP / diffusion / UnivNet
// (reference: tortoise/models/hifigan_decoder.py:159-294 HifiganGenerator, called from tortoise/api_fast.py:420, 517).
//
// Unlike UnivNet (32 channels: VALU kernels), this generator is 512 -> 256 -> 128 -> 64 -> 32 channels wide with k = 3 / 7 / 11
// dilated convolutions: ~0.5 TFLOP per 9 s of audio, GEMM-shaped.  Everything therefore runs token-major ([samples][channels],
// channels padded to a multiple of 64 with zero weights) through the engine's MFMA conv-GEMM:
//   * a dilated conv1d is the tap GEMM with a row stride between taps (GemmArgs::dilation);
//   * ConvTranspose1d(k = 2u, stride u, padding u/2) is ONE 2-tap GEMM over the input rows with N = u * C_out: row j holds
//     the u output phases (t + u/2 = u j + r receives x[j] w[:, :, r] + x[j-1] w[:, :, r+u]), so the [rows+1][u * C] result
//     IS the upsampled [u * rows][C] tensor shifted by u/2 rows - no scatter, no zero insertion;
//   * every LeakyReLU rides an epilogue: conv1 of a ResBlock applies it to its output, conv2 / the transposed conv add the
//     skip and emit the activated operand copy of the next conv next to the f32 stream (GemmArgs::act_t);
//   * the multi-receptive-field mean of the three ResBlocks + the next LeakyReLU + the operand cast is one elementwise pass.
// A call decodes a ragged batch (include/tortoise_mi355x_hifi.h; tt_hifi_run is its n = 1 case): sequence b owns a slot of P rows at
// every stage (P0 = longest T2 + 1 after the interpolations, times the upsampling so far) and holds rows_b valid rows at its start.  The
// tap convolutions run over all slots at once with the per-sequence valid-length loader (GemmArgs::seq_vlen): a tap that reaches past
// rows_b or before the slot start reads zero, exactly the zero padding of a sequence decoded alone, so no "x[rows] = 0" memset is needed.
// conv_pre keeps one launch per sequence (each has its own cond_layer(g) bias row).  k-order per output element does not depend on M or on
// the tile (gemm_impl.h), so every sequence is bit-identical to decoding it alone.
#include "runtime.h"
#include "../../include/tortoise_mi355x.h"
#include "../../include/tortoise_mi355x_hifi.h"

using namespace tt;

namespace {

// per-sequence row counts and row offsets of one batched pass (kernel argument: no host -> device copy)
struct HifiSeqs {
  int n_in[TT_HIFI_MAX_BATCH], n_out[TT_HIFI_MAX_BATCH];  // rows read / written per sequence
  int src[TT_HIFI_MAX_BATCH], dst[TT_HIFI_MAX_BATCH];     // first row of each sequence in the source / destination
};

// F.interpolate(mode="linear", align_corners=False, scale_factor=s) along rows of a token-major tensor: rs = (float)(1 / s);
// sequence blockIdx.y reads q.n_in rows at row q.src and writes q.n_out rows at row q.dst
template <typename OT>
__global__ void interp_rows_kernel(const float* __restrict__ src, OT* __restrict__ dst, const HifiSeqs q, int C, float rs) {
  const int b = blockIdx.y, t = blockIdx.x;
  if (t >= q.n_out[b]) return;
  const int Tin = q.n_in[b];
  src += (size_t)q.src[b] * C;
  dst += (size_t)q.dst[b] * C;
  float pos = rs * ((float)t + 0.5f) - 0.5f;
  pos = pos < 0.f ? 0.f : pos;
  const int i0 = min((int)pos, Tin - 1), i1 = min(i0 + 1, Tin - 1);
  const float l1 = fminf(fmaxf(pos - (float)i0, 0.f), 1.f), l0 = 1.0f - l1;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    dst[(size_t)t * C + c] = (OT)(l0 * src[(size_t)i0 * C + c] + l1 * src[(size_t)i1 * C + c]);
}

// vlen[l * TT_HIFI_MAX_BATCH + b] = valid rows of sequence b at level l (frames q.n_out[b] times the upsampling of the first l stages)
__global__ void hifi_vlen_kernel(const HifiSeqs q, int n, tt_hifi_config c, int* __restrict__ vlen) {
  const int b = threadIdx.x;
  if (b >= n) return;
  int rows = q.n_out[b];
  for (int l = 0; l <= c.num_stages; ++l) {
    vlen[l * TT_HIFI_MAX_BATCH + b] = rows;
    if (l < c.num_stages) rows *= c.up_factor[l];
  }
}

// wav[q.dst[b] + i] = slots[q.src[b] + i] for i < q.n_out[b]
__global__ void gather_rows_kernel(const float* __restrict__ slots, float* __restrict__ wav, const HifiSeqs q) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < q.n_out[b]; i += gridDim.x * blockDim.x) wav[(size_t)q.dst[b] + i] = slots[(size_t)q.src[b] + i];
}

// out[r][c] = T(lrelu((z0 + z1 + z2)[r][c] / nk, slope)), 4 channels per thread
template <typename T>
__global__ void mrf_combine_kernel(const float* __restrict__ z0, const float* __restrict__ z1, const float* __restrict__ z2, int nk,
                                   T* __restrict__ out, size_t n4, float slope) {
  const float inv = 1.0f / (float)nk;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 a = ((const float4*)z0)[i];
    if (nk > 1) { const float4 b = ((const float4*)z1)[i]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
    if (nk > 2) { const float4 b = ((const float4*)z2)[i]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
    float v[4] = {a.x * inv, a.y * inv, a.z * inv, a.w * inv};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * slope;
    ((typename Vec<T>::x4*)out)[i] = pack4<T>(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace

struct tt_hifi : EngineHandle {
  tt_hifi_config cfg;
  tt_hifi_weights w;
  std::vector<tt_hifi_resblock> res;
  int cw[TT_HIFI_MAX_STAGES + 1];   // real channel width per level (level 0 = after conv_pre)
  int cp[TT_HIFI_MAX_STAGES + 1];   // padded to a multiple of 64
  float* lat1 = nullptr;   // [sum 4 T_b][in] first interpolation, back to back
  void* lat2 = nullptr;    // [n P0][in] T, one slot per sequence
  void* g_t = nullptr;     // [n][cond] T
  float* bias0 = nullptr;  // [n][c0] conv_pre bias + cond_layer(g_b)
  int* vlen = nullptr;     // [num_stages + 1][TT_HIFI_MAX_BATCH] valid rows per sequence and level (hifi_vlen_kernel)
  int cap_rows = 0;        // slot rows at level 0 one call may hold (tt_hifi_batch_capacity)
  void* a_in = nullptr;    // [rows + 1][C] T: activated input of the next transposed conv (last row zero)
  float* o32 = nullptr;    // transposed-conv output, flat [(rows + 1) * u][C]
  void* o_t = nullptr;     // its activated operand copy
  float* xa = nullptr; float* xb = nullptr;
  float* z[3] = {nullptr, nullptr, nullptr};
  void* t1 = nullptr;      // lrelu(conv1) T
  void* xt = nullptr;      // lrelu(x) T between dilations
  size_t cap_elems = 0;    // element capacity of every stage buffer
};

// elements of the widest stage buffer for `rows0` slot rows at level 0 (the transposed-conv output of stage i: rows0 * U_i * u_i rows of
// Cp_{i+1}, plus the u_i rows its ResBlocks' view reads past the end)
static int hifi_elems(const tt_hifi* e, int rows0, size_t* need) {
  size_t rows = rows0, mx = (size_t)rows0 * e->cp[0];
  for (int i = 0; i < e->cfg.num_stages; ++i) {
    rows *= e->cfg.up_factor[i];
    mx = std::max(mx, (rows + e->cfg.up_factor[i]) * e->cp[i + 1]);
  }
  *need = mx;
  return 0;
}

extern "C" {

int tt_hifi_output_frames(int n_latents) {  // F.interpolate output lengths (hifigan_decoder.py:272-281): floor(n * 4), floor(. * 24000 / 22050)
  const int t1 = (int)floor((double)n_latents * (1024.0 / 256.0));
  return (int)floor((double)t1 * (24000.0 / 22050.0));
}

int tt_hifi_create(const tt_hifi_config* cfg, const tt_hifi_weights* w, tt_hifi** out) {
  TT_REQUIRE(cfg && (cfg->dtype == DT_BF16 || cfg->dtype == DT_F16), "tt_hifi_create: dtype must be TT_BF16 or TT_F16 (the fp32 verification mode covers the AR / CLVP / diffusion / vocoder stages)");
  TT_REQUIRE(cfg && w && out, "tt_hifi_create: null argument");
  TT_REQUIRE(cfg->num_stages >= 1 && cfg->num_stages <= TT_HIFI_MAX_STAGES && cfg->num_kernels >= 1 && cfg->num_kernels <= 3 &&
             cfg->num_dilations >= 1 && cfg->num_dilations <= 3, "tt_hifi_create: %d stages / %d kernels / %d dilations unsupported", cfg->num_stages, cfg->num_kernels, cfg->num_dilations);
  TT_REQUIRE(cfg->in_channels % 64 == 0 && cfg->cond_channels % 64 == 0 && cfg->initial_channel % 64 == 0 && cfg->max_latents >= 1, "tt_hifi_create: widths must be multiples of 64");
  for (int i = 0; i < cfg->num_stages; ++i)
    TT_REQUIRE(cfg->up_factor[i] >= 2 && cfg->up_factor[i] % 2 == 0 && (cfg->initial_channel >> (i + 1)) >= 4, "tt_hifi_create: stage %d (factor %d, %d channels) unsupported", i, cfg->up_factor[i], cfg->initial_channel >> (i + 1));
  tt_hifi* e = new tt_hifi();
  e->cfg = *cfg;
  e->w = *w;
  e->res.assign(w->res_host, w->res_host + cfg->num_stages * cfg->num_kernels);
  for (int i = 0; i <= cfg->num_stages; ++i) {
    e->cw[i] = cfg->initial_channel >> i;
    e->cp[i] = std::max(64, round_up(e->cw[i], 64));
  }
  const int T2max = tt_hifi_output_frames(cfg->max_latents);
  e->cap_rows = T2max + 1;
  size_t need = 0;
  hifi_elems(e, e->cap_rows, &need);
  e->cap_elems = need + 4096;
  int rc = e->open("tt_hifi_create", false);
  // (sum of 4 T_b <= sum of T2_b < n P0 <= cap_rows: the first interpolation fits the level-0 slot rows)
  if (!rc) rc = e->arena.alloc_t(&e->lat1, (size_t)(e->cap_rows + 8) * cfg->in_channels);
  if (!rc) rc = e->arena.alloc(&e->lat2, (size_t)(e->cap_rows + 8) * cfg->in_channels * 2);
  if (!rc) rc = e->arena.alloc(&e->g_t, (size_t)TT_HIFI_MAX_BATCH * cfg->cond_channels * 2 + 256);
  if (!rc) rc = e->arena.alloc_t(&e->bias0, (size_t)TT_HIFI_MAX_BATCH * cfg->initial_channel);
  if (!rc) rc = e->arena.alloc_t(&e->vlen, (size_t)(TT_HIFI_MAX_STAGES + 1) * TT_HIFI_MAX_BATCH);
  if (!rc) rc = e->arena.alloc(&e->a_in, e->cap_elems * 2);
  if (!rc) rc = e->arena.alloc_t(&e->o32, e->cap_elems);
  if (!rc) rc = e->arena.alloc(&e->o_t, e->cap_elems * 2);
  if (!rc) rc = e->arena.alloc_t(&e->xa, e->cap_elems);
  if (!rc) rc = e->arena.alloc_t(&e->xb, e->cap_elems);
  for (int j = 0; j < 3 && !rc; ++j) rc = e->arena.alloc_t(&e->z[j], e->cap_elems);
  if (!rc) rc = e->arena.alloc(&e->t1, e->cap_elems * 2);
  if (!rc) rc = e->arena.alloc(&e->xt, e->cap_elems * 2);
  if (rc) {
    tt_hifi_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_hifi_destroy(tt_hifi* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_hifi_batch_abi_version(void) { return 1; }  // ABI changes

size_t tt_hifi_batch_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_hifi_config);
    case 1: return sizeof(tt_hifi_weights);
    case 2: return sizeof(tt_hifi_resblock);
  }
  return 0;
}

int tt_hifi_batch_capacity(const tt_hifi* e) { return e ? e->cap_rows : 0; }

int tt_hifi_run_batch(tt_hifi* e, int n, const float* latents, const int* lengths, const float* g, float* wav, void* stream) {
  TT_REQUIRE(e && latents && lengths && g && wav, "tt_hifi_run_batch: null argument");
  TT_REQUIRE(n >= 1 && n <= TT_HIFI_MAX_BATCH, "tt_hifi_run_batch: %d sequences (1 .. %d per call)", n, TT_HIFI_MAX_BATCH);
  const tt_hifi_config& c = e->cfg;
  int U = 1;  // samples per interpolated frame
  for (int i = 0; i < c.num_stages; ++i) U *= c.up_factor[i];
  HifiSeqs q1, q2, qo;  // first / second interpolation, output gather
  int P0 = 0, lat_rows = 0, lat1_rows = 0, wav_rows = 0;
  for (int b = 0; b < n; ++b) {
    const int T = lengths[b];
    TT_REQUIRE(T >= 1 && T <= c.max_latents, "tt_hifi_run_batch: sequence %d has %d latents (1 .. %d)", b, T, c.max_latents);
    const int T1 = (int)floor((double)T * 4.0), T2 = tt_hifi_output_frames(T);
    TT_REQUIRE(T2 >= 1, "tt_hifi_run_batch: sequence %d has no output frames", b);
    q1.n_in[b] = T; q1.n_out[b] = T1; q1.src[b] = lat_rows; q1.dst[b] = lat1_rows;
    q2.n_in[b] = T1; q2.n_out[b] = T2; q2.src[b] = lat1_rows;
    qo.n_out[b] = T2 * U; qo.dst[b] = wav_rows;
    lat_rows += T; lat1_rows += T1; wav_rows += T2 * U;
    P0 = std::max(P0, T2 + 1);
  }
  TT_REQUIRE((long)n * P0 <= e->cap_rows, "tt_hifi_run_batch: %d slots of %d frames exceed the handle's %d (max_latents %d)", n, P0, e->cap_rows, c.max_latents);
  for (int b = 0; b < n; ++b) { q2.dst[b] = b * P0; qo.src[b] = b * P0 * U; }
  const int last = n - 1;
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    const int dt = c.dtype, IN = c.in_channels, C0 = c.initial_channel;
    int T1max = 0, T2max = 0;
    for (int b = 0; b < n; ++b) { T1max = std::max(T1max, q1.n_out[b]); T2max = std::max(T2max, q2.n_out[b]); }
    // latents -> x4 -> x24000/22050 (linear), operand type, one slot of P0 frames per sequence
    interp_rows_kernel<float><<<dim3(T1max, n), 256, 0, s>>>(latents, e->lat1, q1, IN, (float)(1.0 / (1024.0 / 256.0)));
    if (dt == DT_BF16) interp_rows_kernel<bf16><<<dim3(T2max, n), 256, 0, s>>>(e->lat1, (bf16*)e->lat2, q2, IN, (float)(1.0 / (24000.0 / 22050.0)));
    else interp_rows_kernel<f16><<<dim3(T2max, n), 256, 0, s>>>(e->lat1, (f16*)e->lat2, q2, IN, (float)(1.0 / (24000.0 / 22050.0)));
    hifi_vlen_kernel<<<1, TT_HIFI_MAX_BATCH, 0, s>>>(q2, n, c, e->vlen);
    TT_CHECK_HIP(hipGetLastError());
    // conv_pre bias + cond_layer(g_b): one M = n GEMM, the conv_pre bias rides as the residual (ldres 0: the same row for every sequence)
    TT_TRY(cast_pad_launch(dt, g, c.cond_channels, e->g_t, c.cond_channels, n, c.cond_channels, c.cond_channels, s));
    GemmArgs gm = gemm_args(e->g_t, c.cond_channels, e->w.w_cond, c.cond_channels, n, C0, c.cond_channels);
    gm.bias = e->w.b_cond; gm.res = e->w.b_pre; gm.ldres = 0; gm.out_f32 = e->bias0; gm.ldo32 = C0;
    TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
    // conv_pre (k7) -> lrelu(0.1) -> operand of the first transposed conv: one launch per sequence (its own bias row)
    for (int b = 0; b < n; ++b) {
      const int T2 = q2.n_out[b];
      gm = gemm_args(offset_t(e->lat2, (size_t)b * P0 * IN), IN, e->w.w_pre, 7 * IN, T2, C0, 7 * IN);
      gm.taps = 7; gm.seq_len = T2; gm.bias = e->bias0 + (size_t)b * C0; gm.act = ACT_LRELU; gm.slope = c.lrelu_slope;
      gm.out_t = offset_t(e->a_in, (size_t)b * P0 * e->cp[0]); gm.ldot = e->cp[0];
      TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
    }
    int P = P0, rows_last = q2.n_out[last];  // slot rows / valid rows of the last sequence at this level
    for (int i = 0; i < c.num_stages; ++i) {
      const int u = c.up_factor[i], Cin = e->cp[i], C = e->cp[i + 1], p = u / 2;
      const int Pn = P * u, R_last = rows_last * u;
      const int* vl_in = e->vlen + i * TT_HIFI_MAX_BATCH;
      const int* vl_out = e->vlen + (i + 1) * TT_HIFI_MAX_BATCH;
      // ConvTranspose1d as a 2-tap GEMM over rows_b + 1 input rows of every slot (row rows_b reads zero): flat output row t + p
      gm = gemm_args(e->a_in, Cin, e->w.w_up[i], 2 * Cin, last * P + rows_last + 1, u * C, 2 * Cin);
      gm.taps = 2; gm.seq_len = P; gm.seq_vlen = vl_in; gm.bias = e->w.b_up[i]; gm.out_f32 = e->o32; gm.ldo32 = u * C; gm.out_t = e->o_t; gm.ldot = u * C;
      gm.act_t = ACT_LRELU; gm.slope_t = c.lrelu_slope;
      TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
      // the ResBlocks see slot b of Pn rows at flat row b Pn + p, its first R_b rows valid
      const int M = last * Pn + R_last;
      const float* o32 = e->o32 + (size_t)p * C;
      const void* o_t = offset_t(e->o_t, (size_t)p * C);
      for (int j = 0; j < c.num_kernels; ++j) {
        const tt_hifi_resblock& rb = e->res[i * c.num_kernels + j];
        const int ks = c.kernel_size[j];
        const float* x32 = o32;
        const void* xop = o_t;
        for (int d = 0; d < c.num_dilations; ++d) {
          const bool lastd = d == c.num_dilations - 1;
          gm = gemm_args(xop, C, rb.w1[d], ks * C, M, C, ks * C);   // convs1[d]: dilated, LeakyReLU on the output
          gm.taps = ks; gm.dilation = c.dilation[d]; gm.seq_len = Pn; gm.seq_vlen = vl_out; gm.bias = rb.b1[d]; gm.act = ACT_LRELU; gm.slope = c.lrelu_slope;
          gm.out_t = e->t1; gm.ldot = C;
          TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
          float* xn = lastd ? e->z[j] : (d & 1 ? e->xb : e->xa);
          gm = gemm_args(e->t1, C, rb.w2[d], ks * C, M, C, ks * C);  // convs2[d] + skip; next dilation's activated operand
          gm.taps = ks; gm.seq_len = Pn; gm.seq_vlen = vl_out; gm.bias = rb.b2[d]; gm.res = x32; gm.ldres = C; gm.out_f32 = xn; gm.ldo32 = C;
          if (!lastd) { gm.out_t = e->xt; gm.ldot = C; gm.act_t = ACT_LRELU; gm.slope_t = c.lrelu_slope; }
          TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
          x32 = xn;
          xop = e->xt;
        }
      }
      // mean of the ResBlocks -> LeakyReLU (0.1 between stages, 0.01 = F.leaky_relu default before conv_post) -> operand type
      const bool final_stage = i == c.num_stages - 1;
      const size_t n4 = (size_t)M * C / 4;
      const int blocks = (int)std::min<size_t>((n4 + 255) / 256, 8192);
      const float slope = final_stage ? 0.01f : c.lrelu_slope;
      if (dt == DT_BF16) mrf_combine_kernel<bf16><<<blocks, 256, 0, s>>>(e->z[0], e->z[1], e->z[2], c.num_kernels, (bf16*)e->a_in, n4, slope);
      else mrf_combine_kernel<f16><<<blocks, 256, 0, s>>>(e->z[0], e->z[1], e->z[2], c.num_kernels, (f16*)e->a_in, n4, slope);
      TT_CHECK_HIP(hipGetLastError());
      P = Pn;
      rows_last = R_last;
    }
    // conv_post (k7) -> tanh; one sequence writes its samples in place, a batch goes through the slots and a gather
    const int CL = e->cp[c.num_stages];
    float* out = n == 1 ? wav : e->xa;
    gm = gemm_args(e->a_in, CL, e->w.w_post, 7 * CL, last * P + rows_last, 1, 7 * CL);
    gm.taps = 7; gm.seq_len = P; gm.seq_vlen = e->vlen + c.num_stages * TT_HIFI_MAX_BATCH; gm.bias = e->w.b_post; gm.act = ACT_TANH;
    gm.out_f32 = out; gm.ldo32 = 1;
    TT_TRY(gemm_launch(dt, EPI_STD, gm, s));
    if (n > 1) {
      int Smax = 0;
      for (int b = 0; b < n; ++b) Smax = std::max(Smax, qo.n_out[b]);
      gather_rows_kernel<<<dim3(std::min((Smax + 255) / 256, 1024), n), 256, 0, s>>>(e->xa, wav, qo);
      TT_CHECK_HIP(hipGetLastError());
    }
    return 0;
  });
}

int tt_hifi_run(tt_hifi* e, const float* latents, int T, const float* g, float* wav, int* n_samples, void* stream) {
  TT_REQUIRE(e && latents && g && wav && n_samples, "tt_hifi_run: null argument");
  TT_REQUIRE(T >= 1 && T <= e->cfg.max_latents, "tt_hifi_run: %d latents exceed capacity %d", T, e->cfg.max_latents);
  TT_TRY(tt_hifi_run_batch(e, 1, latents, &T, g, wav, stream));
  int U = 1;
  for (int i = 0; i < e->cfg.num_stages; ++i) U *= e->cfg.up_factor[i];
  *n_samples = tt_hifi_output_frames(T) * U;
  return 0;
}

}  // extern "C"
