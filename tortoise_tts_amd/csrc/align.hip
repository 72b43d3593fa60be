// wav2vec2 CTC aligner of the redaction path (reference: tortoise/utils/wav2vec_alignment.py:63-90 running
// transformers.Wav2Vec2ForCTC, feat_extract_norm "layer", do_stable_layer_norm) - include/tortoise_mi355x_align.h.
// New kernels: the 24 -> 16 kHz polyphase resampler with the clip statistics, feature-encoder layer 0 (Conv1d(1, 512, 10, stride 5) +
// LayerNorm + GELU with the normalisation applied on load) and the per-frame argmax.  Everything else is composed of the engine's
// launches in the token-major layout: the strided 512 -> 512 convolutions are plain GEMMs whose A rows overlap (lda = stride * 512 < K =
// k * 512: output row t reads input rows stride * t .. stride * t + k - 1, which are contiguous), each followed by LayerNorm + GELU in one
// row-norm launch; the grouped positional convolution is one tap GEMM per group; the encoder layers are pre-LN transformer layers.
#include "stage_blocks.h"
#include "../../include/tortoise_mi355x_align.h"
#include "../../include/tortoise_mi355x_test.h"

using namespace tt;

namespace tt {

constexpr int kResampleTaps = 23;  // 2 * width + orig with width = ceil(6 * 3 / 1.98) = 10 (torchaudio _get_sinc_resample_kernel)
constexpr int kResampleWidth = 10;
constexpr int kResampleBlock = 256;  // conv frames (3 input -> 2 output samples) per workgroup

static inline __host__ __device__ int resample_len(int S) { return (int)(((long)2 * S + 2) / 3); }  // ceil(2 S / 3)
static inline int resample_blocks(int S) { return cdiv(S / 3 + 1, kResampleBlock); }

// y[2 f + p] = sum_t taps[p][t] * x[3 f + t - 10] (zero outside the clip) for the ceil(2 S / 3) outputs torchaudio keeps; partial[b] =
// (sum y, sum y^2) in double over workgroup b's outputs.
__global__ __launch_bounds__(kResampleBlock) void w2v_resample_kernel(const float* __restrict__ x, int S, const float* __restrict__ taps,
                                                                       float* __restrict__ y, double* __restrict__ partial) {
  __shared__ float tp[2 * kResampleTaps];
  __shared__ double red[2][kResampleBlock / 64];
  const int tid = threadIdx.x;
  if (tid < 2 * kResampleTaps) tp[tid] = taps[tid];
  __syncthreads();
  const int L = resample_len(S);
  const int f = blockIdx.x * kResampleBlock + tid;
  const int base = 3 * f - kResampleWidth;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int o = 2 * f + p;
    if (o < L) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < kResampleTaps; ++t) {
        const int i = base + t;
        const float v = (i >= 0 && i < S) ? x[i] : 0.f;
        acc += tp[p * kResampleTaps + t] * v;
      }
      y[o] = acc;
      s += acc;
      q += (double)acc * acc;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off);
    q += __shfl_xor(q, off);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = q; }
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0, tq = 0.0;
    for (int w = 0; w < kResampleBlock / 64; ++w) { ts += red[0][w]; tq += red[1][w]; }
    partial[2 * blockIdx.x] = ts;
    partial[2 * blockIdx.x + 1] = tq;
  }
}

// stats = {mean, 1 / sqrt(var + 1e-7)} with torch's default (unbiased) variance over the n resampled samples
__global__ __launch_bounds__(256) void w2v_stats_kernel(const double* __restrict__ partial, int nblocks, int n, float* __restrict__ stats,
                                                        int* guard) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int b = tid; b < nblocks; b += 256) { s += partial[2 * b]; q += partial[2 * b + 1]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off);
    q += __shfl_xor(q, off);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = q; }
  __syncthreads();
  if (tid == 0) {
    const double ts = red[0][0] + red[0][1] + red[0][2] + red[0][3], tq = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double mean = ts / n;
    const double var = n > 1 ? fmax(tq - ts * mean, 0.0) / (n - 1) : 0.0;
    stats[0] = (float)mean;
    stats[1] = (float)(1.0 / sqrt((double)(float)var + 1e-7));
    if (guard && !(var < INFINITY)) atomicAdd(guard, 1);
  }
}

// Feature-encoder layer 0: one wave per output frame, lane l owns channels 8 l .. 8 l + 7 (C = 512) and keeps their KW taps in registers
// across the frames it visits.  out[f][c] = GELU(LayerNorm_c(b[c] + sum_t w[c][t] * xn[stride f + t])), xn = (y - mean) * rstd.
template <typename T, int KW>
__global__ __launch_bounds__(256) void w2v_conv0_kernel(const float* __restrict__ y, const float* __restrict__ stats, int F, int stride,
                                                        const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ g,
                                                        const float* __restrict__ beta, T* __restrict__ out_t, float* __restrict__ out_f32, int* guard) {
  constexpr int C = 512, CPL = C / 64;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int c0 = lane * CPL;
  float wr[CPL][KW], br[CPL], gr[CPL], er[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
#pragma unroll
    for (int t = 0; t < KW; ++t) wr[j][t] = w[(c0 + j) * KW + t];
    br[j] = bias[c0 + j];
    gr[j] = g[c0 + j];
    er[j] = beta[c0 + j];
  }
  const float mean = stats[0], rstd = stats[1];
  for (int f = wave; f < F; f += nwaves) {
    float xs[KW];
#pragma unroll
    for (int t = 0; t < KW; ++t) xs[t] = (y[(size_t)f * stride + t] - mean) * rstd;
    float acc[CPL];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < KW; ++t) a += wr[j][t] * xs[t];
      acc[j] = a + br[j];
      sum += acc[j];
    }
    const float mu = wave_sum(sum) * (1.0f / C);
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) sq += (acc[j] - mu) * (acc[j] - mu);
    const float var = wave_sum(sq) * (1.0f / C);
    if (guard && lane == 0 && !(var < INFINITY)) atomicAdd(guard, 1);
    const float r = rsqrtf(var + 1e-5f);
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j] = gelu_erf((acc[j] - mu) * r * gr[j] + er[j]);
    T* o = out_t + (size_t)f * C + c0;
    *(typename Vec<T>::x4*)o = pack4<T>(acc[0], acc[1], acc[2], acc[3]);
    *(typename Vec<T>::x4*)(o + 4) = pack4<T>(acc[4], acc[5], acc[6], acc[7]);
    if (out_f32) {
      float* p = out_f32 + (size_t)f * C + c0;
      *(float4*)p = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *(float4*)(p + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
  }
}

// ids[f] = argmax over the first V columns of logits row f (ties: the lowest index, as torch.argmax); out (optional) [T][V] gets the row.
__global__ __launch_bounds__(256) void w2v_argmax_kernel(const float* __restrict__ logits, int ld, int T, int V, int* __restrict__ ids,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= T) return;
  const float* row = logits + (size_t)f * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    const float v = row[c];
    if (out) out[(size_t)f * V + c] = v;
    if (v > best || bi == 0x7fffffff) { best = v; bi = c; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) ids[f] = bi;
}

int w2v_resample_launch(const float* x, int S, const float* taps, float* y, double* partial, float* stats, int* guard, hipStream_t s) {
  TT_REQUIRE(S >= 1, "w2v resample: empty clip");
  const int nb = resample_blocks(S);
  w2v_resample_kernel<<<nb, kResampleBlock, 0, s>>>(x, S, taps, y, partial);
  w2v_stats_kernel<<<1, 256, 0, s>>>(partial, nb, resample_len(S), stats, guard);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

int w2v_conv0_launch(int dtype, const float* y, const float* stats, int F, int k, int stride, const float* w, const float* b, const float* g,
                     const float* beta, void* out_t, float* out_f32, int* guard, hipStream_t s) {
  TT_REQUIRE(k == 10 && F >= 1 && stride >= 1, "w2v conv0: kernel %d (10 is built) over %d frames", k, F);
  const int blocks = std::min(cdiv(F, 4), 2048);
  TT_DISPATCH_T(dtype, T, (w2v_conv0_kernel<T, 10><<<blocks, 256, 0, s>>>(y, stats, F, stride, w, b, g, beta, (T*)out_t, out_f32, guard)));
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

int w2v_argmax_launch(const float* logits, int ld, int T, int V, int* ids, float* out, hipStream_t s) {
  TT_REQUIRE(T >= 1 && V >= 1 && ld >= V, "w2v argmax: bad shape T=%d V=%d ld=%d", T, V, ld);
  w2v_argmax_kernel<<<cdiv(T, 4), 256, 0, s>>>(logits, ld, T, V, ids, out);
  TT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace tt

struct tt_w2v : EngineHandle {  // guard: resample statistics, conv-0 LayerNorms and every row norm; snapshot at the end of every run
  tt_w2v_config cfg;
  tt_w2v_weights w;
  std::vector<tt_gpt_layer> L;
  int es = 2;
  int max_frames = 0, max_c0 = 0, max_c1 = 0;
  float* y16 = nullptr; double* partial = nullptr; float* stats = nullptr;
  void* ca = nullptr; void* cb = nullptr; float* cf = nullptr;  // feature-encoder rows: T ping-pong [max_c0] / [max_c1] x conv_dim, f32 [max_c1] x conv_dim
  float* x = nullptr;                                           // [frames][dim] f32 residual stream
  void* xt = nullptr; void* h = nullptr; void* attn = nullptr; void* ff = nullptr;
  void* q = nullptr; void* k = nullptr; void* vt = nullptr;
  float* logits = nullptr;                                      // [frames][vocab_pad]
};

// frames after every feature-encoder layer of a clip of n 16 kHz samples (0 once a layer has no complete window)
static int w2v_conv_frames(const tt_w2v_config& c, int n, int upto) {
  for (int i = 0; i <= upto; ++i) n = n >= c.conv_kernel[i] ? (n - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
  return n;
}

static int w2v_rownorm(tt_w2v* e, float* x, int M, int D, const float* g, const float* b, float eps, int act, void* out_t, float* out_f32,
                       hipStream_t s) {
  return rownorm_launch(e->cfg.dtype, layernorm_args(x, M, D, g, b, eps, act, out_t, out_f32, e->guard.dev), s);
}

static int w2v_forward(tt_w2v* e, const float* audio, int S, int* ids, float* logits_out, hipStream_t s) {
  const tt_w2v_config& c = e->cfg;
  const int dt = c.dtype, CD = c.conv_dim, D = c.dim, H = c.heads;
  const int n16 = resample_len(S);
  TT_TRY(w2v_resample_launch(audio, S, e->w.resample_taps, e->y16, e->partial, e->stats, e->guard.dev, s));
  int F = w2v_conv_frames(c, n16, 0);
  TT_TRY(w2v_conv0_launch(dt, e->y16, e->stats, F, c.conv_kernel[0], c.conv_stride[0], e->w.w_conv0, e->w.b_conv0, e->w.ln_conv_g[0],
                          e->w.ln_conv_b[0], e->ca, nullptr, e->guard.dev, s));
  void* cur = e->ca;
  for (int i = 1; i < TT_W2V_CONV_LAYERS; ++i) {
    const int k = c.conv_kernel[i], st = c.conv_stride[i];
    const int Fo = (F - k) / st + 1;
    // overlapping A rows: output row t reads rows st t .. st t + k - 1 of the previous layer = K = k * CD contiguous elements at st t * CD
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(cur, st * CD, e->w.w_conv[i], k * CD, Fo, CD, k * CD, e->w.b_conv[i], e->cf), s));
    void* nxt = cur == e->ca ? e->cb : e->ca;
    const bool last = i == TT_W2V_CONV_LAYERS - 1;
    // LayerNorm + GELU; the last layer's rows stay f32 (in place) for the feature projection's LayerNorm
    TT_TRY(w2v_rownorm(e, e->cf, Fo, CD, e->w.ln_conv_g[i], e->w.ln_conv_b[i], 1e-5f, ACT_GELU_ERF, last ? nullptr : nxt, last ? e->cf : nullptr, s));
    cur = nxt;
    F = Fo;
  }
  const int T = F;
  // feature projection: LayerNorm(conv_dim) -> Linear(conv_dim, dim)
  TT_TRY(w2v_rownorm(e, e->cf, T, CD, e->w.fp_ln_g, e->w.fp_ln_b, c.eps, ACT_NONE, cur, nullptr, s));
  TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(cur, CD, e->w.w_fp, CD, T, D, CD, e->w.b_fp, e->x), s));
  // positional convolution: h += GELU(conv_g(h) + b) per group g of cg channels, taps centred at pos_kernel / 2 = the reference's padding
  // pos_kernel / 2 with the last output frame dropped (Wav2Vec2SamePadLayer)
  TT_TRY(cast_pad_launch(dt, e->x, D, e->xt, D, T, D, D, s));
  const int cg = D / c.pos_groups, KP = c.pos_kernel * cg;
  for (int gi = 0; gi < c.pos_groups; ++gi) {
    GemmArgs g = gemm_args(offset_t(e->xt, (size_t)gi * cg, e->es), D, offset_t(e->w.w_pos, (size_t)gi * cg * KP, e->es), KP, T, cg, KP);
    g.taps = c.pos_kernel; g.seq_len = T;
    g.bias = e->w.b_pos + gi * cg; g.act = ACT_GELU_ERF; g.res = e->x + gi * cg; g.ldres = D; g.out_f32 = e->x + gi * cg; g.ldo32 = D;
    TT_TRY(gemm_launch(dt, EPI_STD, g, s));
  }
  // pre-LN encoder layers (Wav2Vec2EncoderLayerStableLayerNorm): h += out_proj(attn(LN1 h)); h += fc2(gelu(fc1(LN2 h))).  The steps -
  // the LayerNorm block, the head-split attention pair, the residual GEMM - are the ones of stage_blocks.h that xenc.h and the
  // AttentionBlocks use.  The loop itself is deliberately not shared with gpt2.hip gpt_trunk_full, which issues the same sequence: that
  // loop is causal, uses tanh-GELU, writes K / V into the handle's per-layer prefix cache, takes its buffers from tt_ar and builds its
  // argument blocks with gpt2.hip's own builders (their bytes are graph-key material) - a common loop would have to parameterise all of
  // that on the decode hot path.
  for (int l = 0; l < c.layers; ++l) {
    const tt_gpt_layer& w = e->L[l];
    TT_TRY(w2v_rownorm(e, e->x, T, D, w.ln1_g, w.ln1_b, c.eps, ACT_NONE, e->h, nullptr, s));
    TT_TRY(heads_attention(dt, e->h, w.w_qkv, w.b_qkv, e->q, e->k, e->vt, e->attn, 1, T, D, H, s));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_residual_args(e->attn, D, w.w_proj, D, T, D, D, w.b_proj, e->x, e->x), s));
    TT_TRY(w2v_rownorm(e, e->x, T, D, w.ln2_g, w.ln2_b, c.eps, ACT_NONE, e->h, nullptr, s));
    GemmArgs g = gemm_args(e->h, D, w.w_fc, D, T, c.ff_dim, D);
    g.bias = w.b_fc; g.act = ACT_GELU_ERF; g.out_t = e->ff; g.ldot = c.ff_dim;
    TT_TRY(gemm_launch(dt, EPI_STD, g, s));
    TT_TRY(gemm_launch(dt, EPI_STD, gemm_residual_args(e->ff, c.ff_dim, w.w_proj2, c.ff_dim, T, D, c.ff_dim, w.b_proj2, e->x, e->x), s));
  }
  // head: encoder.layer_norm -> lm_head -> argmax per frame
  TT_TRY(w2v_rownorm(e, e->x, T, D, e->w.lnf_g, e->w.lnf_b, c.eps, ACT_NONE, e->h, nullptr, s));
  TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->h, D, e->w.w_head, D, T, c.vocab_pad, D, e->w.b_head, e->logits), s));
  return w2v_argmax_launch(e->logits, c.vocab_pad, T, c.vocab, ids, logits_out, s);
}

extern "C" {

int tt_align_abi_version(void) { return 1; }  // ABI changes

size_t tt_align_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(tt_w2v_config);
    case 1: return sizeof(tt_w2v_weights);
  }
  return 0;
}

int tt_w2v_frames(const tt_w2v* e, int samples) {
  if (!e || samples < 1) return 0;
  return w2v_conv_frames(e->cfg, resample_len(samples), TT_W2V_CONV_LAYERS - 1);
}

int tt_w2v_create(const tt_w2v_config* cfg, const tt_w2v_weights* w, tt_w2v** out) {
  TT_REQUIRE(cfg && w && out, "tt_w2v_create: null argument");
  const tt_w2v_config& c = *cfg;
  TT_REQUIRE(c.dtype == DT_BF16 || c.dtype == DT_F16 || c.dtype == DT_F32, "tt_w2v_create: unknown dtype %d", c.dtype);
  TT_REQUIRE(c.heads * 64 == c.dim && c.dim % 128 == 0 && c.layers >= 1 && c.ff_dim % 64 == 0, "tt_w2v_create: unsupported dims (64-wide heads, dim a multiple of 128)");
  TT_REQUIRE(c.conv_dim == 512 && c.conv_kernel[0] == 10, "tt_w2v_create: the feature encoder is built for 512 channels and a first kernel of 10");
  for (int i = 1; i < TT_W2V_CONV_LAYERS; ++i)
    TT_REQUIRE(c.conv_kernel[i] >= 1 && c.conv_stride[i] >= 1 && c.conv_stride[i] <= c.conv_kernel[i] + 1, "tt_w2v_create: conv layer %d: kernel %d stride %d", i, c.conv_kernel[i], c.conv_stride[i]);
  TT_REQUIRE(c.conv_stride[0] >= 1 && c.pos_groups >= 1 && c.dim % c.pos_groups == 0 && (c.dim / c.pos_groups) % 64 == 0 && c.pos_kernel >= 2,
             "tt_w2v_create: positional conv of %d groups over %d channels (64-channel multiples per group)", c.pos_groups, c.dim);
  TT_REQUIRE(c.vocab >= 1 && c.vocab_pad >= c.vocab && c.vocab_pad % 64 == 0 && c.max_samples >= 1, "tt_w2v_create: bad vocab / capacity");
  TT_REQUIRE(w->resample_taps && w->w_conv0 && w->layers_host && w->w_head && w->w_pos && w->w_fp, "tt_w2v_create: null weight");
  tt_w2v* e = new tt_w2v();
  e->cfg = c;
  e->w = *w;
  e->L.assign(w->layers_host, w->layers_host + c.layers);
  e->es = dtype_bytes(c.dtype);
  const size_t es = e->es;
  const int n16 = resample_len(c.max_samples);
  e->max_c0 = std::max(w2v_conv_frames(c, n16, 0), 1);
  e->max_c1 = std::max(w2v_conv_frames(c, n16, 1), 1);
  e->max_frames = std::max(w2v_conv_frames(c, n16, TT_W2V_CONV_LAYERS - 1), 1);
  const size_t Tm = (size_t)round_up(e->max_frames, 64) + 64, D = c.dim, CD = c.conv_dim;
  int rc = e->open("tt_w2v_create", true);
  if (!rc) rc = e->arena.alloc_t(&e->y16, (size_t)n16 + 64);
  if (!rc) rc = e->arena.alloc_t(&e->partial, 2 * (size_t)resample_blocks(c.max_samples));
  if (!rc) rc = e->arena.alloc_t(&e->stats, 4);
  if (!rc) rc = e->arena.alloc(&e->ca, ((size_t)e->max_c0 + 64) * CD * es);
  if (!rc) rc = e->arena.alloc(&e->cb, ((size_t)e->max_c1 + 64) * CD * es);
  if (!rc) rc = e->arena.alloc_t(&e->cf, ((size_t)e->max_c1 + 64) * CD);
  if (!rc) rc = e->arena.alloc_t(&e->x, Tm * D);
  if (!rc) rc = e->arena.alloc(&e->xt, Tm * D * es);
  if (!rc) rc = e->arena.alloc(&e->h, Tm * D * es);
  if (!rc) rc = e->arena.alloc(&e->attn, Tm * D * es);
  if (!rc) rc = e->arena.alloc(&e->ff, Tm * c.ff_dim * es);
  if (!rc) rc = e->arena.alloc(&e->q, Tm * D * es);
  if (!rc) rc = e->arena.alloc(&e->k, Tm * D * es);
  if (!rc) rc = e->arena.alloc(&e->vt, Tm * D * es);
  if (!rc) rc = e->arena.alloc_t(&e->logits, Tm * c.vocab_pad);
  if (rc) {
    tt_w2v_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_w2v_destroy(tt_w2v* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_w2v_run(tt_w2v* e, const float* audio, int samples, int* frame_ids, float* logits, void* stream) {
  TT_REQUIRE(e && audio && frame_ids, "tt_w2v_run: null argument");
  TT_REQUIRE(samples >= 1 && samples <= e->cfg.max_samples, "tt_w2v_run: %d samples (1 .. %d)", samples, e->cfg.max_samples);
  TT_REQUIRE(tt_w2v_frames(e, samples) >= 1, "tt_w2v_run: a clip of %d samples is shorter than the model's receptive field", samples);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_TRY(w2v_forward(e, audio, samples, frame_ids, logits, s));
    return e->guard.snapshot(s);
  });
}

int tt_w2v_guard(tt_w2v* e, int reset) {
  if (!e) { set_error("tt_w2v_guard: null handle"); return -1; }
  return e->read_guard(reset, "tt_w2v_guard", "aligner", e->cfg.dtype);
}

// ------------------------------------------------------------------------------ operator-level test entries (tortoise_mi355x_test.h)
size_t tt_op_w2v_resample_workspace(int S) { return 2 * sizeof(double) * (size_t)resample_blocks(S > 0 ? S : 1); }

int tt_op_w2v_resample(const float* x, int S, const float* taps, float* y, float* stats, void* workspace, void* stream) {
  return w2v_resample_launch(x, S, taps, y, (double*)workspace, stats, nullptr, (hipStream_t)stream);
}

int tt_op_w2v_conv0(int dtype, const float* y, const float* stats, int frames, int k, int stride, const float* w, const float* b, const float* g,
                    const float* beta, void* out_t, float* out_f32, void* stream) {
  return w2v_conv0_launch(dtype, y, stats, frames, k, stride, w, b, g, beta, out_t, out_f32, nullptr, (hipStream_t)stream);
}

int tt_op_w2v_argmax(const float* logits, int ld, int T, int V, int* ids, float* out, void* stream) {
  return w2v_argmax_launch(logits, ld, T, V, ids, out, (hipStream_t)stream);
}

}  // extern "C"
