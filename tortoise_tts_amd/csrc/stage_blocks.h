// The launch sequences the model stages (xenc.h, clvp / cvvp / cond / align / classify / diffusion .hip) are assembled from, each written
// once: the norm argument blocks, the head-split attention pair, the reference's AttentionBlock, the GEMM epilogue field sets that recur,
// the stride-2 convolution front of the clip encoders and the pooled-latent tail of the ranking towers.  Host code only: every block
// issues engine launches (ops.h) in the token-major layout and owns no kernel.  gpt2.hip keeps its own builders (its argument bytes are
// graph-key material).
#pragma once
#include "runtime.h"
#include "../../include/tortoise_mi355x.h"

namespace tt {

// ------------------------------------------------------------------------------ norm argument blocks
// Every field the builders do not name stays zero.  Both output strides are always set; a launch ignores the stride of an output whose
// pointer is null.  Dense rows: x [M][D] f32 -> out_t [M][D] T and / or out_f32 [M][D].
static inline RowNormArgs rownorm_args(int mode, float* x, int M, int D, const float* g, const float* b, float eps, int act, void* out_t,
                                       float* out_f32, int* guard) {
  RowNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ldx = D; a.M = M; a.D = D; a.mode = mode; a.g1 = g; a.b1 = b; a.eps1 = eps; a.act = act;
  a.out_t = out_t; a.ldot = D; a.out_f32 = out_f32; a.ldo32 = D;
  a.guard = guard;
  return a;
}
static inline RowNormArgs layernorm_args(float* x, int M, int D, const float* g, const float* b, float eps, int act, void* out_t, float* out_f32,
                                         int* guard) {
  return rownorm_args(NORM_LAYER, x, M, D, g, b, eps, act, out_t, out_f32, guard);
}
static inline RowNormArgs rmsnorm_args(float* x, int M, int D, const float* g, float eps, void* out_t, int* guard) {
  return rownorm_args(NORM_RMS, x, M, D, g, nullptr, eps, ACT_NONE, out_t, nullptr, guard);
}
// GroupNorm32 over B samples of S rows: x [B][S][C] f32 -> out_t [B][S][C] T and / or out_f32; partial = the statistics workspace
static inline GroupNormArgs groupnorm_args(const float* x, int B, int S, int C, const float* g, const float* b, float eps, int act, void* out_t,
                                           float* out_f32, float* partial, int* guard) {
  GroupNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.B = B; a.S = S; a.C = C; a.gamma = g; a.beta = b; a.eps = eps; a.act = act;
  a.out_t = out_t; a.ldot = C; a.out_f32 = out_f32; a.ldo32 = C; a.partial = partial;
  a.guard = guard;
  return a;
}

// ------------------------------------------------------------------------------ GEMM epilogue field sets on top of gemm_args
// out[M][N] f32 = res + A W^T + bias (res == out: the residual stream updated in place)
static inline GemmArgs gemm_residual_args(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* res,
                                          float* out) {
  GemmArgs g = gemm_args(A, lda, W, ldw, M, N, K);
  g.bias = bias; g.res = res; g.ldres = N; g.out_f32 = out; g.ldo32 = N;
  return g;
}
// out[M][N] f32 = A W^T + bias (bias may be null)
static inline GemmArgs gemm_f32_args(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, float* out) {
  GemmArgs g = gemm_args(A, lda, W, ldw, M, N, K);
  g.bias = bias; g.out_f32 = out; g.ldo32 = N;
  return g;
}
// A `taps`-tap convolution over sequences of seq_len rows (A [M][cin], W [N][taps][cin]) + bias; the caller names the output
static inline GemmArgs gemm_conv_args(const void* A, int cin, const void* W, int taps, int M, int seq_len, int N, const float* bias) {
  GemmArgs g = gemm_args(A, cin, W, taps * cin, M, N, taps * cin);
  g.taps = taps; g.seq_len = seq_len; g.bias = bias;
  return g;
}

// ------------------------------------------------------------------------------ attention
// The optional parts of heads_attention.
struct HeadsAttnOpts {
  const float* relpos = nullptr;    // [H][129] additive relative-position bias (FlashArgs::relpos)
  const float* inv_freq = nullptr;  // x-transformers rotary on the first rot_dim dims of q, k and v, between the two launches
  int rot_dim = 0;
  int nv_period = 0;                // padded batch: batch row b has nv[b % nv_period] valid rows (FlashArgs::nv)
  const int* nv = nullptr;
};
// softmax(q k^T / 8) v over B sequences of n rows with H heads of 64: h [B n][D] T (the normalised rows) -> out [B n][D] T.  The QKV
// projection's epilogue scatters q (scaled by 1/8: (q 64^-1/4) . (k 64^-1/4)), k and v^T into the flash layouts q / k / vt.
static inline int heads_attention(int dt, const void* h, const void* w_qkv, const float* b_qkv, void* q, void* k, void* vt, void* out, int B, int n,
                                  int D, int H, hipStream_t s, const HeadsAttnOpts& o = HeadsAttnOpts()) {
  const int n_pad = round_up(n, 32);
  GemmArgs g = gemm_args(h, D, w_qkv, D, B * n, 3 * D, D);
  g.bias = b_qkv; g.seq_len = n; g.dmodel = D; g.heads = H; g.q = q; g.k = k; g.vt = vt; g.seq_pad = n_pad; g.q_scale = 0.125f;
  TT_TRY(gemm_launch(dt, EPI_QKV_HEADS, g, s));
  if (o.inv_freq) TT_TRY(rotary_launch(dt, q, k, vt, o.inv_freq, B * H, n, n_pad, o.rot_dim, s));
  FlashArgs f;
  memset(&f, 0, sizeof(f));
  f.q = q; f.k = k; f.vt = vt; f.out = out; f.ldo = D; f.BH = B * H; f.heads = H; f.n = n; f.n_pad = n_pad;
  f.relpos = o.relpos;
  f.nv_period = o.nv_period;
  for (int u = 0; u < o.nv_period; ++u) f.nv[u] = o.nv[u];
  return flash_attention_launch(dt, f, s);
}

// Work buffers of attention_block: act / att [B n][C] T, q / k / vt the flash layouts, the GroupNorm partials, the stage's guard or null
struct AttnBlockBufs {
  void* act; void* q; void* k; void* vt; void* att;
  float* gn_partial;
  int* guard;
};
// AttentionBlock (arch_util.py:80-123) with 64-wide heads: out = in + proj(attn(qkv(GroupNorm32(in)))), token-major [B][n][C], one GroupNorm
// sample per sequence.  (The denoiser keeps its own norm and projection around heads_attention: diffusion.hip run_attn_block.)
static inline int attention_block(int dt, const tt_attn_block& w, const float* in, float* out, int B, int n, int C, int H, const AttnBlockBufs& b,
                                  hipStream_t s) {
  TT_TRY(groupnorm_launch(dt, groupnorm_args(in, B, n, C, w.norm_g, w.norm_b, 1e-5f, ACT_NONE, b.act, nullptr, b.gn_partial, b.guard), s));
  HeadsAttnOpts o;
  o.relpos = w.relpos;
  TT_TRY(heads_attention(dt, b.act, w.w_qkv, w.b_qkv, b.q, b.k, b.vt, b.att, B, n, C, H, s, o));
  return gemm_launch(dt, EPI_STD, gemm_residual_args(b.att, C, w.w_proj, C, B * n, C, C, w.b_proj, in, out), s);
}

// ------------------------------------------------------------------------------ the clip encoders' front
// A clip's mel [mc][T] f32 channels-first -> mel_t [T][mc] f32 -> mel_op [T][mp] T, the zero-padded operand rows of the first convolution
static inline int mel_operand(int dt, const float* mel, int mc, int mp, int T, float* mel_t, void* mel_op, hipStream_t s) {
  TT_TRY(transpose_launch(mel, mel_t, mc, T, s));
  return cast_pad_launch(dt, mel_t, mc, mel_op, mp, T, mc, mp, s);
}
// Conv1d(cin -> N, `taps` taps, stride 2, "same" padding) over T rows = the stride-1 tap GEMM at every position into `full`, then its
// even rows (even_idx[i] = 2 i, even_rows_index_launch at create) into `even`: ceil(T / 2) rows.  f32_out: both are f32 rows, else T rows,
// gathered as 4-byte words.
static inline int conv_stride2(int dt, const void* A, int cin, const void* W, int taps, int T, int N, const float* bias, void* full, void* even,
                               bool f32_out, const int* even_idx, hipStream_t s) {
  GemmArgs g = gemm_conv_args(A, cin, W, taps, T, T, N, bias);
  if (f32_out) { g.out_f32 = (float*)full; g.ldo32 = N; }
  else { g.out_t = full; g.ldot = N; }
  TT_TRY(gemm_launch(dt, EPI_STD, g, s));
  return gather_rows_launch((const float*)full, even_idx, (float*)even, (T + 1) / 2, f32_out ? N : N * dtype_bytes(dt) / 4, s);
}

// ------------------------------------------------------------------------------ the ranking towers' tail
// enc [B][n][D] f32 -> mean over the n rows -> latent [B][LD] f32 = pooled W^T (no bias); pooled / pooled_t: [B][D] f32 / T work rows
static inline int pooled_latent(int dt, const float* enc, int B, int n, int D, const void* w_latent, int LD, float* pooled, void* pooled_t,
                                float* latent, hipStream_t s) {
  TT_TRY(mean_rows_launch(enc, pooled, B, n, D, s));
  TT_TRY(cast_pad_launch(dt, pooled, D, pooled_t, D, B, D, D, s));
  return gemm_launch(dt, EPI_STD, gemm_f32_args(pooled_t, D, w_latent, D, B, LD, D, nullptr, latent), s);
}

}  // namespace tt
