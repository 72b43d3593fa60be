/* tortoise_mi355x_test.h - operator-level TEST entry points and A/B diagnostics of libtortoise_mi355x.so.
 *
 * NOT part of the drop-in boundary (include/tortoise_mi355x.h is what a maintainer binds): tests/ calls single kernels through these to
 * hold them against torch references, scripts/ uses the ttx_* switch for in-situ A/B runs.  Same conventions as the product header
 * (0 / negative return codes, device pointers, hipStream_t as void*).  Symbols here may change without an ABI version bump.
 */
#ifndef TORTOISE_MI355X_TEST_H
#define TORTOISE_MI355X_TEST_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Process-wide A/B switch of a kernel family; returns the previous value.  Set it before an engine captures its graphs.
 *   TTX_FLASH32   1 (default) = 32-query waves on v_mfma_f32_32x32x16 for non-causal sequences of more than 128 rows, 0 = 16-query waves
 *   TTX_GEMM_P8   1 (default) = the 8-wave eight-phase 256 x 256 tile (csrc/gemm_p8.h) where it applies, 0 = the 16-wave two-stage tile
 *                 (bit-identical results)
 *   TTX_VOC_MFMA  1 (default) = UnivNet's dilated 32 -> 32 convolutions and location-variable convolutions (hop 64 / 256) on
 *                 v_mfma_f32_32x32x2_f32 (exact f32), 0 = the thread-per-sample VALU kernels
 *   TTX_GEMM_SKINNY 1 (default) = 32 x 16 / 64 x 16 tiles for the weight-streaming GEMMs of decode batches of <= 64 rows, 0 = 64 x 64 tiles
 *                 (bit-identical results)
 *   TTX_AR_GEMV   a level: autoregressive handles created with max_batch <= 4 (the streaming engine) run the decode step's GEMMs
 *                 2 (default) = GEMV-shaped with the layer norms inside the QKV / c_fc launches (csrc/gemv.hip: five launches per layer),
 *                 1 = GEMV-shaped behind row-norm launches of their own (seven), 0 = on the MFMA tiles.  Read at tt_ar_create.
 *   TTX_NR_SELECT_LONG 0 (default) = the denoiser's noise-floor select keeps a row of up to TT_NR_REG_FRAMES frames in registers, 1 = it
 *                 re-reads the row every round whatever its length, the form of longer clips (bit-identical results) */
#define TTX_FLASH32 0
#define TTX_GEMM_P8 1
#define TTX_VOC_MFMA 2
#define TTX_GEMM_SKINNY 3
#define TTX_AR_GEMV 4
#define TTX_NR_SELECT_LONG 5
int ttx_kernel_variant(int which, int v);

/* ============================================================================================
 * Operator-level entry points (used by tests/ to check single kernels against torch references)
 * ============================================================================================ */
int tt_op_gemm(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int taps, int seq_len,
               int splitk, const float* bias, int act, const float* res, float* out_f32, void* out_t, void* stream);
/* tap convolution over seq_len-row slots with per-sequence valid lengths (the ragged HiFi-GAN batch, include/tortoise_mi355x_hifi.h):
 * slot b = rows b * seq_len .. holds seq_vlen[b] (DEVICE int) valid rows; taps past them or before the slot read zero; tap t reads row
 * s + (t - taps / 2) * dilation; M may end inside the last slot.  Same epilogue arguments as tt_op_gemm; 16-bit operand types. */
int tt_op_gemm_segv(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int taps, int dilation, int seq_len,
                    const int* seq_vlen, const float* bias, int act, const float* res, float* out_f32, void* out_t, void* stream);
/* Every GEMM form in one entry: the fields of csrc/gemm.h GemmArgs that a caller sets (same meanings; a zero leading dimension of an output
 * or of the skip means N, seq_len 0 means M, q_scale 0 means 1).  tt_op_gemm_ex(dtype, epi, d, ran, stream): epi 0 standard, 1 QKV heads, 2 QKV decode, 3 GEGLU;
 * the problem goes to the product dispatch unchanged.  ran (optional, int[4]) receives what actually launched, recorded on the host by the
 * launch path: {tile (0 64x64, 1 128x64, 2 128x128, 3 256x256, 4 32x16, 5 64x16), standard-epilogue variant after any fallback to the
 * generic kernel (0 GEN, 1 NONE, 2 SLAB, 3 GELU_T, 4 ST_F32, 5 ST_RES, 6 ST_A2, 7 BIAS_T, 8 SERIAL; -1 another epilogue), eight-phase
 * 256 x 256 kernel (0 / 1), shared-halo 3-tap kernel (0 / 1)}. */
typedef struct tt_op_gemm_desc {
  const void* A;
  const void* W;
  const void* A2;        /* k >= k_split reads A2[m][k - k_split]; a2_slot (DEVICE int, optional) offsets A2 by *a2_slot * a2_slot_stride */
  const int* a2_slot;
  size_t a2_slot_stride;
  int lda, ldw, lda2, k_split;
  int M, N, K, taps, dilation, seq_len, splitk, serial_k;
  const int* seq_vlen;   /* DEVICE int per sequence (tap convolutions over ragged slots) */
  const float* bias;
  const float* res;
  float* out_f32;
  void* out_t;
  int act, ldres, ldo32, ldot;
  float slope;
  int act_t;
  float slope_t;
  float* gn_part;        /* GroupNorm statistics partials [row_tile][2][N / 16][2] */
  int gn_seq, gn_vperiod;
  int gn_vlen[32];
  int dmodel, heads, seq_pad, tmax;
  float q_scale;
  void* q;
  void* k;
  void* v;
  void* vt;
  const int* step;       /* DEVICE int: the KV slot EPI_QKV_DECODE writes */
  void* qbuf;
  void* kc;
  void* vc;
} tt_op_gemm_desc;
size_t tt_op_gemm_desc_size(void);
int tt_op_gemm_ex(int dtype, int epi, const tt_op_gemm_desc* d, int* ran, void* stream);
/* rows per statistics tile of the kernel tt_op_gemm_ex would pick for d (the part_rows its consumer needs) */
int tt_op_gemm_stat_rows(int dtype, const tt_op_gemm_desc* d);
/* GroupNorm32 apply on statistics a GEMM epilogue left (gemm_part of part_rows-row tiles; the path of the denoiser's GroupNorms): x f32
 * [B][S][C]; vperiod > 0: sample b has vlen[b % vperiod] valid rows (host ints), the rest are left out of the statistics and written as
 * zeros (1 <= vlen[i] <= S).  Same outputs as tt_op_groupnorm. */
int tt_op_groupnorm_part(int dtype, const float* x, int B, int S, int C, const float* g, const float* b, const float* scale_shift, int act,
                         const float* gemm_part, int part_rows, int vperiod, const int* vlen, void* out_t, float* out_f32, float* workspace,
                         void* stream);
/* Every row-norm form in one entry: the fields of csrc/ops.h RowNormArgs that a caller sets, with the same meanings and no defaults (every
 * leading dimension is given; mode 0 none, 1 LayerNorm, 2 RMSNorm).  tt_op_rownorm_ex(dtype, d, ran, stream) passes the problem to the product
 * dispatch unchanged.  ran (optional, int[4]) receives what launched, recorded on the host by the launch path: {kernel (0 generic, 1 narrow,
 * 2 wave), compiled slab count of the narrow kernel or -1 (a run-time loop), BIAS, RMS (the narrow kernel's template arguments; the other
 * kernels: add_bias set, mode == 2)}. */
typedef struct tt_op_rownorm_desc {
  float* x;                /* [M][ldx] f32 rows (read unless x_in; written when write_x) */
  int ldx;
  const float* x_in;       /* optional separate source rows [M][ldxin] */
  int ldxin;
  int M, D;
  const float* add_bias;   /* [D] */
  const float* add_slabs;  /* [nslab][M][ldslab], slab_stride floats apart */
  int nslab;
  size_t slab_stride;
  int ldslab;
  int write_x;
  int mode;
  const float* g1;
  const float* b1;
  float eps1;
  const float* g2;         /* optional second LayerNorm on the first one's output */
  const float* b2;
  float eps2;
  void* out_t;
  int ldot;
  float* out_f32;
  int ldo32;
  const int* f32_slot;     /* DEVICE int: the f32 copy goes to out_f32 + (*f32_slot + f32_slot_base) * f32_slot_stride */
  int f32_slot_base;
  size_t f32_slot_stride;
  const int* f32_row_slot; /* DEVICE int [M]: row r files its f32 copy under f32_row_slot[r] (+ f32_slot_base); negative: nothing filed */
  int row_blocks;
  int* guard;              /* DEVICE counter of rows with a non-finite value */
  int act;
} tt_op_rownorm_desc;
size_t tt_op_rownorm_desc_size(void);
int tt_op_rownorm_ex(int dtype, const tt_op_rownorm_desc* d, int* ran, void* stream);
/* Every GroupNorm32 form in one entry: the caller-set fields of csrc/ops.h GroupNormArgs (x f32 [B][S][C]; partial = a workspace of
 * tt_op_groupnorm_workspace(B, S) bytes; gemm_part / part_rows = statistics a GEMM epilogue left; vperiod > 0: sample b has
 * vlen[b % vperiod] valid rows, the rest are left out of the statistics and written as zeros).  ran (optional, int[4]): {stand-alone
 * statistics pass ran (0 / 1), apply kernel (0 generic, 1 the C = 1024 kernel), rows per apply block, fused-statistics template of the
 * C = 1024 kernel (0 / 1)}. */
typedef struct tt_op_groupnorm_desc {
  const float* x;
  int B, S, C;
  const float* gamma;
  const float* beta;
  float eps;
  const float* scale_shift;  /* optional: y = y * (1 + scale) + shift, block b / ss_batch_div of [..][2C], ss_batch_stride floats apart (0: shared) */
  size_t ss_batch_stride;
  int ss_batch_div;
  int act;
  void* out_t;
  int ldot;
  float* out_f32;
  int ldo32;
  float* partial;
  const float* gemm_part;
  int part_rows;
  int vperiod;
  int vlen[32];
  int* guard;                /* DEVICE counter of (workgroup, group) pairs with non-finite statistics */
} tt_op_groupnorm_desc;
size_t tt_op_groupnorm_desc_size(void);
int tt_op_groupnorm_ex(int dtype, const tt_op_groupnorm_desc* d, int* ran, void* stream);
int tt_op_layernorm(int dtype, const float* x, int M, int D, const float* g, const float* b, float eps, int rms,
                    void* out_t, float* out_f32, void* stream);
int tt_op_groupnorm(int dtype, const float* x, int B, int S, int C, const float* g, const float* b, const float* scale_shift,
                    int act, void* out_t, float* out_f32, float* workspace, void* stream);
size_t tt_op_groupnorm_workspace(int B, int S);
/* the fused ResBlock in_layers launch (TT_DIFF_OPT_FUSED_GN; diffusion_decoder.py:60-80): out_f32[B*S][N] = W . act(GroupNorm32(x)) + bias,
 * x f32 [B][S][1024] token-major, act = 3 (SiLU); 256 < B*S <= 4096, S >= 32, N % 256 == 0, 16-bit operand types */
int tt_op_gn_gemm(int dtype, const float* x, int B, int S, const float* gamma, const float* beta, int act, const void* W,
                  const float* bias, int N, float* out_f32, float* workspace, void* stream);
size_t tt_op_gn_gemm_workspace(int B, int S);
/* flash attention (csrc/ops.h FlashArgs): q T [B * heads][n][64] pre-scaled, k T [B * heads][n][64], vt T [B * heads][64][n_pad] (V transposed;
 * n_pad a multiple of 32 covering n), relpos f32 [heads][129] or NULL, out T [B][n][heads * 64].  Columns n .. n_pad of vt must hold FINITE
 * values: the kernels load them (clamped to n_pad - 8) and multiply them by numerators that are exact zeros, so any finite value leaves the
 * output untouched and a NaN or an infinity would reach it.  The engine's V^T buffers are zeroed when they are made and afterwards hold nothing
 * but V values of the QKV epilogue (an earlier pass's where another n_pad moved the layout), so there the columns are finite as long as V is. */
int tt_op_flash_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int heads, int n, int n_pad,
                          int causal, const float* relpos, void* stream);
/* the same with padded batch rows and the kernel choice exposed: batch row b attends to (and computes) its first nv[b % nv_period] rows only
 * (nv: HOST int [nv_period], nv_period <= 32, every entry in 1 .. n; NULL / 0: all n rows); rows of out beyond them are not written.
 * variant 0 = chosen from the shape, 1 = never the key-split form, 2 = never the 32-query-wave kernel. */
int tt_op_flash_attention_rows(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int heads, int n, int n_pad,
                               int causal, const float* relpos, const int* nv, int nv_period, int variant, void* stream);
/* what the last flash-attention launch of the calling thread started, recorded on the host by the launch path: ran = {kernel (0 flash_kernel,
 * 1 flash_lds_kernel, 2 flash32_kernel, 3 the fp32 verification kernel; -1 before the first launch), NQ (16-query blocks per wave: the template
 * argument, 2 for flash32_kernel, 0 for the fp32 kernel), KS (key halves per staged tile: the template argument, 0 where there is none)} */
int tt_op_flash_ran(int ran[3]);
/* the decode step's attention (HF GPT2Attention under tortoise/models/autoregressive.py:150-163, one query per (sequence, head)):
 * q T [B][heads * 64] pre-scaled by 1/8; shared prefix kp, vp T [heads][P1][64]; per-sequence caches kc T [B][heads][8][tmax][8]
 * (key-major 16-byte chunks), vc T [B][heads][tmax][64] with own keys 0 .. tgen - 1 valid; out T [B][heads * 64].
 * variant 0 = chosen from the shape, 1 = per-wave prefix kernel, 2 / 3 = shared-prefix kernel with 16 / 4 sequences per workgroup */
int tt_op_decode_attention(int dtype, const void* q, const void* kp, const void* vp, int P1, const void* kc, const void* vc, int tmax,
                           int tgen, void* out, int B, int heads, int variant, void* stream);
/* the decode step's QKV projection and attention in ONE launch (TT_AR_OPT_FUSED_QKV_ATTN; csrc/decode_attention.hip decode_qkv_attn_kernel):
 * h T [B][1024] the LN1 rows, w_qkv T [3072][1024], b_qkv f32 [3072] or NULL.  Own keys 0 .. tgen - 2 are in kc / vc (layouts above); the
 * launch writes slot tgen - 1 of both from h w_qkv^T + b_qkv (the bits of the EPI_QKV_DECODE GEMM), attends [prefix | own keys
 * 0 .. tgen - 1] and writes out T [B][1024]; q_out T [B][1024] (or NULL) receives the scaled query rows.  16 heads, B % 16 == 0,
 * 16-bit operand types; the prefix, the score rows and the activation rows must fit the LDS.  Slots >= tgen - 1 of the caches may hold
 * anything on entry (NaN included): nothing of them reaches the outputs. */
int tt_op_decode_qkv_attention(int dtype, const void* h, const void* w_qkv, const float* b_qkv, float q_scale, const void* kp, const void* vp,
                               int P1, void* kc, void* vc, int tmax, int tgen, void* q_out, void* out, int B, int heads, void* stream);
/* the decode attention of a session handle (TT_AR_OPT_SESSIONS): row b attends its own prefix kp / vp + b * prefix_stride elements
 * ([heads][p1_rows[b]][64]) and its own keys 0 .. slot_rows[b]; a negative slot skips the row (its output is not written).  p1_rows and
 * slot_rows are DEVICE int [B]; p1_cap >= every p1_rows[b] sizes the LDS. */
int tt_op_decode_attention_rows(int dtype, const void* q, const void* kp, const void* vp, long long prefix_stride, const int* p1_rows, int p1_cap,
                                const void* kc, const void* vc, int tmax, const int* slot_rows, void* out, int B, int heads, void* stream);
/* GEMV-shaped decode GEMM (csrc/gemv.hip): A T [M][K], W T [N][K], M <= 16, K in {1024, 2048, 4096}, N % 4 == 0;
 * epi 0: out_f32 [M][N] = A W^T + bias; 1: out_f32 += A W^T + bias (residual rows, in place); 2: out_t T [M][N] = gelu_tanh(A W^T + bias) */
int tt_op_gemv(int dtype, const void* A, const void* W, int M, int N, int K, const float* bias, int epi, float* out_f32, void* out_t, void* stream);
/* out_t[M][N] = gelu_tanh(LayerNorm(x[M][1024] f32; g, b, eps) W^T + bias): the same kernel with the layer norm inside */
int tt_op_gemv_ln(int dtype, const float* x, const float* g, const float* b, float eps, const void* W, int M, int N, const float* bias, void* out_t, void* stream);
int tt_op_sample(const float* logits, int ldl, int B, int V, unsigned* seen, const tt_sampling* s, int step, int* unfinished,
                 int stop_token, int* codes, int ldcodes, void* stream);
/* The typical-sampling mask alone (csrc/sampling.hip typical_mask_kernel; reference tortoise/utils/typical_sampling.py:11-33): out f32 [B][ldl]
 * = logits with every token outside the typical set of mass `mass` at -inf; the set is formed on the repetition-penalised scores (seen:
 * [B][(V+31)/32] bit mask of the ids generated so far), kept tokens carry their raw logit. */
int tt_op_typical_mask(const float* logits, int ldl, int B, int V, const unsigned* seen, float repetition_penalty, float mass, float* out,
                       void* stream);
int tt_op_conv1d(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int T, int k, int dilation,
                 int reflect, float in_slope, int out_act, float out_slope, void* stream);
int tt_op_convt1d(const float* x, const float* w, const float* bias, float* y, int C, int Tin, int stride, float in_slope, void* stream);
/* location-variable convolution + gate (vocoder.py:182-216, 178-179); kernels [L][ldk] in the operand type `dtype` (TT_F32: float) */
int tt_op_lvc(int dtype, const float* x_in, const void* kernels, int ldk, int koff, const float* bias, int ldb, int boff, float* x, int L,
              int hop, void* stream);
/* The three audio-rate UnivNet launches with every argument: the caller-set fields of csrc/ops.h Conv1dArgs, ConvT1dArgs and LvcArgs with the
 * same meanings; the problem goes to conv1d_direct_launch / convt1d_launch / lvc_launch unchanged.  seq_n, seq_mul, seq_frames are the ragged
 * batch (VocSeqs; include/tortoise_mi355x_univnet.h): seq_n = 0 is one sequence that fills the tensor; seq_n = 1 .. 32 sequences own slot b of
 * every tensor ([C][P], P = T / Tin / L * hop columns; Tin * stride for the transposed convolution's output) and their first
 * seq_frames[b] * seq_mul columns are valid (the LVC: seq_frames[b] frames of hop columns, seq_mul unused; its kernel and bias rows are
 * b * L + l).  in_slope >= 0 applies LeakyReLU to the input, negative none; out_act 0 none, 4 LeakyReLU(out_slope), 5 tanh.  With reflect set
 * every sequence must be longer than (k / 2) * dilation columns: the launcher refuses anything shorter.  ran (optional, int[4]) receives what
 * launched, recorded on the host by the launch path ({-1, 0, 0, 0} when the launcher refused the problem):
 *   conv1d   {kernel (0 conv1d_direct_kernel<32>, 1 conv1d_direct_kernel<1>, 2 conv1d_mfma_kernel), grid.x, grid.y, 0}
 *   convt1d  {0, grid.x, grid.y, grid.z}
 *   lvc      {kernel (0 lvc_kernel, 1 lvc_mfma_kernel), HOP template argument, kernel element type (0 f32, 1 bf16, 2 f16), 0} */
typedef struct tt_op_conv1d_desc {
  const float* x;        /* [Cin][T] */
  const float* w;        /* [Cout][Cin][k] */
  const float* bias;     /* [Cout] or NULL */
  float* y;              /* [Cout][T] */
  int Cin, Cout, T, k, dilation;
  int seq_n, seq_mul;
  int seq_frames[32];
  int reflect;
  float in_slope;
  int out_act;
  float out_slope;
} tt_op_conv1d_desc;
size_t tt_op_conv1d_desc_size(void);
int tt_op_conv1d_ex(const tt_op_conv1d_desc* d, int* ran, void* stream);
typedef struct tt_op_convt1d_desc {
  const float* x;        /* [C][Tin] */
  const float* w;        /* [C][C][2 * stride] */
  const float* bias;     /* [C] */
  float* y;              /* [C][Tin * stride] */
  int C, Tin, stride;
  float in_slope;
  int seq_n, seq_mul;
  int seq_frames[32];
} tt_op_convt1d_desc;
size_t tt_op_convt1d_desc_size(void);
int tt_op_convt1d_ex(const tt_op_convt1d_desc* d, int* ran, void* stream);
typedef struct tt_op_lvc_desc {
  const float* x_in;     /* [32][L * hop] */
  const void* kernels;   /* [L][ldk] in the type dtype (TT_BF16 / TT_F16 / TT_F32), the [32][64][3] block at column koff */
  int ldk, koff, dtype;
  const float* bias;     /* [L][ldb], the [64] block at column boff */
  int ldb, boff;
  float* x;              /* [32][L * hop], updated in place */
  int L, hop;
  int seq_n, seq_mul;
  int seq_frames[32];
  float in_slope;
  int* guard;            /* DEVICE counter of waves that staged a non-finite kernel value, or NULL */
} tt_op_lvc_desc;
size_t tt_op_lvc_desc_size(void);
int tt_op_lvc_ex(const tt_op_lvc_desc* d, int* ran, void* stream);

/* wav2vec2 aligner front (csrc/align.hip, include/tortoise_mi355x_align.h).  Resampler: y f32 [ceil(2 S / 3)] = torchaudio's 24 -> 16 kHz
 * resample of x f32 [S] with taps f32 [2][23]; stats f32 [2] = {mean, 1 / sqrt(unbiased var + 1e-7)} of y; workspace of
 * tt_op_w2v_resample_workspace(S) bytes. */
size_t tt_op_w2v_resample_workspace(int S);
int tt_op_w2v_resample(const float* x, int S, const float* taps, float* y, float* stats, void* workspace, void* stream);
/* feature-encoder layer 0: out [frames][512] = GELU(LayerNorm(Conv1d(1, 512, k, stride)((y - stats[0]) * stats[1]) + b; g, beta, 1e-5));
 * w f32 [512][k] (k = 10); out_t in the operand type `dtype`, out_f32 optional */
int tt_op_w2v_conv0(int dtype, const float* y, const float* stats, int frames, int k, int stride, const float* w, const float* b, const float* g,
                    const float* beta, void* out_t, float* out_f32, void* stream);
/* row LayerNorm followed by an activation (ACT_* code) in one launch: out = act(LayerNorm(x[M][D]; g, b, eps)) */
int tt_op_layernorm_act(int dtype, const float* x, int M, int D, const float* g, const float* b, float eps, int act, void* out_t, float* out_f32,
                        void* stream);
/* ids int32 [T] = per-row argmax of logits f32 [T][ld] over the first V columns (ties: lowest index); out (optional) f32 [T][V] gets the rows */
int tt_op_w2v_argmax(const float* logits, int ld, int T, int V, int* ids, float* out, void* stream);

/* Tortoise detector kernels (csrc/classify.hip, include/tortoise_mi355x_classify.h).  Statistics partials: `part` workspaces of
 * tt_op_cls_workspace(L) bytes, [block][16][2] sum / sum of squares in double.  init: out f32 [n][32] = Conv1d(1, 32, 3, pad 1)(x f32 [n]),
 * w f32 [32][3]; stats: f32 [16][2] = {mean, 1 / sqrt(var + 1e-5)} of the 16 groups of a [L][C] tensor from the partials of `nblocks`
 * workgroups; conv: out f32 [Lout][cout] = Conv1d(cin, cout, 5, stride, pad 2)(stride 1: SiLU(GroupNorm16(x; stats, gamma, beta)), stride 4: x)
 * + b (+ res), w in the operand type [cout][5][cin], partials of out when part != NULL (cout <= 64); attention: out [nq][512] (operand
 * type) = QKVAttentionLegacy(4 heads of 128) of qkv f32 [n][1536] for the first nq queries; head: logits f32 [2] = w f32 [2][512] x[0] + b,
 * emb (optional) f32 [512] = x[0] */
size_t tt_op_cls_workspace(int L);
int tt_op_cls_init(const float* x, int n, const float* w, const float* b, float* out, void* part, void* stream);
int tt_op_cls_stats(const void* part, int nblocks, int L, int C, float* stats, void* stream);
int tt_op_cls_conv(int dtype, int cin, int cout, int stride, const float* x, int Lin, const float* stats, const float* gamma, const float* beta,
                   const void* w, const float* b, const float* res, float* out, void* part, void* stream);
int tt_op_cls_attention(int dtype, const float* qkv, int n, int nq, void* out, void* stream);
int tt_op_cls_head(const float* x, const float* w, const float* b, float* logits, float* emb, void* stream);

/* Formant correction staged (csrc/formant.hip, include/tortoise_mi355x_fmt.h; `h` is a tt_fmt handle).  tt_op_fmt_run is tt_fmt_run with three
 * optional outputs, each clip's at stage_offsets[c] (host array, in units of one frame's gains: a multiple of 4): spectrum f32 [T][2 * bins_pad]
 * (re, im interleaved, at spectrum + 2 * stage_offsets[c]), logmag f32 [T][bins_pad] (step 2), gains f32 [T][bins_pad] (step 4, clamped).
 * tt_op_fmt_synth runs steps 5 to 7 alone from a given spectrum and given gains in those layouts. */
int tt_op_fmt_run(void* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* warp_index, int n_clips, float* out,
                  const long long* out_offsets, float* spectrum, float* logmag, float* gains, const long long* stage_offsets, void* stream);
int tt_op_fmt_synth(void* h, const float* spectrum, const float* gains, const long long* stage_offsets, const int* clip_lengths, int n_clips,
                    float* out, const long long* out_offsets, void* stream);

/* The denoiser staged (csrc/denoise.hip, include/tortoise_mi355x_nr.h; `h` is a tt_nr handle).  tt_op_nr_run is tt_nr_run with three optional
 * outputs (device f32), clip c's at stage_offsets[c] (host array, element units; the spectrum's at twice that): spectrum [T][2 * bins_pad]
 * (re, im interleaved), power [bins_pad][T] (transposed, as the select reads it) and gains [T][bins_pad].  The floor is tt_nr_run's own
 * floor_out.  Nothing is staged for a TT_NR_SHORT clip. */
struct tt_nr_params;
int tt_op_nr_run(void* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* noise_first_frame,
                 const int* noise_frames, const struct tt_nr_params* params, int n_clips, float* out, const long long* out_offsets, float* floor_out,
                 int* status_out, float* spectrum, float* power, float* gains, const long long* stage_offsets, void* stream);

/* F0 tracker staged (csrc/f0.hip, include/tortoise_mi355x_f0.h; `h` is a tt_f0 handle).  tt_op_f0_track is tt_f0_track with one more output:
 * dprime f64 [frm_off[n_clips]][TT_F0_LAG_MAX + 1], the normalised difference d'(0 .. T) of every frame, sliced by frm_off like lag.
 * tt_op_f0_group: the frames a workgroup of the kernel owns (the sizes at which a clip begins another group). */
int tt_op_f0_track(void* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off, int* lag,
                   float* f0, float* aper, int* n_voiced, int* status, double* dprime, void* stream);
int tt_op_f0_group(void);

/* Viterbi F0 path staged (csrc/f0_viterbi.hip, include/tortoise_mi355x_f0v.h; `h` is a tt_f0v handle).  The candidate tables of a batch are
 * c_lag i32, c_dp f64 and c_f0 f32 [frm_off[n_clips]][8], sliced by frm_off like lag: slots 0 .. 6 the candidates by ascending lag (lag 0 =
 * absent), slot 7 tt_f0_track's own pick.  tt_op_f0v_candidates runs the first launch alone and gives the tables back (no costs: a clip's
 * status is tt_f0_track's).  tt_op_f0v_path runs the second launch alone on tables the caller gives: frames i32 [n_clips] is F of every
 * clip (0: EMPTY; more than the handle's, a short frame slice, bad lags or costs: REFUSED), par's lag_lo prices the octave cost. */
int tt_op_f0v_candidates(void* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off,
                         int* c_lag, double* c_dp, float* c_f0, int* status, void* stream);
int tt_op_f0v_path(void* h, int n_clips, const int* frames, const int* par, const double* cost, const int* frm_off, const int* c_lag,
                   const double* c_dp, const float* c_f0, int* lag, float* f0, float* aper, int* state, int* n_voiced, double* path_cost,
                   int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
