// Kernel launchers shared by the stage runners (gpt2 / clvp / diffusion / univnet) and by the
// operator-level C-ABI entry points the parity tests call.  All pointers are device pointers.
#pragma once
#include "common.h"
#include "gemm.h"

namespace tt {

// ------------------------------------------------------------------------------ row norms
enum NormMode { NORM_NONE = 0, NORM_LAYER = 1, NORM_RMS = 2 };
struct RowNormArgs {
  float* x;            // [M][ldx] f32 residual stream (read unless x_in; written when write_x)
  int ldx;
  const float* x_in;   // optional separate source rows
  int ldxin;
  int M, D;
  const float* add_bias;   // [D], added before the norm (bias of the preceding split-K GEMM)
  const float* add_slabs;  // [nslab][M][ldslab] partial sums of the preceding split-K GEMM
  int nslab;
  size_t slab_stride;
  int ldslab;
  int write_x;         // store the updated row back to x
  int mode;            // NormMode
  const float* g1;
  const float* b1;
  float eps1;
  const float* g2;     // optional second LayerNorm applied to the first one's output
  const float* b2;
  float eps2;
  void* out_t;         // normalised row in the GEMM operand type
  int ldot;
  float* out_f32;      // optional f32 copy of the normalised row
  int ldo32;
  // optional (rownorm_kernel only - the wave form of the same body is built without the slots, the narrow kernel has none; rownorm_launch
  // routes such a problem accordingly): the f32 copy goes to out_f32 + (*f32_slot + f32_slot_base) * f32_slot_stride - a device-side
  // step counter selects the destination block, so a captured decode step can file its row under the step it belongs to
  const int* f32_slot;
  int f32_slot_base;
  size_t f32_slot_stride;
  // optional, session handles (rownorm_kernel only, as f32_slot): row r files its f32 copy under its own counter f32_row_slot[r] (+ f32_slot_base);
  // a negative counter files nothing for that row
  const int* f32_row_slot;
  int row_blocks;      // 1: always one workgroup per row (the decode step: a row's arithmetic order must not depend on how many rows the batch has)
  int* guard;          // optional device counter: += 1 per workgroup / wave that saw a non-finite input value (operand-overflow guard)
  int act;             // activation applied to the normalised row before it is emitted (ACT_NONE; LayerNorm only: the wav2vec2
                       // feature encoder's LayerNorm + GELU, csrc/align.hip)
};
int rownorm_launch(int dtype, const RowNormArgs& a, hipStream_t stream);
// What the last rownorm_launch of this thread started, recorded on the host (as g_gemm_ran; the operator-level tests assert it):
// kernel 0 generic (block per row), 1 narrow, 2 wave (wave per row; the generic kernel's body); nslab = the compiled slab count of the narrow
// kernel, -1 where the count is a run-time loop;
// bias / rms = the narrow kernel's template arguments (the other kernels: whether add_bias is set / the mode is NORM_RMS)
struct RowNormRan { int kernel, nslab, bias, rms; };
extern thread_local RowNormRan g_rownorm_ran;  // norm.hip

// ------------------------------------------------------------------------------ group norm
struct GroupNormArgs {
  const float* x;  // [B][S][C]
  int B, S, C;
  const float* gamma;
  const float* beta;
  float eps;
  const float* scale_shift;  // optional [B?][2C]: y = y * (1 + scale) + shift
  size_t ss_batch_stride;    // 0 when every batch row shares one timestep embedding
  int ss_batch_div;          // batch row b reads block b / ss_batch_div (>= 1; 0 is treated as 1): rows of one timestep share it
  int act;
  void* out_t;
  int ldot;
  float* out_f32;
  int ldo32;
  float* partial;  // workspace, groupnorm_partial_floats(B, S) floats
  const float* gemm_part;  // optional: statistics already emitted by the producing GEMM's epilogue (gemm.hip
                           // run_epilogue) as [row_tile][2][C/16][2]; the separate statistics pass is skipped
  int part_rows;           // rows per row tile of gemm_part
  double inv_count;        // set by groupnorm_launch: 1 / (S * C / 32)
  // padded batches (several utterances of different lengths in one pass): sample b has vlen[b % vperiod] valid rows <= S; the
  // statistics cover the valid rows only and the rows beyond them are written as ZEROS (they are the zero padding the next
  // convolution sees past the end of a shorter sequence).  vperiod == 0: every sample has S rows.
  int vperiod;
  int vlen[32];
  int* guard;  // optional device counter: += 1 per (workgroup, group) whose statistics came out non-finite (operand-overflow guard)
};
int groupnorm_launch(int dtype, const GroupNormArgs& a, hipStream_t stream);
// What the last groupnorm_launch of this thread started: stats = the stand-alone statistics pass ran; apply 0 generic, 1 the C == 1024
// kernel; rows = rows per apply block; fused = the C == 1024 kernel's fused-statistics template
struct GroupNormRan { int stats, apply, rows, fused; };
extern thread_local GroupNormRan g_groupnorm_ran;  // norm.hip
size_t groupnorm_partial_floats(int B, int S);
size_t groupnorm_partial_floats_rows(size_t rows);  // enough for ANY batch whose samples total at most `rows` rows

// ------------------------------------------------------------------------------ attention
struct FlashArgs {
  const void* q;   // [BH][n][64], pre-scaled by 1/sqrt(64)
  const void* k;   // [BH][n][64]
  const void* vt;  // [BH][64][n_pad]
  void* out;       // [B][n][ldo] with head h at columns h*64..
  int ldo;
  int BH, heads, n, n_pad;
  int causal;
  const float* relpos;  // optional [heads][129] additive bias indexed by clamp(key - query, -64, 64) + 64
  // padded batches: batch row b attends to its first nv[b % nv_period] keys only (and only those queries are computed); n stays
  // the row stride of the operands.  nv_period == 0: all n rows are valid.
  int nv_period;
  int nv[32];
  int variant;  // 0: chosen from the shape; 1: never the key-split form; 2: never the 32-query-wave kernel (microbenchmarks / A-B runs)
};
int flash_attention_launch(int dtype, const FlashArgs& a, hipStream_t stream);
int flash_f32_launch(const FlashArgs& a, hipStream_t stream);  // fp32 verification mode (attention_f32.hip)
// What the last flash_attention_launch of this thread started, recorded on the host (as g_gemm_ran; the operator-level tests assert it):
// kernel 0 flash_kernel, 1 flash_lds_kernel, 2 flash32_kernel, 3 flash_f32_kernel (the fp32 verification form); nq = 16-query blocks per wave
// (the NQ template argument; 2 for the 32-query waves of flash32_kernel, 0 for the fp32 form's wave per query); ks = the KS template argument
// (key halves of a staged tile), 0 for the two kernels that have none
enum FlashKernelId { FLASH_RAN_REG = 0, FLASH_RAN_LDS = 1, FLASH_RAN_32 = 2, FLASH_RAN_F32 = 3 };
struct FlashRan { int kernel, nq, ks; };
extern thread_local FlashRan g_flash_ran;  // attention.hip

struct DecodeAttnArgs {
  const void* q;    // [B][heads*64], pre-scaled
  const void* kp;   // shared prefix keys   [heads][P1][64]
  const void* vp;   // shared prefix values [heads][P1][64]
  int P1;
  const void* kc;   // per-sequence keys   [B][heads][8][tmax][8]
  const void* vc;   // per-sequence values [B][heads][tmax][64]
  int tmax;
  const int* step;  // device int: slot of the newest generated key (keys 0..*step are valid)
  int host_tgen;    // host-side copy of *step + 1 for profiling estimates only (0 when unknown)
  void* out;        // [B][heads*64]
  int B, heads;
  int variant;      // 0: chosen from the shape; 1: per-wave prefix kernel; 2 / 3: shared-prefix kernel with 16 / 4 sequences per workgroup
  // several utterances in one batch (ngroups > 1): sequence b belongs to group b / group_size, whose prefix K / V start
  // prefix_group_stride ELEMENTS after the previous group's and hold p1_tab[group] rows (P1 = the largest of them: LDS sizing)
  int ngroups, group_size;
  size_t prefix_group_stride;
  int p1_tab[16];
  // session handles (row_slot != null): every sequence is its own utterance with its own state in device memory.  Row b attends its
  // prefix (prefix_group_stride * b elements in, row_p1[b] rows) and its own keys 0 .. row_slot[b]; a negative slot skips the row.
  // P1 is then the prefix CAPACITY (LDS sizing); nothing per row is baked into the launch.
  const int* row_slot;
  const int* row_p1;
};
int decode_attention_launch(int dtype, const DecodeAttnArgs& a, hipStream_t stream);
// LDS bytes of the session-row decode attention for a prefix capacity p1_cap and tmax own keys (it must stay <= DECODE_LDS_CAP)
size_t decode_attention_session_lds(int p1_cap, int tmax);
constexpr size_t DECODE_LDS_CAP = 160 * 1024;
int decode_attn_f32_launch(const DecodeAttnArgs& a, hipStream_t stream);  // fp32 verification mode (attention_f32.hip)

// The decode step's QKV projection and attention in ONE launch (decode_attention.hip decode_qkv_attn_kernel): a workgroup = one head x 16
// sequences computes the 16 x 192 tile of the QKV GEMM it needs itself (K = 1024), appends the new K / V rows at slot *step and
// attends [prefix | own keys 0 .. *step].  q, k, v carry the bits of gemm_glds<.., EpiQkvDecode>, the output those of
// decode_attn_lds_kernel.  16-bit operands, model_dim 1024, 16 heads of 64, B % 16 == 0, one prefix group, no session rows.
struct DecodeQkvAttnArgs {
  DecodeAttnArgs d;     // d.q is not read; d.step = slot the new key is written to (own keys 0 .. *step - 1 are already in the cache)
  const void* h;        // [B][1024] T  LN1 rows
  const void* w_qkv;    // [3072][1024] T
  const float* b_qkv;   // [3072] or null
  float q_scale;
  void* q_out;          // [B][1024] T or null: the scaled query rows (operator-level tests; the engine does not need them)
};
// LDS bytes of the fused launch for this prefix length / cache capacity; it is eligible while they stay <= DECODE_LDS_CAP
size_t decode_qkv_attention_lds(int P1, int tmax);
int decode_qkv_attention_launch(int dtype, const DecodeQkvAttnArgs& a, hipStream_t stream);

// ------------------------------------------------------------------------------ GEMV-shaped decode GEMMs (gemv.hip): M <= 16 rows
enum GemvEpi { GEMV_F32 = 0, GEMV_RES = 1, GEMV_GELU_T = 2, GEMV_QKV = 3 };
struct GemvArgs {
  const void* A;      // [M][lda] T activation rows
  int lda;
  const void* W;      // [N][ldw] T
  int ldw;
  int M, N, K;        // M <= 16 (5 .. 16: the wide session handles); K in {1024, 2048, 4096}; N % 4 == 0
  const float* bias;  // [N] or null
  int epi;            // GemvEpi
  float* out_f32;     // GEMV_F32: [M][ldo32] = A W^T + bias; GEMV_RES: the residual rows, updated in place (x += A W^T + bias)
  int ldo32;
  void* out_t;        // GEMV_GELU_T: [M][ldot] T = gelu_tanh(A W^T + bias)
  int ldot;
  // GEMV_QKV (the decode step's QKV projection: q pre-scaled into qbuf, K / V appended at slot *step; layouts as DecodeAttnArgs)
  const int* step;
  void* qbuf;
  void* kc;
  void* vc;
  int heads, tmax, dmodel;
  float q_scale;
  const int* row_slot;  // optional (session handles): row r appends at its own slot row_slot[r] instead of *step; negative: no store
  // fused LayerNorm (GEMV_QKV / GEMV_GELU_T, K == 1024): when ln_x is set the activation rows are LayerNorm(ln_x[M][ldx] f32; ln_g, ln_b, ln_eps) and A is unused
  const float* ln_x;
  int ldx;
  const float* ln_g;
  const float* ln_b;
  float ln_eps;
  int* guard;  // counts rows whose variance is not finite (norm.hip's overflow guard), or null
  // optional (M > 4): rows r with row_live[r] < 0 may be left out - a group of rows none of which is live is neither read, multiplied
  // nor stored (a wide session handle's free and finished slots: their outputs are never read)
  const int* row_live;
};
bool gemv_supported(int dtype, const GemvArgs& a);
int gemv_launch(int dtype, const GemvArgs& a, hipStream_t stream);

// ------------------------------------------------------------------------------ AR sampling
// one row's sampling scalars (session handles keep them in device memory, one entry per row: SampleArgs.rows)
struct SampleScalars {
  float rep_penalty, temperature, top_p;
  int top_k;
  float typical_mass;
};
struct SampleArgs {
  const float* logits;  // [B][ldl]; ldl == 0 broadcasts one row per utterance group (the shared-prefix prefill logits), ldg apart
  int ldl, ldg;
  int B, V;
  unsigned* seen;       // [B][(V+31)/32] bitmask of ids already in input_ids (repetition penalty)
  float rep_penalty, temperature, top_p;
  int top_k;
  const float* exp_noise;  // optional [max_steps][B][V] Exp(1) draws (parity runs); else Philox
  unsigned long long seed;
  int row_offset;          // global candidate index of row 0 (sharding-invariant Philox streams)
  const int* state;        // device: state[0] = tokens sampled so far
  int* unfinished;         // [B]
  int stop_token;
  int* codes;              // [B][ldcodes]
  int ldcodes;
  int* next_tok;           // [B]
  int* unfinished_count;   // [max_steps]: number of unfinished rows after each sampling step
  // optional fusion of the next decode step's embedding: embed_x[b][:] = tok_emb[tok][:] + pos_emb[step + pos_offset][:]
  float* embed_x;          // [B][D] or null
  const float* tok_emb;
  const float* pos_emb;
  int D, pos_offset;
  int pos_len;               // rows of pos_emb: the embedding of a token whose position lies beyond the table is skipped (it is never fed)
  // several utterances in one batch (ngroups > 1): row b is candidate b % group_size of group b / group_size; Philox key
  // group_seeds[group], broadcast logits (ldl == 0) row `group`
  int ngroups, group_size;
  unsigned long long group_seeds[16];
  // keys_dev != null: the Philox keys are read from device memory instead (keys_dev[group], keys_dev[0] without groups), so that a
  // captured step graph does not bake the seed of one call in and can be replayed by the next (tt_ar_generate)
  const unsigned long long* keys_dev;
  const int* row_offset_dev;  // != null: row_offset is read from device memory as well (same reason)
  int* guard;                 // optional device counter: += 1 per wave that read a NaN / +inf logit
  // typical sampling (tts(typical_sampling=True, typical_mass): tortoise/utils/typical_sampling.py, autoregressive.py:558): with
  // 0 < typical_mass < 1 a first launch writes the rows with every token outside the typical set at -inf to typical_out (laid out
  // like `logits`: same ldl / ldg), and the sampler reads those rows instead; 0 = off
  float typical_mass;
  float* typical_out;
  // session handles (sess != null): every row is its own utterance, with its state in sess = int[4][B] (SessRow planes).  A row
  // samples only while sess[SESS_RUN][b] == 1, at its own step sess[SESS_N][b] (Philox counter, codes column, mel position) with
  // Philox key keys_dev[b] and candidate index 0; its first token is drawn from pre_logits + b * ldl (its admission prefill), later
  // ones from `logits`.  state[0] counts the steps of the call (unfinished_count index).  Rows that do not sample zero their embed_x row.
  int* sess;
  const float* pre_logits;
  // per-row sampling scalars (session handles; rows != null): row b samples with rows[b] (block-uniform, read once) instead of the five
  // scalars above, which are then unused.  Each launch covers all B rows and a row is served by the launch that owns it: the fast
  // sampler (top_k 1 .. 256; it also zeroes the rows that do not sample), the full-sort sampler (any other top_k) and, for rows with
  // typical_mass != 0, the typical mask ahead of both.  row_launch (SampleRowLaunch bits) says which of the two optional launches run.
  const SampleScalars* rows;
  int row_launch;
};
enum SampleRowLaunch { SAMPLE_ROWS_WIDE = 1, SAMPLE_ROWS_TYPICAL = 2 };
// which sampler serves a row with this top_k (the fast one: 1 .. 256)
static inline __host__ __device__ bool sample_fast_k(int top_k) { return top_k >= 1 && top_k <= 256; }
// planes of the per-row session state (tt_ar session handles): int[4][max_batch]
enum SessPlane { SESS_N = 0, SESS_SLOT = 1, SESS_RUN = 2, SESS_P1 = 3 };
enum SessRun { SESS_FREE = 0, SESS_RUNNING = 1, SESS_FINISHED = 2 };
int sample_launch(const SampleArgs& a, hipStream_t stream);
// the typical-sampling mask alone: rows of a.logits -> a.typical_out (sample_launch runs it ahead of the sampler when a.typical_mass != 0)
int typical_mask_launch(const SampleArgs& a, hipStream_t stream);
// state[0] += 1, state[1] = newest token's index; with `progress` (host-mapped int[2]) also publishes {tokens so far, first step
// after which unfinished_count was 0} for the host's launch loop (state[2] mirrors the latter on the device)
int ar_state_advance_launch(int* state, const int* unfinished_count, int* progress, hipStream_t stream);
int ar_begin_launch(int* state, unsigned* seen, int* unfinished, int* unfinished_count, int B, int V, int max_steps,
                    int start_token, hipStream_t stream);
// session handles: the step counter of every running row advances (SESS_SLOT = index of the token just sampled, SESS_N += 1); a row
// whose token was the stop token becomes SESS_FINISHED (slot -1: it neither decodes nor samples again).  state[0] / state[2] and the
// progress words count the steps of the call as ar_state_advance_launch does.
int ar_sess_advance_launch(int* state, int* sess, int B, const int* unfinished, const int* unfinished_count, int* progress, hipStream_t stream);
// session handles: row `row` starts a new session with a prefix of P1 rows (seen mask and unfinished flag as ar_begin_launch sets them)
int ar_sess_admit_launch(int* sess, int B, int row, int P1, unsigned* seen, int* unfinished, int V, int start_token, hipStream_t stream);
// session handles: row `row` is freed
int ar_sess_close_launch(int* sess, int B, int row, hipStream_t stream);

// x[b][:] = tok_emb[tok[b]][:] + pos_emb[state[1] + pos_offset][:]   (pos_offset 2: kv_cache=True rule, 1: kv_cache=False rule)
int ar_embed_launch(const int* tok, const int* state, const float* tok_emb, const float* pos_emb, float* x, int B, int D, int pos_offset,
                    hipStream_t stream);
// session handles: the same per row at its own slot row_slot[b]; rows with a negative slot get a zero row
int ar_embed_rows_launch(const int* tok, const int* row_slot, const float* tok_emb, const float* pos_emb, float* x, int B, int D, int pos_offset,
                         hipStream_t stream);

// ------------------------------------------------------------------------------ small fused ops
// (GEGLU is formed in the projection GEMM's epilogue: gemm.h EPI_GEGLU)
// x-transformers rotary on the first rot dims (rot = 32) of q, k ([BH][n][64]) and vt ([BH][64][n_pad])
int rotary_launch(int dtype, void* q, void* k, void* vt, const float* inv_freq, int BH, int n, int n_pad, int rot,
                  hipStream_t stream);
// dst[r][:] = src[idx[r]][:]   (f32 rows of C floats)
int gather_rows_launch(const float* src, const int* idx, float* dst, int rows, int C, hipStream_t stream);
// idx[i] = 2 i for i < n: the gather index of a stride-2 convolution's outputs (stage_blocks.h conv_stride2)
int even_rows_index_launch(int* idx, int n, hipStream_t stream);
// dst[b][:] = mean over n rows of src[b][n][:]
int mean_rows_launch(const float* src, float* dst, int B, int n, int C, hipStream_t stream);
// CLVP tail: out[b] = <normalize(t[b or 0]), normalize(s[b])> * exp(temperature)
int clvp_score_launch(const float* t, int t_rows, const float* s, const float* temperature, float* out, int B, int D,
                      hipStream_t stream);
// f32 -> T with optional column zero-padding: dst[r][0..cpad) = src[r][0..c) | 0
int cast_pad_launch(int dtype, const float* src, int lds, void* dst, int ldd, int rows, int c, int cpad, hipStream_t stream);
// dst[j][r][:] = src[r][:] for j < reps (f32 rows of C floats; r < rows)
int repeat_rows_launch(const float* src, float* dst, int rows, int reps, int C, hipStream_t stream);
// broadcast a [C] vector over rows
int broadcast_rows_launch(const float* vec, float* dst, int rows, int C, hipStream_t stream);
// f32 transpose: dst[c][r] = src[r][c]
int transpose_launch(const float* src, float* dst, int rows, int cols, hipStream_t stream);
// [rows][C] f32 -> SiLU -> T
int silu_cast_launch(int dtype, const float* src, void* dst, int n, hipStream_t stream);

// Diffusion p_sample epilogue (utils/diffusion.py:312-418, 487-531), token-major model output.
struct PSampleStep {    // same layout as tt_diff_step (include/tortoise_mi355x.h)
  int timestep;
  float min_log, max_log, cfk, sqrt_recip, sqrt_recipm1, coef1, coef2, nonzero;
};
struct PSampleArgs {
  const PSampleStep* steps;  // device array; entry *slot is used
  const int* slot;           // device int (advanced by slot_advance_launch)
  float* x;             // [S][C] f32 state, updated in place
  void* x_t;            // [2][S][cpad] operand copy for the next step's inp_block (both batch rows)
  int cpad;
  const float* out;     // [2][S][2C] model output rows: batch 0 = conditioned, batch 1 = unconditioned
  int has_uncond;
  const float* noise;   // [n_steps][C][S] channels-first draws (reference layout); entry *slot is used
  int S, C;
  float* mel_out;       // optional [C][S] channels-first denormalised mel written on the last step
  float mel_scale, mel_shift;
  int ld_rows;          // rows between the two batch rows of `out` / `x_t` (0: S; padded batches: the common padded length)
  // optional indirection (a sampler-step graph kept between calls must not bake caller pointers in): when `io` is set, noise and
  // mel_out are read from io[0] / io[1] of this utterance's device-side pointer pair instead of the two fields above
  const void* const* io;
  int* guard;           // optional device counter: += 1 per wave that read a non-finite model output (the x0 clamp would hide it)
};
int psample_launch(int dtype, const PSampleArgs& a, hipStream_t stream);
int slot_advance_launch(int* slot, const float* ss_all, float* ss_cur, int row_floats, int last_slot, hipStream_t stream);

// Deterministic solver epilogue (include/tortoise_mi355x_solver.h): x' = a x + b x0 + c x0_prev on the guided, clamped x0.  Same layout,
// step table and step counter as the p_sample epilogue.
struct SolverStep {     // same layout as tt_solver_step
  int timestep;
  float cfk, sqrt_recip, sqrt_recipm1, a, b, c;
};
struct SolverArgs {
  const SolverStep* steps;   // device array; entry *slot is used
  const int* slot;
  float* x;             // [S][C] f32 state, updated in place
  float* hist;          // [S][C] f32 x0 of the step before: read only when the step's c != 0, always written
  void* x_t;            // optional [2][S][cpad] operand copy for the next step's inp_block (both batch rows)
  int cpad;
  const float* out;     // [2][S][2C] model output rows; only eps (cols 0..C-1) is read
  int has_uncond;
  int S, C;
  float* mel_out;       // optional [C][S] channels-first denormalised mel
  float mel_scale, mel_shift;
  int ld_rows;          // as PSampleArgs
  const void* const* io;  // optional: mel_out is read from io[1] (the {step_noise, mel_out} pair of PSampleArgs; io[0] is unused)
  int* guard;           // optional device counter: += 1 per wave that read a non-finite model output
};
int solver_update_launch(int dtype, const SolverArgs& a, hipStream_t stream);

// ------------------------------------------------------------------------------ UnivNet (fp32 VALU)
// A ragged batch at the audio rate (include/tortoise_mi355x_univnet.h): sequence b owns slot b of every tensor - [C][P] each, P the T / Tin /
// L * hop of the launch's arguments - and its first frames[b] * mul columns are valid.  The grid carries the sequence index; every output
// element is computed with the one-sequence formula on the sequence's own length.  n = 0: one sequence that fills the tensor.
constexpr int kVocSeqs = 32;  // TT_VOC_MAX_BATCH
struct VocSeqs {
  int n, mul;
  int frames[kVocSeqs];
};
struct Conv1dArgs {
  const float* x;  // [Cin][T]
  const float* w;  // [Cout][Cin][k]
  const float* bias;
  float* y;        // [Cout][T]
  int Cin, Cout, T, k, dilation;
  VocSeqs seq;     // ragged batch: x [n][Cin][T], y [n][Cout][T]
  int reflect;     // reflect padding (k/2 * dilation each side) instead of zeros; every sequence must be longer than k/2 * dilation columns
  float in_slope;  // LeakyReLU applied to the input when >= 0 (negative: none)
  int out_act;     // ACT_NONE / ACT_LRELU / 5 = tanh
  float out_slope;
};
int conv1d_direct_launch(const Conv1dArgs& a, hipStream_t stream);
struct ConvT1dArgs {
  const float* x;  // [C][Tin]
  const float* w;  // [Cin][Cout][2*stride]
  const float* bias;
  float* y;        // [C][Tin*stride]
  int C, Tin, stride;
  float in_slope;
  VocSeqs seq;     // ragged batch: x [n][C][Tin], y [n][C][Tin*stride]
};
int convt1d_launch(const ConvT1dArgs& a, hipStream_t stream);
struct LvcArgs {
  const float* x_in;    // [32][T] conv output (LeakyReLU applied here)
  const void* kernels;  // [L][ldk] row l holds layer j's [32][64][3] block at column koff, in the operand type `dtype` (round 6: the
  int ldk, koff;        // KernelPredictor GEMM writes its result once, in 16 bits; f32 in the fp32 verification mode / the operator tests)
  int dtype;            // DT_BF16 / DT_F16 / DT_F32
  const float* bias;    // [L][ldb], layer j's [64] block at column boff
  int ldb, boff;
  float* x;             // [32][T] residual stream: x += sigmoid(o[:32]) * tanh(o[32:])
  int L, hop;
  VocSeqs seq;          // ragged batch: x_in, x [n][32][L * hop], kernels / bias rows b * L + l; sequence b has frames[b] frames (mul unused)
  float in_slope;
  int* guard;           // optional device counter: += 1 per wave that staged a non-finite predicted kernel value (operand-overflow guard; 1 .. 4 per frame)
};
int lvc_launch(const LvcArgs& a, hipStream_t stream);
// What the last conv1d_direct_launch / convt1d_launch / lvc_launch of this host thread started (tt_op_conv1d_ex, tt_op_convt1d_ex, tt_op_lvc_ex;
// include/tortoise_mi355x_test.h).  kernel = -1: the launcher refused the problem and started nothing.
//   conv1d   {kernel (0 conv1d_direct_kernel<32>, 1 conv1d_direct_kernel<1>, 2 conv1d_mfma_kernel), grid.x, grid.y, 0}
//   convt1d  {0, grid.x, grid.y, grid.z}
//   lvc      {kernel (0 lvc_kernel, 1 lvc_mfma_kernel), HOP, kernel element type (0 f32, 1 bf16, 2 f16), 0}
struct VocRan { int kernel, a, b, c; };
extern thread_local VocRan g_voc_ran;  // univnet.hip

}  // namespace tt
