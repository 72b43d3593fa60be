// Stage 1: UnifiedVoice's GPT-2 trunk (30 x 1024 x 16 heads) as an MI355X-native engine.
//   * prefill:   every candidate of an utterance shares the same [cond | text | start] prefix, so it is
//                evaluated once (M = P+1 rows) and its K/V are shared by all sequences
//                (the reference recomputes it B times: autoregressive.py:134-144 + repeat_interleave).
//   * decode:    KV-cached step for B sequences, seven launches per layer: LayerNorm (folds the split-K slabs + bias of the MLP projection
//                before it into the residual stream), QKV GEMM (K / V appended by its epilogue), decode attention, attention projection
//                (split-K slabs), LayerNorm (folds them), c_fc GEMM + gelu, MLP projection (slabs).  Sampling on device; the whole step
//                is replayed from one hipGraph.  Batches of <= 64 sequences (the per-rank share of a candidate-sharded job) run their
//                GEMMs on 16-column tiles so that the weight stream is spread over 192 - 512 workgroups (gemm_impl.h Tile).
//                At 256 / 512 candidates (full rounds of the attention's 16-sequence workgroups) the QKV GEMM and the attention are ONE launch
//                (decode_attention.hip decode_qkv_attn_kernel, TT_AR_OPT_FUSED_QKV_ATTN; same bits): six launches per layer.
//                (A five-launch form - LayerNorm folded into the GEMMs algebraically, split-K folded in-launch behind arrival tickets -
//                was built and measured 0.7 - 10 % slower at every batch size from 16 to 256: profiles/r05_ab_ar_five_launch_step.txt,
//                profiles/r06_ab_small_batch_decode.txt; it is not in the library.)
//   * latents:   teacher-forced full pass for the CLVP winners (autoregressive.py:454-506).
// The host side of a step is argument builders (each launch described once), two layer forms (ar_layer_mfma, ar_layer_gemv), one step
// runner (ar_run_steps) and one finish (ar_finish): DESIGN.md 4, "How a decode step is assembled and paced".
#include "runtime.h"
#include <unistd.h>
#include <chrono>
#include "../../include/tortoise_mi355x.h"

using namespace tt;

struct ArParams {
  unsigned long long keys[16];
  int row_offset;
  int pad[3];
  SampleScalars rows[16];  // session handles: each row's sampling scalars (SampleArgs.rows), taken at its session's first step
};

struct tt_ar : EngineHandle {
  tt_ar_config cfg;
  tt_ar_weights w;
  std::vector<tt_gpt_layer> L;
  int D, H, V;
  int es = 2;               // bytes per operand element (2: bf16 / fp16, 4: the fp32 verification mode)
  int Vp = 0;               // vocabulary padded to a multiple of 4: row stride of the logits and rows of the padded head copy
  void* w_head_p = nullptr; // [Vp][D] T  lm_head weight with zero rows appended (8194 -> 8196: every epilogue access of the head GEMM
  float* b_head_p = nullptr;//            is a whole aligned quad - the run-time-ragged generic kernel cost 24 us per step instead of ~12)
  // shared prefix cache [layers][H][P1][64] (row-major) and per-sequence cache
  void* kp = nullptr; void* vp = nullptr;
  void* kc = nullptr; void* vc = nullptr;
  size_t prefix_layer_elems = 0, gen_layer_elems = 0;
  int tmax = 0;
  // activations
  float* x = nullptr;      // [rows][D] residual stream
  void* h = nullptr;       // [rows][D]  T
  void* ff = nullptr;      // [rows][4D] T
  void* attn = nullptr;    // [rows][D]  T
  void* q = nullptr;       // full pass: [BH][n][64]; decode: [B][D]
  void* kfull = nullptr;   // full pass scratch keys
  void* vt = nullptr;      // full pass V^T [BH][64][n_pad]
  float* slabs = nullptr;  // split-K partials [MAX_SPLIT][max_batch][D]
  float* logits = nullptr; // [max_batch][V]
  float* typ_logits = nullptr;  // [max_batch][Vp]: the rows the sampler reads under typical sampling (tt_sampling.typical_mass)
  int* state = nullptr; unsigned* seen = nullptr; int* unfinished = nullptr; int* unfinished_count = nullptr;
  int* next_tok = nullptr;
  // guard (EngineHandle): rows with a non-finite value seen by the row norms / the sampler, snapshot at the end of every generation /
  // latent pass (tt_ar_guard)
  int max_rows = 0;
  int P1 = 0;      // current prefix length (incl. start token); with several groups the longest one
  int G = 1;       // utterances (groups) of the current batch, each with its own prefix: kp / vp are [group][layer][H][max_prefix][64]
  int P1g[16] = {0};
  unsigned prefilled = 0;  // bit g: group g's prefix has been evaluated for the current batch
  int B = 0;       // current batch
  int logits_rows = 0;
  bool logits_from_prefill = false;
  int host_slot = -1;  // host mirror of state[1]; only feeds the profiler's byte estimates
  // streaming (api_fast.py:389-414 consumes the (token, latent) pairs of the sampling loop): lm_head's input norm also files its f32
  // row - final_norm(ln_f(hidden)), the reference's per-step latent - under [latent index][sequence]; small batches only
  float* lat = nullptr;
  int lat_batch = 0;
  int gen_done = 0;    // tokens sampled by the running generation (tt_ar_generate / tt_ar_generate_chunk)
  bool gen_finished = false;
  // The captured decode step is kept between calls: everything a call can change is either device data (token / slot counters, the
  // Philox keys below, the prefix caches) or part of step.key - the bytes of the sampler's argument block plus the batch / group /
  // prefix-length values the launchers bake into the graph.  A call with the same key replays the graph; any other key re-captures.
  ArParams* par_dev = nullptr;    // Philox key per utterance group (group 0 alone without groups) + row_offset of the call
  ArParams* par_host = nullptr;   // pinned staging of the same
  KeptGraph step;                 // the decode step; step.captures feeds tt_ar_stat(0)
  // The sampler writes into a code buffer the HANDLE owns ([max_batch][tmax], stop-filled at the start of a generation) and the
  // finished columns are copied to the caller's buffer at the end of a call: the caller's pointer is not part of the kept graph.
  int* codes_own = nullptr;
  // Progress words in pinned host memory, written by the step's last kernel (system-scope stores): [0] tokens sampled so far,
  // [1] index of the first token after which every row had stopped (-1: none yet).  The host launches steps at most `lookahead`
  // ahead of [0] and stops launching when [1] turns >= 0: no queue drain inside the loop (round 3: a D2H copy + stream
  // synchronisation every 8 steps), at most `lookahead` surplus steps after the last row stopped.
  int* progress_host = nullptr;
  int* progress_dev = nullptr;
  int lookahead = 6;
  // Handles that decode at most 4 sequences (the streaming engine of api_fast.py: max_batch = 1): the decode step's GEMMs run GEMV-shaped
  // (gemv.hip) - a property of the HANDLE, not of a call's batch, so a handle's kernels never change between calls
  int gemv = 0;  // 0 | 1 GEMV launches | 2 GEMV launches that also do the layer norm in front of them (five launches per layer)
  int drains = 0;     // host-side queue drains the launch loop fell back to (0 when the progress words arrive)
  bool typical = false;  // the last generation ran the typical-sampling mask ahead of the sampler (one more launch per step)
  // Session handles (TT_AR_OPT_SESSIONS): every row is one streaming session with its own state in device memory (sess: int[4][max_batch],
  // SessPlane) - admitted (tt_ar_prefill_group into its slot), advanced (tt_ar_generate_chunk) and retired (TT_AR_OPT_SESSION_CLOSE)
  // independently of the others, all through ONE captured step graph.  Its prefix lives in prefix-cache group `slot`; its first token
  // is drawn from pre_logits[slot], the logits of its admission.  The host mirror below is refreshed at the end of every call.
  int sessions = 0;               // the option's value: 1 (<= 4 rows) | 2 (a wide handle: 5 .. 16 rows, gemv.hip's gemv_rows_kernel)
  int* sess = nullptr;
  int* sess_host = nullptr;       // pinned copy of sess, read back at the end of a chunk
  float* pre_logits = nullptr;    // [max_batch][Vp]
  int s_n[16] = {0}, s_run[16] = {0};
  bool s_key_pending[16] = {false};
  tt_sampling s_scalars;          // the sampling scalars of the running sessions (exp_noise / seeds / group_seeds unused)
  // The scalars of every row are device data (par_dev->rows): the step graph bakes in only which optional sampler launches the running
  // rows need (SampleRowLaunch bits), one kept graph per combination - step for none (default settings), sess_steps[c - 1] for c.
  KeptGraph sess_steps[3];
  int sess_launch = 0;            // the combination of the last chunk (tt_ar_stat(2))
  // TT_AR_OPT_SESSION_SAMPLING: tt_ar_generate_chunk takes one tt_sampling per slot; s_rows[r] = what slot r's session started with
  int sess_sampling = 0;
  int admissions = 0;
  tt_sampling s_rows[16];
  // TT_AR_OPT_FUSED_QKV_ATTN: the decode step's QKV projection and attention as ONE launch where the batch is eligible (ar_fused_qkv_attn)
  int fused_qkv = 1;
  int cu_count = 0;
};

// Whether the decode step of the current batch takes decode_qkv_attn_kernel instead of the QKV GEMM + decode attention.  Decided from the
// handle's configuration and the batch geometry alone (what the kept graph's key holds), so that capture and eager replay agree:
// 16-bit operands, 16 heads of 64, one or two FULL rounds of 16-sequence workgroups on the chip's CUs (256 and 512 candidates on the
// MI355X: the batches the launch was measured ahead at; 128 candidates would need an 8-row form and 272 .. 496 run a second,
// partly filled round - neither was measured, so they keep two launches), one prefix group, no session rows, no GEMV-shaped step, and
// the prefix + score rows + activation rows + weight rings within the LDS.
static bool ar_fused_qkv_attn(const tt_ar* e) {
  if (!e->fused_qkv || e->cfg.dtype == DT_F32 || e->D != 1024 || e->H != 16 || e->G != 1 || e->sessions || e->gemv) return false;
  const int wgs = e->B * e->H / 16;
  if (e->B % 16 != 0 || e->cu_count < 1 || (wgs != e->cu_count && wgs != 2 * e->cu_count) || e->P1 < 1) return false;
  return decode_qkv_attention_lds(e->P1, e->tmax) <= DECODE_LDS_CAP;
}

// rows the GEMV-shaped step of a handle serves: a wide session handle's, or the <= 4 of the others (a property of the handle)
static inline int ar_gemv_rows(const tt_ar* e) { return e->sessions == 2 ? 16 : 4; }
// a wide session handle leaves the GEMV products of its free and finished rows out (GemvArgs.row_live = the slot plane)
static inline const int* ar_gemv_live(const tt_ar* e) { return e->sessions == 2 ? e->sess + SESS_SLOT * e->cfg.max_batch : nullptr; }

namespace tt { int g_ar_gemv = 2; }  // ttx_kernel_variant(TTX_AR_GEMV), read at tt_ar_create: handles of <= 4 sequences run 0 = the MFMA decode GEMMs | 1 = GEMV launches | 2 = GEMVs with the layer norms inside

static const int MAX_SPLIT = 8;

// ------------------------------------------------------------------------------ argument builders: each launch is described once
// LayerNorm weights of a trunk row norm; g2 / b2: the second norm lm_head applies on top (final_norm over ln_f)
struct LnW { const float* g1; const float* b1; const float* g2 = nullptr; const float* b2 = nullptr; };
static inline LnW ar_head_ln(const tt_ar* e) { return LnW{e->w.lnf_g, e->w.lnf_b, e->w.final_norm_g, e->w.final_norm_b}; }
// What a split-K projection leaves for the next row norm to add into the residual stream: its bias and `nslab` slabs of e->slabs
struct Pending { const float* bias = nullptr; int nslab = 0; };

// x [M][D] rows (+ the pending bias / slabs [nslab][slab_rows][D]) -> LayerNorm (-> second LayerNorm) -> h_out [M][D] T.  One workgroup
// per row; a caller that wants the f32 copy of the normalised rows sets out_f32 itself or files it as a latent (ar_file_latent).
static RowNormArgs ar_norm_args(const tt_ar* e, float* x, void* h_out, int M, const LnW& w, const Pending& pend = Pending(), int slab_rows = 0) {
  RowNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ldx = e->D; a.M = M; a.D = e->D;
  a.add_bias = pend.bias;
  a.add_slabs = pend.nslab ? e->slabs : nullptr;
  a.nslab = pend.nslab; a.slab_stride = (size_t)slab_rows * e->D; a.ldslab = e->D;  // (the stride is read per slab: unread without slabs)
  a.write_x = (pend.bias || pend.nslab) ? 1 : 0;
  a.mode = NORM_LAYER;
  a.g1 = w.g1; a.b1 = w.b1; a.eps1 = 1e-5f;
  a.g2 = w.g2; a.b2 = w.b2; a.eps2 = w.g2 ? 1e-5f : 0.f;
  a.out_t = h_out; a.ldot = e->D;
  a.row_blocks = 1;
  a.guard = e->guard.dev;
  return a;
}
// The f32 copy of lm_head's normalised rows is the reference's per-step latent.  lat_index >= 0 files the row(s) as that latent of
// sequence lat_row (prefill: 0); -1: under the device-side step counter (the decode step feeding token i - 1 produces latent i; a
// session row under its own counter); -2, or a handle / batch without latent capture: nothing
static void ar_file_latent(const tt_ar* e, RowNormArgs* a, int lat_index, int lat_row) {
  if (!e->lat || lat_index == -2 || a->M > e->lat_batch) return;
  a->out_f32 = e->lat; a->ldo32 = e->D;
  a->f32_slot_stride = (size_t)e->lat_batch * e->D;
  if (lat_index >= 0) a->out_f32 += (size_t)lat_index * a->f32_slot_stride + (size_t)lat_row * e->D;
  else if (e->sessions) { a->f32_row_slot = e->sess + SESS_SLOT * e->cfg.max_batch; a->f32_slot_base = 1; }  // every row its own index
  else { a->f32_slot = e->state + 1; a->f32_slot_base = 1; }
}
static int ar_norm(tt_ar* e, float* x, int M, const LnW& w, const Pending& pend, int slab_rows, hipStream_t s) {
  return rownorm_launch(e->cfg.dtype, ar_norm_args(e, x, e->h, M, w, pend, slab_rows), s);
}
// lm_head = Sequential(final_norm, mel_head) applied to ln_f(x) (autoregressive.py:42, 174): its input norm
static int ar_head_norm(tt_ar* e, float* x, int M, const Pending& pend, int slab_rows, hipStream_t s, int lat_index = -2, int lat_row = 0) {
  RowNormArgs a = ar_norm_args(e, x, e->h, M, ar_head_ln(e), pend, slab_rows);
  ar_file_latent(e, &a, lat_index, lat_row);
  return rownorm_launch(e->cfg.dtype, a, s);
}
// row P of e->x = the start token's input row: mel_embedding[start] + mel_pos_embedding[0]  (autoregressive.py:137-141)
static int ar_start_row(tt_ar* e, int P, hipStream_t s) {
  RowNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = e->x + (size_t)P * e->D; a.ldx = e->D; a.M = 1; a.D = e->D;
  a.x_in = e->w.mel_emb + (size_t)e->cfg.start_mel_token * e->D; a.ldxin = e->D;
  a.add_bias = e->w.mel_pos;  // row 0
  a.write_x = 1; a.mode = NORM_NONE;
  return rownorm_launch(e->cfg.dtype, a, s);
}

// A GEMV-shaped launch over the decode step's e->B rows (a wide session handle: its live rows): [M][N] = A [M][K] W[N][K]^T + bias.
// The caller adds the fields of its epilogue.
static GemvArgs ar_gemv_args(const tt_ar* e, const void* A, int lda, const void* W, int ldw, int N, int K, const float* bias, int epi) {
  GemvArgs v;
  memset(&v, 0, sizeof(v));
  v.A = A; v.lda = lda; v.W = W; v.ldw = ldw; v.M = e->B; v.N = N; v.K = K; v.bias = bias; v.epi = epi;
  v.row_live = ar_gemv_live(e);
  return v;
}
// the LayerNorm of the rows of x in front of the product (gemv == 2), instead of a launch of its own
static void ar_gemv_ln(const tt_ar* e, GemvArgs* v, const float* g, const float* b) {
  v->ln_x = e->x; v->ldx = e->D; v->ln_g = g; v->ln_b = b; v->ln_eps = 1e-5f; v->guard = e->guard.dev;
}

static inline void* ar_kc(const tt_ar* e, int l) { return offset_t(e->kc, (size_t)l * e->gen_layer_elems, e->es); }
static inline void* ar_vc(const tt_ar* e, int l) { return offset_t(e->vc, (size_t)l * e->gen_layer_elems, e->es); }

// Decode attention of layer l over the e->B rows: one shared prefix, one prefix per utterance group, or (session handles) one per row
static DecodeAttnArgs ar_attn_args(const tt_ar* e, int l) {
  DecodeAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = e->q;
  a.kp = offset_t(e->kp, (size_t)l * e->prefix_layer_elems, e->es);
  a.vp = offset_t(e->vp, (size_t)l * e->prefix_layer_elems, e->es);
  a.P1 = e->P1; a.kc = ar_kc(e, l); a.vc = ar_vc(e, l); a.tmax = e->tmax; a.step = e->state + 1;
  a.out = e->attn; a.B = e->B; a.heads = e->H; a.host_tgen = e->host_slot + 1;
  if (e->G > 1) {
    a.ngroups = e->G; a.group_size = e->B / e->G;
    a.prefix_group_stride = (size_t)e->cfg.layers * e->prefix_layer_elems;
    for (int gi = 0; gi < e->G; ++gi) a.p1_tab[gi] = e->P1g[gi];
  }
  if (e->sessions) {  // every row its own prefix group, prefix length and newest slot - all device data; P1 = the capacity
    a.P1 = e->cfg.max_prefix; a.step = nullptr; a.host_tgen = 0;
    a.row_slot = e->sess + SESS_SLOT * e->cfg.max_batch; a.row_p1 = e->sess + SESS_P1 * e->cfg.max_batch;
    a.prefix_group_stride = (size_t)e->cfg.layers * e->prefix_layer_elems;
  }
  return a;
}

// What the two generation paths share of the sampler's argument block.  Filled in place from memset(0): the block's bytes (padding
// included) are part of the kept step graph's key.  The utterance path adds its scalars, exp_noise, groups and typical_mass; the
// session path rows, row_launch, sess and pre_logits.  The Philox keys and the row offset go through device memory (seed / group_seeds
// / row_offset stay zero): neither the seed nor the candidate range of a call is part of the step graph.
static void ar_sample_args(const tt_ar* e, int B, SampleArgs* sa) {
  memset(sa, 0, sizeof(*sa));
  sa->B = B; sa->V = e->V; sa->seen = e->seen;
  sa->state = e->state; sa->unfinished = e->unfinished; sa->stop_token = e->cfg.stop_mel_token;
  sa->codes = e->codes_own; sa->ldcodes = e->tmax; sa->next_tok = e->next_tok; sa->unfinished_count = e->unfinished_count;
  sa->embed_x = e->x; sa->tok_emb = e->w.mel_emb; sa->pos_emb = e->w.mel_pos; sa->D = e->D; sa->pos_offset = e->cfg.mel_pos_offset;
  sa->pos_len = e->cfg.mel_pos_len;
  sa->guard = e->guard.dev;
  sa->typical_out = e->typ_logits;
  sa->keys_dev = e->par_dev->keys;
  sa->row_offset_dev = &e->par_dev->row_offset;
  sa->logits = e->logits; sa->ldl = e->Vp; sa->ldg = e->Vp;  // every row its own logits (ldg is unused then; set so that every step shares one key)
}

// GPT2Model.forward over full sequences (causal), in place on e->x [B*n][D].
static int gpt_trunk_full(tt_ar* e, int B, int n, bool to_prefix, hipStream_t s, int group = 0) {
  const int D = e->D, H = e->H, M = B * n, dt = e->cfg.dtype;
  const int n_pad = round_up(n, 32);
  for (int l = 0; l < e->cfg.layers; ++l) {
    const tt_gpt_layer& w = e->L[l];
    TT_TRY(ar_norm(e, e->x, M, LnW{w.ln1_g, w.ln1_b}, Pending(), 0, s));
    GemmArgs g = gemm_args(e->h, D, w.w_qkv, D, M, 3 * D, D);
    g.bias = w.b_qkv; g.seq_len = n; g.dmodel = D; g.heads = H;
    g.q = e->q;
    const size_t pl = ((size_t)group * e->cfg.layers + l) * e->prefix_layer_elems;
    g.k = to_prefix ? offset_t(e->kp, pl, e->es) : e->kfull;
    g.v = to_prefix ? offset_t(e->vp, pl, e->es) : nullptr;
    g.vt = e->vt; g.seq_pad = n_pad; g.q_scale = 0.125f;
    TT_TRY(gemm_launch(dt, EPI_QKV_HEADS, g, s));
    FlashArgs f;
    memset(&f, 0, sizeof(f));
    f.q = e->q; f.k = g.k; f.vt = e->vt; f.out = e->attn; f.ldo = D;
    f.BH = B * H; f.heads = H; f.n = n; f.n_pad = n_pad; f.causal = 1;
    TT_TRY(flash_attention_launch(dt, f, s));
    g = gemm_args(e->attn, D, w.w_proj, D, M, D, D);
    g.bias = w.b_proj; g.res = e->x; g.ldres = D; g.out_f32 = e->x; g.ldo32 = D;
    TT_TRY(gemm_launch(dt, EPI_STD, g, s));
    TT_TRY(ar_norm(e, e->x, M, LnW{w.ln2_g, w.ln2_b}, Pending(), 0, s));
    g = gemm_args(e->h, D, w.w_fc, D, M, 4 * D, D);
    g.bias = w.b_fc; g.act = ACT_GELU_TANH; g.out_t = e->ff; g.ldot = 4 * D;
    TT_TRY(gemm_launch(dt, EPI_STD, g, s));
    g = gemm_args(e->ff, 4 * D, w.w_proj2, 4 * D, M, D, 4 * D);
    g.bias = w.b_proj2; g.res = e->x; g.ldres = D; g.out_f32 = e->x; g.ldo32 = D;
    TT_TRY(gemm_launch(dt, EPI_STD, g, s));
  }
  return 0;
}

// Split-K factor of the decode projections.  Deliberately independent of the batch size: the k-order
// of every output element is then the same for any B, so a candidate's logits (and therefore its
// sampled codes) do not depend on how the candidates are sharded across GPUs.
static int pick_split(int N, int K) {
  // decode GEMMs run 64x64 tiles with 256-deep k-stages: aim for ~256 blocks at the full candidate batch
  // (4 row tiles) and at least one whole stage per split.  (In-situ A/B, round 3: 8 slabs for proj2 +4.8 %, 2 slabs for proj +0.9 %.)
  const int tiles = 4 * cdiv(N, 64);
  int sk = 256 / (tiles > 0 ? tiles : 1);
  const int nk = K / 256;
  if (sk > MAX_SPLIT) sk = MAX_SPLIT;
  if (sk > nk) sk = nk;
  if (sk < 1) sk = 1;
  return sk;
}

// The logits of M rows of e->h: into the decode step's logits from row logits_row0 on, or (out: a session's admission) into a
// row of their own outside them
static int ar_head_gemm(tt_ar* e, int M, hipStream_t s, int logits_row0 = 0, float* out = nullptr) {
  float* dst = out ? out : e->logits + (size_t)logits_row0 * e->Vp;
  if (out || (e->gemv && M <= ar_gemv_rows(e))) {
    GemvArgs v = ar_gemv_args(e, e->h, e->D, e->w_head_p, e->D, e->Vp, e->D, e->b_head_p, GEMV_F32);
    v.M = M; v.out_f32 = dst; v.ldo32 = e->Vp;
    if (out || logits_row0 != 0 || M != e->cfg.max_batch) v.row_live = nullptr;  // (only the decode step's rows have a slot plane)
    TT_TRY(gemv_launch(e->cfg.dtype, v, s));
  } else {
    GemmArgs g = gemm_args(e->h, e->D, e->w_head_p, e->D, M, e->Vp, e->D);
    g.bias = e->b_head_p; g.out_f32 = dst; g.ldo32 = e->Vp;
    TT_TRY(gemm_launch(e->cfg.dtype, EPI_STD, g, s));
  }
  if (!out) e->logits_rows = logits_row0 + M;
  return 0;
}

// ------------------------------------------------------------------------------ the decode layer, in its two forms
// GEMV form (handles of <= 4 sequences, wide session handles: <= 16): no split-K - the projections update x in place and the norms
// fold nothing.  Five launches with the layer norms inside the GEMVs (gemv == 2), seven with norms of their own.
static int ar_layer_gemv(tt_ar* e, int l, hipStream_t s) {
  const tt_gpt_layer& w = e->L[l];
  const int D = e->D, dt = e->cfg.dtype, nb = e->B;
  const bool ln_inside = e->gemv == 2;
  if (!ln_inside) TT_TRY(ar_norm(e, e->x, nb, LnW{w.ln1_g, w.ln1_b}, Pending(), nb, s));
  GemvArgs v = ar_gemv_args(e, e->h, D, w.w_qkv, D, 3 * D, D, w.b_qkv, GEMV_QKV);  // QKV: q scaled, K / V appended at the newest slot
  v.step = e->state + 1; v.qbuf = e->q; v.kc = ar_kc(e, l); v.vc = ar_vc(e, l);
  v.heads = e->H; v.tmax = e->tmax; v.dmodel = D; v.q_scale = 0.125f;
  if (e->sessions) { v.step = nullptr; v.row_slot = e->sess + SESS_SLOT * e->cfg.max_batch; }
  if (ln_inside) ar_gemv_ln(e, &v, w.ln1_g, w.ln1_b);
  TT_TRY(gemv_launch(dt, v, s));
  TT_TRY(decode_attention_launch(dt, ar_attn_args(e, l), s));
  v = ar_gemv_args(e, e->attn, D, w.w_proj, D, D, D, w.b_proj, GEMV_RES);  // attention projection
  v.out_f32 = e->x; v.ldo32 = D;
  TT_TRY(gemv_launch(dt, v, s));
  if (!ln_inside) TT_TRY(ar_norm(e, e->x, nb, LnW{w.ln2_g, w.ln2_b}, Pending(), nb, s));
  v = ar_gemv_args(e, e->h, D, w.w_fc, D, 4 * D, D, w.b_fc, GEMV_GELU_T);  // c_fc + gelu
  v.out_t = e->ff; v.ldot = 4 * D;
  if (ln_inside) ar_gemv_ln(e, &v, w.ln2_g, w.ln2_b);
  TT_TRY(gemv_launch(dt, v, s));
  v = ar_gemv_args(e, e->ff, 4 * D, w.w_proj2, 4 * D, D, 4 * D, w.b_proj2, GEMV_RES);  // MLP projection
  v.out_f32 = e->x; v.ldo32 = D;
  return gemv_launch(dt, v, s);
}

// One residual projection of the MFMA layer: x += A [B][K] W[D][K]^T + bias, K split pick_split() ways.  Either the partial sums go
// to e->slabs and *pend reports what the next row norm must add (bias + slabs), or - >= 1024 sequences (several utterances per batch):
// one block per output tile fills the chip - they are folded inside the launch in slab order (gemm.h serial_k: the same bits as
// slabs + row norm, without the slab traffic) and nothing is pending.
static int ar_proj(tt_ar* e, const void* A, const void* W, const float* bias, int K, Pending* pend, hipStream_t s) {
  const int D = e->D, nb = e->B;
  const int sk = pick_split(D, K);
  GemmArgs g = gemm_args(A, K, W, K, nb, D, K);
  if (nb >= 1024 && sk > 1) {
    g.serial_k = sk; g.bias = bias; g.res = e->x; g.ldres = D; g.out_f32 = e->x; g.ldo32 = D;
    *pend = Pending();
  } else {
    g.splitk = sk; g.out_f32 = e->slabs; g.ldo32 = D;
    *pend = Pending{bias, sk};
  }
  return gemm_launch(e->cfg.dtype, EPI_STD, g, s);
}

// MFMA form, seven launches: LayerNorm (folds what the layer before left pending), QKV GEMM (K / V appended by its epilogue), decode
// attention, attention projection, LayerNorm (folds it), c_fc GEMM + gelu, MLP projection (left pending for the next layer's norm).
// fused (ar_fused_qkv_attn): the QKV GEMM and the attention are one launch - six.
static int ar_layer_mfma(tt_ar* e, int l, bool fused, Pending* pend, hipStream_t s) {
  const tt_gpt_layer& w = e->L[l];
  const int D = e->D, dt = e->cfg.dtype, nb = e->B;
  TT_TRY(ar_norm(e, e->x, nb, LnW{w.ln1_g, w.ln1_b}, *pend, nb, s));
  if (fused) {  // the workgroups of the attention project their own q / k / v rows (e->q is not written)
    DecodeQkvAttnArgs f;
    memset(&f, 0, sizeof(f));
    f.d = ar_attn_args(e, l);
    f.h = e->h; f.w_qkv = w.w_qkv; f.b_qkv = w.b_qkv; f.q_scale = 0.125f;
    TT_TRY(decode_qkv_attention_launch(dt, f, s));
  } else {
    GemmArgs g = gemm_args(e->h, D, w.w_qkv, D, nb, 3 * D, D);
    g.bias = w.b_qkv;
    g.dmodel = D; g.heads = e->H; g.q_scale = 0.125f;
    g.step = e->state + 1; g.qbuf = e->q;
    g.kc = ar_kc(e, l); g.vc = ar_vc(e, l);
    g.tmax = e->tmax;
    TT_TRY(gemm_launch(dt, EPI_QKV_DECODE, g, s));
    TT_TRY(decode_attention_launch(dt, ar_attn_args(e, l), s));
  }
  TT_TRY(ar_proj(e, e->attn, w.w_proj, w.b_proj, D, pend, s));
  TT_TRY(ar_norm(e, e->x, nb, LnW{w.ln2_g, w.ln2_b}, *pend, nb, s));
  GemmArgs g = gemm_args(e->h, D, w.w_fc, D, nb, 4 * D, D);
  g.bias = w.b_fc; g.act = ACT_GELU_TANH; g.out_t = e->ff; g.ldot = 4 * D;
  TT_TRY(gemm_launch(dt, EPI_STD, g, s));
  return ar_proj(e, e->ff, w.w_proj2, w.b_proj2, 4 * D, pend, s);
}

// One KV-cached decode step for the e->B sequences up to the logits, all on stream s: the layers in the handle's form, lm_head's
// input norm (which folds what the last layer left pending and files the step's latent) and lm_head.  The fed tokens are in
// e->next_tok (or, `embedded`, the sampler already wrote this step's input rows into e->x: the generation paths).
static int decode_step_enqueue(tt_ar* e, hipStream_t s, bool embedded = false) {
  const int B = e->B;
  if (!embedded) TT_TRY(ar_embed_launch(e->next_tok, e->state, e->w.mel_emb, e->w.mel_pos, e->x, B, e->D, e->cfg.mel_pos_offset, s));
  const bool fused = ar_fused_qkv_attn(e);
  Pending pend;
  for (int l = 0; l < e->cfg.layers; ++l) TT_TRY(e->gemv ? ar_layer_gemv(e, l, s) : ar_layer_mfma(e, l, fused, &pend, s));
  TT_TRY(ar_head_norm(e, e->x, B, pend, B, s, -1));
  return ar_head_gemm(e, B, s);
}

// ------------------------------------------------------------------------------ running steps: one pacing loop, one finish
// The bytes of everything a captured step bakes in that a later call could change: the sampler's argument block + the geometry words
// the launchers read from the handle.
static std::vector<unsigned char> ar_step_key(const SampleArgs& sa, const int* geo, int n_geo) {
  std::vector<unsigned char> key(sizeof(sa) + n_geo * sizeof(int));
  memcpy(key.data(), &sa, sizeof(sa));
  memcpy(key.data() + sizeof(sa), geo, n_geo * sizeof(int));
  return key;
}

// Launches decode steps [first, last) on stream s: replays of `graph` (captured from step_enqueue(s, -1) unless the kept one has the
// key of sa + geo), or with graph == null step_enqueue(s, step) itself.  The host stays at most e->lookahead steps ahead of the progress words the
// last kernel of every step writes, and stops launching once they say that every row has stopped.  *launched = steps put on the stream.
template <typename F>
static int ar_run_steps(tt_ar* e, hipStream_t s, KeptGraph* graph, const SampleArgs& sa, const int* geo, int n_geo, F&& step_enqueue, int first,
                        int last, const char* who, int* launched) {
  *launched = 0;
  if (graph) {
    const auto key = ar_step_key(sa, geo, n_geo);
    TT_TRY(graph->ensure(s, key.data(), key.size(), who, [&]() -> int { return step_enqueue(s, -1); }));
  }
  volatile int* prog = e->progress_host;
  for (int step = first; step < last; ++step) {
    const auto wait0 = std::chrono::steady_clock::now();
    while (step - prog[0] >= e->lookahead && prog[1] < 0) {
      // 200 ms of wall time without the expected progress (not a spin count: a slow first replay - code-object load, a profiler - must
      // not look like lost progress words): fall back to a queue drain, always correct, only slower - and take the progress from the
      // DEVICE state the words mirror, so a host that cannot see the mapped words still paces and ends the loop correctly
      if (std::chrono::steady_clock::now() - wait0 > std::chrono::milliseconds(200)) {
        int st3[3] = {0, 0, -1};
        hipError_t ce = hipStreamSynchronize(s);
        if (ce == hipSuccess) ce = hipMemcpy(st3, e->state, sizeof(st3), hipMemcpyDeviceToHost);
        if (ce != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(ce)); return -2; }
        prog[0] = st3[0];
        if (st3[2] >= 0) prog[1] = st3[2];
        e->drains += 1;
        break;
      }
      usleep(50);
    }
    if (prog[1] >= 0) break;
    TT_TRY(graph ? graph->launch(s, who) : step_enqueue(s, step));
    *launched += 1;
  }
  return 0;
}

// The end of a generation call, after ar_run_steps returned rc: the first `cols` columns of `rows` rows of the handle's code buffer go
// to the caller's [rows][ldcodes] buffer (the caller's pointer is not part of the kept graph), a session handle reads its state planes
// back, the guard is snapshot, and the stream is synchronised: one host-visible completion point per call.  On any error the stream is
// drained and `graph` dropped: a failed replay leaves nothing to trust.
static int ar_finish(tt_ar* e, hipStream_t s, KeptGraph& graph, int rc, int* codes, int ldcodes, int cols, int rows, bool read_sessions, const char* who) {
  if (!rc) {
    hipError_t ce = hipMemcpy2DAsync(codes, (size_t)ldcodes * sizeof(int), e->codes_own, (size_t)e->tmax * sizeof(int), (size_t)cols * sizeof(int),
                                     (size_t)rows, hipMemcpyDeviceToDevice, s);
    if (ce == hipSuccess && read_sessions) ce = hipMemcpyAsync(e->sess_host, e->sess, (size_t)4 * rows * sizeof(int), hipMemcpyDeviceToHost, s);
    if (ce != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(ce)); rc = -2; }
    if (!rc) rc = e->guard.snapshot(s);
    if (!rc && (ce = hipStreamSynchronize(s)) != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(ce)); rc = -2; }
  }
  if (rc) {
    (void)hipStreamSynchronize(s);
    graph.drop();
  }
  return rc;
}

// ------------------------------------------------------------------------------ admission checks: they run before anything of a
// running generation is touched (before sb.run), so a refused call leaves it resumable
static inline bool typical_mass_ok(float m) { return m == 0.f || (m > 0.f && m < 1.f); }
// The sampling scalars of one call (slot < 0) or of one slot's session.  positive: temperature, top_p and repetition_penalty must be
// > 0 (the session paths; the utterance path leaves them to the sampler).
static int ar_check_scalars(const char* who, int slot, const tt_sampling& q, bool positive) {
  const bool pos_ok = !positive || (q.temperature > 0.f && q.top_p > 0.f && q.repetition_penalty > 0.f);
  if (slot >= 0) {
    TT_REQUIRE(pos_ok && typical_mass_ok(q.typical_mass), "%s: slot %d: bad sampling parameters (temperature %g, top_p %g, repetition_penalty %g, typical_mass %g)", who, slot,
               (double)q.temperature, (double)q.top_p, (double)q.repetition_penalty, (double)q.typical_mass);
    return 0;
  }
  TT_REQUIRE(typical_mass_ok(q.typical_mass), "tt_ar_generate: typical_mass %g outside (0, 1) (0 = off)", (double)q.typical_mass);  // (one text on every path)
  TT_REQUIRE(pos_ok, "%s: bad sampling parameters", who);
  return 0;
}
// n_more further tokens after `done` fit the caller's code columns, the KV slots and the mel position table
static int ar_check_chunk(const tt_ar* e, const char* who, int slot, int done, int n_more, int ldcodes) {
  char pre[24] = "";
  if (slot >= 0) snprintf(pre, sizeof(pre), "slot %d: ", slot);
  const int target = done + n_more;
  TT_REQUIRE(n_more >= 1 && target <= ldcodes && target <= e->tmax, "%s: %s%d + %d tokens exceed capacity (%d code columns, %d KV slots)", who, pre, done, n_more, ldcodes,
             e->tmax);
  TT_REQUIRE(target - 2 + e->cfg.mel_pos_offset < e->cfg.mel_pos_len, "%s: %s%d tokens exceed the mel position table", who, pre, target);
  return 0;
}

extern "C" {

int tt_ar_create(const tt_ar_config* cfg, const tt_ar_weights* w, tt_ar** out) {
  TT_REQUIRE(cfg && w && out, "tt_ar_create: null argument");
  TT_REQUIRE(cfg->heads * 64 == cfg->model_dim, "tt_ar_create: head_dim must be 64 (model_dim=%d heads=%d)", cfg->model_dim, cfg->heads);
  TT_REQUIRE(cfg->model_dim % 64 == 0 && cfg->model_dim <= 4096, "tt_ar_create: unsupported model_dim %d", cfg->model_dim);
  TT_REQUIRE(cfg->max_batch > 0 && cfg->max_prefix > 1 && cfg->max_new_tokens > 0, "tt_ar_create: bad capacity");
  TT_REQUIRE(cfg->vocab <= 10240, "tt_ar_create: vocab %d exceeds the sampler's 10240 limit", cfg->vocab);
  TT_REQUIRE(cfg->mel_pos_offset == 1 || cfg->mel_pos_offset == 2, "tt_ar_create: mel_pos_offset must be 2 (kv_cache=True rule) or 1 (kv_cache=False rule), got %d", cfg->mel_pos_offset);
  TT_REQUIRE(cfg->max_groups >= 0 && cfg->max_groups <= 16, "tt_ar_create: max_groups %d outside 0 .. 16", cfg->max_groups);
  TT_REQUIRE(cfg->dtype == DT_BF16 || cfg->dtype == DT_F16 || cfg->dtype == DT_F32, "tt_ar_create: unknown dtype %d", cfg->dtype);
  TT_REQUIRE(cfg->dtype != DT_F32 || cfg->max_groups <= 1, "tt_ar_create: the fp32 verification mode decodes one utterance per batch");
  tt_ar* e = new tt_ar();
  e->cfg = *cfg;
  if (e->cfg.max_groups < 1) e->cfg.max_groups = 1;
  e->w = *w;
  e->L.assign(w->layers_host, w->layers_host + cfg->layers);
  e->D = cfg->model_dim; e->H = cfg->heads; e->V = cfg->vocab;
  e->es = dtype_bytes(cfg->dtype);
  const size_t es = e->es;
  // KV slots per sequence, rounded up to 8: the K cache is chunk-major with a chunk stride of 16 tmax bytes, and strides within ~100 bytes of a
  // multiple of 4 KB (tmax = 254, 506, 508, 510, 516 ...) cost the decode attention up to 30 % (scripts/attn_stride.py, profiles/r06_attn_phase_stamps.txt);
  // a multiple of 8 slots is a multiple of 128 bytes and cannot fall inside that band
#ifdef TT_KV_NO_ROUND  // (A/B builds)
  e->tmax = cfg->max_new_tokens;
#else
  e->tmax = round_up(cfg->max_new_tokens, 8);
#endif
  const int D = e->D, H = e->H;
  int rc = e->open("tt_ar_create", true);
  {
    int dev = 0;
    if (!rc && (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&e->cu_count, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)) e->cu_count = 0;
  }
  e->max_rows = std::max(std::max(cfg->max_prefix, cfg->max_full_rows), cfg->max_batch);
  const size_t rows = (size_t)e->max_rows + 64;
  e->prefix_layer_elems = (size_t)H * cfg->max_prefix * 64;
  e->gen_layer_elems = (size_t)cfg->max_batch * H * e->tmax * 64;
  const int npad_max = round_up(e->max_rows, 32) + 32;
  if (!rc) rc = e->arena.alloc(&e->kp, (e->prefix_layer_elems * cfg->layers * e->cfg.max_groups + 4096) * es);
  if (!rc) rc = e->arena.alloc(&e->vp, (e->prefix_layer_elems * cfg->layers * e->cfg.max_groups + 4096) * es);
  if (!rc) rc = e->arena.alloc(&e->kc, (e->gen_layer_elems * cfg->layers + 4096) * es);
  if (!rc) rc = e->arena.alloc(&e->vc, (e->gen_layer_elems * cfg->layers + 4096) * es);
  if (!rc) rc = e->arena.alloc_t(&e->x, rows * D);
  if (!rc) rc = e->arena.alloc(&e->h, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->ff, rows * 4 * D * es);
  if (!rc) rc = e->arena.alloc(&e->attn, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->q, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->kfull, rows * D * es);
  // V^T scratch: per (batch, head) 64 rows of n_pad keys; total keys <= max_rows (+ padding per sequence)
  if (!rc) rc = e->arena.alloc(&e->vt, ((size_t)H * 64 * ((size_t)npad_max + 32 * (size_t)cfg->max_batch)) * es);
  if (!rc) rc = e->arena.alloc_t(&e->slabs, (size_t)MAX_SPLIT * cfg->max_batch * D);
  e->Vp = round_up(e->V, 4);
  if (!rc) rc = e->arena.alloc_t(&e->logits, (size_t)cfg->max_batch * e->Vp);
  if (!rc) rc = e->arena.alloc_t(&e->typ_logits, (size_t)cfg->max_batch * e->Vp);
  if (!rc) rc = e->arena.alloc(&e->w_head_p, (size_t)e->Vp * D * es);   // (arena memory is zeroed: the padding rows / bias entries are 0)
  if (!rc) rc = e->arena.alloc_t(&e->b_head_p, e->Vp);
  if (!rc && hipMemcpy(e->w_head_p, w->w_mel_head, (size_t)e->V * D * es, hipMemcpyDeviceToDevice) != hipSuccess) { set_error("tt_ar_create: copying the head weight failed"); rc = -2; }
  if (!rc && hipMemcpy(e->b_head_p, w->b_mel_head, (size_t)e->V * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) { set_error("tt_ar_create: copying the head bias failed"); rc = -2; }
  if (!rc) rc = e->arena.alloc_t(&e->state, 4);
  if (!rc) rc = e->arena.alloc_t(&e->seen, (size_t)cfg->max_batch * ((e->V + 31) / 32));
  if (!rc) rc = e->arena.alloc_t(&e->unfinished, cfg->max_batch);
  if (!rc) rc = e->arena.alloc_t(&e->unfinished_count, e->tmax + 8);
  if (!rc) rc = e->arena.alloc_t(&e->next_tok, cfg->max_batch);
  if (!rc && cfg->max_batch <= 8) {  // the streaming path decodes one sequence (api_fast.py): [tmax + 1][max_batch][D] f32
    e->lat_batch = cfg->max_batch;
    rc = e->arena.alloc_t(&e->lat, (size_t)(e->tmax + 1) * e->lat_batch * D);
  }
  if (!rc) rc = e->arena.alloc_t(&e->par_dev, 1);
  if (!rc) rc = e->arena.alloc_t(&e->codes_own, (size_t)cfg->max_batch * e->tmax);
  if (!rc && (hipHostMalloc((void**)&e->par_host, sizeof(ArParams)) != hipSuccess ||
              hipHostMalloc((void**)&e->progress_host, 4 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
              hipHostGetDevicePointer((void**)&e->progress_dev, e->progress_host, 0) != hipSuccess)) {
    set_error("tt_ar_create: hipHostMalloc failed");
    rc = -2;
  }
  if (!rc) {
    e->progress_host[0] = 0; e->progress_host[1] = -1; e->progress_host[2] = e->progress_host[3] = 0;
  }
  // GEMV-shaped decode step: <= 4 sequences per handle, 16-bit operands, the trunk's K in {1024, 2048, 4096} (gemv.hip)
  e->gemv = (cfg->max_batch <= 4 && cfg->dtype != DT_F32 && cfg->max_groups <= 1 && D == 1024) ? tt::g_ar_gemv : 0;
  if (rc) {
    tt_ar_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_ar_destroy(tt_ar* e) {
  if (!e) return;
  e->close();
  e->step.drop();
  for (KeptGraph& g : e->sess_steps) g.drop();
  if (e->par_host) (void)hipHostFree(e->par_host);
  if (e->progress_host) (void)hipHostFree(e->progress_host);
  if (e->sess_host) (void)hipHostFree(e->sess_host);
  delete e;
}

// What every prefill shares: [prefix | start token] (P + 1 rows) through the trunk, their K / V into prefix-cache group `group` (per-layer
// stride of the prefix cache = its capacity H * max_prefix * 64: group g, layer l at (g * layers + l) strides).  The start-token row's
// hidden state is left in row P of e->x for the caller's head.
static int ar_prefill_trunk(tt_ar* e, const float* prefix_emb, int P, int group, hipStream_t s) {
  TT_CHECK_HIP(hipMemcpyAsync(e->x, prefix_emb, (size_t)P * e->D * sizeof(float), hipMemcpyDeviceToDevice, s));
  TT_TRY(ar_start_row(e, P, s));
  return gpt_trunk_full(e, 1, P + 1, true, s, group);
}

// Session handles: admit a session into slot `slot` of the S = max_batch rows.  The running rows are untouched: the prefix goes to
// prefix-cache group `slot`, its logits to pre_logits[slot], its start-token latent to latent 0 of row `slot`.
static int ar_admit(tt_ar* e, int slot, int S, const float* prefix_emb, int P, hipStream_t stream) {
  TT_REQUIRE(S == e->cfg.max_batch && slot >= 0 && slot < S, "tt_ar_prefill_group: slot %d of %d (a session handle has %d slots)", slot, S, e->cfg.max_batch);
  TT_REQUIRE(P >= 1 && P + 1 <= e->cfg.max_prefix, "tt_ar_prefill: prefix of %d rows exceeds capacity %d", P + 1, e->cfg.max_prefix);
  TT_REQUIRE(e->s_run[slot] == SESS_FREE, "tt_ar_prefill_group: slot %d holds a session (close it with TT_AR_OPT_SESSION_CLOSE first)", slot);
  return e->sb.run(stream, [&](hipStream_t s) -> int {
    const int P1 = P + 1;
    TT_TRY(ar_prefill_trunk(e, prefix_emb, P, slot, s));
    TT_TRY(ar_head_norm(e, e->x + (size_t)P * e->D, 1, Pending(), 1, s, 0, slot));
    TT_TRY(ar_head_gemm(e, 1, s, 0, e->pre_logits + (size_t)slot * e->Vp));
    TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->codes_own + (size_t)slot * e->tmax), e->cfg.stop_mel_token, (size_t)e->tmax, s));
    TT_TRY(ar_sess_admit_launch(e->sess, S, slot, P1, e->seen, e->unfinished, e->V, e->cfg.start_mel_token, s));
    e->P1g[slot] = P1;
    e->s_n[slot] = 0;
    e->s_run[slot] = SESS_RUNNING;
    e->s_key_pending[slot] = true;
    e->admissions += 1;
    return 0;
  });
}

int tt_ar_prefill_group(tt_ar* e, int group, int n_groups, const float* prefix_emb, int P, void* stream) {
  TT_REQUIRE(e && prefix_emb, "tt_ar_prefill: null argument");
  if (e->sessions) return ar_admit(e, group, n_groups, prefix_emb, P, (hipStream_t)stream);
  TT_REQUIRE(n_groups >= 1 && n_groups <= e->cfg.max_groups && group >= 0 && group < n_groups, "tt_ar_prefill_group: group %d of %d (capacity %d groups)", group, n_groups, e->cfg.max_groups);
  TT_REQUIRE(P >= 1 && P + 1 <= e->cfg.max_prefix, "tt_ar_prefill: prefix of %d rows exceeds capacity %d", P + 1, e->cfg.max_prefix);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    if (n_groups != e->G || group == 0) {  // a new batch starts with its group 0
      e->G = n_groups;
      e->prefilled = 0;
    }
    e->P1g[group] = P + 1;
    e->prefilled |= 1u << group;
    e->P1 = 0;
    for (int gi = 0; gi < n_groups; ++gi)
      if ((e->prefilled >> gi) & 1u) e->P1 = std::max(e->P1, e->P1g[gi]);
    TT_TRY(ar_prefill_trunk(e, prefix_emb, P, group, s));
    // logits row `group`; group 0's start-token row is latent 0 of the batch
    TT_TRY(ar_head_norm(e, e->x + (size_t)P * e->D, 1, Pending(), 1, s, group == 0 ? 0 : -2));
    TT_TRY(ar_head_gemm(e, 1, s, group));
    e->logits_from_prefill = e->prefilled == (n_groups >= 32 ? ~0u : (1u << n_groups) - 1u);
    return 0;
  });
}

int tt_ar_prefill(tt_ar* e, const float* prefix_emb, int P, void* stream) { return tt_ar_prefill_group(e, 0, 1, prefix_emb, P, stream); }

int tt_ar_get_logits(tt_ar* e, float* dst, int rows, void* stream) {
  TT_REQUIRE(e && dst && rows >= 1 && rows <= e->logits_rows, "tt_ar_get_logits: %d rows requested, %d available", rows, e ? e->logits_rows : 0);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_CHECK_HIP(hipMemcpy2DAsync(dst, (size_t)e->V * sizeof(float), e->logits, (size_t)e->Vp * sizeof(float), (size_t)e->V * sizeof(float), (size_t)rows,
                                  hipMemcpyDeviceToDevice, s));
    return 0;
  });
}

int tt_ar_begin(tt_ar* e, int B, void* stream) {
  TT_REQUIRE(e && B >= 1 && B <= e->cfg.max_batch, "tt_ar_begin: batch %d exceeds capacity", B);
  TT_REQUIRE(!e->sessions, "tt_ar_begin: a session handle decodes with tt_ar_generate_chunk");
  TT_REQUIRE(e->P1 > 0, "tt_ar_begin: call tt_ar_prefill first");
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    e->B = B;
    e->host_slot = -1;
    return ar_begin_launch(e->state, e->seen, e->unfinished, e->unfinished_count, B, e->V, e->tmax + 8, e->cfg.start_mel_token, s);
  });
}

int tt_ar_decode_step(tt_ar* e, const int* tokens, void* stream) {
  TT_REQUIRE(e && tokens && e->B > 0 && !e->sessions, "tt_ar_decode_step: call tt_ar_begin first");
  // the step about to run writes KV slot host_slot + 1 and reads mel position row host_slot + 1 + mel_pos_offset
  TT_REQUIRE(e->host_slot + 1 < e->tmax, "tt_ar_decode_step: all %d KV slots of this handle are used", e->tmax);
  TT_REQUIRE(e->host_slot + 1 + e->cfg.mel_pos_offset < e->cfg.mel_pos_len, "tt_ar_decode_step: step %d is beyond the mel position table (%d rows)", e->host_slot + 1, e->cfg.mel_pos_len);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    TT_CHECK_HIP(hipMemcpyAsync(e->next_tok, tokens, (size_t)e->B * sizeof(int), hipMemcpyDeviceToDevice, s));
    TT_TRY(ar_state_advance_launch(e->state, nullptr, nullptr, s));  // state[1] = slot of the token being fed
    e->host_slot += 1;
    e->logits_from_prefill = false;
    return decode_step_enqueue(e, s);
  });
}

// The checks of a generation that depend on the sampling arguments and the handle's state
static int ar_generate_check(const tt_ar* e, int B, bool fresh, const tt_sampling* sp) {
  TT_TRY(ar_check_scalars("tt_ar_generate", -1, *sp, false));
  TT_REQUIRE(e->G <= 1 || (B % e->G == 0 && (B / e->G) % 4 == 0), "tt_ar_generate: %d sequences do not split into %d groups of a multiple of 4", B, e->G);
  TT_REQUIRE(!fresh || e->logits_from_prefill, "tt_ar_generate: the logits buffer does not hold the prefill logits of all %d group(s); call tt_ar_prefill / tt_ar_prefill_group first", e->G);
  return 0;
}

// Sampling loop shared by tt_ar_generate (fresh = true: the whole utterance) and tt_ar_generate_chunk (streaming: the loop
// is resumed where the previous chunk stopped; every per-step quantity lives in device-side state, so resuming is just
// replaying the step graph again).  Tokens [e->gen_done, target) are produced; codes is the caller's [B][ldcodes] buffer.
static int ar_generate_run(tt_ar* e, int B, bool fresh, int target, int ldcodes, const tt_sampling* sp, int* codes, int* n_steps_host,
                           int* finished_host, hipStream_t s) {
  SampleArgs sa;
  ar_sample_args(e, B, &sa);
  sa.rep_penalty = sp->repetition_penalty; sa.temperature = sp->temperature; sa.top_p = sp->top_p; sa.top_k = sp->top_k;
  sa.exp_noise = sp->exp_noise;
  sa.typical_mass = sp->typical_mass;
  e->typical = sp->typical_mass != 0.f;
  for (int gi = 0; gi < 16; ++gi) e->par_host->keys[gi] = sp->seed;
  e->par_host->row_offset = sp->row_offset;
  if (e->G > 1) {
    sa.ngroups = e->G; sa.group_size = B / e->G;
    for (int gi = 0; gi < e->G; ++gi) e->par_host->keys[gi] = sp->group_seeds ? sp->group_seeds[gi] : sp->seed;
  }
  // (par_host and the progress words are free again: every earlier generation ended with a stream synchronisation)
  TT_CHECK_HIP(hipMemcpyAsync(e->par_dev, e->par_host, sizeof(ArParams), hipMemcpyHostToDevice, s));
  volatile int* prog = e->progress_host;
  if (fresh) {
    e->B = B;
    e->gen_done = 0;
    e->gen_finished = false;
    prog[0] = 0;
    prog[1] = -1;
    TT_TRY(ar_begin_launch(e->state, e->seen, e->unfinished, e->unfinished_count, B, e->V, e->tmax + 8, e->cfg.start_mel_token, s));
    TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)codes, e->cfg.stop_mel_token, (size_t)B * ldcodes, s));
    TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)e->codes_own, e->cfg.stop_mel_token, (size_t)B * e->tmax, s));
    // token 0: every row samples from the shared prefill logits (ldl == 0: one row per group); every later one from its own row
    sa.ldl = 0;
    e->logits_from_prefill = false;
    TT_TRY(sample_launch(sa, s));
    sa.ldl = e->Vp;
    TT_TRY(ar_state_advance_launch(e->state, e->unfinished_count, e->progress_dev, s));
    e->gen_done = 1;
  } else {
    prog[0] = e->gen_done;
    // Resumed chunk (streaming): between two chunks the caller may have run tt_ar_latents / tt_ar_prefill, which use e->x as
    // their residual stream, so the input row the sampler fused into e->x for the next step is gone.  Rebuild it from the
    // device-side state (newest token, its index): mel_embedding[next_tok] + mel_pos_embedding[state[1] + offset].
    TT_TRY(ar_embed_launch(e->next_tok, e->state, e->w.mel_emb, e->w.mel_pos, e->x, B, e->D, e->cfg.mel_pos_offset, s));
  }

  const bool use_graph = graphs_enabled() && target - e->gen_done > 1;
  // what the captured step bakes in besides device pointers owned by the handle: the sampler's argument block (scalars, the optional
  // injected-noise pointer) and the batch geometry / range structure the launchers read from the handle
  int geo[24] = {B, e->G, e->P1, g_prof_on ? 1 : 0};
  for (int gi = 0; gi < 16; ++gi) geo[4 + gi] = gi < e->G ? e->P1g[gi] : 0;
  geo[20] = ar_fused_qkv_attn(e) ? 1 : 0;
  auto step_enqueue = [&](hipStream_t st, int step) -> int {
    if (step >= 0) e->host_slot = step - 1;  // (eager launches: the profiler's byte estimates follow the step)
    TT_TRY(decode_step_enqueue(e, st, true));
    TT_TRY(sample_launch(sa, st));
    return ar_state_advance_launch(e->state, e->unfinished_count, e->progress_dev, st);
  };
  int launched = 0;
  const int rc = ar_run_steps(e, s, use_graph ? &e->step : nullptr, sa, geo, 24, step_enqueue, e->gen_done, target, "tt_ar_generate", &launched);
  const int steps_done = e->gen_done + launched;
  TT_TRY(ar_finish(e, s, e->step, rc, codes, ldcodes, steps_done, B, false, "tt_ar_generate"));
  const int first_zero = prog[1];
  const bool finished = first_zero >= 0;
  e->gen_done = finished ? (first_zero + 1 < steps_done ? first_zero + 1 : steps_done) : steps_done;
  e->gen_finished = finished;
  e->host_slot = e->gen_done - 1;
  if (n_steps_host) *n_steps_host = e->gen_done;
  if (finished_host) *finished_host = finished ? 1 : 0;
  return 0;
}

int tt_ar_generate(tt_ar* e, int B, int max_new, const tt_sampling* sp, int* codes, int* n_steps_host, void* stream) {
  TT_REQUIRE(e && sp && codes, "tt_ar_generate: null argument");
  TT_REQUIRE(B >= 1 && B <= e->cfg.max_batch, "tt_ar_generate: batch %d exceeds capacity %d", B, e->cfg.max_batch);
  TT_REQUIRE(max_new >= 1 && max_new <= e->tmax, "tt_ar_generate: max_new %d exceeds capacity %d", max_new, e->tmax);
  TT_REQUIRE(max_new - 2 + e->cfg.mel_pos_offset < e->cfg.mel_pos_len, "tt_ar_generate: max_new %d exceeds the mel position table", max_new);
  TT_REQUIRE(!e->sessions, "tt_ar_generate: a session handle decodes with tt_ar_generate_chunk");
  TT_REQUIRE(e->P1 > 0, "tt_ar_generate: call tt_ar_prefill first");
  TT_TRY(ar_generate_check(e, B, true, sp));
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    return ar_generate_run(e, B, true, max_new, max_new, sp, codes, n_steps_host, nullptr, s);
  });
}

static bool same_scalars(const tt_sampling& a, const tt_sampling& b) {
  return a.temperature == b.temperature && a.top_p == b.top_p && a.repetition_penalty == b.repetition_penalty && a.top_k == b.top_k &&
         a.typical_mass == b.typical_mass;
}

// Session handles: every running row advances by up to n_more tokens through the kept step graph of the optional sampler launches its
// rows need.  A row stops advancing at its stop token; the loop ends early once no row runs.  codes [S][ldcodes]; n_total_host /
// finished_host [S].  sp: one tt_sampling for every row, or with TT_AR_OPT_SESSION_SAMPLING one per slot (sp[S]).
static int ar_sessions_chunk(tt_ar* e, int S, int n_more, int ldcodes, const tt_sampling* sp, int* codes, int* n_total_host, int* finished_host,
                             hipStream_t stream) {
  const char* who = "tt_ar_generate_chunk";
  TT_REQUIRE(S == e->cfg.max_batch, "tt_ar_generate_chunk: a session handle advances all %d slots (got %d)", e->cfg.max_batch, S);
  if (!e->sess_sampling) {
    TT_REQUIRE(sp->exp_noise == nullptr, "tt_ar_generate_chunk: injected exp_noise is not available on a session handle");
    TT_TRY(ar_check_scalars(who, -1, *sp, true));
  }
  bool running = false, others = false;
  for (int r = 0; r < S; ++r) {
    if (e->s_run[r] != SESS_RUNNING) continue;
    running = true;
    others = others || !e->s_key_pending[r];
    TT_TRY(ar_check_chunk(e, who, r, e->s_n[r], n_more, ldcodes));
    if (e->sess_sampling) {  // (entries of free and finished slots are not read)
      const tt_sampling& q = sp[r];
      TT_REQUIRE(q.exp_noise == nullptr && q.group_seeds == nullptr, "tt_ar_generate_chunk: slot %d: exp_noise and group_seeds are not available with per-session sampling (seed is the key)", r);
      TT_TRY(ar_check_scalars(who, r, q, true));
      TT_REQUIRE(e->s_key_pending[r] || (same_scalars(q, e->s_rows[r]) && q.seed == e->s_rows[r].seed),
                 "tt_ar_generate_chunk: slot %d: sampling settings differ from those its session started with", r);
    }
  }
  // the sampling scalars belong to the handle while a session that already sampled runs (unless each session has its own)
  TT_REQUIRE(e->sess_sampling || !others || same_scalars(*sp, e->s_scalars), "tt_ar_generate_chunk: sampling settings differ from those of the running sessions");
  return e->sb.run(stream, [&](hipStream_t s) -> int {
    if (running) {
      if (!e->sess_sampling) e->s_scalars = *sp;
      // a session's key and scalars are taken at its first step; the others keep theirs
      int launch = 0;
      for (int r = 0; r < S; ++r) {
        if (e->s_run[r] != SESS_RUNNING) continue;
        if (e->s_key_pending[r]) {
          const tt_sampling& q = e->sess_sampling ? sp[r] : *sp;
          e->par_host->keys[r] = e->sess_sampling ? q.seed : (sp->group_seeds ? sp->group_seeds[r] : sp->seed);
          SampleScalars& sc = e->par_host->rows[r];
          sc.rep_penalty = q.repetition_penalty; sc.temperature = q.temperature; sc.top_p = q.top_p; sc.top_k = q.top_k; sc.typical_mass = q.typical_mass;
          e->s_rows[r] = q;
          e->s_rows[r].exp_noise = nullptr;
          e->s_rows[r].group_seeds = nullptr;
          e->s_rows[r].seed = e->par_host->keys[r];
        }
        const SampleScalars& sc = e->par_host->rows[r];
        if (!sample_fast_k(sc.top_k)) launch |= SAMPLE_ROWS_WIDE;
        if (sc.typical_mass != 0.f) launch |= SAMPLE_ROWS_TYPICAL;
      }
      e->par_host->row_offset = 0;
      SampleArgs sa;
      ar_sample_args(e, S, &sa);
      sa.rows = e->par_dev->rows; sa.row_launch = launch;  // (the five scalars of the argument block stay zero: every row reads its own)
      sa.sess = e->sess; sa.pre_logits = e->pre_logits;
      e->typical = (launch & SAMPLE_ROWS_TYPICAL) != 0;
      e->sess_launch = launch;
      TT_CHECK_HIP(hipMemcpyAsync(e->par_dev, e->par_host, sizeof(ArParams), hipMemcpyHostToDevice, s));
      // the counters of this call: state[0] = its steps so far, state[2] = the step after which no row ran (-1: none yet)
      TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)e->state, 0, 1, s));
      TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->state + 1), -1, 2, s));
      TT_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)e->unfinished_count, 0, (size_t)e->tmax + 8, s));
      // the input rows of the next step (a prefill / latent pass since the last chunk used e->x as its residual stream)
      TT_TRY(ar_embed_rows_launch(e->next_tok, e->sess + SESS_SLOT * S, e->w.mel_emb, e->w.mel_pos, e->x, S, e->D, e->cfg.mel_pos_offset, s));
      volatile int* prog = e->progress_host;
      prog[0] = 0;
      prog[1] = -1;
      auto step_enqueue = [&](hipStream_t st, int) -> int {
        TT_TRY(decode_step_enqueue(e, st, true));
        TT_TRY(sample_launch(sa, st));
        return ar_sess_advance_launch(e->state, e->sess, S, e->unfinished, e->unfinished_count, e->progress_dev, st);
      };
      KeptGraph& graph = launch ? e->sess_steps[launch - 1] : e->step;
      // baked in: the sampler's argument block (pointers and the combination of optional launches) and the profiler switch - no
      // batch, prefix length, step or sampling scalar of any row
      const int geo[4] = {S, -1, e->cfg.max_prefix, g_prof_on ? 1 : 0};
      int launched = 0;
      const int rc = ar_run_steps(e, s, graphs_enabled() ? &graph : nullptr, sa, geo, 4, step_enqueue, 0, n_more, who, &launched);
      TT_TRY(ar_finish(e, s, graph, rc, codes, ldcodes, std::min(ldcodes, e->tmax), S, true, who));
      for (int r = 0; r < S; ++r) {
        if (e->s_run[r] == SESS_RUNNING) e->s_key_pending[r] = false;
        e->s_n[r] = e->sess_host[SESS_N * S + r];
        e->s_run[r] = e->sess_host[SESS_RUN * S + r];
      }
    }
    for (int r = 0; r < S; ++r) {
      n_total_host[r] = e->s_n[r];
      finished_host[r] = e->s_run[r] == SESS_FINISHED ? 1 : 0;
    }
    return 0;
  });
}

int tt_ar_generate_chunk(tt_ar* e, int B, int first, int n_more, int ldcodes, const tt_sampling* sp, int* codes, int* n_total_host,
                         int* finished_host, void* stream) {
  TT_REQUIRE(e && sp && codes && n_total_host && finished_host, "tt_ar_generate_chunk: null argument");
  if (e->sessions) return ar_sessions_chunk(e, B, n_more, ldcodes, sp, codes, n_total_host, finished_host, (hipStream_t)stream);
  TT_REQUIRE(B >= 1 && B <= e->cfg.max_batch, "tt_ar_generate_chunk: batch %d exceeds capacity %d", B, e->cfg.max_batch);
  TT_REQUIRE(e->P1 > 0, "tt_ar_generate_chunk: call tt_ar_prefill first");
  TT_REQUIRE(first || (e->gen_done >= 1 && e->B == B), "tt_ar_generate_chunk: no generation of %d rows to resume", B);
  const int done = first ? 0 : e->gen_done;
  TT_TRY(ar_check_chunk(e, "tt_ar_generate_chunk", -1, done, n_more, ldcodes));
  const bool stopped = !first && e->gen_finished;  // every row already stopped
  if (!stopped) TT_TRY(ar_generate_check(e, B, first != 0, sp));
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    if (stopped) {
      *n_total_host = e->gen_done;
      *finished_host = 1;
      return 0;
    }
    return ar_generate_run(e, B, first != 0, done + n_more, ldcodes, sp, codes, n_total_host, finished_host, s);
  });
}

int tt_ar_stream_latents(tt_ar* e, int B, int n, float* out, void* stream) {
  TT_REQUIRE(e && out, "tt_ar_stream_latents: null argument");
  TT_REQUIRE(e->lat != nullptr, "tt_ar_stream_latents: this handle was created with max_batch %d > 8 (no per-step latent capture)", e->cfg.max_batch);
  if (e->sessions) {  // [S][n][D]: row r's latents 0 .. n - 1, each row counted from its own admission
    int most = 0;
    for (int r = 0; r < e->cfg.max_batch; ++r) most = std::max(most, e->s_n[r]);
    TT_REQUIRE(B == e->cfg.max_batch && n >= 1 && n <= std::max(most, 1), "tt_ar_stream_latents: %d x %d latents requested, the sessions hold %d x at most %d", B, n,
               e->cfg.max_batch, most);
    return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
      const size_t row = (size_t)e->D * sizeof(float);
      for (int r = 0; r < B; ++r)
        TT_CHECK_HIP(hipMemcpy2DAsync(out + (size_t)r * n * e->D, row, e->lat + (size_t)r * e->D, (size_t)B * row, row, (size_t)n, hipMemcpyDeviceToDevice, s));
      return 0;
    });
  }
  TT_REQUIRE(B >= 1 && B <= e->lat_batch && B == e->B && n >= 1 && n <= e->gen_done, "tt_ar_stream_latents: %d x %d latents requested, generation holds %d x %d", B, n, e->B, e->gen_done);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    const size_t row = (size_t)e->D * sizeof(float);
    for (int b = 0; b < B; ++b) {
      float* dst = out + (size_t)b * n * e->D;
      // latent 0 is the start-token row of the shared prefill (one copy for every sequence)
      TT_CHECK_HIP(hipMemcpyAsync(dst, e->lat, row, hipMemcpyDeviceToDevice, s));
      if (n > 1)
        TT_CHECK_HIP(hipMemcpy2DAsync(dst + e->D, row, e->lat + ((size_t)e->lat_batch + b) * e->D, (size_t)e->lat_batch * row, row, (size_t)(n - 1),
                                      hipMemcpyDeviceToDevice, s));
    }
    return 0;
  });
}

int tt_ar_latents(tt_ar* e, const float* emb, int k, int n, float* out, void* stream) {
  TT_REQUIRE(e && emb && out && k >= 1 && n >= 1, "tt_ar_latents: bad arguments");
  TT_REQUIRE(k * n <= e->max_rows && k <= e->cfg.max_batch, "tt_ar_latents: %d x %d rows exceed capacity %d", k, n, e->max_rows);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    const int D = e->D, M = k * n;
    TT_CHECK_HIP(hipMemcpyAsync(e->x, emb, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    TT_TRY(gpt_trunk_full(e, k, n, false, s));
    RowNormArgs a = ar_norm_args(e, e->x, nullptr, M, ar_head_ln(e));  // the latents are the f32 rows alone
    a.out_f32 = out; a.ldo32 = D;
    a.row_blocks = 0;  // (a teacher-forced pass of >= 1024 rows takes the wave-per-row kernel)
    TT_TRY(rownorm_launch(e->cfg.dtype, a, s));
    return e->guard.snapshot(s);
  });
}

// Operand-overflow guard (fp16 operands saturate at 65504): row norms / sampler launches that met a non-finite value since the
// last reset, as of the end of the last finished tt_ar_generate[_chunk] (which synchronise) or tt_ar_latents (after the caller
// synchronised its stream).  reset != 0 clears the counter.  Returns the count (>= 0) or a negative error.
int tt_ar_guard(tt_ar* e, int reset) {
  if (!e) { set_error("tt_ar_guard: null handle"); return -1; }
  return e->read_guard(reset, "tt_ar_guard", "autoregressive", e->cfg.dtype);
}

// Counters for tests / diagnostics: 0 = decode-step graph captures so far, 1 = queue drains of the launch loop (expected 0),
// 2 = kernel launches of one decode step (layers + head + sampler + step counter).
int tt_ar_stat(tt_ar* e, int which) {
  if (!e) { set_error("tt_ar_stat: null handle"); return -1; }
  const int per_step = (ar_fused_qkv_attn(e) ? 6 : 7) * e->cfg.layers + 4 + (e->typical ? 1 : 0) + (e->sessions && (e->sess_launch & SAMPLE_ROWS_WIDE) ? 1 : 0);
  int captures = e->step.captures;
  for (const KeptGraph& g : e->sess_steps) captures += g.captures;
  return which == 0 ? captures : which == 1 ? e->drains : which == 2 ? per_step : -1;
}

// Engine options of a handle (defaults in brackets):
//   TT_AR_OPT_LOOKAHEAD      [6]  decode steps the host may run ahead of the device (>= 1)
//   TT_AR_OPT_SESSIONS       [0]  1: the handle serves streaming sessions, one per row (fresh handles of <= 4 rows, 16-bit, max_groups >= max_batch)
//                                 2: the same on a wide handle of <= 16 rows
//   TT_AR_OPT_SESSION_CLOSE       retire the session in slot `value` of a session handle
//   TT_AR_OPT_SESSION_SAMPLING [0] 1: tt_ar_generate_chunk takes one tt_sampling per slot (session handles, before the first admission)
//   TT_AR_OPT_FUSED_QKV_ATTN [1]  0: eligible batches keep the QKV GEMM and the decode attention as two launches (A/B runs; same codes)
int tt_ar_set_option(tt_ar* e, int option, int value) {
  TT_REQUIRE(e != nullptr, "tt_ar_set_option: null handle");
  switch (option) {
    case TT_AR_OPT_LOOKAHEAD:
      TT_REQUIRE(value >= 1 && value <= 64, "tt_ar_set_option: lookahead %d outside 1 .. 64", value);
      e->lookahead = value;
      break;
    case TT_AR_OPT_SESSIONS: {
      const tt_ar_config& c = e->cfg;
      TT_REQUIRE((value == 1 || value == 2) && !e->sessions, "tt_ar_set_option: sessions are switched on once, with value 1 or 2 (got %d)", value);
      if (value == 1)
        TT_REQUIRE(c.max_batch <= 4 && c.dtype != DT_F32 && c.max_groups >= c.max_batch && e->D == 1024,
                   "tt_ar_set_option: sessions need max_batch <= 4, 16-bit operands, max_groups >= max_batch and model_dim 1024 (max_batch %d, dtype %d, max_groups %d)",
                   c.max_batch, c.dtype, c.max_groups);
      else  // a wide session handle: the same conditions, up to 16 rows
        TT_REQUIRE(c.max_batch <= 16 && c.dtype != DT_F32 && c.max_groups >= c.max_batch && e->D == 1024,
                   "tt_ar_set_option: wide sessions need max_batch <= 16, 16-bit operands, max_groups >= max_batch and model_dim 1024 (max_batch %d, dtype %d, "
                   "max_groups %d)",
                   c.max_batch, c.dtype, c.max_groups);
      TT_REQUIRE(e->P1 == 0 && e->step.captures == 0 && !e->step.exec, "tt_ar_set_option: sessions must be switched on before the first prefill");
      // a session row stages its whole prefix capacity in the decode attention's LDS (about 600 prefix rows at 500 tokens)
      TT_REQUIRE(decode_attention_session_lds(c.max_prefix, e->tmax) <= DECODE_LDS_CAP,
                 "tt_ar_set_option: sessions need the prefix capacity in the attention's LDS: max_prefix %d with %d KV slots needs %zu bytes, %zu available",
                 c.max_prefix, e->tmax, decode_attention_session_lds(c.max_prefix, e->tmax), DECODE_LDS_CAP);
      int rc = e->arena.alloc_t(&e->sess, (size_t)4 * c.max_batch);
      if (!rc && e->lat_batch < c.max_batch) {  // (tt_ar_create files streaming latents for handles of <= 8 rows)
        e->lat_batch = c.max_batch;
        rc = e->arena.alloc_t(&e->lat, (size_t)(e->tmax + 1) * e->lat_batch * e->D);
      }
      if (!rc) rc = e->arena.alloc_t(&e->pre_logits, (size_t)c.max_batch * e->Vp);
      if (!rc && hipHostMalloc((void**)&e->sess_host, (size_t)4 * c.max_batch * sizeof(int)) != hipSuccess) {
        set_error("tt_ar_set_option: hipHostMalloc failed");
        rc = -2;
      }
      TT_TRY(rc);
      // (arena memory is zeroed: every row starts SESS_FREE.  The slot plane of a free row must read -1)
      TT_CHECK_HIP(hipMemset(e->sess + SESS_SLOT * c.max_batch, 0xff, (size_t)c.max_batch * sizeof(int)));
      TT_CHECK_HIP(hipDeviceSynchronize());
      // the GEMV-shaped step of a <= 4-sequence handle (wide: <= 16), for the whole life of the handle (its level as tt_ar_create picks it)
      e->gemv = tt::g_ar_gemv ? tt::g_ar_gemv : 2;
      e->sessions = value;
      e->B = c.max_batch;
      memset(e->s_n, 0, sizeof(e->s_n));
      memset(e->s_run, 0, sizeof(e->s_run));
      break;
    }
    case TT_AR_OPT_FUSED_QKV_ATTN:
      TT_REQUIRE(value == 0 || value == 1, "tt_ar_set_option: TT_AR_OPT_FUSED_QKV_ATTN takes 0 or 1 (got %d)", value);
      e->fused_qkv = value;
      break;
    case TT_AR_OPT_SESSION_SAMPLING:
      TT_REQUIRE(e->sessions, "tt_ar_set_option: TT_AR_OPT_SESSION_SAMPLING needs a session handle (TT_AR_OPT_SESSIONS)");
      TT_REQUIRE(value == 1 && !e->sess_sampling, "tt_ar_set_option: per-session sampling is switched on once, with value 1 (got %d)", value);
      TT_REQUIRE(e->admissions == 0, "tt_ar_set_option: per-session sampling must be switched on before the first admission");
      e->sess_sampling = 1;
      break;
    case TT_AR_OPT_SESSION_CLOSE:
      TT_REQUIRE(e->sessions, "tt_ar_set_option: TT_AR_OPT_SESSION_CLOSE needs a session handle (TT_AR_OPT_SESSIONS)");
      TT_REQUIRE(value >= 0 && value < e->cfg.max_batch && e->s_run[value] != SESS_FREE, "tt_ar_set_option: slot %d holds no session to close", value);
      TT_TRY(ar_sess_close_launch(e->sess, e->cfg.max_batch, value, e->sb.own));
      e->s_run[value] = SESS_FREE;
      e->s_n[value] = 0;
      e->s_key_pending[value] = false;
      break;
    default: TT_REQUIRE(false, "tt_ar_set_option: unknown option %d", option);
  }
  return 0;
}

}  // extern "C"
