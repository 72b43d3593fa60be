// CVVP candidate scoring - the optional second ranking model of tts(cvvp_amount > 0) (reference: tortoise/models/cvvp.py:63-131,
// driven per conditioning clip at tortoise/api.py:464-472).  Two CollapsingTransformers (cvvp.py:19-51):
//   conditioning side: mel clip [80][T] -> Conv1d(k 5, stride 2) -> Conv1d(k 3, stride 2) -> tower -> to_conditioning_latent
//   speech side:       candidate codes -> embedding -> tower -> to_speech_latent
//   tower: the x-transformers Encoder CLVP also uses (xenc.h; ff_mult = 1) -> LayerNorm -> 1x1 conv -> AttentionBlock (GroupNorm32, 64-wide
//          heads, no relative positions) -> 1x1 conv -> mean over time
// score[b] = mean over clips of <normalize(cond latent), normalize(speech latent b)> * exp(temperature).  The conditioning latent of a clip
// does not depend on the candidate, so it is evaluated once per clip (the reference repeats the clip B times).  Nothing here is a new kernel:
// the stage is composed of the engine's GEMM / norm / flash / rotary launches in the token-major layout of the other stages; a stride-2
// convolution is the stride-1 tap GEMM followed by an even-row gather (stage_blocks.h conv_stride2, shared with cond.hip), and the
// AttentionBlock and the pooled-latent tail are stage_blocks.h attention_block / pooled_latent.
#include "xenc.h"

using namespace tt;

struct CvvpTower {
  tt_cvvp_tower w;
  std::vector<tt_clvp_layer> L;
};

struct tt_cvvp : EngineHandle {  // guard: bumped by the row norms / GroupNorm statistics, snapshot at the end of every tt_cvvp_score
  tt_cvvp_config cfg;
  tt_cvvp_weights w;
  CvvpTower cond, speech;
  size_t rows = 0;
  float* x = nullptr; void* h = nullptr; void* gg = nullptr; void* attn = nullptr;
  void* q = nullptr; void* k = nullptr; void* vt = nullptr;
  float* ha = nullptr; float* hb = nullptr;   // [rows][dim] f32 streams of the pre_combiner
  void* act = nullptr;                        // [rows][dim] T
  float* gn_partial = nullptr;
  float* pooled = nullptr; void* pooled_t = nullptr;
  float* cond_latent = nullptr;               // [16][dim]
  float* speech_latent = nullptr;             // [max sequences][dim]
  float* clip_scores = nullptr;               // [16][max sequences]
  float* mel_t = nullptr; void* mel_op = nullptr; void* c0 = nullptr; void* c0e = nullptr;  // conditioning front: [T][mel], [T][mel_pad], [T][dim/2], [T/2][dim/2]
  int* even_idx = nullptr;
  int max_seqs = 0;
};

// e->x holds the embedded rows [B * n][dim]; leaves the tower's latent rows in latent_out [B][dim]
static int cvvp_tower_run(tt_cvvp* e, const CvvpTower& t, int B, int n, float* latent_out, hipStream_t s) {
  const int D = e->cfg.dim, H = e->cfg.heads, dt = e->cfg.dtype;
  const int M = B * n;
  XencBufs xb{e->x, e->h, e->gg, e->attn, e->q, e->k, e->vt, e->guard.dev};
  TT_TRY(xenc_layers_run(dt, xb, t.L.data(), e->cfg.depth, t.w.inv_freq, D, H, D, e->cfg.rot_dim, B, n, s));
  TT_TRY(rownorm_launch(dt, layernorm_args(e->x, M, D, t.w.norm_g, t.w.norm_b, 1e-5f, ACT_NONE, e->h, nullptr, e->guard.dev), s));
  // pre_combiner.0
  TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->h, D, t.w.w_pre0, D, M, D, D, t.w.b_pre0, e->ha), s));
  // pre_combiner.1: AttentionBlock, one GroupNorm sample per sequence.  (attention_block applies the block's relpos table when the weights
  // carry one; the reference's CVVP block has none - tt_cvvp_tower documents relpos = NULL - so the flash launch gets the null it always got.)
  const AttnBlockBufs ab{e->act, e->q, e->k, e->vt, e->attn, e->gn_partial, e->guard.dev};
  TT_TRY(attention_block(dt, t.w.attn, e->ha, e->hb, B, n, D, H, ab, s));
  // pre_combiner.2, then masked_mean with the all-ones eval mask (cvvp.py:46-51)
  TT_TRY(cast_pad_launch(dt, e->hb, D, e->act, D, M, D, D, s));
  TT_TRY(gemm_launch(dt, EPI_STD, gemm_f32_args(e->act, D, t.w.w_pre2, D, M, D, D, t.w.b_pre2, e->ha), s));
  return pooled_latent(dt, e->ha, B, n, D, t.w.w_latent, D, e->pooled, e->pooled_t, latent_out, s);
}

extern "C" {

int tt_cvvp_create(const tt_cvvp_config* cfg, const tt_cvvp_weights* w, tt_cvvp** out) {
  TT_REQUIRE(cfg && w && out, "tt_cvvp_create: null argument");
  TT_REQUIRE(cfg->dtype == DT_BF16 || cfg->dtype == DT_F16 || cfg->dtype == DT_F32, "tt_cvvp_create: unknown dtype %d", cfg->dtype);
  TT_REQUIRE(cfg->heads * 64 == cfg->dim && cfg->dim % 128 == 0 && cfg->depth >= 1, "tt_cvvp_create: unsupported dims (64-wide heads, dim a multiple of 128)");
  TT_REQUIRE(cfg->mel_pad % 64 == 0 && cfg->mel_pad >= cfg->mel_channels && cfg->max_rows >= 64 && cfg->max_cond_frames >= 32, "tt_cvvp_create: bad shape");
  TT_REQUIRE(w->speech_emb && w->temperature && w->w_cond0 && w->w_cond1 && w->cond.layers_host && w->speech.layers_host, "tt_cvvp_create: null weight");
  tt_cvvp* e = new tt_cvvp();
  e->cfg = *cfg;
  e->w = *w;
  e->cond.w = w->cond; e->cond.L.assign(w->cond.layers_host, w->cond.layers_host + cfg->depth);
  e->speech.w = w->speech; e->speech.L.assign(w->speech.layers_host, w->speech.layers_host + cfg->depth);
  const int D = cfg->dim;
  const size_t es = dtype_bytes(cfg->dtype);
  const size_t rows = (size_t)std::max(cfg->max_rows, cfg->max_cond_frames) + 64;
  e->rows = rows;
  e->max_seqs = cfg->max_rows / 8 + 8;  // a candidate has >= 8 codes
  int rc = e->open("tt_cvvp_create", true);
  if (!rc) rc = e->arena.alloc_t(&e->x, rows * D);
  if (!rc) rc = e->arena.alloc(&e->h, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->gg, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->attn, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->q, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->k, rows * D * es);
  if (!rc) rc = e->arena.alloc(&e->vt, (size_t)D * (rows + 32 * (size_t)e->max_seqs) * es);
  if (!rc) rc = e->arena.alloc_t(&e->ha, rows * D);
  if (!rc) rc = e->arena.alloc_t(&e->hb, rows * D);
  if (!rc) rc = e->arena.alloc(&e->act, rows * D * es);
  if (!rc) rc = e->arena.alloc_t(&e->gn_partial, groupnorm_partial_floats_rows(rows));  // any number of sequences in `rows` rows
  if (!rc) rc = e->arena.alloc_t(&e->pooled, (size_t)e->max_seqs * D);
  if (!rc) rc = e->arena.alloc(&e->pooled_t, (size_t)e->max_seqs * D * es);
  if (!rc) rc = e->arena.alloc_t(&e->cond_latent, (size_t)16 * D);
  if (!rc) rc = e->arena.alloc_t(&e->speech_latent, (size_t)e->max_seqs * D);
  if (!rc) rc = e->arena.alloc_t(&e->clip_scores, (size_t)16 * e->max_seqs);
  const size_t cf = (size_t)cfg->max_cond_frames + 64;
  if (!rc) rc = e->arena.alloc_t(&e->mel_t, cf * cfg->mel_pad);
  if (!rc) rc = e->arena.alloc(&e->mel_op, cf * cfg->mel_pad * es);
  if (!rc) rc = e->arena.alloc(&e->c0, cf * (D / 2) * es);
  if (!rc) rc = e->arena.alloc(&e->c0e, cf * (D / 2) * es);
  if (!rc) rc = e->arena.alloc_t(&e->even_idx, cf);
  if (!rc) rc = even_rows_index_launch(e->even_idx, (int)cf, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) { set_error("tt_cvvp_create: index fill failed"); rc = -2; }
  if (rc) {
    tt_cvvp_destroy(e);
    return rc;
  }
  *out = e;
  return 0;
}

void tt_cvvp_destroy(tt_cvvp* e) {
  if (!e) return;
  e->close();
  delete e;
}

int tt_cvvp_score(tt_cvvp* e, const float* mels, int n_clips, int T, const int* codes, int B, int n, float* scores, void* stream) {
  TT_REQUIRE(e && mels && codes && scores, "tt_cvvp_score: null argument");
  TT_REQUIRE(n_clips >= 1 && n_clips <= 16 && T >= 29 && T <= e->cfg.max_cond_frames, "tt_cvvp_score: %d clips of %d frames (1 .. 16 clips, 29 .. %d frames)", n_clips, T, e->cfg.max_cond_frames);
  TT_REQUIRE(B >= 1 && n >= 8 && (size_t)B * n <= (size_t)e->cfg.max_rows && B <= e->max_seqs, "tt_cvvp_score: B=%d n=%d exceed capacity %d rows (n must be >= 8)", B, n, e->cfg.max_rows);
  return e->sb.run((hipStream_t)stream, [&](hipStream_t s) -> int {
    const int D = e->cfg.dim, D2 = D / 2, MC = e->cfg.mel_channels, MP = e->cfg.mel_pad, dt = e->cfg.dtype;
    const int T2 = (T + 1) / 2, T3 = (T2 + 1) / 2;  // Conv1d(stride 2) with "same" padding: ceil(n / 2) outputs, output j = the stride-1 result at 2 j
    for (int c = 0; c < n_clips; ++c) {
      TT_TRY(mel_operand(dt, mels + (size_t)c * MC * T, MC, MP, T, e->mel_t, e->mel_op, s));
      TT_TRY(conv_stride2(dt, e->mel_op, MP, e->w.w_cond0, 5, T, D2, e->w.b_cond0, e->c0, e->c0e, false, e->even_idx, s));
      TT_TRY(conv_stride2(dt, e->c0e, D2, e->w.w_cond1, 3, T2, D, e->w.b_cond1, e->ha, e->x, true, e->even_idx, s));
      TT_TRY(cvvp_tower_run(e, e->cond, 1, T3, e->cond_latent + (size_t)c * D, s));
    }
    TT_TRY(gather_rows_launch(e->w.speech_emb, codes, e->x, B * n, D, s));
    TT_TRY(cvvp_tower_run(e, e->speech, B, n, e->speech_latent, s));
    for (int c = 0; c < n_clips; ++c)
      TT_TRY(clvp_score_launch(e->cond_latent + (size_t)c * D, 1, e->speech_latent, e->w.temperature, e->clip_scores + (size_t)c * B, B, D, s));
    TT_TRY(mean_rows_launch(e->clip_scores, scores, 1, n_clips, B, s));                   // mean over the clips (api.py:468)
    return e->guard.snapshot(s);
  });
}

int tt_cvvp_guard(tt_cvvp* e, int reset) {
  if (!e) { set_error("tt_cvvp_guard: null handle"); return -1; }
  return e->read_guard(reset, "tt_cvvp_guard", "CVVP", e->cfg.dtype);
}

}  // extern "C"
