/*
 * wav2vec2 CTC aligner of the redaction path (tts() with [bracketed] text and enable_redaction=True).
 *
 * Reference: tortoise/utils/wav2vec_alignment.py (Wav2VecAlignment.align / redact) running
 * transformers.Wav2Vec2ForCTC("jbetker/wav2vec2-large-robust-ft-libritts-voxpopuli") on every returned clip.
 * The aligner is a separate model from its own weight source and only bracketed text uses it, so it has
 * its own header, version and struct sizes; it is exported from the same library as tortoise_mi355x.h.
 *
 * One clip of S samples at 24 kHz:
 *   torchaudio resample 24 kHz -> 16 kHz (2-phase polyphase FIR, taps from the host) -> (x - mean) / sqrt(var + 1e-7)
 *   -> feature encoder: Conv1d(1, 512, k0, s0) + LayerNorm + GELU, then 512 -> 512 convs (kernel conv_kernel[i], stride 2) + LayerNorm + GELU
 *   -> LayerNorm(512) -> Linear(512, dim) -> h + GELU(grouped Conv1d(dim, dim, pos_kernel, groups pos_groups)(h))
 *   -> `layers` pre-LN transformer layers (non-causal, q scaled by 1/8) -> LayerNorm -> lm_head -> per-frame argmax.
 * Only the configuration the reference uses is implemented (feat_extract_norm "layer", do_stable_layer_norm, conv_bias, erf GELU,
 * 64-wide heads); the host refuses any other config.json.
 */
#ifndef TORTOISE_MI355X_ALIGN_H
#define TORTOISE_MI355X_ALIGN_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_W2V_CONV_LAYERS 7

typedef struct tt_w2v_config {
  int dtype;                              /* TT_BF16 / TT_F16 / TT_F32 (verification mode) */
  int dim, heads, layers, ff_dim;         /* 1024, 16, 24, 4096 */
  int conv_dim;                           /* 512: every feature-encoder layer */
  int conv_kernel[TT_W2V_CONV_LAYERS];    /* 10, 3, 3, 3, 3, 2, 2 */
  int conv_stride[TT_W2V_CONV_LAYERS];    /* 5, 2, 2, 2, 2, 2, 2 */
  int pos_kernel, pos_groups;             /* 128, 16 */
  int vocab, vocab_pad;                   /* lm_head rows; vocab_pad = rows of the packed head (multiple of 64, zero rows past vocab) */
  int max_samples;                        /* longest 24 kHz clip tt_w2v_run accepts */
  float eps;                              /* layer_norm_eps of the encoder / feature projection (the conv LayerNorms use 1e-5) */
} tt_w2v_config;

typedef struct tt_w2v_weights {
  const float* resample_taps;             /* f32 [2][23]: torchaudio's sinc kernel for 24000 -> 16000 (lowpass width 6, rolloff 0.99) */
  const float* w_conv0;                   /* f32 [conv_dim][conv_kernel[0]] */
  const float* b_conv0;
  const void* w_conv[TT_W2V_CONV_LAYERS]; /* [1..6]: T [conv_dim][k][conv_dim] ([out][tap][in]); [0] unused */
  const float* b_conv[TT_W2V_CONV_LAYERS];
  const float* ln_conv_g[TT_W2V_CONV_LAYERS];
  const float* ln_conv_b[TT_W2V_CONV_LAYERS];
  const float* fp_ln_g; const float* fp_ln_b; /* feature_projection.layer_norm */
  const void* w_fp; const float* b_fp;    /* T [dim][conv_dim] */
  const void* w_pos; const float* b_pos;  /* T [pos_groups][dim/pos_groups][pos_kernel][dim/pos_groups]: weight norm folded */
  const tt_gpt_layer* layers_host;        /* HOST array of `layers` entries: ln1 = layer_norm, w_qkv = [q; k; v] [3 dim][dim] with bias,
                                           * w_proj = out_proj, ln2 = final_layer_norm, w_fc = intermediate_dense, w_proj2 = output_dense */
  const float* lnf_g; const float* lnf_b; /* encoder.layer_norm */
  const void* w_head; const float* b_head; /* T [vocab_pad][dim], f32 [vocab_pad] */
} tt_w2v_weights;

typedef struct tt_w2v tt_w2v;

int tt_align_abi_version(void);
size_t tt_align_struct_size(int which);  /* 0: tt_w2v_config, 1: tt_w2v_weights */

int tt_w2v_create(const tt_w2v_config* cfg, const tt_w2v_weights* w, tt_w2v** out);
void tt_w2v_destroy(tt_w2v* h);
/* Frames the model produces for a clip of `samples` samples at 24 kHz (0: shorter than the receptive field). */
int tt_w2v_frames(const tt_w2v* h, int samples);
/* audio: device f32 [samples] at 24 kHz.  frame_ids: device int32 [frames] = argmax over the vocabulary of every frame's logits (ties:
 * lowest index).  logits: optional device f32 [frames][vocab].  Asynchronous on `stream`. */
int tt_w2v_run(tt_w2v* h, const float* audio, int samples, int* frame_ids, float* logits, void* stream);
/* Non-finite values the stage met during its last finished run (>= 0), or a negative error; reset != 0 clears the count. */
int tt_w2v_guard(tt_w2v* h, int reset);

#ifdef __cplusplus
}
#endif
#endif
