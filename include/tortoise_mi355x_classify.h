/*
 * Tortoise detector: classify_audio_clip (reference tortoise/api.py, tortoise/is_this_from_tortoise.py).
 *
 * AudioMiniEncoderWithClassifierHead(2, spec_dim=1, embedding_dim=512, depth=5, downsample_factor=4, resnet_blocks=2, attn_blocks=4,
 * num_attn_heads=4, base_channels=32, dropout=0, kernel_size=5) from tortoise/models/classifier.py over one 24 kHz clip:
 *   Conv1d(1, 32, 3, pad 1)
 *   -> per level l = 0..4 at C = 32 * 2^l: 2 x ResBlock (x + conv5(SiLU(GN(conv5(SiLU(GN(x))))))) then Conv1d(C, 2C, 5, stride 4, pad 2)
 *   -> GroupNorm(1024) -> SiLU -> Conv1d(1024, 512, 1)
 *   -> 4 x AttentionBlock(512, 4 heads of 128, legacy [q|k|v] per head, no relative position bias)
 *   -> frame 0 -> Linear(512, 2).
 * GroupNorm has 16 groups at 32 and 64 channels and 32 above (arch_util.normalization), eps 1e-5, f32 statistics.
 * A separate model from its own weight file, so it has its own header, version and struct sizes; it is exported from the same
 * library as tortoise_mi355x.h.
 */
#ifndef TORTOISE_MI355X_CLASSIFY_H
#define TORTOISE_MI355X_CLASSIFY_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_CLS_DEPTH 5
#define TT_CLS_RES_BLOCKS 2
#define TT_CLS_ATTN_BLOCKS 4

typedef struct tt_cls_config {
  int dtype;               /* TT_BF16 / TT_F16 / TT_F32 (verification mode) */
  int spec_dim;            /* 1 */
  int base_channels;       /* 32 */
  int depth;               /* 5 */
  int resnet_blocks;       /* 2 */
  int kernel_size;         /* 5 */
  int downsample_factor;   /* 4 */
  int embedding_dim;       /* 512 */
  int attn_blocks;         /* 4 */
  int heads;               /* 4 */
  int classes;             /* 2 */
  int max_samples;         /* longest clip tt_cls_run accepts */
} tt_cls_config;

typedef struct tt_cls_resblock {
  const float* gn1_g; const float* gn1_b;  /* in_layers.0 */
  const void* w1; const float* b1;         /* in_layers.2: T [C][5][C] ([out][tap][in]) */
  const float* gn2_g; const float* gn2_b;  /* out_layers.0 */
  const void* w2; const float* b2;         /* out_layers.3 */
} tt_cls_resblock;

typedef struct tt_cls_attn {
  const float* norm_g; const float* norm_b;
  const void* w_qkv; const float* b_qkv;   /* T [1536][512], legacy per-head [q|k|v] rows */
  const void* w_proj; const float* b_proj; /* T [512][512] */
} tt_cls_attn;

typedef struct tt_cls_weights {
  const float* w_init; const float* b_init;                    /* f32 [32][3], [32] */
  tt_cls_resblock res[TT_CLS_DEPTH][TT_CLS_RES_BLOCKS];
  const void* w_down[TT_CLS_DEPTH]; const float* b_down[TT_CLS_DEPTH]; /* T [2C][5][C] */
  const float* final_g; const float* final_b;                  /* enc.final.0: GroupNorm(1024) */
  const void* w_final; const float* b_final;                   /* enc.final.2: T [512][1024] */
  tt_cls_attn attn[TT_CLS_ATTN_BLOCKS];
  const float* w_head; const float* b_head;                    /* f32 [2][512], [2] */
} tt_cls_weights;

typedef struct tt_cls tt_cls;

int tt_cls_abi_version(void);
size_t tt_cls_struct_size(int which);  /* 0: tt_cls_config, 1: tt_cls_weights */
/* Longest clip any handle can take: beyond it a 32-bit element offset of the widest activation would overflow. */
int tt_cls_max_samples(void);

int tt_cls_create(const tt_cls_config* cfg, const tt_cls_weights* w, tt_cls** out);
void tt_cls_destroy(tt_cls* h);
/* clip: device f32 [n] at 24 kHz (1 <= n <= max_samples).  logits: device f32 [2] (head output of frame 0; the caller's softmax gives the
 * class probabilities).  embedding: optional device f32 [512] = enc(clip)[:, :, 0].  Asynchronous on `stream`. */
int tt_cls_run(tt_cls* h, const float* clip, int n, float* logits, float* embedding, void* stream);
/* Non-finite values the stage met during its last finished run (>= 0), or a negative error; reset != 0 clears the count. */
int tt_cls_guard(tt_cls* h, int reset);

#ifdef __cplusplus
}
#endif
#endif
