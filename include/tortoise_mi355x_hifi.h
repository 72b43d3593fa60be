/*
 * Batched HiFi-GAN decoding of the streaming path: several latent sequences of different lengths, each with its own conditioning
 * vector, decoded in one pass of csrc/hifigan.hip.  tt_hifi_run (tortoise_mi355x.h) is the one-sequence case of the same code, and
 * every sequence of a batch comes out bit-identical to decoding it alone.
 *
 * Layout: every sequence gets a slot of P0 = tt_hifi_output_frames(max T_i) + 1 interpolated frames (P0 * prod(up_factor[0..i))
 * rows at upsampling stage i); the tap convolutions stop at each sequence's own length, so the padding never reaches a valid sample.
 * A batch fits a handle when n * P0 <= tt_hifi_batch_capacity(h) = tt_hifi_output_frames(max_latents) + 1 and n <= TT_HIFI_MAX_BATCH:
 * max_latents is a per-call budget of padded slots.  The handle's HBM is sized by that budget alone (about 1.16 GB for max_latents = 508
 * at the reference's widths, computed from the buffer formulas, not measured), so batching adds no memory; a batch of sequences
 * of very different lengths is better split by length (the Python stage does).
 *
 * A separate header with its own version and struct-size query (tortoise_mi355x.h is frozen at its ABI version); exported from the
 * same library.
 */
#ifndef TORTOISE_MI355X_HIFI_H
#define TORTOISE_MI355X_HIFI_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_HIFI_MAX_BATCH 64

int tt_hifi_batch_abi_version(void);
size_t tt_hifi_batch_struct_size(int which);  /* 0: tt_hifi_config, 1: tt_hifi_weights, 2: tt_hifi_resblock (the structs tt_hifi_create takes) */
/* Padded interpolated frames one call may hold: n * (tt_hifi_output_frames(max T_i) + 1) must not exceed it. */
int tt_hifi_batch_capacity(const tt_hifi* h);
/* n sequences (1 <= n <= TT_HIFI_MAX_BATCH): latents device f32 [sum T_i][in_channels] back to back, lengths HOST int [n] (T_i >= 1),
 * g device f32 [n][cond_channels] -> wav device f32 [sum S_i] back to back, S_i = tt_hifi_output_frames(T_i) * prod(up_factor).
 * Asynchronous on `stream`. */
int tt_hifi_run_batch(tt_hifi* h, int n, const float* latents, const int* lengths, const float* g, float* wav, void* stream);

#ifdef __cplusplus
}
#endif
#endif
