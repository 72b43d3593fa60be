/*
 * Batched UnivNet vocoding: several mel spectrograms of different lengths, each with its own noise, rendered in one pass of
 * csrc/vocoder.hip + csrc/univnet.hip.  tt_voc_run (tortoise_mi355x.h) is the one-sequence case of the same code, and every sequence
 * of a batch comes out bit-identical to rendering it alone (bf16, fp16 and the fp32 verification mode).
 *
 * Layout: every sequence gets a slot of L_pad = max S_i + 10 mel frames (L_pad * hop audio-rate columns at each LVC block).  The ten
 * frames of -11.5129 follow each sequence's own last frame; the KernelPredictor tap convolutions, the reflect padding of conv_pre /
 * conv_post, the zero-padded dilated convolutions and the location-variable convolutions stop at each sequence's own length, so the
 * padding never reaches a valid sample.  A batch fits a handle when n * L_pad <= tt_voc_batch_capacity(h) = max_frames + 10 and
 * n <= TT_VOC_MAX_BATCH: max_frames is a per-call budget of padded slots.  The handle's HBM is sized by that budget alone - about
 * 150 KB per frame by the buffer formulas of tt_voc_create (49 KB of predicted kernels in the 16-bit operand type + three 32-channel
 * f32 audio-rate rows of 256 samples), i.e. about 0.33 GB per full-length slot (2186 frames at max_mel_tokens = 500) and about 5.2 GB
 * for sixteen of them; computed, not measured - so batching adds no memory.  A batch of sequences of very different lengths is better
 * split by length (the Python stage does).
 *
 * A separate header with its own version and struct-size query (tortoise_mi355x.h is frozen at its ABI version); exported from the
 * same library.
 */
#ifndef TORTOISE_MI355X_UNIVNET_H
#define TORTOISE_MI355X_UNIVNET_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_VOC_MAX_BATCH 32

int tt_voc_batch_abi_version(void);
size_t tt_voc_batch_struct_size(int which);  /* 0: tt_voc_config, 1: tt_voc_weights, 2: tt_voc_block (the structs tt_voc_create takes) */
/* Padded mel frames one call may hold: n * (max S_i + 10) must not exceed it. */
int tt_voc_batch_capacity(const tt_voc* h);
/* n sequences (1 <= n <= TT_VOC_MAX_BATCH): mel HOST array of n device pointers, f32 [mel_channels][S_i] each; S HOST int [n] (S_i >= 1);
 * z HOST array of n device pointers, f32 [64][S_i + 10] each -> audio HOST array of n device pointers, f32 [S_i * 256] each.
 * Asynchronous on `stream`; the overflow guard (tt_voc_guard) is snapshot once per call. */
int tt_voc_run_batch(tt_voc* h, int n, const float* const* mel, const int* S, const float* const* z, float* const* audio, void* stream);

#ifdef __cplusplus
}
#endif
#endif
