/*
 * CTC forced alignment (Viterbi) of a known text against per-frame logits, on the device: where in the audio every character is spoken.
 * The logits are what tt_w2v_run (tortoise_mi355x_align.h) returns with `logits` set; one call takes a ragged batch of clips and every
 * clip's outputs are bit-identical to running it alone.
 *
 *   states    s = 0 .. 2L for a target of L tokens: even states are blank, odd state 2l + 1 is token l
 *   start     a[0][0] = lp[0][blank], a[0][1] = lp[0][y_0], every other state -inf        (lp = the f32 log-softmax of the frame's logits)
 *   step      a[t][s] = lp[t][lab(s)] + best(a[t-1][s], a[t-1][s-1], a[t-1][s-2]); the skip from s - 2 only for odd s with lab(s) != lab(s-2)
 *   ties      staying wins over s - 1, s - 1 wins over s - 2: a move needs a strictly greater value
 *   end       state 2L, unless a[T-1][2L-1] is strictly greater
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_CTC_H
#define TORTOISE_MI355X_CTC_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_CTC_MAX_TOKENS 511  /* longest target: 2 * 511 + 1 = 1023 states, 16 per lane of one wave */
#define TT_CTC_MAX_VOCAB 2048
#define TT_CTC_MAX_CLIPS 1024

/* per-clip status */
#define TT_CTC_OK 0
#define TT_CTC_INFEASIBLE 1 /* fewer frames than tokens + adjacent repeats: no path exists */
#define TT_CTC_EMPTY 2      /* empty target or no frames */
#define TT_CTC_REFUSED 3    /* the clip exceeds the handle (frames, tokens) or a target id is the blank / outside the vocabulary */

typedef struct tt_ctc tt_ctc;

int tt_ctc_abi_version(void);

/* max_frames >= 1, 1 <= max_tokens <= TT_CTC_MAX_TOKENS, 1 <= max_clips <= TT_CTC_MAX_CLIPS, 2 <= vocab <= TT_CTC_MAX_VOCAB, 0 <= blank < vocab.
 * The handle owns the backpointer workspace (256 bytes per frame and clip). */
int tt_ctc_create(int max_frames, int max_tokens, int max_clips, int vocab, int blank, tt_ctc** out);
void tt_ctc_destroy(tt_ctc* h);

/* Ragged batch of n clips (1 <= n <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   logits    f32 [frame_off[n]][vocab]  rows of clip i: frame_off[i] .. frame_off[i+1]; finite values
 *   targets   i32 [tok_off[n]]           token ids of clip i: tok_off[i] .. tok_off[i+1]; never == blank
 *   frame_off, tok_off  i32 [n + 1], non-decreasing from 0
 * out:
 *   path      i32 [frame_off[n]]         state index 0 .. 2L of every frame
 *   spans     i32 [tok_off[n]][2]        first and last frame of every token
 *   conf      f32 [tok_off[n]]           mean over the token's frames of exp(lp[t][token])
 *   score     f32 [n]                    sum over the frames of lp[t][lab(path[t])]
 *   status    i32 [n]                    TT_CTC_*; a clip whose status is not TT_CTC_OK gets its status written and nothing else */
int tt_ctc_align(tt_ctc* h, int n, const float* logits, const int* frame_off, const int* targets, const int* tok_off, int* path, int* spans,
                 float* conf, float* score, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
