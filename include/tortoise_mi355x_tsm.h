/*
 * Speaking-rate control: WSOLA time-scale modification (waveform-similarity overlap-add; Verhelst & Roelands 1993) of 24 kHz f32 audio on
 * the device.  The duration changes, the pitch does not.  One call takes a ragged batch of clips, each with its own rate, and every
 * clip's outputs are bit-identical to running it alone.
 *
 *   constants  W = 768 (window, 32 ms), Hs = 384 (synthesis hop), search offsets d = -256 .. 255 (512 candidates: one period down to 47 Hz),
 *              w[j] = 0.5 - 0.5 cos(2 pi j / W), the periodic Hann window: w[j] + w[j + Hs] = 1.  Samples outside [0, n) read as 0.
 *   rate       fixed point, rq = round(rate * 65536), 32768 <= rq <= 131072 (rate 0.5 .. 2.0): host and device agree on every integer
 *   n_out      max(1, (n * 65536 + rq / 2) / rq)                  (integer division, 64-bit)
 *   frames     K = ceil(n_out / Hs) + 1; frame k covers the output samples [(k - 1) Hs, (k + 1) Hs)
 *   nominal    a_k = ((k - 1) * Hs * rq + 32768) >> 16 for k >= 1  (64-bit)
 *   start      p_0 = -Hs, d_0 = 0: the first hop of the output is the input's
 *   step       for k >= 1, with the template t_j = x[p_(k-1) + Hs + j], j < W (what would follow the previous frame naturally):
 *                c(d) = sum_j t_j x[a_k + d + j]      E(d) = sum_j x[a_k + d + j]^2      s(d) = c(d) / sqrt(E(d) + 1e-20)
 *                p_k = a_k + argmax_d s(d)
 *   ties       the smaller |d| wins, and of +-d the negative one: all-zero audio takes d = 0 everywhere
 *   output     y[m] = sum_k w[m - (k - 1) Hs] x[p_k + m - (k - 1) Hs], m < n_out: exactly two frames cover each sample
 *
 * All arithmetic is f32 (sums in ascending j, one fused multiply-add per term; correctly rounded sqrt and division); the window is
 * computed in fp64 on the host, rounded to f32 and uploaded at create.  At rate 1 the normalised score makes d = 0 a maximiser
 * (Cauchy-Schwarz): the output is the input.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_TSM_H
#define TORTOISE_MI355X_TSM_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_TSM_WINDOW 768
#define TT_TSM_HOP 384
#define TT_TSM_SEARCH 256        /* offsets -TT_TSM_SEARCH .. TT_TSM_SEARCH - 1 */
#define TT_TSM_RATE_ONE 65536    /* rq of rate 1.0 */
#define TT_TSM_RATE_MIN 32768    /* rq of rate 0.5 */
#define TT_TSM_RATE_MAX 131072   /* rq of rate 2.0 */
#define TT_TSM_SAMPLE_RATE 24000
#define TT_TSM_MAX_SAMPLES 8388608 /* longest clip a handle can be made for (2^23 samples, 5.8 minutes) */
#define TT_TSM_MAX_CLIPS 64

/* per-clip status */
#define TT_TSM_OK 0
#define TT_TSM_EMPTY 1   /* a clip of no samples */
#define TT_TSM_REFUSED 2 /* the clip exceeds the handle's max_samples, its rq is outside TT_TSM_RATE_MIN .. TT_TSM_RATE_MAX, or its
                            slices of out / offsets do not have tt_tsm_out_samples / tt_tsm_frames entries */

typedef struct tt_tsm tt_tsm;

int tt_tsm_abi_version(void);

/* 1 <= max_samples <= TT_TSM_MAX_SAMPLES, 1 <= max_clips <= TT_TSM_MAX_CLIPS.  The handle owns the window table. */
int tt_tsm_create(int max_samples, int max_clips, tt_tsm** out);
void tt_tsm_destroy(tt_tsm* h);

/* Plain host functions (no device, no handle): n_out and K of a clip of n samples at rate rq; 0 for n < 1, n > TT_TSM_MAX_SAMPLES or an rq
 * outside the range. */
int tt_tsm_out_samples(int n, int rq);
int tt_tsm_frames(int n, int rq);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   rq        i32 [n_clips]              rate of clip i, 16.16 fixed point
 *   in_off, out_off, frame_off  i32 [n_clips + 1], non-decreasing from 0; clip i has tt_tsm_out_samples(n_i, rq_i) entries of out and
 *                                        tt_tsm_frames(n_i, rq_i) entries of offsets
 * out:
 *   out       f32 [out_off[n_clips]]     the stretched clips
 *   offsets   i32 [frame_off[n_clips]]   the chosen d_k of every frame, d_0 = 0
 *   status    i32 [n_clips]              TT_TSM_*; a clip whose status is not TT_TSM_OK gets its status written and nothing else */
int tt_tsm_stretch(tt_tsm* h, int n_clips, const float* audio, const int* in_off, const int* rq, float* out, const int* out_off, int* offsets,
                   const int* frame_off, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
