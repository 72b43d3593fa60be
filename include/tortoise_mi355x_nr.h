/*
 * Stationary-noise reduction of a voice clip by spectral subtraction on the device (csrc/denoise.hip).
 *
 * Meant for the clips a voice is cloned from: hiss or room noise in them ends in both conditioning latents.  The stage does not care about
 * the sample rate (voice clips arrive at 22.05 kHz, finished clips at 24 kHz); seconds become frames on the host.  All f32, N = n_fft,
 * H = hop, B = N / 2 + 1 bins, T = 1 + n / H frames:
 *
 *   1  re, im of frame t     tt_fmt's step 1: centred frames, reflect padding, the window folded into `basis`;
 *      P[t][b] = re^2 + im^2 as written: two products, one add, each rounded
 *   2  the noise power S[b] of the clip, one of
 *        auto    S[b] = P_(k)[b] * quantile_scale, P_(k)[b] the k-th smallest of P[0 .. T)[b] (k = 0: the minimum), k = tt_nr_rank: an EXACT
 *                order statistic - the k-th element of the device's own column sorted, ties and all; values are compared by bit pattern,
 *                as unsigned integers, which is the order of non-negative f32 and defined for every input.  quantile_scale is
 *                c = 1 / (-ln(1 - q)): the power of a stationary Gaussian noise bin is exponentially distributed, its q-quantile is
 *                -ln(1 - q) times its mean
 *        region  S[b] = the mean of P[t][b] over noise_first_frame <= t < noise_first_frame + noise_frames: an f32 sum in an order fixed
 *                by the range alone, divided by the count
 *   3  Pbar[t][b] = w sum_{dt = -Rt .. Rt} sum_{db = -Rb .. Rb} P[clamp(t + dt, 0, T - 1)][clamp(b + db, 0, B - 1)], dt the outer loop, both
 *      ascending, w = f32(1 / ((2 Rt + 1)(2 Rb + 1))): isolated cells do not survive as musical noise
 *   4  G[t][b] = g_min if Pbar <= beta S, else max(g_min, 1 - beta S / Pbar); 0 for b >= B
 *   5  Z = G (re, im), then tt_fmt's steps 6 and 7: the inverse with the synthesis window folded in, the overlap-add normalised by
 *      sum window^2 in increasing t, no atomics.  With G = 1 the chain is the identity to rounding.
 *
 * A clip with digital silence in more than a fraction q of its frames has an auto floor of exactly 0 and nothing is removed from it: give
 * such a clip a region.  The defaults of the Python layer come from this arithmetic and one synthetic family; NOBODY HAS RUN A REAL
 * RECORDING OR A TRAINED CHECKPOINT THROUGH THEM.
 *
 * One call takes several clips (ragged: offsets + lengths); every clip's samples and floor are bit-identical to running it alone.
 *
 * Its own header, version and struct sizes; exported from the same library as tortoise_mi355x.h.  Errors are reported through
 * tt_last_error(); every argument check happens before any device work, and a refused call writes nothing.
 */
#ifndef TORTOISE_MI355X_NR_H
#define TORTOISE_MI355X_NR_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_NR_MAX_CLIPS 16        /* clips of one tt_nr_run call */
#define TT_NR_MAX_SAMPLES 4194304 /* longest clip a handle can be made for */
#define TT_NR_MIN_FRAMES 32       /* auto mode: a clip of fewer frames is copied (TT_NR_SHORT) */
#define TT_NR_MIN_REGION 8        /* region mode: frames of the shortest region */
#define TT_NR_QUANTILE_DEN 10000  /* q = quantile_num / 10000 */
#define TT_NR_MAX_SMOOTH 4        /* Rt, Rb <= 4 */
#define TT_NR_REG_FRAMES 1024     /* frames the select holds in registers; longer clips make passes over the row */

#define TT_NR_OK 0      /* denoised */
#define TT_NR_SHORT 1   /* auto mode with fewer than TT_NR_MIN_FRAMES frames: the clip is copied bit for bit, its floor is 0 */
#define TT_NR_REFUSED 2 /* kept for callers that report per clip; tt_nr_run itself refuses the whole call (-1) and writes nothing */

typedef struct tt_nr_config {
  int n_fft;       /* frame length = window length; a multiple of hop and of 64 */
  int hop;         /* frame step; a multiple of 8 */
  int bins_pad;    /* >= n_fft / 2 + 1, a multiple of 32; table entries beyond n_fft / 2 are zero */
  int max_samples; /* longest clip (n_fft / 2 + 1 .. TT_NR_MAX_SAMPLES) */
  int max_clips;   /* clips per call (1 .. TT_NR_MAX_CLIPS) */
} tt_nr_config;

typedef struct tt_nr_tables {
  const float* basis;   /* device f32 [n_fft][2 * bins_pad]: tt_fmt_tables.basis */
  const float* inverse; /* device f32 [2 * bins_pad][n_fft]: tt_fmt_tables.inverse */
} tt_nr_tables;

typedef struct tt_nr_params {
  int quantile_num;     /* q = quantile_num / TT_NR_QUANTILE_DEN, 100 .. 5000 (0.01 .. 0.5) */
  float quantile_scale; /* c = f32(1 / (-ln(1 - q))), computed by the caller in fp64 and rounded once; finite, > 0 */
  float beta;           /* over-subtraction, 1 .. 4 */
  float g_min;          /* 10^(-reduction_db / 20): 0.01 <= g_min < 1 */
  int smooth_frames;    /* Rt, 0 .. TT_NR_MAX_SMOOTH */
  int smooth_bins;      /* Rb, 0 .. TT_NR_MAX_SMOOTH */
} tt_nr_params;

typedef struct tt_nr tt_nr;

int tt_nr_abi_version(void);
size_t tt_nr_struct_size(int which);  /* 0: tt_nr_config, 1: tt_nr_tables, 2: tt_nr_params */

/* The tables stay the caller's and must outlive the handle. */
int tt_nr_create(const tt_nr_config* cfg, const tt_nr_tables* tables, tt_nr** out);
void tt_nr_destroy(tt_nr* h);
/* Frames of a clip of n samples: 1 + n / hop. */
int tt_nr_frames(const tt_nr* h, int n);

/* Host arithmetic, no handle and no device (csrc/denoise_host.h).
 * tt_nr_rank: k = floor(q (frames - 1)) in integers, quantile_num * (frames - 1) / TT_NR_QUANTILE_DEN; -1 for an argument out of range.
 * tt_nr_region: the frames t < frames with start <= t hop and t hop + hop <= end (start, end in samples, 0 <= start <= end) -> *first and
 * *count (0 when there is none); -1 for an argument out of range. */
int tt_nr_rank(int quantile_num, int frames);
int tt_nr_region(long long start, long long end, int hop, int frames, int* first, int* count);

/* wav: device f32.  Clip c is wav[clip_offsets[c] .. + clip_lengths[c]) (host arrays, element units), n_fft / 2 + 1 <= length <= max_samples.
 * noise_frames[c] = 0 selects auto for clip c; otherwise its floor is the mean over the frames noise_first_frame[c] .. + noise_frames[c]
 * (at least TT_NR_MIN_REGION of them, inside the clip).  One tt_nr_params for the call.  The clip's clip_lengths[c] output samples are
 * written at out + out_offsets[c], its floor at floor_out + c * bins_pad (device f32 [n_clips][bins_pad], zero beyond n_fft / 2), its status
 * (TT_NR_OK / TT_NR_SHORT) at status_out[c], a HOST array that is filled before the call returns: the status is decided from the lengths
 * alone.  out must not overlap wav.  Asynchronous on `stream`. */
int tt_nr_run(tt_nr* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* noise_first_frame,
              const int* noise_frames, const tt_nr_params* params, int n_clips, float* out, const long long* out_offsets, float* floor_out,
              int* status_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
