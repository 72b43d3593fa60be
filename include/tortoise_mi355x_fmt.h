/*
 * Formant-preserving pitch: cepstral envelope correction of a finished clip on the device (csrc/formant.hip).
 *
 * Raising the pitch by resampling by p = 2^(s / 12) gives Y(w) = X(w / p): the spectral envelope moves with the pitch.  The envelope the clip
 * should have is its own envelope read at p w, so the correction is one function of one clip and one number, the warp alpha (= p after a
 * pitch shift; 2^(-f / 12) moves the formants of an unshifted clip up by f semitones).  All f32, N = n_fft, H = hop, B = N / 2 + 1 bins:
 *
 *   1  re, im of frame t      tt_mel's STFT: centred frames, reflect padding, the window folded into `basis` (same table layout)
 *   2  L_b = 0.5 log(re^2 + im^2 + 1e-10)
 *   3  c_q = sum_b L_b A[b][q]                          (A = wt_b cos(2 pi q b / N) / N, wt_0 = wt_{N/2} = 1, else 2; q < Q <= 64)
 *   4  g_b = clamp(sum_q c_q D[q][b], +- ln(10) G / 20)  (D = 2 h_q (cos(q min(alpha w_b, pi)) - cos(q w_b)), row 0 zero; G = 0: no clamp)
 *   5  Z = (re, im) exp(g_b)
 *   6  y_t[k] = sum_j Z_j inverse[j][k]                 (j = 2 b: re, 2 b + 1: im; window[k] wt_b / N folded into `inverse`)
 *   7  out[j] = sum_t y_t[k] / sum_t window[k]^2, k = j + N / 2 - t H, over the frames t with 0 <= k < N in increasing t, no atomics
 *
 * window[k] is read from column 0 of `basis` (the cos column of bin 0).  One call takes several clips (ragged: offsets + lengths), each with
 * its own index into `warps`; every clip's output is bit-identical to running it alone.
 *
 * Its own header, version and struct sizes; exported from the same library as tortoise_mi355x.h.  Errors are reported through
 * tt_last_error(); every argument check happens before any device work, and a refused call writes nothing.
 */
#ifndef TORTOISE_MI355X_FMT_H
#define TORTOISE_MI355X_FMT_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_FMT_MAX_CLIPS 16 /* clips of one tt_fmt_run call */
#define TT_FMT_MAX_WARPS 16 /* distinct warps of one handle */
#define TT_FMT_Q_PAD 64     /* row length of A, rows of every D */

typedef struct tt_fmt_config {
  int n_fft;          /* frame length = window length; a multiple of hop and of 64 */
  int hop;            /* frame step; a multiple of 8 */
  int bins_pad;       /* >= n_fft / 2 + 1, a multiple of 32; table entries beyond n_fft / 2 are zero */
  int q;              /* cepstral coefficients kept (1 .. 64); the tables are zero from q on */
  float max_gain_db;  /* G >= 0: |g| <= ln(10) G / 20; 0: no clamp */
  int max_samples;    /* longest clip */
  int max_clips;      /* clips per call (1 .. TT_FMT_MAX_CLIPS) */
  int n_warps;        /* matrices in `warps` (1 .. TT_FMT_MAX_WARPS) */
} tt_fmt_config;

typedef struct tt_fmt_tables {
  const float* basis;    /* device f32 [n_fft][2 * bins_pad]: tt_mel_tables.basis */
  const float* inverse;  /* device f32 [2 * bins_pad][n_fft]: row 2 b = window[k] wt_b cos(2 pi b k / n_fft) / n_fft, row 2 b + 1 = -window[k] wt_b sin(...) / n_fft */
  const float* cepstrum; /* device f32 [bins_pad][64]: A */
  const float* warps;    /* device f32 [n_warps][64][bins_pad]: one D per warp */
} tt_fmt_tables;

typedef struct tt_fmt tt_fmt;

int tt_fmt_abi_version(void);
size_t tt_fmt_struct_size(int which);  /* 0: tt_fmt_config, 1: tt_fmt_tables */

/* The tables stay the caller's and must outlive the handle. */
int tt_fmt_create(const tt_fmt_config* cfg, const tt_fmt_tables* tables, tt_fmt** out);
void tt_fmt_destroy(tt_fmt* h);
/* Frames of a clip of n samples: 1 + n / hop. */
int tt_fmt_frames(const tt_fmt* h, int n);

/* wav: device f32.  Clip c is wav[clip_offsets[c] .. + clip_lengths[c]) (host arrays, element units), n_fft / 2 + 1 <= length <= max_samples,
 * corrected with warps[warp_index[c]] (host array); its clip_lengths[c] output samples are written at out + out_offsets[c].  out must not
 * overlap wav.  Asynchronous on `stream`. */
int tt_fmt_run(tt_fmt* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, const int* warp_index, int n_clips,
               float* out, const long long* out_offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
