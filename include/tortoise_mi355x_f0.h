/*
 * Fundamental frequency: a YIN tracker (de Cheveigne & Kawahara 2002) on f32 audio at 24 kHz.  One call takes a ragged batch of clips, each
 * with its own parameters, and every clip's outputs are bit-identical to running it alone.
 *
 *   constants  H = 240 (hop, 10 ms, as tt_sil's), W = 960 (integration window, 40 ms), LAG_MIN = 24 (1000 Hz), LAG_MAX = T = 480 (50 Hz).
 *              F = ceil(n / H) frames; frame f reads x[b .. b + W + T) with b = f H - 720; samples outside the clip are 0; its time is f H.
 *   difference for tau = 1 .. T:  d(tau) = sum_{j < W} (x[b+j] - x[b+j+tau])^2.  The device forms every term in f32 as one rounded
 *              subtraction e = x[b+j] - x[b+j+tau] followed by one FMA acc = fma(e, e, acc), and sums the 960 terms in a fixed order of
 *              its own (at most W + 2 rounded operations on any path from a sample to the sum).  All terms are non-negative, so
 *                |d32 - d| <= gamma_(W+2) d,  gamma_k = k u / (1 - k u),  u = 2^-24.
 *              (That relative bound is the reason for the direct form: E(0) + E(tau) - 2 r(tau) from a correlation cancels exactly where
 *              the decision is made.)
 *   normalised c(tau) = sum_{j = 1 .. tau} d(j), accumulated in f64 from the f32 values (any order: at most 16 rounded additions on a path);
 *              d'(tau) = ((double)d(tau) * tau) / c(tau) in f64 (two rounded operations), d'(tau) = 1 where c(tau) = 0, d'(0) = 1.
 *   power      P = sum_{j < W} x[b+j]^2 in f64 (x^2 exact, at most 21 rounded additions on a path).
 *   pick       per clip (lag_lo, lag_hi) with LAG_MIN <= lo <= hi <= LAG_MAX, a threshold thr in [0, 2] and a power floor floor_e >= 0.
 *              t0 = the smallest tau in [lo, hi] with d'(tau) < thr.
 *              t0 exists:  t^ = the smallest tau >= t0 with tau = hi or d'(tau+1) >= d'(tau); the frame is voiced iff P >= floor_e.
 *              no t0:      t^ = the first argmin of d' over [lo, hi]; the frame is unvoiced.
 *   refine     for 2 <= t^ <= T - 1:  a, b, c = d'(t^-1), d'(t^), d'(t^+1), den = (a - 2 b) + c,
 *              delta = clamp(0.5 (a - c) / den, -1, 1) if den > 0, else 0 (t^ = T: 0).  All in f64.
 *              f0 = (float)(24000 / (t^ + delta)) for a voiced frame, 0 for an unvoiced one.
 *   outputs    per frame lag (i32) = t^, f0 (f32), aper (f32) = (float)d'(t^), the aperiodicity; per clip n_voiced and status.
 *   status     OK.  EMPTY: a clip of no samples.  REFUSED: a parameter is out of range or not finite, the clip exceeds the handle's
 *              max_samples, or its frame slice is too short.  A clip whose status is EMPTY or REFUSED gets its status written and nothing
 *              else.
 *
 * Audio is finite and small enough that no d(tau) overflows f32 (|x| < 2^60 is plenty).
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_F0_H
#define TORTOISE_MI355X_F0_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_F0_HOP 240                /* H */
#define TT_F0_WINDOW 960             /* W */
#define TT_F0_LEAD 720               /* frame f starts at f H - TT_F0_LEAD */
#define TT_F0_LAG_MIN 24             /* 1000 Hz */
#define TT_F0_LAG_MAX 480            /* T: 50 Hz */
#define TT_F0_SAMPLE_RATE 24000
#define TT_F0_MAX_SAMPLES 8388608    /* longest clip a handle can be made for (2^23 samples) */
#define TT_F0_MAX_CLIPS 64

/* per-clip status */
#define TT_F0_OK 0
#define TT_F0_EMPTY 1
#define TT_F0_REFUSED 2

typedef struct tt_f0 tt_f0;

int tt_f0_abi_version(void);

/* 1 <= max_samples <= TT_F0_MAX_SAMPLES, 1 <= max_clips <= TT_F0_MAX_CLIPS.  The handle owns no buffer a call reads back: a call is one
 * launch for the frames and one for the per-clip count. */
int tt_f0_create(int max_samples, int max_clips, tt_f0** out);
void tt_f0_destroy(tt_f0* h);

/* Plain host function (no device, no handle): F = ceil(n / H) of a clip of n samples; 0 for n < 1 or n > TT_F0_MAX_SAMPLES. */
int tt_f0_frames(int n);

/* Plain host function: the lags of a frequency range, lag_lo = ceil(24000 / fmax) and lag_hi = floor(24000 / fmin), for
 * 50 <= fmin <= fmax <= 1000 Hz with at least one whole lag inside; anything else is an error and writes nothing. */
int tt_f0_lags(double fmin, double fmax, int* lag_lo, int* lag_hi);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]
 *   in_off    i32 [n_clips + 1]          non-decreasing from 0
 *   par       i32 [n_clips, 2]           (lag_lo, lag_hi) of clip i
 *   thr       f64 [n_clips, 2]           (thr, floor_e) of clip i
 *   frm_off   i32 [n_clips + 1]          clip i's slice of lag / f0 / aper has at least tt_f0_frames(n_i) entries
 * out:
 *   lag       i32 [frm_off[n_clips]]     t^
 *   f0        f32 [frm_off[n_clips]]     Hz, 0 where unvoiced
 *   aper      f32 [frm_off[n_clips]]     d'(t^)
 *   n_voiced  i32 [n_clips]              (not written for an EMPTY or REFUSED clip)
 *   status    i32 [n_clips]              TT_F0_OK / EMPTY / REFUSED */
int tt_f0_track(tt_f0* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const int* frm_off, int* lag,
                float* f0, float* aper, int* n_voiced, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
