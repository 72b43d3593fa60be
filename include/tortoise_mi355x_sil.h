/*
 * Pauses and silence: find the speech in f32 audio at 24 kHz, cut the silence at a clip's ends, cap over-long pauses inside it.  One call
 * takes a ragged batch of clips, each with its own parameters, and every clip's outputs are bit-identical to running it alone.
 *
 *   constants  S = 120 (slot, 5 ms), Hf = 240 (frame hop, 10 ms = 2 slots), Wf = 480 (frame, 4 slots), X = 120 (cross-fade and fade length)
 *   energy     all in f64.  Slot s holds samples s S .. min(n, (s + 1) S) - 1 (the last slot may be partial; slots past the end are 0):
 *                q_s = fma((double)x, (double)x, q_s) over the slot's samples in ascending order, from q_s = 0   (x^2 is exact in f64: one
 *                                                                                                              rounding per sample)
 *              F = ceil(n / Hf) frames; frame f holds slots 2f .. 2f + 3:
 *                e_f = ((q_2f + q_2f+1) + q_2f+2) + q_2f+3                                                     (three rounded additions)
 *              E = max_f e_f (exact)
 *              A frame energy is the result of at most K = 4 S + 3 = 483 rounded operations on non-negative terms:
 *              |e_f - exact| <= gamma_K exact, gamma_K = K u / (1 - K u), u = 2^-53.
 *   activity   thr = max(floor_e, rel * E) (one rounded f64 product); frame f is active iff e_f > thr.
 *              rel in [0, 1] and floor_e >= 0 (finite) per clip: the host passes rel = 10^(-top_db / 10), floor_e = Wf 10^(floor_db / 10).
 *   speech     min_sil, pad (frames, 0 .. TT_SIL_MAX_FRAMES_PARAM) per clip.  prev(f) / next(f): the nearest active frame at or before / at
 *              or after f.  Frame f is speech iff it is active, or both exist and next - prev - 1 < min_sil (a short gap is bridged), or
 *              prev exists and f - prev <= pad, or next exists and next - f <= pad.  (Equal to: bridge the gaps between active frames that
 *              are shorter than min_sil, then dilate by pad.)
 *   regions    the maximal runs of speech frames [fa, fb), in samples [a_r, b_r) = [fa Hf, min(fb Hf, n)), ascending; R of them,
 *              R <= tt_sil_max_regions(n) = (F + 1) / 2.
 *   edit       lead, trail, max_pause (samples) per clip; -1: leave alone; else 0 <= lead, trail <= TT_SIL_MAX_SAMPLES and
 *              X <= max_pause <= TT_SIL_MAX_SAMPLES.  With R >= 1 and M = max_pause:
 *                leading gap  G0 = a_0: if lead >= 0 and G0 > lead the first D0 = G0 - lead samples are dropped (else D0 = 0)
 *                trailing gap Gt = n - b_(R-1): if trail >= 0 and Gt > trail the last Dt = Gt - trail samples are dropped (else Dt = 0)
 *                inner gap r = 1 .. R - 1, G = a_r - b_(r-1): cut iff M >= 0 and G >= M + X.  Its first M1 = (M + X + 1) / 2 and last
 *                M2 = (M + X) / 2 samples are kept and overlapped by X, so exactly M remain.
 *              The output is described by K = 1 + (number of cut gaps) segments (o_k, i_k, l_k): outputs o_k .. o_k + l_k - 1 are inputs
 *              i_k .. i_k + l_k - 1; o_0 = 0, i_0 = D0, o_(k+1) = o_k + l_k; a segment ends M1 samples into a cut gap and the next one
 *              begins at a_r - M2 + X; n_out = n - D0 - Dt - sum (G - M) = o_(K-1) + l_(K-1).
 *                value     v = x[i_k + m - o_k] for output m of segment k: a bit-for-bit copy, except
 *                cross-fade  the last X outputs of every segment but the last, j = m - (o_(k+1) - X) = 0 .. X - 1:
 *                              head = x[i_k + m - o_k], tail = x[i_(k+1) - X + j], w_j = (float)(2 j + 1) / (float)(2 X)
 *                              v = fmaf(w_j, tail - head, head)                                  (three rounded f32 operations)
 *                fades     Xe = min(X, n_out).  If D0 > 0, outputs m < Xe fade in with j = m; if Dt > 0, outputs m >= n_out - Xe fade
 *                          out with j' = n_out - 1 - m:
 *                              y = v * w_j, then y = y * w_j'                      (two rounded f32 operations for each that applies)
 *                          The order is fixed, though no sample meets two of the three: a region that borders a cut gap or a cut end
 *                          does not reach the clip's end, so it is whole frames, at least Hf = 2 X samples; a cross-fade therefore lies
 *                          at least Hf outputs from a cut end, and when both ends are cut n_out >= Hf.
 *                everything else: y = v.
 *   map        input sample s -> output: with k the last segment whose i_k <= s (k = 0 before the first): min(o_k + l_k, o_k + max(0, s - i_k)).
 *   status     OK: something was cut.  UNCHANGED: nothing was cut; out is the input bit for bit (K = 1, segment (0, 0, n)).
 *              SILENT: no active frame (all-zero audio included); the clip is returned unchanged, never emptied (R = 0, K = 1).
 *              EMPTY: a clip of no samples.  REFUSED: a parameter is out of range, the clip exceeds the handle's max_samples, or a slice
 *              (regions, segments, energies) is too short for the clip.  tt_sil_find reports OK or SILENT for a clip it has read.
 *              A clip whose status is EMPTY or REFUSED gets its status written and nothing else.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_SIL_H
#define TORTOISE_MI355X_SIL_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_SIL_SLOT 120               /* S */
#define TT_SIL_HOP 240                /* Hf */
#define TT_SIL_FRAME 480              /* Wf */
#define TT_SIL_FADE 120               /* X */
#define TT_SIL_SAMPLE_RATE 24000
#define TT_SIL_MAX_SAMPLES 8388608    /* longest clip a handle can be made for (2^23 samples) */
#define TT_SIL_MAX_CLIPS 64
#define TT_SIL_MAX_FRAMES_PARAM 6000  /* min_sil and pad: at most 60 s */

/* per-clip status */
#define TT_SIL_OK 0
#define TT_SIL_UNCHANGED 1
#define TT_SIL_SILENT 2
#define TT_SIL_EMPTY 3
#define TT_SIL_REFUSED 4

typedef struct tt_sil tt_sil;

int tt_sil_abi_version(void);

/* 1 <= max_samples <= TT_SIL_MAX_SAMPLES, 1 <= max_clips <= TT_SIL_MAX_CLIPS.  The handle owns the slot energies and frame labels of a call. */
int tt_sil_create(int max_samples, int max_clips, tt_sil** out);
void tt_sil_destroy(tt_sil* h);

/* Plain host functions (no device, no handle): F = ceil(n / Hf) and (F + 1) / 2 of a clip of n samples; 0 for n < 1 or n > TT_SIL_MAX_SAMPLES. */
int tt_sil_frames(int n);
int tt_sil_max_regions(int n);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   in_off    i32 [n_clips + 1]          non-decreasing from 0
 *   thr       f64 [n_clips, 2]           (rel, floor_e) of clip i
 *   par       i32 [n_clips, 2]           (min_sil, pad) of clip i
 *   reg_off   i32 [n_clips + 1]          clip i's slice of `regions` has at least tt_sil_max_regions(n_i) entries
 *   frm_off   i32 [n_clips + 1] or NULL  with `energies`: clip i's slice has at least tt_sil_frames(n_i) entries
 * out:
 *   n_regions i32 [n_clips]              R
 *   regions   i32 [reg_off[n_clips], 2]  (a_r, b_r), the first R entries of the clip's slice
 *   peak      f64 [n_clips]              E
 *   energies  f64 [frm_off[n_clips]] or NULL   e_f
 *   status    i32 [n_clips]              TT_SIL_OK / SILENT / EMPTY / REFUSED */
int tt_sil_find(tt_sil* h, int n_clips, const float* audio, const int* in_off, const double* thr, const int* par, const int* reg_off,
                const int* frm_off, int* n_regions, int* regions, double* peak, double* energies, int* status, void* stream);

/* tt_sil_find plus the edit, with no host round trip in between.  As above, and
 *   par       i32 [n_clips, 5]           (min_sil, pad, lead, trail, max_pause) of clip i
 *   seg_off   i32 [n_clips + 1]          clip i's slice of `segments` has at least tt_sil_max_regions(n_i) entries
 * out:
 *   out       f32 [in_off[n_clips]]      sliced like the input: the first n_out samples of clip i's slice; must not overlap `audio`
 *   n_out     i32 [n_clips]
 *   n_segments i32 [n_clips]             K
 *   segments  i32 [seg_off[n_clips], 3]  (o_k, i_k, l_k), the first K entries of the clip's slice
 *   status    i32 [n_clips]              TT_SIL_* */
int tt_sil_trim(tt_sil* h, int n_clips, const float* audio, const int* in_off, const double* thr, const int* par, const int* reg_off,
                const int* seg_off, float* out, int* n_out, int* n_regions, int* regions, int* n_segments, int* segments, double* peak,
                int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
