/*
 * Octave-robust fundamental frequency: a Viterbi path over YIN period candidates, on f32 audio at 24 kHz.  tt_f0_track
 * (tortoise_mi355x_f0.h) picks every frame on its own; this keeps up to seven candidates a frame and chooses among them with a dynamic
 * programme over the whole clip, so a run of frames that reads an octave high or low is pulled back by its neighbours.  One call takes a
 * ragged batch of clips, each with its own parameters and costs, and every clip's outputs are bit-identical to running it alone.
 *
 *   d', P      everything up to and including d'(tau), tau = 0 .. T, and P is tt_f0_track's: the constants H, W, T, the f32 term, the f64
 *              normalisation (tortoise_mi355x_f0.h).  Per clip the same (lag_lo, lag_hi) = (lo, hi), thr and floor_e.
 *   candidates of a frame, from its d' table:
 *              a lag tau in [lo, hi] is a dip iff d'(tau) < d'(tau-1) and (tau == T or d'(tau+1) >= d'(tau)).
 *              The K = 7 dips with the smallest d' are kept, ties to the smaller lag, and numbered by ascending lag as states 0 .. k-1,
 *              k <= 7.  States k .. 6 are absent.  State 7 is "unvoiced" and always exists.  If P < floor_e every voiced state of the
 *              frame is absent.  Per candidate: lag (i32, 0 = absent), dp = d'(lag) (f64), f0 = (float)(24000 / (lag + delta)) with
 *              tt_f0_track's parabola and clamp.  Slot 7 of a frame's table holds tt_f0_track's own pick: lag = t^, dp = d'(t^), f0 = 0.
 *   costs      all f64, every operation a single rounded operation in the order written, no fused contraction.
 *              L2[tau] = log2(tau), tau = 1 .. 480: a table of 481 doubles (entry 0 unused) the HOST computes once and hands to
 *              tt_f0v_create; no transcendental runs on the device.  Per clip four non-negative finite parameters (oct, jump, vuv, uv).
 *                local(t, s), s voiced      dp + oct * (L2[lag] - L2[lo])
 *                local(t, 7)                uv
 *                trans(j -> s) both voiced  jump * fabs(L2[lag_s] - L2[lag_j])
 *                        exactly one voiced vuv
 *                        both unvoiced      0
 *   recursion  a[0][s] = local(0, s);  a[t][s] = local(t, s) + min_j (a[t-1][j] + trans(j -> s)) over the present j, the smallest j wins
 *              a tie.  The end state is the smallest s with minimal a[F-1][s]; backtrace from it.
 *   outputs    per frame lag, f0, aper, state (0 .. 7).  A voiced state: the chosen candidate's lag and f0, aper = (float)dp.  State 7:
 *              f0 = 0, lag and aper are tt_f0_track's (slot 7), so unvoiced rows read as they do there.  Per clip n_voiced (frames whose
 *              state is not 7), cost = a[F-1][end] (f64) and status.
 *   status     TT_F0_OK / TT_F0_EMPTY / TT_F0_REFUSED with tt_f0_track's meanings; a cost that is negative or not finite is REFUSED too.
 *              A clip that is not OK gets its status written and nothing else.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_F0V_H
#define TORTOISE_MI355X_F0V_H
#include "tortoise_mi355x_f0.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_F0V_STATES 8              /* seven candidates and "unvoiced" */
#define TT_F0V_UNVOICED 7
#define TT_F0V_TABLE 481             /* doubles of the log2 table: entries 0 .. TT_F0_LAG_MAX */

typedef struct tt_f0v tt_f0v;

int tt_f0v_abi_version(void);

/* 1 <= max_samples <= TT_F0_MAX_SAMPLES, 1 <= max_clips <= TT_F0_MAX_CLIPS; log2_table: TT_F0V_TABLE HOST doubles, entry tau = log2(tau)
 * (entry 0 unused), finite and non-decreasing from entry 1.  The handle owns the table's device copy, the candidate tables (8 x 16 bytes a
 * frame and clip) and the backpointers (4 bytes a frame and clip) of its largest batch. */
int tt_f0v_create(int max_samples, int max_clips, const double* log2_table, tt_f0v** out);
void tt_f0v_destroy(tt_f0v* h);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.  Two launches:
 * the candidates of every frame, then one wave per clip along the path.
 *   audio, in_off, par, thr, frm_off   as tt_f0_track's
 *   cost      f64 [n_clips, 4]           (oct, jump, vuv, uv) of clip i
 * out:
 *   lag       i32 [frm_off[n_clips]]
 *   f0        f32 [frm_off[n_clips]]     Hz, 0 where the path is unvoiced
 *   aper      f32 [frm_off[n_clips]]
 *   state     i32 [frm_off[n_clips]]     0 .. 7
 *   n_voiced  i32 [n_clips]              (not written for an EMPTY or REFUSED clip, like path_cost)
 *   path_cost f64 [n_clips]
 *   status    i32 [n_clips]              TT_F0_OK / EMPTY / REFUSED */
int tt_f0v_track(tt_f0v* h, int n_clips, const float* audio, const int* in_off, const int* par, const double* thr, const double* cost,
                 const int* frm_off, int* lag, float* f0, float* aper, int* state, int* n_voiced, double* path_cost, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
