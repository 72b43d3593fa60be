/*
 * Time-varying pitch: the band-limited resampler of tortoise_mi355x_rs.h along a pitch map.  A clip carries a table of segments, each with
 * its own pitch ratio P_i / 65536; the constants, the prototype table, cq, H, c32 and the per-tap formula are the rs header's, unchanged,
 * with Q = 65536.  One call takes a ragged batch of clips, each with its own table, and every clip's outputs are bit-identical to running
 * it alone.  The table of one segment (0, 0, 0, P) gives tt_rs_resample(P, 65536)'s bits.
 *
 *   table      S segments (m_i, thi_i, tlo_i, P_i), 1 <= S <= TT_RSW_MAX_SEGMENTS, i32 [4 S]: from output sample m_i on, where the input
 *              stands at t_i = thi_i * 65536 + tlo_i in units of 1 / 65536 sample (0 <= tlo_i < 65536; t_i can reach 2^39, hence two i32),
 *              the clip is read at P_i / 65536 input samples per output sample, TT_RSW_P_MIN <= P_i <= TT_RSW_P_MAX (+-12 semitones).
 *              (m_0, t_0) = (0, 0); m_i strictly increasing;
 *              continuity  t_(i+1) = t_i + (m_(i+1) - m_i) * P_i  (64-bit, exact: no rounding anywhere);  t_(S-1) < n * 65536
 *   sample m   i the last segment with m_i <= m;  pos = t_i + (m - m_i) * P_i  (64-bit);  input index pos >> 16, phase r = pos & 65535;
 *              the value is the rs header's `sample m` from its tap loop on, with that index and phase, Q = 65536 and the cq, H, c32 of
 *              (P_i, 65536): taps j = index - H .. index + H + 1 ascending, one FMA each; samples outside [0, n) read as 0
 *   n_out      m_(S-1) + ceil((n * 65536 - t_(S-1)) / P_(S-1))                                (64-bit)
 *   peak       max |y[m]| over the clip's outputs
 *
 *   plan       from input-domain segments (b_i, P_i), b_0 = 0 < b_1 < .. < b_S = n, every segment of at least TT_RSW_MIN_SEGMENT samples:
 *              m_0 = t_0 = 0;  L_i = max(1, ceil((b_(i+1) * 65536 - t_i) / P_i));  m_(i+1) = m_i + L_i;  t_(i+1) by continuity.
 *              Every length is measured from the achieved t_i, so 0 <= t_(i+1) - b_(i+1) * 65536 < P_i: under two input samples, and it
 *              does not accumulate.  Proof, by induction from t_0 = b_0 = 0: t_i < b_i * 65536 + 131072 = (b_i + 2) * 65536
 *              <= b_(i+1) * 65536, so D = b_(i+1) * 65536 - t_i > 0, L_i = ceil(D / P_i) >= 1 (the max never acts), and
 *              t_(i+1) - b_(i+1) * 65536 = L_i P_i - D lies in [0, P_i).  For i = S - 1 the same line gives t_(S-1) < n * 65536.
 *
 * The position never jumps: it is continuous and exact across a border.  The FILTER changes there: each output is a band-limited
 * interpolation of the input at its own segment's cutoff (rho min(1, 65536 / P_i) of the Nyquist frequency) and half-width, so two
 * neighbouring outputs on either side of a border are read through two different low-passes.  Nothing is cross-faded.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check that does not need the data happens before any device work, the table itself is checked on the device.
 */
#ifndef TORTOISE_MI355X_RSW_H
#define TORTOISE_MI355X_RSW_H
#include "tortoise_mi355x_rs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_RSW_MAX_SEGMENTS 64
#define TT_RSW_MIN_SEGMENT 2   /* input samples a planned segment covers at least */
#define TT_RSW_P_MIN 32768     /* -12 semitones */
#define TT_RSW_P_MAX 131072    /* +12 semitones */

/* per-clip status */
#define TT_RSW_OK 0
#define TT_RSW_EMPTY 1   /* a clip of no samples */
#define TT_RSW_REFUSED 2 /* the clip exceeds the handle's max_samples, its table has no or too many segments or breaks one of the table's
                            rules, or its slice of out does not have tt_rsw_out_samples entries */

typedef struct tt_rsw tt_rsw;

int tt_rsw_abi_version(void);

/* Plain host functions (no device, no handle; host pointers).  A table is i32 [4 S]: (m_i, thi_i, tlo_i, P_i) of every segment.
 *   tt_rsw_plan         starts i32 [S] = b_0 .. b_(S-1) (b_S = n), ps i32 [S] -> table_out i32 [4 S]; 0, or -1 (n outside 1 .. TT_RS_MAX_SAMPLES,
 *                       S outside 1 .. TT_RSW_MAX_SEGMENTS, b_0 != 0, a segment under TT_RSW_MIN_SEGMENT samples, a ratio outside the range)
 *   tt_rsw_out_samples  n_out of the clip along the table; 0 for a table that breaks a rule */
int tt_rsw_plan(int n, int n_segments, const int* starts, const int* ps, int* table_out);
int tt_rsw_out_samples(int n, int n_segments, const int* table);

/* 1 <= max_samples <= TT_RS_MAX_SAMPLES, 1 <= max_clips <= TT_RS_MAX_CLIPS, 1 <= max_segments <= TT_RSW_MAX_SEGMENTS.  The handle owns
 * the prototype table. */
int tt_rsw_create(int max_samples, int max_clips, int max_segments, tt_rsw** out);
void tt_rsw_destroy(tt_rsw* h);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   seg       i32 [4 seg_off[n_clips]]   the tables: clip i has the segments seg_off[i] .. seg_off[i+1], four entries each
 *   in_off, seg_off, out_off  i32 [n_clips + 1], non-decreasing from 0; clip i has tt_rsw_out_samples entries of out
 * out:
 *   out       f32 [out_off[n_clips]]     the resampled clips
 *   peak      f32 [n_clips] or NULL      max |y| of clip i (zeroed and filled in this call)
 *   status    i32 [n_clips]              TT_RSW_*; a clip whose status is not TT_RSW_OK gets its status written and nothing else */
int tt_rsw_resample(tt_rsw* h, int n_clips, const float* audio, const int* in_off, const int* seg, const int* seg_off, float* out,
                    const int* out_off, float* peak, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
