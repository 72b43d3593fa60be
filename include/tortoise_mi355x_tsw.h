/*
 * Time-varying speaking rate: the WSOLA time-stretch of tortoise_mi355x_tsm.h along a rate map.  A clip carries a table of segments, each
 * with its own rate; everything but the nominal analysis position is the tsm header's algorithm unchanged (constants, start, step, ties,
 * output, f32 and summation order).  One call takes a ragged batch of clips, each with its own table, and every clip's outputs are
 * bit-identical to running it alone.  The table of one segment (0, 0, rq) gives tt_tsm_stretch's bits.
 *
 *   table      S segments (m_i, a_i, rq_i), 1 <= S <= TT_TSW_MAX_SEGMENTS: from output sample m_i on, where the input stands at sample a_i,
 *              the clip runs at rate rq_i (16.16, TT_TSM_RATE_MIN .. TT_TSM_RATE_MAX).  (m_0, a_0) = (0, 0); m_i strictly increasing;
 *              continuity  a_(i+1) = a_i + (((m_(i+1) - m_i) * rq_i + 32768) >> 16)  (64-bit);  a_(S-1) < n
 *   nominal    a_k = a_i + ((((k - 1) Hs - m_i) * rq_i + 32768) >> 16) for k >= 1, i the last segment with m_i <= (k - 1) Hs  (64-bit);
 *              a_k does not decrease in k, within a segment and across a border
 *   n_out      m_(S-1) + max(1, ((n - a_(S-1)) * 65536 + rq_(S-1) / 2) / rq_(S-1))          (integer division, 64-bit)
 *   frames     K = ceil(n_out / Hs) + 1
 *
 *   plan       from input-domain segments (b_i, rq_i), b_0 = 0 < b_1 < .. < b_S = n, every segment of at least 2 input samples:
 *              m_0 = a_0 = 0;  L_i = max(1, ((b_(i+1) - a_i) * 65536 + rq_i / 2) / rq_i);  m_(i+1) = m_i + L_i;  a_(i+1) by continuity.
 *              Every length is measured from the achieved a_i, so the rounding does not accumulate: |a_i - b_i| <= 1.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check that does not need the data happens before any device work, the table itself is checked on the device.
 */
#ifndef TORTOISE_MI355X_TSW_H
#define TORTOISE_MI355X_TSW_H
#include "tortoise_mi355x_tsm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_TSW_MAX_SEGMENTS 64
#define TT_TSW_MIN_SEGMENT 2 /* input samples a planned segment covers at least */

/* per-clip status */
#define TT_TSW_OK 0
#define TT_TSW_EMPTY 1   /* a clip of no samples */
#define TT_TSW_REFUSED 2 /* the clip exceeds the handle's max_samples, its table has no or too many segments or breaks one of the table's
                            rules, or its slices of out / offsets do not have tt_tsw_out_samples / tt_tsw_frames entries */

typedef struct tt_tsw tt_tsw;

int tt_tsw_abi_version(void);

/* Plain host functions (no device, no handle; host pointers).  A table is i32 [3 S]: (m_i, a_i, rq_i) of every segment.
 *   tt_tsw_plan         starts i32 [S] = b_0 .. b_(S-1) (b_S = n), rqs i32 [S] -> table_out i32 [3 S]; 0, or -1 (n outside 1 .. TT_TSM_MAX_SAMPLES,
 *                       S outside 1 .. TT_TSW_MAX_SEGMENTS, b_0 != 0, a segment under TT_TSW_MIN_SEGMENT samples, a rate outside the range)
 *   tt_tsw_out_samples  n_out of the clip along the table; 0 for a table that breaks a rule
 *   tt_tsw_frames       K; 0 likewise */
int tt_tsw_plan(int n, int n_segments, const int* starts, const int* rqs, int* table_out);
int tt_tsw_out_samples(int n, int n_segments, const int* table);
int tt_tsw_frames(int n, int n_segments, const int* table);

/* 1 <= max_samples <= TT_TSM_MAX_SAMPLES, 1 <= max_clips <= TT_TSM_MAX_CLIPS, 1 <= max_segments <= TT_TSW_MAX_SEGMENTS.  The handle owns
 * the window table. */
int tt_tsw_create(int max_samples, int max_clips, int max_segments, tt_tsw** out);
void tt_tsw_destroy(tt_tsw* h);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   seg       i32 [3 seg_off[n_clips]]   the tables: clip i has the segments seg_off[i] .. seg_off[i+1], three entries each
 *   in_off, seg_off, out_off, frame_off  i32 [n_clips + 1], non-decreasing from 0; clip i has tt_tsw_out_samples entries of out and
 *                                        tt_tsw_frames entries of offsets
 * out:
 *   out       f32 [out_off[n_clips]]     the stretched clips
 *   offsets   i32 [frame_off[n_clips]]   the chosen d_k of every frame, d_0 = 0
 *   status    i32 [n_clips]              TT_TSW_*; a clip whose status is not TT_TSW_OK gets its status written and nothing else */
int tt_tsw_stretch(tt_tsw* h, int n_clips, const float* audio, const int* in_off, const int* seg, const int* seg_off, float* out,
                   const int* out_off, int* offsets, const int* frame_off, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
