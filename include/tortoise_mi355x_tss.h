/*
 * Streaming at another speaking rate: the WSOLA time-stretch of tortoise_mi355x_tsm.h fed in chunks.  Whatever the chunking, the
 * concatenation of what a stream emits - samples and chosen offsets - is bit for bit what tt_tsm_stretch returns for the whole clip.
 * Followed by a tt_rss stream at (pq, 65536) it is the whole-clip pitch chain.
 *
 *   algorithm  everything of tortoise_mi355x_tsm.h: W, Hs, the search range S = 256, the window, rq, a_k, the scores, the tie rule and the
 *              overlap-add.  The clip's length n enters that header only through n_out, K and the zeros read at and beyond n.
 *   look-ahead frame k >= 1 reads its region x[a_k - 256 .. a_k + LOOK), LOOK = 2 S - 1 + Hs + W - S = 1407 (the 512 candidate windows and
 *              the 768 samples behind any choice + Hs: the next template), and the template frame k - 1 left.  a_k does not depend on the
 *              path, so frame k is COMPLETE once a_k + LOOK <= n, n the inputs so far: it is then what the whole-clip call computes,
 *              whatever follows.
 *   frames     a_k does not decrease in k, so the complete frames are 1 .. done(n):
 *                done(n) = 0 for n < LOOK, else (((n - LOOK + 1) << 16) - 32768 - 1) / (Hs rq) + 1          (64-bit integer division)
 *   emission   after a push that brings a stream's total to n the frames 1 .. done(n) have run and ready(n) = done(n) Hs outputs exist;
 *              the push emits the outputs m_out .. ready - 1 and, where asked, the offsets d_k of the frames it ran (d_0 = 0 comes with
 *              frame 1).  For every final length N >= n: done(n) <= K(N) - 1 and done(n) Hs <= n_out(N) - nothing is emitted early that
 *              the whole-clip call would not produce.
 *   flush      the stream ends at n >= 1: the frames up to K - 1 run with zeros at and beyond n (at most 8 of them, at rate 0.5) and ready
 *              becomes n_out = tt_tsm_out_samples(n, rq); the offsets emitted over the stream are the clip's K.  A flush at n = 0 emits
 *              nothing (tt_tsm_stretch answers that clip with TT_TSM_EMPTY).
 *   latency    output m is out once the input reaches (the start of its hop's frame) + LOOK: 1407 input samples, 58.6 ms at 24 kHz
 *   state      after a push the next frame k' = done(n) + 1 has a_k' + LOOK > n, so it reaches back to x[a_k' - 256] with
 *              n - (a_k' - 256) <= 1662: a slot keeps the last TT_TSS_HIST = 1664 inputs (positions n - 1664 .. n - 1, zeros before
 *              sample 0) and the 768-sample template x[p_(k'-1) + Hs ..) on the device, and nothing else.  The history has two copies; a
 *              push reads one and writes the other, and the slot's parity says which is current.  The chosen positions p_k never come
 *              back to the host: every count the host keeps (n_in, frames, m_out) is a function of (n, rq, flush).
 *
 * Positions are 32-bit: a stream takes at most TT_TSM_MAX_SAMPLES inputs between tt_tss_open and its flush.  A rate change inside a stream
 * is not provided.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work, and a refused call leaves every slot as it was.
 */
#ifndef TORTOISE_MI355X_TSS_H
#define TORTOISE_MI355X_TSS_H
#include "tortoise_mi355x_tsm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_TSS_LOOK 1407         /* look-ahead of a frame beyond its nominal position, in input samples */
#define TT_TSS_HIST 1664         /* inputs of history per slot (>= 1662) */
#define TT_TSS_MAX_STREAMS 64

typedef struct tt_tss tt_tss;

int tt_tss_abi_version(void);

/* 1 <= max_streams <= TT_TSS_MAX_STREAMS slots, all closed.  The handle owns the window, the histories and the templates. */
int tt_tss_create(int max_streams, tt_tss** out);
void tt_tss_destroy(tt_tss* h);

/* Opens (or re-opens, whatever state it was in) slot 0 <= slot < max_streams for a stream at rate rq (TT_TSM_RATE_MIN .. TT_TSM_RATE_MAX):
 * n_in = m_out = frames = 0.  No device work. */
int tt_tss_open(tt_tss* h, int slot, int rq);
int tt_tss_close(tt_tss* h, int slot);

/* Host counters of an open or finished slot (any pointer may be NULL); -1 for a closed slot.  frames: the frames 1 .. frames have run. */
int tt_tss_state(tt_tss* h, int slot, int* n_in, int* m_out, int* frames, int* finished);

/* Plain host functions (no device, no handle).
 *   tt_tss_frames_done  done(n) above; -1 for n < 0, n > TT_TSM_MAX_SAMPLES or an rq outside the range.
 *   tt_tss_ready        the outputs a push of n_chunk samples emits on a stream that holds n_before samples and has emitted
 *                       done(n_before) Hs; flush != 0: the push ends the stream.  -1 for a negative count, n_before + n_chunk >
 *                       TT_TSM_MAX_SAMPLES or an rq outside the range. */
int tt_tss_frames_done(int n, int rq);
int tt_tss_ready(int n_before, int n_chunk, int rq, int flush);

/* One push for n_push streams (1 <= n_push <= max_streams): ONE launch, one workgroup per stream; asynchronous on `stream`, no host
 * synchronisation, nothing uploaded beyond the kernel's arguments and nothing copied back.
 *   slots, n_chunk, flush   host int [n_push]: distinct open slots, n_chunk >= 0, n_in + n_chunk <= TT_TSM_MAX_SAMPLES
 *   audio    device f32 [sum n_chunk]: the chunks one after the other in array order; finite values
 *   out      device f32 [sum tt_tss_ready(...)]: what each slot emits, one after the other in array order
 *   offsets  NULL, or device i32: the d_k of the frames each slot ran in this push, one slot after the other in array order - per slot
 *            (frames after) - (frames before) entries, and one more (d_0 = 0, first) in the push that runs the slot's frame 1
 * A slot pushed with flush != 0 is finished: a later push to it is refused until tt_tss_open.  Slots not named are untouched. */
int tt_tss_push(tt_tss* h, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, int* offsets,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif
