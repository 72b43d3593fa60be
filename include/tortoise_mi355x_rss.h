/*
 * Streaming at another sample rate: the resampler of tortoise_mi355x_rs.h fed in chunks.  Whatever the chunking, the concatenation of what
 * a stream emits is bit for bit what tt_rs_resample returns for the whole clip.
 *
 *   filter     everything of tortoise_mi355x_rs.h: the table, (P, Q), cq, c32, H, and for output m = 0, 1, ...
 *                num = m P, i = num / Q, r = num % Q                                      (64-bit)
 *                for each tap j = i - H .. i + H + 1, ascending:
 *                  u   = (|(j - i) Q - r| cq) / Q
 *                  k   = u >> 16,  a = (u & 65535) / 65536
 *                  h_j = c32 * fma(a, tab[k + 1] - tab[k], tab[k]) for k < Z L, else 0      (three rounded f32 operations)
 *                  y   = fma(h_j, x[j], y), from y = 0                                      (one FMA per term)
 *              x[j] reads 0 for j < 0, and for j >= n once the stream has been flushed at n samples; such zeros are multiplied like any
 *              sample, not skipped
 *   emission   output m needs the inputs up to i + H + 1.  After a push that brings a stream's total to n samples the outputs ready are
 *                ready(n) = ceil((n - H - 1) Q / P) for n - H - 1 > 0, else 0               (64-bit)
 *              exactly the m with floor(m P / Q) + H + 1 <= n - 1.  A flush (the stream ends at n) makes ready = ceil(n Q / P), which is
 *              tt_rs_out_samples.  A push emits the outputs m_out .. ready - 1, then m_out = ready.
 *   latency    H + 1 input samples: 37 for P <= Q (1.5 ms at 24 kHz), at most 286
 *   history    the earliest tap of a push's outputs lies at or after n_prev - (2 H + 1), n_prev the total before the push: the slot keeps
 *              the last TT_RSS_HIST = 576 >= 2 * 285 + 1 inputs on the device, positions n - 576 .. n - 1, zeros before sample 0.  There
 *              are two copies; a push reads one and writes the other (so one launch can both filter and advance the history), and the
 *              slot's parity says which is current.
 *   forms      TT_RSS_TABLE  any ratio: the whole-clip kernel's tile steps; h_j is formed per tap from the table as above.
 *              TT_RSS_BANK   ratios with Q (2 H + 2) <= TT_RSS_BANK_MAX: tt_rss_open tabulates bank[r][d] = h_j for every phase
 *                            r = 0 .. Q - 1 and tap d = -H .. H + 1 with the very operations above, and a push is the plain FIR
 *                            y = fma(bank[m P mod Q][d], x[i + d], y) over d ascending.  The same values in the same order: the same bits.
 *              TT_RSS_AUTO   per slot, at open: the bank form where Q (2 H + 2) <= TT_RSS_BANK_MAX and Q <= TT_RSS_AUTO_MAX_Q (few
 *                            phases: 8, 16, 32, 48 and 96 kHz from 24 kHz), else the table form (DESIGN.md 5.29 has the measurements)
 *
 * Positions are 32-bit: a stream takes at most TT_RS_MAX_SAMPLES inputs between tt_rss_open and its flush.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work, and a refused call leaves every slot as it was.
 */
#ifndef TORTOISE_MI355X_RSS_H
#define TORTOISE_MI355X_RSS_H
#include "tortoise_mi355x_rs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_RSS_HIST 576          /* inputs of history per slot (>= 2 * 285 + 1) */
#define TT_RSS_MAX_STREAMS 64
#define TT_RSS_BANK_MAX 16384    /* floats of a slot's phase bank: Q (2 H + 2) */
#define TT_RSS_AUTO_MAX_Q 16     /* TT_RSS_AUTO takes the bank form up to this many phases */

/* form */
#define TT_RSS_AUTO 0
#define TT_RSS_TABLE 1
#define TT_RSS_BANK 2

typedef struct tt_rss tt_rss;

int tt_rss_abi_version(void);

/* 1 <= max_streams <= TT_RSS_MAX_STREAMS slots, all closed; form: TT_RSS_*.  The handle owns the table, the histories and the banks. */
int tt_rss_create(int max_streams, int form, tt_rss** out);
void tt_rss_destroy(tt_rss* h);

/* Opens (or re-opens, whatever state it was in) slot 0 <= slot < max_streams for a stream at ratio (P, Q), a ratio tt_rs_resample accepts:
 * n_in = m_out = 0.  Where the slot takes the bank form its bank is built on `stream` (asynchronous).  A TT_RSS_BANK handle refuses a
 * ratio whose bank does not fit. */
int tt_rss_open(tt_rss* h, int slot, int P, int Q, void* stream);
int tt_rss_close(tt_rss* h, int slot);

/* Host counters of an open or finished slot (any pointer may be NULL); -1 for a closed slot.  form: TT_RSS_TABLE or TT_RSS_BANK. */
int tt_rss_state(tt_rss* h, int slot, int* n_in, int* m_out, int* finished, int* form);

/* Plain host function (no device, no handle): the outputs a push of n_chunk samples emits on a stream that holds n_in_before samples and
 * has emitted ready(n_in_before); flush != 0: the push ends the stream.  -1 for a ratio tt_rs_resample refuses, a negative count or
 * n_in_before + n_chunk > TT_RS_MAX_SAMPLES. */
int tt_rss_ready(int n_in_before, int n_chunk, int P, int Q, int flush);

/* One push for n_push streams (1 <= n_push <= max_streams); asynchronous on `stream`, no host synchronisation, nothing copied back.
 *   slots, n_chunk, flush   host int [n_push]: distinct open slots, n_chunk >= 0, n_in + n_chunk <= TT_RS_MAX_SAMPLES
 *   audio   device f32 [sum n_chunk]: the chunks one after the other in array order; finite values
 *   out     device f32 [sum tt_rss_ready(...)]: what each slot emits, one after the other in array order
 * A slot pushed with flush != 0 is finished: a later push to it is refused until tt_rss_open.  Slots not named are untouched. */
int tt_rss_push(tt_rss* h, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
