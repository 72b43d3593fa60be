/*
 * Levelling a stream of 24 kHz mono f32 audio on the device: BS.1770 loudness measured causally on the prefix heard so far, a slew-limited
 * gain towards a loudness target (or a fixed gain), and the 5 ms look-ahead limiter of tortoise_mi355x_loud.h under a gain that moves.  Up to
 * TT_LVS_MAX_STREAMS streams are fed in chunks.  Whatever the chunking, the concatenation of what a stream emits is bit for bit what one
 * push of the whole clip with flush emits, and nothing a stream computes depends on the other streams of a push.
 *
 * Taken over from tortoise_mi355x_loud.h, by reference: the K-weighting with its operation order; the segments of S = 150 samples and
 * state' = M state + end values; hops H = 2400 and blocks B = 9600; z_j, both gates and L (with loud_gate_kernel's summation order:
 * thread-strided over 256, then the fixed tree); the true-peak phases and P[n]; Lh = 120 and the Hann window w.
 *
 *   measurement  runs on the stream's absolute grid: segment s covers the samples 150 s .. 150 s + 149 of the stream, whatever push brought
 *                them.  The carried state (four f64) and the running hop's partial sum (f64) live in the slot between pushes; the samples of
 *                a segment that is not complete yet, and the two samples before it, wait in the slot's history (f32 -> f64 is exact).
 *                Hop h is complete once n_in >= (h + 1) H; q_h is loud.h's: its 16 segment sums added in ascending order from 0.
 *                For h >= 3, L_h, blocks_abs, blocks_rel and status_h are exactly tt_loud_measure's of the prefix x[0 .. (h + 1) H): the
 *                gates over the blocks 0 .. h - 3 in the same order.  For h < 3 the status is SHORT (L_h = -HUGE_VAL, no blocks).  The partial hop at a
 *                flush is never measured: no block contains it.
 *   steering     per stream a mode, TT_LVS_ADAPT or TT_LVS_FIXED, and gain0, an f32 linear gain.  ADAPT has a target T (LUFS), boost and
 *                cut (dB, >= 0) and rise and fall (dB per second, >= 0); all five are given as f32 and widened to f64.  The dB trajectory
 *                is f64, one rounded operation per operation written here:
 *                  G_-1 = 20 * log10((double) gain0)
 *                  D_h  = min(max(T - L_h, -cut), boost)  where status_h is OK, else D_h = G_(h-1)   (SHORT and SILENT hold the gain)
 *                  G_h  = G_(h-1) + min(max(D_h - G_(h-1), -(0.1 * fall)), 0.1 * rise)
 *                  gl_h = (f32) 10^(G_h / 20), the power in f64 as tt_loud_normalize forms its gain;  gl_-1 = gl_-2 = gain0, the f32 as given
 *                FIXED: gl_h = gain0 and G_h = G_-1 for every h; the measurement runs and is reported all the same.
 *   sample gain  n in hop h' = n / H, k = n - h' H:  t = (f32) k / 2400.f,  g[n] = fmaf(t, gl_(h'-1) - gl_(h'-2), gl_(h'-2))  - three
 *                rounded f32 operations.  What the stream knows when hop h' begins (everything through hop h' - 1) is where the ramp over
 *                hop h' ends: no sample waits for a measurement, the gain is continuous, and where the two ends are equal g[n] is that value.
 *   limiting     TT_LVS_NONE: y[n] = g[n] x[n].  TT_LVS_LOOKAHEAD with the linear ceiling c: loud.h's formulas with g[n] for g,
 *                  r[n] = min(1, c / (g[n] max(P[n-1], P[n]))),  m[n] = min r[k] over |k - n| <= Lh,
 *                  s[n] = min(r[n], 1 - sum_k w[k] (1 - m[n+k])),  y[n] = (g[n] x[n]) s[n]
 *                with r = 1 and P = 0 before sample 0 and, once the stream is flushed, from its end on (samples outside the stream read 0).
 *                r[n] carries sample n's own gain, so |y[n]| <= c up to the roundings as in loud.h.
 *   emission     y[n] reads s[n], that m[n - Lh .. n + Lh], that r[n - 2 Lh .. n + 2 Lh], that P[n - 2 Lh - 1 .. n + 2 Lh], that
 *                x[n - 2 Lh - 8 .. n + 2 Lh + 8]: the forward reach is D = 2 Lh + 8 = TT_LVS_DELAY = 248 samples (10.3 ms), and so is the
 *                backward one.  g[k] for k <= n + 2 Lh needs hop k / H - 1 complete, which it is once sample k is in.
 *                NONE is ready up to n_in, LOOKAHEAD up to max(n_in - D, 0), a flush makes everything ready; a push emits
 *                n_out .. ready - 1.  The slot keeps its last TT_LVS_HIST inputs (>= 2 D for the limiter, >= S + 1 for the measurement)
 *                in two copies: a push reads one and writes the other.
 *   readings     the running maximum of P[n] and of |y[n]| over the emitted samples n < n_out and the count of those with s[n] < 1, as
 *                order-independent integer maxima on the bits of non-negative floats and an integer count.  NONE emits without a delay
 *                and P[n] reaches 8 samples ahead: it reads P as 0 and counts none.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work, and a refused call leaves every slot as it was.
 */
#ifndef TORTOISE_MI355X_LVS_H
#define TORTOISE_MI355X_LVS_H
#include "tortoise_mi355x_loud.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_LVS_MAX_STREAMS 64
#define TT_LVS_DELAY 248              /* D = 2 Lh + 8 */
#define TT_LVS_HIST 512               /* inputs a slot keeps between pushes */
#define TT_LVS_DEFAULT_HOPS 36000     /* one hour */
#define TT_LVS_MAX_HOPS 864000        /* a day: the most a handle can be made for; a stream holds at most max_hops * 2400 samples */
#define TT_LVS_TILE 1024              /* outputs of one workgroup of the apply launch */

/* steering */
#define TT_LVS_ADAPT 0
#define TT_LVS_FIXED 1
/* limiting */
#define TT_LVS_NONE 0
#define TT_LVS_LOOKAHEAD 1

typedef struct tt_lvs tt_lvs;

int tt_lvs_abi_version(void);

/* 1 <= max_streams <= TT_LVS_MAX_STREAMS, 1 <= max_hops <= TT_LVS_MAX_HOPS (0: TT_LVS_DEFAULT_HOPS).  The handle owns 40 bytes per slot
 * and hop (q_h, L_h, G_h, status_h, the two block counts, gl_h) and 4 KB of history per slot. */
int tt_lvs_create(int max_streams, int max_hops, tt_lvs** out);
void tt_lvs_destroy(tt_lvs* h);

/* Opens (or reopens) `slot` as a new stream.  steer: TT_LVS_ADAPT / FIXED; limit: TT_LVS_NONE / LOOKAHEAD.  gain0 positive and finite;
 * target finite (|T| <= 1e30); ceiling positive and finite; boost, cut, rise, fall >= 0 and finite.  FIXED ignores target, boost, cut,
 * rise and fall but checks them; NONE ignores the ceiling but checks it.  Host only: the settings travel with every push. */
int tt_lvs_open(tt_lvs* h, int slot, int steer, int limit, float gain0, float target, float ceiling, float boost, float cut, float rise,
                float fall);
int tt_lvs_close(tt_lvs* h, int slot);

/* Host counters only (any pointer may be null): inputs taken, outputs emitted, hops measured, flushed. */
int tt_lvs_state(tt_lvs* h, int slot, int* n_in, int* n_out, int* hops_done, int* finished);

/* Plain host function: the outputs a push of n_chunk samples emits on a stream that holds n_in_before; -1 for counts it refuses. */
int tt_lvs_ready(int n_in_before, int n_chunk, int limit, int flush);

/* One call for all streams of a round: n_push distinct open slots, slots / n_chunk / flush host arrays of n_push entries.
 *   audio  f32 device: the chunks packed in the order of `slots` (finite values)
 *   out    f32 device: what each slot emits, packed in the same order, tt_lvs_ready entries each (may not overlap audio)
 * Two launches on `stream`; the per-slot items go as kernel arguments: no upload, no copy back, no synchronisation.  A flushed slot is
 * finished until it is opened again.  A push that would pass the handle's max_hops hops on a slot is refused. */
int tt_lvs_push(tt_lvs* h, int n_push, const int* slots, const int* n_chunk, const int* flush, const float* audio, float* out, void* stream);

/* The slot's latest readings, copied to host memory and synchronised on `stream` (any pointer may be null):
 *   lufs, status, blocks_abs, blocks_rel, gain_db (G), gain (gl) of the last measured hop (before the first: -HUGE_VAL, SHORT, 0, 0,
 *   G_-1, gain0); peak: max P[n] (0 in TT_LVS_NONE), out_peak: max |y[n]|, limited: samples with s[n] < 1, all over n < n_out. */
int tt_lvs_read(tt_lvs* h, int slot, double* lufs, int* status, int* blocks_abs, int* blocks_rel, double* gain_db, float* gain, float* peak,
                float* out_peak, int* limited, void* stream);

/* The per-hop history first_hop .. first_hop + count - 1 (within the hops measured) copied to host arrays of `count` entries (any may be
 * null) and synchronised on `stream`. */
int tt_lvs_trace(tt_lvs* h, int slot, int first_hop, int count, double* q, double* lufs, double* gain_db, int* status, int* blocks_abs,
                 int* blocks_rel, void* stream);

#ifdef __cplusplus
}
#endif
#endif
