/*
 * Loudness normalisation and true-peak limiting of 24 kHz mono f32 audio on the device: integrated loudness after ITU-R BS.1770-4 / EBU R 128
 * (K-weighting, 400 ms blocks, absolute and relative gate), a 4x oversampled true-peak reading, and a gain to a loudness target under a
 * true-peak ceiling.  One call takes a ragged batch of clips, each with its own target and ceiling, and every clip's outputs are
 * bit-identical to running it alone: nothing a clip computes depends on anything but the clip.
 *
 *   K-weighting  two biquads designed for fs = 24000 from the analog prototype (the formulas of libebur128 / pyloudnorm), in fp64 on the host.
 *                With K = tan(pi f0 / fs):
 *                  shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *                             a0 = 1 + K/Q + K^2, b0 = (Vh + Vb K/Q + K^2)/a0, b1 = 2 (K^2 - Vh)/a0, b2 = (Vh - Vb K/Q + K^2)/a0,
 *                             a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0
 *                  high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, b = (1, -2, 1) (not normalised), a1 and a2 as above with this K and Q
 *                each section y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], the shelf first, from a zero state at every
 *                clip's first sample.  (At fs = 48000 the formulas give the standard's printed tables to 1e-14.)
 *   precision    the filter and every sum of squares are f64: the recursive part has sum |impulse response| = 6.9e4 at 24 kHz, so f32 rounding
 *                could reach 1e-2 relative. 
 *                One section's sample is b0 x[n], then + b1 x[n-1], + b2 x[n-2], - a2 y[n-2], - a1 y[n-1] in THIS order (the a1 term last: it
 *                alone waits for the previous sample), one fused multiply-add per term; the high-pass's three input terms are x[n], then the
 *                fused - 2 x[n-1], then a plain + x[n-2].
 *   segments     the recurrence is cut into segments of S = 150 samples (16 per hop).  Every segment is run from a zero state (with its true
 *                input history) and leaves the four values (shelf y[n-1], y[n-2]; high-pass y[n-1], y[n-2]) behind its last sample; the true
 *                states follow from state' = M state + those four, M the 4 x 4 transition of 150 samples (host, extended precision, rounded
 *                to f64; spectral radius 0.47); every segment is then run again from its true state.
 *   blocks       hop H = 2400 samples (100 ms), block B = 9600 (400 ms, 75 % overlap).  q_h = sum of y^2 over hop h (the last may be partial):
 *                per segment in ascending n, the segments of a hop in ascending order.  hops(n) = ceil(n / H).  Block j covers the hops
 *                j .. j+3 and exists when j H + B <= n: blocks(n) = (n - B) / H + 1 for n >= B.  z_j = (((q_j + q_j+1) + q_j+2) + q_j+3) / B,
 *                l_j = -0.691 + 10 log10 z_j.
 *   gates        absolute: l_j > -70, evaluated as z_j > 10^(-6.9309); relative: 10 LU below -0.691 + 10 log10 mean(z_j) over the blocks above
 *                the absolute gate, evaluated as z_j > 0.1 mean.  L = -0.691 + 10 log10 mean(z_j) over the blocks above both.
 *   status       n < B: SHORT.  No block above -70: SILENT.  Both report L = -HUGE_VAL, gain 1, and normalize returns their samples bit for bit.
 *   true peak    4x oversampling, 16 taps per phase: for p in 0..3 and t in -7..8, a = t - p/4, h_p[t] = sinc(a) (0.5 + 0.5 cos(pi a / 8)) for
 *                |a| < 8, else 0; phase 0 is the exact delta; every phase is normalised to sum 1 in fp64, then rounded to f32
 *                (the f32 values are tabulated in csrc/loudness.hip: they are part of this text, not of a libm).
 *                u_p[n] = sum_t h_p[t] x[n+t], samples outside the clip read 0, f32, one fused multiply-add per term from 0 in ascending t.
 *                P[n] = max_p |u_p[n]| (so P[n] >= |x[n]| exactly) for 0 <= n < len, P = 0 outside; TP = max_n P[n].
 *   gain         target T (LUFS) and ceiling c (linear) per clip: g = (f32) 10^((T - L) / 20), the power in f64 on the device.
 *   NONE         y = g x.
 *   SCALE        g' = min(g, c / TP) (f32 division; TP = 0 leaves g), y = g' x: true peak is linear in the gain, so the ceiling holds.
 *   LOOKAHEAD    Lh = 120 samples (5 ms), all f32:
 *                  r[n] = min(1, c / (g max(P[n-1], P[n])))                      (one product, one division; a zero divisor gives 1)
 *                  m[n] = min r[k] over |k - n| <= Lh, r = 1 outside the clip
 *                  s[n] = min(r[n], 1 - sum_k w[k] (1 - m[n+k])), k = -Lh .. Lh    (w the Hann window 0.5 + 0.5 cos(pi k / (Lh + 1)) normalised
 *                                                                                 to sum 1 in fp64 and rounded to f32; one fused multiply-add
 *                                                                                 per term from 0 in ascending k: the smoothed minimum, in the
 *                                                                                 form that is exactly 1 where nothing limits)
 *                  y[n] = (g x[n]) s[n]
 *                m[n+k] <= r[n] for |k| <= Lh and w is a convex weight, so |y[n]| <= c up to the roundings, and y[n] = g x[n] exactly
 *                wherever r is 1 within 2 Lh.  The true peak of the modulated signal is not guaranteed: it is measured and returned.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_LOUD_H
#define TORTOISE_MI355X_LOUD_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_LOUD_SAMPLE_RATE 24000
#define TT_LOUD_HOP 2400
#define TT_LOUD_BLOCK 9600
#define TT_LOUD_SEGMENT 150
#define TT_LOUD_OVERSAMPLE 4
#define TT_LOUD_TAPS 16
#define TT_LOUD_LOOKAHEAD 120
#define TT_LOUD_MAX_SAMPLES 268435456 /* most samples a handle can be made for, over all clips of a call (2^28) */
#define TT_LOUD_MAX_CLIPS 64

/* limiting mode of tt_loud_normalize */
#define TT_LOUD_NONE 0
#define TT_LOUD_SCALE 1
#define TT_LOUD_LOOKAHEAD_MODE 2

/* per-clip status */
#define TT_LOUD_OK 0
#define TT_LOUD_SHORT 1   /* fewer samples than one block: measured (hop energies, true peak), no loudness, samples unchanged */
#define TT_LOUD_SILENT 2  /* no block above the absolute gate: as SHORT */
#define TT_LOUD_EMPTY 3   /* a clip of no samples */
#define TT_LOUD_REFUSED 4 /* the clip ends beyond the handle's max_total_samples, starts before an earlier clip's start or end (in_off decreases), its slice of hop_energy does not have tt_loud_hops entries,
                             or (normalize) its target is not finite or its ceiling not a positive finite number */

typedef struct tt_loud tt_loud;

int tt_loud_abi_version(void);

/* 1 <= max_total_samples <= TT_LOUD_MAX_SAMPLES (over all clips of one call), 1 <= max_clips <= TT_LOUD_MAX_CLIPS.  The handle owns the
 * filter tables and 40 bytes of workspace per segment: its memory is linear in max_total_samples. */
int tt_loud_create(int max_total_samples, int max_clips, tt_loud** out);
void tt_loud_destroy(tt_loud* h);

/* Plain host functions (no device, no handle): hops and blocks of a clip of n samples; 0 for n < 1 or n > TT_LOUD_MAX_SAMPLES. */
int tt_loud_hops(int n);
int tt_loud_blocks(int n);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   in_off, hop_off  i32 [n_clips + 1], non-decreasing from 0; clip i has tt_loud_hops(n_i) entries of hop_energy
 * out, per clip:
 *   lufs        f64   L (-HUGE_VAL for SHORT and SILENT)
 *   true_peak   f32   TP, linear
 *   blocks_abs, blocks_rel  i32   the blocks above the absolute gate, and above both
 *   hop_energy  f64 [hop_off[n_clips]]   q_h
 *   status      i32   TT_LOUD_*; an EMPTY or REFUSED clip gets its status written and nothing else */
int tt_loud_measure(tt_loud* h, int n_clips, const float* audio, const int* in_off, const int* hop_off, double* lufs, float* true_peak,
                    int* blocks_abs, int* blocks_rel, double* hop_energy, int* status, void* stream);

/* tt_loud_measure, then the gain: target f32 [n_clips] (LUFS) and ceiling f32 [n_clips] (linear true peak) per clip, one mode
 * (TT_LOUD_NONE / SCALE / LOOKAHEAD_MODE) for the call.  Besides what measure returns:
 *   out            f32 [in_off[n_clips]]  the clips at their gain (may not overlap audio)
 *   gain           f32   the applied g (NONE, LOOKAHEAD) or g' (SCALE); 1 for SHORT and SILENT
 *   out_true_peak  f32   TP measured on out */
int tt_loud_normalize(tt_loud* h, int n_clips, const float* audio, const int* in_off, const int* hop_off, const float* target,
                      const float* ceiling, int mode, float* out, double* lufs, float* true_peak, int* blocks_abs, int* blocks_rel,
                      double* hop_energy, float* gain, float* out_true_peak, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
