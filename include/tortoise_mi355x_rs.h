/*
 * Pitch and output sample rate: a band-limited resampler for an arbitrary ratio (a Kaiser-windowed sinc, evaluated per output sample from
 * one tabulated prototype) of f32 audio on the device.  One call takes a ragged batch of clips, each with its own ratio, and every clip's
 * outputs are bit-identical to running it alone.
 *
 *   constants  Z = 32 (zero crossings of the prototype on each side), L = 512 (table entries per zero crossing), beta = 10 (Kaiser),
 *              rho = 9 / 10 (the cutoff, as a share of the narrower of the two Nyquist frequencies)
 *   table      tab[t] = sinc(t / L) I0(beta sqrt(1 - (t / (Z L))^2)) / I0(beta), t = 0 .. Z L (16385 values), sinc(x) = sin(pi x) / (pi x):
 *              computed in fp64 on the host, rounded to f32 and uploaded at create
 *   ratio      (P, Q), positive integers: P / Q input samples per output sample.  from -> to Hz: P / Q = from / to, reduced by their gcd.
 *              A pitch ratio alpha: P = round(alpha * 65536), Q = 65536, NOT reduced (16.16 fixed point like the time-stretch's rq).
 *              1 <= P, Q <= 2^20 and 1 / 8 <= P / Q <= 8; gcd(P, Q) = 1 unless Q = 65536
 *   n_out      ceil(n Q / P)                                                              (64-bit)
 *   cutoff     c = rho min(1, Q / P), carried as cq = floor(9 L 65536 Qc / (10 Pc)) with (Pc, Qc) = (P, Q) for P > Q, else (1, 1)   (64-bit)
 *              and as c32 = (float)(0.9 * min(1.0, (double)Q / (double)P)): IEEE double operations, then rounded to f32
 *   half-width H = ceil(Z L 65536 / cq) input samples (integer; 36 for P <= Q, at most 285)
 *   sample m   num = m P, i = num / Q, r = num % Q                                          (64-bit)
 *              for each tap j = i - H .. i + H + 1, ascending:
 *                u   = (|(j - i) Q - r| cq) / Q                                           (64-bit integer division)
 *                k   = u >> 16,  a = (u & 65535) / 65536                                  (a is exact in f32)
 *                h_j = c32 * fma(a, tab[k + 1] - tab[k], tab[k]) for k < Z L, else 0      (three rounded f32 operations)
 *                y   = fma(h_j, x[j], y), from y = 0                                      (one FMA per term)
 *              samples outside [0, n) read as 0
 *   peak       max |y[m]| over the clip's outputs
 *
 * P = Q is still this filter, a low-pass at 0.9 of the Nyquist frequency, and not a copy: a caller who wants no change does not call.
 * Measured on the fp64 restatement of this formula with the f32 table (tests/resample_reference.py, tests/test_resample_cpu.py), at the
 * ratios 1/2, 80/147, 3/2, 3/1, 77936/65536 and 55109/65536: pass-band tones (up to 0.8 rho of the narrower Nyquist) within 1e-4 dB of
 * unity, everything else in those outputs below -117 dB, tones at 1.1x and 1.5x the output Nyquist below -107 dB.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_RS_H
#define TORTOISE_MI355X_RS_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_RS_ZEROS 32                /* Z */
#define TT_RS_PER_ZERO 512            /* L */
#define TT_RS_TABLE 16385             /* Z L + 1 table values */
#define TT_RS_BETA 10                 /* Kaiser beta */
#define TT_RS_RHO_NUM 9               /* rho = 9 / 10 */
#define TT_RS_RHO_DEN 10
#define TT_RS_PITCH_ONE 65536         /* Q of a pitch ratio; P of pitch ratio 1.0 */
#define TT_RS_MAX_TERM 1048576        /* P, Q <= 2^20 */
#define TT_RS_MAX_RATIO 8             /* 1 / 8 <= P / Q <= 8 */
#define TT_RS_MAX_SAMPLES 8388608     /* longest clip a handle can be made for (2^23 samples) */
#define TT_RS_MAX_CLIPS 64

/* per-clip status */
#define TT_RS_OK 0
#define TT_RS_EMPTY 1   /* a clip of no samples */
#define TT_RS_REFUSED 2 /* the ratio is outside the limits or not reduced (unless Q = 65536), the clip exceeds the handle's max_samples, or
                           its slice of out does not have tt_rs_out_samples entries */

typedef struct tt_rs tt_rs;

int tt_rs_abi_version(void);

/* 1 <= max_samples <= TT_RS_MAX_SAMPLES, 1 <= max_clips <= TT_RS_MAX_CLIPS.  The handle owns the prototype table. */
int tt_rs_create(int max_samples, int max_clips, tt_rs** out);
void tt_rs_destroy(tt_rs* h);

/* Plain host function (no device, no handle): n_out of a clip of n samples at ratio (P, Q); 0 for n < 1, n > TT_RS_MAX_SAMPLES or a ratio
 * that tt_rs_resample refuses. */
int tt_rs_out_samples(int n, int P, int Q);

/* Ragged batch of n_clips clips (1 <= n_clips <= max_clips); every pointer is a device pointer; asynchronous on `stream`.
 *   audio     f32 [in_off[n_clips]]      samples of clip i: in_off[i] .. in_off[i+1]; finite values
 *   P, Q      i32 [n_clips]              ratio of clip i
 *   in_off, out_off  i32 [n_clips + 1], non-decreasing from 0; clip i has tt_rs_out_samples(n_i, P_i, Q_i) entries of out
 * out:
 *   out       f32 [out_off[n_clips]]     the resampled clips
 *   peak      f32 [n_clips] or NULL      max |y| of clip i (zeroed and filled in this call)
 *   status    i32 [n_clips]              TT_RS_*; a clip whose status is not TT_RS_OK gets its status written and nothing else */
int tt_rs_resample(tt_rs* h, int n_clips, const float* audio, const int* in_off, const int* P, const int* Q, float* out, const int* out_off,
                   float* peak, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
