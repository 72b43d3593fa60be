/*
 * Mel front-end of the voice_samples path (reference tortoise/api.py:258-299): waveform -> log-mel spectrogram on the device.
 *
 *   spectrum  spec[t][b] = |sum_k x[reflect(t * hop + k - n_fft / 2)] * window[k] * e^(-2 pi i b k / n_fft)|^power   (power 1 or 2)
 *             centred frames, reflect padding, periodic Hann window: torch.stft(center=True, pad_mode="reflect") / torchaudio Spectrogram /
 *             the reference's TacotronSTFT; with clamp_input the samples are clamped to [-1, 1] as they are read.
 *   mel       mel[m][t] = log(max(sum_b fb[m][b] * spec[t][b], floor)) * scale[m]              (scale NULL: no scaling)
 *
 * Both sums run in f32 on the matrix cores (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation).  The tables are the caller's:
 * `basis` holds the windowed cos / -sin columns of each bin side by side, `fb` the mel filter bank, `scale` e.g. 1 / mel_norms.  One call
 * takes several clips (ragged: offsets + lengths) and every clip's output is bit-identical to running it alone.
 *
 * The polyphase windowed-sinc resampler of torchaudio.functional.resample (22.05 -> 24 kHz in front of the diffusion mel) is the third
 * entry: out[n * new + p] = sum_j taps[p][j] * xpad[n * orig + j], xpad = x with `width` zeros in front and `width + orig` behind.
 *
 * Its own header, version and struct sizes; exported from the same library as tortoise_mi355x.h.  Errors are reported through
 * tt_last_error(); every argument check happens before any device work.
 */
#ifndef TORTOISE_MI355X_MEL_H
#define TORTOISE_MI355X_MEL_H
#include <stddef.h>
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_MEL_MAX_CLIPS 16 /* clips of one tt_mel_run / tt_mel_spectrum call */

typedef struct tt_mel_config {
  int n_fft;        /* frame length = window length; a multiple of hop and of 64 */
  int hop;          /* frame step; a multiple of 8 */
  int n_mels;       /* rows of fb (1 .. 128) */
  int bins_pad;     /* row length of fb and half the row length of basis: >= n_fft / 2 + 1, a multiple of 32; columns beyond n_fft / 2 are zero */
  int power;        /* 2: re^2 + im^2; 1: its square root */
  int clamp_input;  /* != 0: samples are clamped to [-1, 1] on the read */
  float floor;      /* clamp of the linear mel before the log (reference: 1e-5) */
  int max_samples;  /* longest clip */
  int max_clips;    /* clips per call (1 .. TT_MEL_MAX_CLIPS) */
} tt_mel_config;

typedef struct tt_mel_tables {
  const float* basis;  /* device f32 [n_fft][2 * bins_pad]: column 2 b = window[k] cos(2 pi b k / n_fft), column 2 b + 1 = -window[k] sin(...) */
  const float* fb;     /* device f32 [n_mels][bins_pad] */
  const float* scale;  /* device f32 [n_mels] multiplied onto the log mel, or NULL */
} tt_mel_tables;

typedef struct tt_mel tt_mel;
typedef struct tt_mel_resampler tt_mel_resampler;

int tt_mel_abi_version(void);
size_t tt_mel_struct_size(int which);  /* 0: tt_mel_config, 1: tt_mel_tables */

/* The tables stay the caller's and must outlive the handle. */
int tt_mel_create(const tt_mel_config* cfg, const tt_mel_tables* tables, tt_mel** out);
void tt_mel_destroy(tt_mel* h);
/* Frames of a clip of n samples: 1 + n / hop. */
int tt_mel_frames(const tt_mel* h, int n);

/* wav: device f32.  Clip c is wav[clip_offsets[c] .. + clip_lengths[c]) (host arrays, element units), n_fft / 2 + 1 <= length <= max_samples:
 * reflect padding is undefined for a shorter clip.  Clip c's log mel is written channels-first at out + out_offsets[c] as f32
 * [n_mels][T_c], T_c = tt_mel_frames(length) - the layout tt_cond_ar_clip / tt_cond_diff_clip take.  Asynchronous on `stream`. */
int tt_mel_run(tt_mel* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, int n_clips, float* out,
               const long long* out_offsets, void* stream);
/* Same inputs; writes clip c's spectrum f32 [T_c][bins_pad] at out + out_offsets[c] (columns beyond n_fft / 2 are zero). */
int tt_mel_spectrum(tt_mel* h, const float* wav, const long long* clip_offsets, const int* clip_lengths, int n_clips, float* out,
                    const long long* out_offsets, void* stream);

/* taps: device f32 [new][2 * width + orig] (the caller's; must outlive the handle); orig / new: the two rates divided by their gcd. */
int tt_mel_resampler_create(const float* taps, int orig, int new_rate, int width, int max_samples, tt_mel_resampler** out);
void tt_mel_resampler_destroy(tt_mel_resampler* h);
/* Output length for n input samples: ceil(new * n / orig). */
int tt_mel_resampled_length(const tt_mel_resampler* h, int n);
/* in: device f32 [n] (1 <= n <= max_samples); out: device f32 [tt_mel_resampled_length(n)].  Asynchronous on `stream`. */
int tt_mel_resample(tt_mel_resampler* h, const float* in, int n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
