"""Host side of the formant correction (include/tortoise_mi355x_fmt.h, csrc/formant.hip, stages.FormantStage): the options of a tts()
call, the warp of a pitch and a formant shift, and the four tables, each computed in fp64 and rounded once to f32."""
import collections
import math

import torch

from . import engine as E
from .pack import MEL_BINS_PAD, MEL_HOP, MEL_N_FFT, stft_basis

SAMPLE_RATE = 24000
N_FFT, HOP, BINS_PAD = MEL_N_FFT, MEL_HOP, MEL_BINS_PAD
BINS = N_FFT // 2 + 1
MIN_SAMPLES = BINS                      # reflect padding is undefined for a shorter clip
WARP_RANGE = (0.5, 2.0)                 # alpha
FORMANT_SHIFT_RANGE = (-12.0, 12.0)     # formant_shift= of a tts() call, semitones
Q_RANGE = (16, E.FMT_Q_PAD)
DEFAULT_LIFTER_MS = 2.0                 # Q = 48: below the pitch period of any voice under 500 Hz
DEFAULT_MAX_GAIN_DB = 24.0
MAX_GAIN_DB_RANGE = (0.0, 200.0)        # 0: no clamp
MODES = (None, "follow", "keep")


def lifter_q(ms=DEFAULT_LIFTER_MS):
    """formant_lifter_ms -> Q = round(ms * 24) cepstral coefficients, 16 .. 64.  ValueError otherwise."""
    try:
        v = float(ms)
    except (TypeError, ValueError):
        raise ValueError(f"formant_lifter_ms={ms!r}: a number of milliseconds") from None
    q = int(round(v * SAMPLE_RATE / 1000.0)) if math.isfinite(v) else -1
    if not Q_RANGE[0] <= q <= Q_RANGE[1]:
        raise ValueError(f"formant_lifter_ms={ms!r} gives {q} cepstral coefficients; the stage takes {Q_RANGE[0]} .. {Q_RANGE[1]} "
                         f"({Q_RANGE[0] / 24:.3f} .. {Q_RANGE[1] / 24:.3f} ms)")
    return q


def max_gain_db(db=DEFAULT_MAX_GAIN_DB):
    """formant_max_gain_db -> float dB in 0 .. 200 (0: no clamp).  ValueError otherwise."""
    try:
        v = float(db)
    except (TypeError, ValueError):
        raise ValueError(f"formant_max_gain_db={db!r}: a number of dB") from None
    if not (MAX_GAIN_DB_RANGE[0] <= v <= MAX_GAIN_DB_RANGE[1]):  # (NaN fails too)
        raise ValueError(f"formant_max_gain_db={db!r} is outside {MAX_GAIN_DB_RANGE[0]} .. {MAX_GAIN_DB_RANGE[1]} dB (0: no clamp)")
    return v


def warp(pitch=None, formant_shift=None):
    """alpha = 2^((s - f) / 12): `pitch` s semitones whose move of the formants is taken back (None: no correction for a pitch), and the
    formants moved up by `formant_shift` f semitones (None: 0).  ValueError for a shift outside +-12 or a combined warp outside [0.5, 2]."""
    s = 0.0 if pitch is None else float(pitch)
    f = 0.0 if formant_shift is None else float(formant_shift)
    if not (math.isfinite(s) and FORMANT_SHIFT_RANGE[0] <= f <= FORMANT_SHIFT_RANGE[1]):
        raise ValueError(f"formant_shift={formant_shift!r} semitones is outside the supported range [{FORMANT_SHIFT_RANGE[0]}, "
                         f"{FORMANT_SHIFT_RANGE[1]}] (pitch={pitch!r})")
    a = 2.0 ** ((s - f) / 12.0)
    if not WARP_RANGE[0] <= a <= WARP_RANGE[1]:
        raise ValueError(f"pitch={s} semitones kept with formant_shift={f} semitones needs an envelope warp of {a:.4f}, outside the "
                         f"supported range [{WARP_RANGE[0]}, {WARP_RANGE[1]}]")
    return a


Params = collections.namedtuple("Params", "alpha q max_gain_db")  # what the chain's formant step runs with


def mode(value):
    """formants= -> True for 'keep'.  ValueError unless 'keep', 'follow' or None."""
    if value not in MODES:
        raise ValueError(f"formants={value!r}: 'keep' (the formants stay where they were before the pitch shift), 'follow' or None (they move "
                         f"with the pitch)")
    return value == "keep"


def params(pitch=None, keep=False, formant_shift=None, lifter_ms=None, gain_db=None):
    """-> Params, or None where nothing is to run (no keyword, 'keep' without a pitch, or a warp of exactly 1).  Everything is validated
    either way."""
    q = lifter_q(DEFAULT_LIFTER_MS if lifter_ms is None else lifter_ms)
    g = max_gain_db(DEFAULT_MAX_GAIN_DB if gain_db is None else gain_db)
    if not keep and formant_shift is None:
        return None
    a = warp(pitch if keep else None, formant_shift)
    return None if a == 1.0 else Params(a, q, g)


def options(kwargs, pitch=None):
    """Takes `formants`, `formant_shift`, `formant_lifter_ms` and `formant_max_gain_db` out of a tts() call's **kwargs -> Params or None
    (neither of the first two given, formants='follow', 'keep' without a pitch, or a warp of exactly 1: nothing is built, nothing changes).
    `pitch`: what resample.options returned."""
    keep = mode(kwargs.pop("formants", None))
    return params(pitch, keep, kwargs.pop("formant_shift", None), kwargs.pop("formant_lifter_ms", None), kwargs.pop("formant_max_gain_db", None))


def refuse_streaming(kwargs, who):
    for k in ("formants", "formant_shift", "formant_lifter_ms", "formant_max_gain_db"):
        if k in kwargs:
            raise ValueError(f"{who}: {k} is not available for streamed audio (the correction overlaps frames of 1024 samples across the "
                             f"pieces' borders, and they are cross-faded as they are made); use tts() / tts_many(), or shift_formants() the "
                             f"collected clip")


def bin_weights(n_fft=N_FFT):
    """wt_b of the half spectrum: 1 for b = 0 and n_fft / 2, else 2; fp64 [n_fft / 2 + 1]"""
    wt = torch.full((n_fft // 2 + 1,), 2.0, dtype=torch.float64)
    wt[0] = wt[-1] = 1.0
    return wt


def window(n_fft=N_FFT):
    """the periodic Hann window of pack.stft_basis, fp64"""
    return 0.5 - 0.5 * torch.cos(torch.arange(n_fft, dtype=torch.float64) * (2.0 * math.pi / n_fft))


def cepstrum_table(q, n_fft=N_FFT, bins_pad=BINS_PAD):
    """A fp64 [bins_pad][64]: A[b][j] = wt_b cos(2 pi j b / n_fft) / n_fft for j < q and b <= n_fft / 2, else 0 (phase reduced in integers)."""
    b = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    j = torch.arange(q, dtype=torch.int64)[None, :]
    A = torch.zeros(bins_pad, E.FMT_Q_PAD, dtype=torch.float64)
    A[:n_fft // 2 + 1, :q] = bin_weights(n_fft)[:, None] * torch.cos(((b * j) % n_fft).double() * (2.0 * math.pi / n_fft)) / n_fft
    return A


def warp_table(alpha, q, n_fft=N_FFT, bins_pad=BINS_PAD):
    """D fp64 [64][bins_pad]: D[j][b] = 2 h_j (cos(j min(alpha w_b, pi)) - cos(j w_b)), h_j = 0.5 (1 + cos(pi j / q)), w_b = 2 pi b / n_fft,
    for 1 <= j < q and b <= n_fft / 2; row 0 (the level cancels) and everything else 0."""
    w = torch.arange(n_fft // 2 + 1, dtype=torch.float64) * (2.0 * math.pi / n_fft)
    j = torch.arange(q, dtype=torch.float64)[:, None]
    h = 0.5 * (1.0 + torch.cos(math.pi * j / q))
    D = torch.zeros(E.FMT_Q_PAD, bins_pad, dtype=torch.float64)
    D[:q, :n_fft // 2 + 1] = 2.0 * h * (torch.cos(j * (float(alpha) * w).clamp(max=math.pi)[None, :]) - torch.cos(j * w[None, :]))
    D[0] = 0.0
    return D


def inverse_basis(n_fft=N_FFT, bins_pad=BINS_PAD):
    """fp64 [2 * bins_pad][n_fft]: row 2 b = window[k] wt_b cos(2 pi b k / n_fft) / n_fft, row 2 b + 1 = -window[k] wt_b sin(2 pi b k / n_fft)
    / n_fft, zero for b > n_fft / 2: the real inverse DFT of a half spectrum with the synthesis window folded in."""
    k = torch.arange(n_fft, dtype=torch.int64)[None, :]
    b = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    ang = ((k * b) % n_fft).double() * (2.0 * math.pi / n_fft)
    s = (bin_weights(n_fft)[:, None] * window(n_fft)[None, :]) / n_fft
    inv = torch.zeros(bins_pad, 2, n_fft, dtype=torch.float64)
    inv[:n_fft // 2 + 1, 0] = s * torch.cos(ang)
    inv[:n_fft // 2 + 1, 1] = -s * torch.sin(ang)
    return inv.reshape(2 * bins_pad, n_fft)


def tables(q, warps):
    """Host tables of a tt_fmt handle, rounded once to f32: {'basis', 'inverse', 'cepstrum', 'warps' [len(warps)][64][bins_pad]}."""
    if not 1 <= len(warps) <= E.FMT_MAX_WARPS:
        raise ValueError(f"{len(warps)} warps for one handle (1 .. {E.FMT_MAX_WARPS})")
    return {"basis": stft_basis().float(), "inverse": inverse_basis().float(), "cepstrum": cepstrum_table(q).float(),
            "warps": torch.stack([warp_table(a, q) for a in warps]).float()}
