"""Host side of the spectral-subtraction denoiser (include/tortoise_mi355x_nr.h, csrc/denoise.hip, stages.DenoiseStage): defaults, ranges
and option parsing, the quantile correction c in fp64, a noise region in seconds -> frames, and the two tables (formant's, rounded once).

**The defaults come from the arithmetic of DESIGN.md 5.38 and one synthetic family (a harmonic vowel in white and pink Gaussian noise).
Nobody has run a real recording or a trained checkpoint through them.**"""
import collections
import math

from . import engine as E
from . import formant as fmt
from .pack import stft_basis

N_FFT, HOP, BINS_PAD, BINS = fmt.N_FFT, fmt.HOP, fmt.BINS_PAD, fmt.BINS
MIN_SAMPLES = BINS                      # reflect padding is undefined for a shorter clip
VOICE_SAMPLE_RATE = 22050               # the clips of voice_samples=
DEFAULTS = dict(reduction_db=12.0, beta=2.0, quantile=0.2, smooth_frames=2, smooth_bins=2)
REDUCTION_DB_RANGE = (0.0, 40.0)        # 0 < .. 40; 0 or None: nothing runs
BETA_RANGE = (1.0, 4.0)
QUANTILE_RANGE = (0.01, 0.5)            # resolved to 1 / 10000
SMOOTH_RANGE = (0, E.NR_MAX_SMOOTH)
STATUS = {E.NR_OK: "ok", E.NR_SHORT: "short", E.NR_REFUSED: "refused"}
INHERIT = "inherit"                     # get_conditioning_latents(denoise=INHERIT): what the constructor was given

# what a call runs with: the keywords as given, and what the library takes (tt_nr_params)
Params = collections.namedtuple("Params", "reduction_db beta quantile smooth_frames smooth_bins quantile_num quantile_scale g_min")


def _number(name, v, lo, hi, open_lo=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name}={v!r}: a number") from None
    if not ((lo < f if open_lo else lo <= f) and f <= hi):  # (NaN fails too)
        raise ValueError(f"{name}={v!r} is outside {'(' if open_lo else '['}{lo}, {hi}]")
    return f


def _radius(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or not SMOOTH_RANGE[0] <= v <= SMOOTH_RANGE[1]:
        raise ValueError(f"{name}={v!r}: an integer in {SMOOTH_RANGE[0]} .. {SMOOTH_RANGE[1]}")
    return v


def quantile_scale(quantile_num):
    """c = 1 / (-ln(1 - q)), q = quantile_num / 10000, in fp64: the q-quantile of an exponentially distributed power is -ln(1 - q) times its
    mean.  The library gets it rounded once to f32."""
    return 1.0 / -math.log1p(-quantile_num / E.NR_QUANTILE_DEN)


def params(reduction_db=DEFAULTS["reduction_db"], beta=DEFAULTS["beta"], quantile=DEFAULTS["quantile"], smooth_frames=DEFAULTS["smooth_frames"],
           smooth_bins=DEFAULTS["smooth_bins"]):
    """-> Params, or None where nothing is to run (reduction_db None or 0).  Everything is validated either way; ValueError otherwise."""
    b = _number("beta", beta, *BETA_RANGE)
    q = _number("quantile", quantile, *QUANTILE_RANGE)
    rt, rb = _radius("smooth_frames", smooth_frames), _radius("smooth_bins", smooth_bins)
    if reduction_db is None:
        return None
    db = _number("reduction_db", reduction_db, *REDUCTION_DB_RANGE)
    if db == 0.0:
        return None
    num = int(round(q * E.NR_QUANTILE_DEN))
    return Params(db, b, q, rt, rb, num, quantile_scale(num), 10.0 ** (-db / 20.0))


def from_option(option):
    """denoise_voice_samples= / denoise= -> Params or None: True is the defaults, a dict their keywords (reduction_db, beta, quantile,
    smooth_frames, smooth_bins), None or False nothing.  ValueError otherwise."""
    if option is None or option is False:
        return None
    if option is True:
        return params()
    if isinstance(option, dict):
        unknown = sorted(set(option) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"denoise: unknown option {unknown[0]!r} (the options are {', '.join(DEFAULTS)})")
        return params(**option)
    raise ValueError(f"denoise={option!r}: True, a dict of options or None")


def keywords(p):
    """Params -> the keywords of denoise_many"""
    return {k: getattr(p, k) for k in DEFAULTS}


def c_params(p):
    """Params -> E.NrParams"""
    c = E.NrParams()
    c.quantile_num, c.quantile_scale, c.beta, c.g_min, c.smooth_frames, c.smooth_bins = p.quantile_num, p.quantile_scale, p.beta, p.g_min, \
        p.smooth_frames, p.smooth_bins
    return c


def frames(n, hop=HOP):
    return 1 + n // hop


def rank(quantile_num, n_frames):
    """k = floor(q (T - 1)) in integers: tt_nr_rank"""
    return quantile_num * (n_frames - 1) // E.NR_QUANTILE_DEN


def region(start, end, n_frames, hop=HOP):
    """the frames t < n_frames with start <= t hop and t hop + hop <= end (samples) -> (first, count): tt_nr_region"""
    lo, hi = -(-start // hop), min(end // hop, n_frames)
    return min(lo, n_frames), max(hi - lo, 0)


def region_frames(noise, n, sample_rate, who="denoise", clip=0):
    """noise=None -> (0, 0), auto; noise=(start_s, end_s) of a clip of n samples -> (first frame, frames), the frames that lie inside the
    region whole.  ValueError for anything else, a region outside the clip or one of fewer than 8 frames."""
    if noise is None:
        return 0, 0
    try:
        a, b = (float(v) for v in noise)
        sr = float(sample_rate)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: clip {clip}: noise={noise!r}: None or (start_s, end_s)") from None
    if not (math.isfinite(a) and math.isfinite(b) and 0.0 <= a <= b and sr > 0 and math.isfinite(sr)):
        raise ValueError(f"{who}: clip {clip}: noise={noise!r} at sample_rate={sample_rate!r}: 0 <= start_s <= end_s")
    s0, s1 = int(math.ceil(a * sr)), min(int(math.floor(b * sr)), n)
    first, count = region(s0, max(s1, s0), frames(n))
    if count < E.NR_MIN_REGION:
        raise ValueError(f"{who}: clip {clip}: noise={noise!r} holds {count} whole frames of {HOP} samples; the noise floor needs at least "
                         f"{E.NR_MIN_REGION} ({E.NR_MIN_REGION * HOP / sr:.3f} s)")
    return first, count


def refuse_streaming(kwargs, who):
    for k in ("denoise", "denoise_voice_samples"):
        if k in kwargs:
            raise ValueError(f"{who}: {k} is not available for streamed audio (the noise floor is an order statistic over all frames of a "
                             f"clip); clean the voice clips with TextToSpeech(denoise_voice_samples=) or denoise() them first")


def noise_dbfs(floor):
    """The level of white noise with this floor, dB re full scale (rms 1): the mean of S over the whole spectrum is sigma^2 sum window^2."""
    s = floor.double().reshape(-1)[:BINS]
    level = float((s * fmt.bin_weights()).sum()) / N_FFT / float((fmt.window() ** 2).sum())
    return 10.0 * math.log10(level) if level > 0 else -math.inf


def tables():
    """Host tables of a tt_nr handle, rounded once to f32: {'basis', 'inverse'} - formant's."""
    return {"basis": stft_basis().float(), "inverse": fmt.inverse_basis().float()}
