"""Host side of the F0 tracker (include/tortoise_mi355x_f0.h, csrc/f0.hip, stages.F0Stage) and of its Viterbi path
(include/tortoise_mi355x_f0v.h, csrc/f0_viterbi.hip, stages.F0ViterbiStage): the options of f0() / shift_pitch(to_hz=) / tts(pitch_hz=),
their integers, the costs of smooth= / f0_smooth=, the track a measurement returns (F0Track), and the shift that carries a measured median
to a target."""
import math
import warnings
from collections import namedtuple

import numpy as np

from . import engine as E

SAMPLE_RATE = E.F0_SAMPLE_RATE
HOP_SECONDS = E.F0_HOP / SAMPLE_RATE                                                  # 10 ms
HZ_RANGE = (SAMPLE_RATE / E.F0_LAG_MAX, SAMPLE_RATE / E.F0_LAG_MIN)                   # 50 .. 1000 Hz: what the lags can say
THRESHOLD_RANGE = (0.0, 2.0)
FLOOR_DB_RANGE = (-200.0, 0.0)
SHIFT_RANGE = (-12.0, 12.0)                                                           # what shift_pitch takes
MIN_VOICED = 10                                                                       # frames a median needs
# YIN's own threshold (de Cheveigne & Kawahara use 0.1 .. 0.15) and a floor chosen from the code: nobody has tuned them on a trained
# checkpoint's audio.
DEFAULTS = dict(fmin=60.0, fmax=500.0, threshold=0.15, floor_db=-50.0)

# what the device takes per clip: par = (lag_lo, lag_hi) i32, thr = (thr, floor_e) f64
Params = namedtuple("Params", "lag_lo lag_hi thr floor_e")
# smooth=: the costs of the Viterbi path, cost = (oct, jump, vuv, uv) f64 per clip.  Praat's shape of costs (octave cost, octave-jump cost,
# voiced / unvoiced cost, and a price for staying unvoiced) on the scale of YIN's aperiodicity d', chosen from the arithmetic: a clean dip
# reads d' below 0.1, a frame of noise above 0.5, and an octave is 1.0 in log2 of the lag.  Nobody has tuned them on a trained checkpoint.
Costs = namedtuple("Costs", "oct jump vuv uv")
SMOOTH_DEFAULTS = dict(octave_cost=0.01, jump_cost=0.35, voicing_cost=0.14, unvoiced_cost=0.30)
# L2[tau] = log2(tau) for tau = 1 .. 480 (entry 0 unused): computed here, once, and handed to tt_f0v_create - the device evaluates no
# transcendental, and a reference that reads this list prices every step with the same 480 doubles
LOG2_TABLE = [0.0] + [math.log2(tau) for tau in range(1, E.F0_LAG_MAX + 1)]
JUMP_SEMITONES = 7.0                                                                  # octave_jumps(): further apart than a fifth


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name}={v!r}: a finite number")
    return float(v)


def lags(fmin, fmax):
    """The Python mirror of tt_f0_lags: (lag_lo, lag_hi) = (ceil(24000 / fmax), floor(24000 / fmin)).  ValueError for a range outside
    50 .. 1000 Hz, fmin > fmax, or a range with no whole lag inside."""
    lo_hz, hi_hz = _number("fmin", fmin), _number("fmax", fmax)
    if not HZ_RANGE[0] <= lo_hz <= hi_hz <= HZ_RANGE[1]:
        raise ValueError(f"fmin={lo_hz} Hz .. fmax={hi_hz} Hz is outside the supported range [{HZ_RANGE[0]:g}, {HZ_RANGE[1]:g}] Hz (fmin <= fmax)")
    lo, hi = math.ceil(SAMPLE_RATE / hi_hz), math.floor(SAMPLE_RATE / lo_hz)
    if not E.F0_LAG_MIN <= lo <= hi <= E.F0_LAG_MAX:
        raise ValueError(f"fmin={lo_hz} Hz .. fmax={hi_hz} Hz holds no whole lag at {SAMPLE_RATE} Hz")
    return lo, hi


def params(fmin=DEFAULTS["fmin"], fmax=DEFAULTS["fmax"], threshold=DEFAULTS["threshold"], floor_db=DEFAULTS["floor_db"]):
    """The options in Hz and dB, validated -> Params.  floor_e = W 10^(floor_db / 10): a frame whose power lies below it is unvoiced
    whatever its periodicity.  ValueError names the option."""
    lo, hi = lags(fmin, fmax)
    thr, flo = _number("threshold", threshold), _number("floor_db", floor_db)
    if not THRESHOLD_RANGE[0] <= thr <= THRESHOLD_RANGE[1]:
        raise ValueError(f"threshold={thr} is outside the supported range [{THRESHOLD_RANGE[0]}, {THRESHOLD_RANGE[1]}]")
    if not FLOOR_DB_RANGE[0] <= flo <= FLOOR_DB_RANGE[1]:
        raise ValueError(f"floor_db={flo} dB is outside the supported range [{FLOOR_DB_RANGE[0]}, {FLOOR_DB_RANGE[1]}]")
    return Params(lo, hi, thr, E.F0_WINDOW * 10.0 ** (flo / 10.0))


def frames(n):
    return -(-int(n) // E.F0_HOP)


def smooth_params(smooth):
    """smooth= of f0() / f0_smooth= of shift_pitch(to_hz=) and tts(pitch_hz=), validated -> Costs, or None for off (None / False).  True: the
    defaults; a dict with any of octave_cost, jump_cost, voicing_cost, unvoiced_cost sets those (the others keep their defaults).  An
    unknown key, or a value that is negative or not a finite number, is a ValueError that names it."""
    if smooth is None or smooth is False:
        return None
    if isinstance(smooth, Costs):
        smooth = dict(zip(SMOOTH_DEFAULTS, smooth))
    elif smooth is True:
        smooth = {}
    elif not isinstance(smooth, dict):
        raise ValueError(f"smooth={smooth!r}: None / False (off), True (the default costs) or a dict with any of {sorted(SMOOTH_DEFAULTS)}")
    unknown = sorted(set(smooth) - set(SMOOTH_DEFAULTS))
    if unknown:
        raise ValueError(f"smooth: unknown key {unknown[0]!r} (the costs are {sorted(SMOOTH_DEFAULTS)})")
    v = {k: _number(k, smooth.get(k, d)) for k, d in SMOOTH_DEFAULTS.items()}
    for k, x in v.items():
        if x < 0:
            raise ValueError(f"{k}={x}: a cost is not negative")
    return Costs(v["octave_cost"], v["jump_cost"], v["voicing_cost"], v["unvoiced_cost"])


def smooth_option(kwargs, pitch_hz, who="tts"):
    """Takes `f0_smooth` out of a call's **kwargs -> Costs, or None (absent, None or False: the plain tracker measures).  It belongs to the
    one f0_many call of pitch_hz= / to_hz=: without that target it is a ValueError."""
    if "f0_smooth" not in kwargs:
        return None
    costs = smooth_params(kwargs.pop("f0_smooth"))
    if costs is not None and pitch_hz is None:
        raise ValueError(f"{who}: f0_smooth= smooths the measurement of {'to_hz' if who.startswith('shift_pitch') else 'pitch_hz'}= and does "
                         "nothing without it: give the target too, or call f0(audio, smooth=...) for the track")
    return costs


def target_hz(name, v):
    """A pitch to land on (to_hz=, pitch_hz=), validated -> float Hz."""
    hz = _number(name, v)
    if not HZ_RANGE[0] <= hz <= HZ_RANGE[1]:
        raise ValueError(f"{name}={hz} Hz is outside the supported range [{HZ_RANGE[0]:g}, {HZ_RANGE[1]:g}] Hz")
    return hz


def shift_to(measured_hz, to_hz, who="shift_pitch", clip=None):
    """The shift that carries a clip whose median F0 is measured_hz (None: no median) to to_hz -> (semitones, clamped): 12 log2(to / measured),
    clamped to +-12 with a warning; a clip with no median is left alone (0 semitones), with a warning."""
    which = "" if clip is None else f" clip {clip}:"
    if measured_hz is None:
        warnings.warn(f"{who}:{which} fewer than {MIN_VOICED} voiced frames, no median F0 to move to {to_hz:g} Hz: the clip is returned as it is",
                      stacklevel=3)
        return 0.0, False
    s = 12.0 * math.log2(to_hz / measured_hz)
    if not SHIFT_RANGE[0] <= s <= SHIFT_RANGE[1]:
        c = min(SHIFT_RANGE[1], max(SHIFT_RANGE[0], s))
        warnings.warn(f"{who}:{which} {measured_hz:.1f} Hz -> {to_hz:g} Hz is {s:+.2f} semitones, outside [{SHIFT_RANGE[0]}, {SHIFT_RANGE[1]}]: "
                      f"clamped to {c:+.0f}", stacklevel=3)
        return c, True
    return s, False


def options(kwargs, pitch=None, who="tts"):
    """Takes `pitch_hz` out of a tts() call's **kwargs -> the target in Hz, or None (absent or None: nothing is built, nothing changes).
    `pitch`: what resample.options returned; the two are exclusive, as pitch_hz is with word_pitches."""
    hz = kwargs.pop("pitch_hz", None)
    if hz is None:
        return None
    hz = target_hz("pitch_hz", hz)
    if pitch is not None or "word_pitches" in kwargs and kwargs["word_pitches"] is not None:
        raise ValueError(f"{who}: pitch_hz= (an absolute pitch) goes with neither pitch= nor word_pitches= (relative ones): give one of them")
    return hz


FORMANT_KEYWORDS = ("formants", "formant_shift", "formant_lifter_ms", "formant_max_gain_db")


def formant_keywords(kwargs):
    """The formant keywords of a tts() call as given (before formant.options takes them out): with pitch_hz= the correction is planned per
    clip, once every clip's own shift is known."""
    return {k: kwargs[k] for k in FORMANT_KEYWORDS if k in kwargs}


def refuse(kwargs, who, why, instead):
    for key in ("pitch_hz", "f0_smooth"):
        if key in kwargs:
            raise ValueError(f"{who}: {key} is not available {why}; {instead}")


def refuse_streaming(kwargs, who):
    refuse(kwargs, who, "for streamed audio (the shift comes from the median F0 of the finished clip, and the pieces leave as they are made)",
           "use tts() / tts_many(), or shift_pitch(to_hz=) the collected clip")


def refuse_long_form(kwargs, who="read_long_form"):
    refuse(kwargs, who, "for a reading (its chunks need ONE shift from a median pooled over all of them, which is not built)",
           "use shift_pitch(to_hz=) on the finished reading, or pitch= in semitones")


def refuse_sharded(kwargs, who):
    refuse(kwargs, who, "on a sharded job (the ranks that return no audio have nothing to measure)",
           "build TextToSpeech(candidate_sharding=False), or shift_pitch(to_hz=) what rank 0 returns")


class F0Track:
    """The F0 of one clip, a frame every 10 ms (frame f stands at f * hop_seconds): hz f32 [F] (0 where unvoiced), aperiodicity f32 [F]
    (YIN's d' at the chosen lag: 0 periodic .. 1 and above noise), lag i32 [F] (the chosen period in samples before refinement).  A track
    measured with smooth= is `smoothed`: state i32 [F] is the candidate the Viterbi path chose in every frame (0 .. 6 by ascending lag, 7
    unvoiced) and path_cost the path's total cost; both are None on a plain track."""

    hop_seconds = HOP_SECONDS

    def __init__(self, hz, aperiodicity, lag, samples=None, state=None, path_cost=None):
        self.hz = np.asarray(hz, dtype=np.float32)
        self.aperiodicity = np.asarray(aperiodicity, dtype=np.float32)
        self.lag = np.asarray(lag, dtype=np.int32)
        self.samples = None if samples is None else int(samples)
        if not (self.hz.ndim == 1 and self.hz.shape == self.aperiodicity.shape == self.lag.shape):
            raise ValueError(f"F0Track: hz {self.hz.shape}, aperiodicity {self.aperiodicity.shape} and lag {self.lag.shape} must be one [F]")
        self.state = None if state is None else np.asarray(state, dtype=np.int32)
        self.path_cost = None if state is None or path_cost is None else float(path_cost)
        if self.state is not None and self.state.shape != self.hz.shape:
            raise ValueError(f"F0Track: state {self.state.shape} must be hz's {self.hz.shape}")

    @property
    def smoothed(self):
        return self.state is not None

    def octave_jumps(self, min_semitones=JUMP_SEMITONES):
        """The adjacent pairs of voiced frames whose F0 lies further apart than min_semitones: what an octave slip of the tracker leaves
        in a track (a voice does not move a fifth in 10 ms)."""
        m = _number("min_semitones", min_semitones)
        if m <= 0:
            raise ValueError(f"min_semitones={m}: a positive interval")
        hz = self.hz.astype(np.float64)
        both = (hz[:-1] > 0) & (hz[1:] > 0)
        st = 12.0 * np.abs(np.log2(hz[1:][both] / hz[:-1][both]))
        return int(np.count_nonzero(st > m))

    def __len__(self):
        return int(self.hz.shape[0])

    @property
    def voiced(self):
        return self.hz > 0

    def times(self):
        """Seconds of every frame, f64 [F]."""
        return np.arange(len(self), dtype=np.float64) * self.hop_seconds

    def _voiced_hz(self, frames_=None):
        hz = self.hz if frames_ is None else self.hz[frames_]
        return hz[hz > 0].astype(np.float64)

    def median_hz(self, min_voiced=MIN_VOICED):
        """The median over the voiced frames, None where fewer than min_voiced are."""
        v = self._voiced_hz()
        return float(np.median(v)) if v.size >= max(1, int(min_voiced)) else None

    def semitones(self, ref_hz):
        """12 log2(hz / ref_hz) of every frame, f64 [F], NaN where unvoiced."""
        ref = target_hz("ref_hz", ref_hz)
        out = np.full(len(self), np.nan)
        v = self.voiced
        out[v] = 12.0 * np.log2(self.hz[v].astype(np.float64) / ref)
        return out

    def range_semitones(self, lo=5, hi=95, min_voiced=MIN_VOICED):
        """The span between the lo-th and the hi-th percentile of the voiced frames, in semitones; None where fewer than min_voiced are."""
        if not 0 <= lo <= hi <= 100:
            raise ValueError(f"range_semitones: percentiles lo={lo!r}, hi={hi!r} (0 <= lo <= hi <= 100)")
        v = self._voiced_hz()
        if v.size < max(1, int(min_voiced)):
            return None
        a, b = np.percentile(v, [lo, hi])
        return float(12.0 * np.log2(b / a))

    def at(self, seconds):
        """hz of the frame nearest to `seconds` (0 where it is unvoiced); ValueError outside the clip."""
        s = _number("seconds", seconds)
        f = int(math.floor(s / self.hop_seconds + 0.5))
        if s < 0 or f >= len(self):
            raise ValueError(f"F0Track.at: {s} s is outside the clip ({len(self)} frames of {self.hop_seconds * 1000:g} ms)")
        return float(self.hz[f])

    def for_words(self, alignment):
        """One median per word of an align.Alignment of this clip: over the voiced frames that stand inside the word's span
        [start, end), None for a word with none."""
        t = np.arange(len(self), dtype=np.int64) * E.F0_HOP * int(alignment.rate)  # frame times in units of 1 / (24000 rate) s
        out = []
        for _, a, b, _ in alignment.words:
            inside = (t >= int(a) * SAMPLE_RATE) & (t < int(b) * SAMPLE_RATE)
            v = self._voiced_hz(inside)
            out.append(float(np.median(v)) if v.size else None)
        return out


def track_of(result, samples=None):
    """One dict of stages.F0Stage.track_many (or stages.F0ViterbiStage.track_many: a smoothed track) -> F0Track."""
    return F0Track(result["f0"], result["aper"], result["lag"], samples, result.get("state"), result.get("path_cost"))
