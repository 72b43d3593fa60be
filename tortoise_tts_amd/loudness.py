"""Host side of the loudness normalisation (include/tortoise_mi355x_loud.h, csrc/loudness.hip, stages.LoudnessStage): the options of a
tts() call, dB <-> linear, and the per-clip result; and of the streaming leveler (include/tortoise_mi355x_lvs.h, csrc/loudness_stream.hip,
stages.StreamLevelStage): its keywords, the settings of a slot and a stream's reading."""
import dataclasses
import math
from typing import Optional

from . import engine as E

LUFS_RANGE = (-70.0, -5.0)      # targets a caller may ask for
TRUE_PEAK_RANGE = (-60.0, 0.0)  # ceilings, dBTP
MODES = {"none": E.LOUD_NONE, "scale": E.LOUD_SCALE, "lookahead": E.LOUD_LOOKAHEAD_MODE}
STATUS = {E.LOUD_OK: "ok", E.LOUD_SHORT: "short", E.LOUD_SILENT: "silent", E.LOUD_EMPTY: "empty", E.LOUD_REFUSED: "refused"}
SCOPES = ("chunk", "whole")


def db(v):
    """Linear amplitude -> dB (-inf for 0)."""
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def linear(d):
    """dB -> linear amplitude."""
    return 10.0 ** (float(d) / 20.0)


@dataclasses.dataclass(frozen=True)
class Level:
    """What a call asks for: a target (LUFS), a true-peak ceiling (dBTP) and how the ceiling is kept."""
    loudness: float
    true_peak: float = -1.0
    limit: str = "scale"

    @property
    def mode(self):
        return MODES[self.limit]

    @property
    def ceiling(self):
        return linear(self.true_peak)


def level(loudness, true_peak=-1.0, limit="scale"):
    """Validated Level.  ValueError for a target outside -70 .. -5 LUFS, a ceiling above 0 dBTP (or below -60) or an unknown limit."""
    loudness, true_peak = float(loudness), float(-1.0 if true_peak is None else true_peak)
    limit = "scale" if limit is None else limit
    if not LUFS_RANGE[0] <= loudness <= LUFS_RANGE[1]:  # (NaN fails too)
        raise ValueError(f"loudness={loudness} LUFS is outside the supported range [{LUFS_RANGE[0]}, {LUFS_RANGE[1]}]")
    if not TRUE_PEAK_RANGE[0] <= true_peak <= TRUE_PEAK_RANGE[1]:
        raise ValueError(f"true_peak={true_peak} dBTP is outside the supported range [{TRUE_PEAK_RANGE[0]}, {TRUE_PEAK_RANGE[1]}]")
    if limit not in MODES:
        raise ValueError(f"limit={limit!r}: expected one of {sorted(MODES)}")
    return Level(loudness, true_peak, limit)


def level_options(kwargs):
    """Takes `loudness`, `true_peak` and `limit` out of a tts() call's **kwargs -> None (loudness absent or None: nothing is built, nothing
    changes) or the validated Level."""
    loudness, true_peak, limit = kwargs.pop("loudness", None), kwargs.pop("true_peak", None), kwargs.pop("limit", None)
    if loudness is None:
        if true_peak is not None or limit is not None:
            raise ValueError("true_peak= and limit= belong to loudness=: give a target in LUFS")
        return None
    return level(loudness, true_peak, limit)


def scope_option(kwargs):
    scope = kwargs.pop("loudness_scope", "chunk")
    if scope not in SCOPES:
        raise ValueError(f"loudness_scope={scope!r}: expected one of {list(SCOPES)}")
    return scope


def refuse_streaming(kwargs, who):
    if any(k in kwargs for k in ("loudness", "true_peak", "limit")):
        raise ValueError(f"{who}: loudness is not available for streamed audio (an integrated loudness needs the whole clip, and the first "
                         f"pieces are delivered before the last exist); use tts() / tts_many(), or normalize() the collected clip")


@dataclasses.dataclass(frozen=True)
class Loudness:
    """One clip's reading.  lufs: integrated loudness (-inf for a clip shorter than 400 ms or without a block above -70 LUFS: status 'short' /
    'silent', such clips are returned unchanged); true_peak_db: dBTP of the input.  After normalize(): gain_db, the applied gain;
    out_true_peak_db, measured on the result; shortfall_lu, how far below the target the ceiling held the clip (0 unless limit='scale' bound)."""
    lufs: float
    true_peak_db: float
    gain_db: Optional[float] = None
    out_true_peak_db: Optional[float] = None
    shortfall_lu: Optional[float] = None
    status: str = "ok"


def reading(r, target=None):
    """A stage result dict (stages.LoudnessStage) -> Loudness."""
    st = STATUS[r["status"]]
    if "gain" not in r:
        return Loudness(r["lufs"], db(r["true_peak"]), status=st)
    gain_db = db(r["gain"])
    shortfall = (target - r["lufs"]) - gain_db if st == "ok" else 0.0
    shortfall = shortfall if shortfall > 1e-5 else 0.0  # (the gain is rounded to f32: 5e-7 dB)
    return Loudness(r["lufs"], db(r["true_peak"]), gain_db, db(r["out_true_peak"]), shortfall, st)


# ------------------------------------------------------------------------------------------------ the streaming leveler
STREAM_LIMITS = {"none": E.LVS_NONE, "lookahead": E.LVS_LOOKAHEAD}
STREAM_GAIN_RANGE = (-60.0, 60.0)  # dB a fixed gain may ask for
# Chosen from the arithmetic, not by ear - nobody has heard a trained checkpoint through them: a stream may be lifted 12 dB and lowered
# 24 dB from where it starts; it falls at 12 dB/s (a too-loud voice is corrected within a second or two) and rises at 3 dB/s (slower than
# the 400 ms blocks react, so a pause does not pump the gain up).
STREAM_LEVEL_DEFAULTS = dict(assume=None, boost=12.0, cut=24.0, rise=3.0, fall=12.0)
STREAM_KEYS = ("stream_loudness", "stream_gain", "stream_true_peak", "stream_limit", "stream_level")


def stream_ready(n_before, n_chunk, limit, flush):
    """The Python mirror of tt_lvs_ready: the outputs a push of n_chunk samples emits on a stream that holds n_before; limit E.LVS_NONE /
    E.LVS_LOOKAHEAD.  Under the limiter a sample is ready once the E.LVS_DELAY behind it are in; a flush makes everything ready."""
    total = lambda n, fl: n if fl or limit == E.LVS_NONE else max(n - E.LVS_DELAY, 0)
    return total(n_before + n_chunk, flush) - total(n_before, False)


def stream_latency(limit):
    """Input samples a stream's output lags by until the flush."""
    return E.LVS_DELAY if limit == E.LVS_LOOKAHEAD else 0


@dataclasses.dataclass(frozen=True)
class StreamSettings:
    """One stream's settings as tt_lvs_open takes them.  steer: E.LVS_ADAPT (towards `target` LUFS) or E.LVS_FIXED (gain0 throughout);
    limit: E.LVS_NONE or E.LVS_LOOKAHEAD under `ceiling` (linear)."""
    steer: int
    limit: int
    gain0: float = 1.0
    target: float = -23.0
    ceiling: float = 1.0
    boost: float = 12.0
    cut: float = 24.0
    rise: float = 3.0
    fall: float = 12.0

    def args(self):
        import ctypes as C
        return (self.steer, self.limit) + tuple(C.c_float(v) for v in (self.gain0, self.target, self.ceiling, self.boost, self.cut, self.rise,
                                                                         self.fall))


def stream_settings(loudness=None, gain=None, true_peak=None, limit=None, level=None):
    """The validated StreamSettings of stream_loudness= (a target in LUFS: ADAPT) or stream_gain= (dB: FIXED) - exactly one of them -,
    stream_true_peak= (dBTP; giving it, or a target alone, selects the look-ahead limiter, at -1 dBTP by default), stream_limit=
    ('lookahead' | 'none') and stream_level= (a dict over STREAM_LEVEL_DEFAULTS).  ValueError for anything else."""
    if (loudness is None) == (gain is None):
        raise ValueError("give exactly one of stream_loudness= (a target in LUFS) and stream_gain= (a fixed gain in dB)")
    opts = dict(STREAM_LEVEL_DEFAULTS)
    if level is not None:
        if not isinstance(level, dict) or set(level) - set(opts):
            raise ValueError(f"stream_level={level!r}: a dict with keys out of {sorted(opts)}")
        opts.update(level)
    for k in ("boost", "cut", "rise", "fall"):
        v = opts[k] = float(opts[k])
        if not 0.0 <= v <= 1000.0:  # (NaN fails too)
            raise ValueError(f"stream_level[{k!r}]={v}: expected 0 .. 1000 (dB for boost and cut, dB per second for rise and fall)")
    if limit is not None and limit not in STREAM_LIMITS:
        raise ValueError(f"stream_limit={limit!r}: expected one of {sorted(STREAM_LIMITS)}")
    if true_peak is not None and not TRUE_PEAK_RANGE[0] <= float(true_peak) <= TRUE_PEAK_RANGE[1]:
        raise ValueError(f"stream_true_peak={true_peak} dBTP is outside the supported range [{TRUE_PEAK_RANGE[0]}, {TRUE_PEAK_RANGE[1]}]")
    if limit == "none" and true_peak is not None:
        raise ValueError("stream_true_peak= needs the limiter: stream_limit='none' keeps no ceiling")
    if limit is None:
        limit = "lookahead" if (true_peak is not None or loudness is not None) else "none"
    ceiling = linear(-1.0 if true_peak is None else float(true_peak))
    if loudness is not None:
        T = float(loudness)
        if not LUFS_RANGE[0] <= T <= LUFS_RANGE[1]:
            raise ValueError(f"stream_loudness={T} LUFS is outside the supported range [{LUFS_RANGE[0]}, {LUFS_RANGE[1]}]")
        gain0 = 1.0
        if opts["assume"] is not None:
            a = float(opts["assume"])
            if not LUFS_RANGE[0] <= a <= LUFS_RANGE[1]:
                raise ValueError(f"stream_level['assume']={a} LUFS is outside the supported range [{LUFS_RANGE[0]}, {LUFS_RANGE[1]}]")
            gain0 = linear(min(max(T - a, -opts["cut"]), opts["boost"]))
        return StreamSettings(E.LVS_ADAPT, STREAM_LIMITS[limit], gain0, T, ceiling, opts["boost"], opts["cut"], opts["rise"], opts["fall"])
    g = float(gain)
    if opts["assume"] is not None:
        raise ValueError("stream_level['assume'] belongs to stream_loudness=")
    if not STREAM_GAIN_RANGE[0] <= g <= STREAM_GAIN_RANGE[1]:
        raise ValueError(f"stream_gain={g} dB is outside the supported range [{STREAM_GAIN_RANGE[0]}, {STREAM_GAIN_RANGE[1]}]")
    return StreamSettings(E.LVS_FIXED, STREAM_LIMITS[limit], linear(g), -23.0, ceiling, opts["boost"], opts["cut"], opts["rise"], opts["fall"])


def stream_options(kwargs):
    """Takes the stream_* leveling keywords out of a streaming call's **kwargs -> None (none given: nothing is built, nothing changes) or the
    validated StreamSettings."""
    v = [kwargs.pop(k, None) for k in STREAM_KEYS]
    if all(x is None for x in v):
        return None
    if v[0] is None and v[1] is None:
        raise ValueError("stream_true_peak=, stream_limit= and stream_level= belong to stream_loudness= or stream_gain=")
    return stream_settings(*v)


@dataclasses.dataclass(frozen=True)
class StreamLevel:
    """A stream's latest reading (stages.StreamLevelStage.read).  lufs: the loudness of the prefix heard so far (-inf while status is 'short'
    or 'silent'); gain_db: where the gain stands; peak_db: true peak (dBTP) of the input emitted so far (-inf without the limiter, which
    alone looks ahead); out_peak_db: SAMPLE peak of the output; limited: emitted samples the limiter pulled down."""
    lufs: float
    gain_db: float
    peak_db: float
    out_peak_db: float
    limited: int
    samples_in: int
    samples_out: int
    status: str = "ok"


def stream_reading(r):
    """A StreamLevelStage.read dict -> StreamLevel."""
    return StreamLevel(r["lufs"], r["gain_db"], db(r["peak"]), db(r["out_peak"]), r["limited"], r["n_in"], r["n_out"], STATUS[r["status"]])
