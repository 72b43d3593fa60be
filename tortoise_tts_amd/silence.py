"""Host side of the silence stage (include/tortoise_mi355x_sil.h, csrc/silence.hip, stages.SilenceStage): the options of a tts() call and of
trim() / speech_regions(), their integers, and the integers that carry a position across an edit."""
import math
from collections import namedtuple

from . import engine as E

SAMPLE_RATE = 24000               # what the engine renders
FRAMES_PER_SECOND = 100           # E.SIL_HOP samples each
# Chosen from the code, not from listening: nobody has run a trained checkpoint's audio through them.
DEFAULTS = dict(lead=0.05, trail=0.1, max_pause=None, top_db=40.0, floor_db=-70.0, min_silence=0.1, pad=0.05)
TOP_DB_RANGE = (0.0, 120.0)       # exclusive at 0: a frame is never louder than the loudest
FLOOR_DB_RANGE = (-200.0, 0.0)
MAX_SECONDS = E.SIL_MAX_SAMPLES // SAMPLE_RATE  # lead, trail, max_pause

# what the device takes per clip: thr = (rel, floor_e) f64, par = (min_sil, pad[, lead, trail, max_pause]) i32; -1: leave alone
Params = namedtuple("Params", "rel floor_e min_sil pad lead trail max_pause")


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name}={v!r}: a finite number")
    return float(v)


def _samples(name, v, least=0.0):
    """Seconds -> round(s * 24000) samples; None -> -1 (leave alone)."""
    if v is None:
        return -1
    s = _number(name, v)
    if not least <= s <= MAX_SECONDS:
        raise ValueError(f"{name}={s} s is outside the supported range [{least}, {MAX_SECONDS}]")
    return int(round(s * SAMPLE_RATE))


def _frames(name, v):
    """Seconds -> round(s * 100) frames of 10 ms."""
    s = _number(name, v)
    if not 0.0 <= s * FRAMES_PER_SECOND <= E.SIL_MAX_FRAMES_PARAM:
        raise ValueError(f"{name}={s} s is outside the supported range [0, {E.SIL_MAX_FRAMES_PARAM // FRAMES_PER_SECOND}]")
    return int(round(s * FRAMES_PER_SECOND))


def params(lead=DEFAULTS["lead"], trail=DEFAULTS["trail"], max_pause=DEFAULTS["max_pause"], top_db=DEFAULTS["top_db"],
           floor_db=DEFAULTS["floor_db"], min_silence=DEFAULTS["min_silence"], pad=DEFAULTS["pad"]):
    """The options in seconds and dB, validated -> Params.  lead / trail / max_pause: None leaves that part of the clip alone; max_pause is
    at least the cross-fade (0.005 s).  ValueError names the option."""
    top, flo = _number("top_db", top_db), _number("floor_db", floor_db)
    if not TOP_DB_RANGE[0] < top <= TOP_DB_RANGE[1]:
        raise ValueError(f"top_db={top} dB is outside the supported range ({TOP_DB_RANGE[0]}, {TOP_DB_RANGE[1]}]")
    if not FLOOR_DB_RANGE[0] <= flo <= FLOOR_DB_RANGE[1]:
        raise ValueError(f"floor_db={flo} dB is outside the supported range [{FLOOR_DB_RANGE[0]}, {FLOOR_DB_RANGE[1]}]")
    return Params(10.0 ** (-top / 10.0), E.SIL_FRAME * 10.0 ** (flo / 10.0), _frames("min_silence", min_silence), _frames("pad", pad),
                  _samples("lead", lead), _samples("trail", trail), _samples("max_pause", max_pause, E.SIL_FADE / SAMPLE_RATE))


def from_option(trim_silence, max_pause=None, who="trim_silence"):
    """trim_silence= (True: the defaults; a dict of params()'s options; None or False: off) and max_pause= (seconds; None: off) of a tts()
    call -> Params, or None where both are off.  max_pause= alone caps the pauses and leaves the ends alone; given with trim_silence= it
    takes the place of the dict's own."""
    if trim_silence is None or trim_silence is False:
        if max_pause is None:
            return None
        return params(lead=None, trail=None, max_pause=max_pause)
    if trim_silence is True:
        opts = {}
    elif isinstance(trim_silence, dict):
        opts = dict(trim_silence)
        unknown = sorted(set(opts) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"{who}: unknown options {unknown} (known: {sorted(DEFAULTS)})")
    else:
        raise ValueError(f"{who}={trim_silence!r}: True, False, None or a dict of {sorted(DEFAULTS)}")
    if max_pause is not None:
        opts["max_pause"] = max_pause
    return params(**opts)


def options(kwargs):
    """Takes `trim_silence` and `max_pause` out of a tts() call's **kwargs -> Params or None (neither given: nothing is built, nothing
    changes)."""
    return from_option(kwargs.pop("trim_silence", None), kwargs.pop("max_pause", None))


def for_long_form(kwargs, pause):
    """read_long_form(pause=seconds): the chunks' calls cut both ends to the speech (lead = trail = 0) and keep their own trim_silence= /
    max_pause= for the inside -> the number of zero samples between two chunks.  Rewrites kwargs['trim_silence'] in place."""
    gap = _samples("pause", pause)
    if gap < 0:
        raise ValueError("pause=None leaves the chunks as they are: do not call for_long_form")
    ts = kwargs.get("trim_silence")
    opts = dict(ts) if isinstance(ts, dict) else {}
    if ts is not None and ts is not True and ts is not False and not isinstance(ts, dict):
        raise ValueError(f"trim_silence={ts!r}: True, False, None or a dict of {sorted(DEFAULTS)}")
    opts["lead"], opts["trail"] = 0.0, 0.0  # (the dict's other options, or the defaults: max_pause= of the call still applies)
    from_option(opts, kwargs.get("max_pause"))  # (refused here, before anything renders)
    kwargs["trim_silence"] = opts
    return gap


def refuse_streaming(kwargs, who):
    for k in ("trim_silence", "max_pause"):
        if k in kwargs:
            raise ValueError(f"{who}: {k} is not available for streamed audio (a pause is known only once the speech after it has been "
                             f"made, and the pieces are cross-faded as they are made); use tts() / tts_many(), or trim() the collected clip")


def frames(n):
    return -(-int(n) // E.SIL_HOP)


def max_regions(n):
    return (frames(n) + 1) // 2


def map_sample(s, segments):
    """Where input sample s lies in the output of an edit with the segment list [(o_k, i_k, l_k)] (the header's `map`): a sample that was
    cut away lands on the cut."""
    s = int(s)
    k = 0
    for j, (_, i, _) in enumerate(segments):
        if int(i) <= s:
            k = j
    o, i, l = (int(v) for v in segments[k])
    return min(o + l, o + max(0, s - i))


def pauses(regions, n):
    """Speech regions [(a, b)] of a clip of n samples -> the pauses between them [(b_r, a_(r+1))] (the silence at the two ends is
    (0, a_0) and (b_last, n), not listed)."""
    return [(int(regions[r][1]), int(regions[r + 1][0])) for r in range(len(regions) - 1)]


STATUS = {E.SIL_OK: "ok", E.SIL_UNCHANGED: "unchanged", E.SIL_SILENT: "silent", E.SIL_EMPTY: "empty", E.SIL_REFUSED: "refused"}
