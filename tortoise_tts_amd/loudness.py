"""Host side of the loudness normalisation (include/tortoise_mi355x_loud.h, csrc/loudness.hip, stages.LoudnessStage): the options of a
tts() call, dB <-> linear, and the per-clip result."""
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
