"""Host side of the speaking-rate control (include/tortoise_mi355x_tsm.h, csrc/tsm.hip, stages.TimeStretchStage): the fixed-point rate, and
the anchors that carry a position in the original clip over to the stretched one."""
import torch

from . import engine as E

RATE_RANGE = (E.TSM_RATE_MIN / E.TSM_RATE_ONE, E.TSM_RATE_MAX / E.TSM_RATE_ONE)  # 0.5 .. 2.0


def rate_q(rate):
    """A speaking rate (2.0: twice as fast, half as long) -> rq = round(rate * 65536).  ValueError outside [0.5, 2.0]."""
    rate = float(rate)
    if not RATE_RANGE[0] <= rate <= RATE_RANGE[1]:  # (NaN fails too)
        raise ValueError(f"speaking rate {rate} is outside the supported range [{RATE_RANGE[0]}, {RATE_RANGE[1]}]")
    return int(round(rate * E.TSM_RATE_ONE))


def rate_for_duration(n, duration):
    """The rate that makes a clip of n samples last `duration` seconds."""
    duration = float(duration)
    if not duration > 0:
        raise ValueError(f"duration={duration} must be positive (seconds)")
    return n / (duration * E.TSM_SAMPLE_RATE)


def speaking_rate(kwargs):
    """Takes `speaking_rate` out of a tts() call's **kwargs -> None (absent, None or exactly 1.0: nothing is stretched) or the validated rate."""
    rate = kwargs.pop("speaking_rate", None)
    if rate is None or float(rate) == 1.0:
        return None
    rate_q(rate)
    return float(rate)


def refuse_streaming(kwargs, who):
    if "speaking_rate" in kwargs:
        raise ValueError(f"{who}: speaking_rate is not available for streamed audio (the pieces are cross-faded as they are made); "
                         f"use tts() / tts_many(), or stretch() the collected clip")


def nominal(k, rq):
    """a_k, the nominal analysis position of frame k >= 1 (the header's integer)."""
    return ((k - 1) * E.TSM_HOP * rq + 32768) >> 16


def anchors(rq, offsets):
    """The chosen offsets of a clip's frames -> int64 [K, 2]: (output sample (k - 1) Hs, input sample p_k) of every frame.  The output around
    an anchor is the input around its partner; a time taken before the stretch is carried across by interpolating between anchors."""
    rows = [(-E.TSM_HOP, -E.TSM_HOP)] + [((k - 1) * E.TSM_HOP, nominal(k, rq) + int(offsets[k])) for k in range(1, len(offsets))]
    return torch.tensor(rows, dtype=torch.int64)
