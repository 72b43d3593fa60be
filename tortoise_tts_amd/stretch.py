"""Host side of the speaking-rate control (include/tortoise_mi355x_tsm.h, csrc/tsm.hip, stages.TimeStretchStage): the fixed-point rate, and
the anchors that carry a position in the original clip over to the stretched one; and of its streaming form
(include/tortoise_mi355x_tss.h, csrc/tsm_stream.hip, stages.StreamStretchStage): the frames done and the outputs ready, and the options of a
streaming call."""
import torch

from . import engine as E
from . import resample as rs

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


def stream_latency():
    """Input samples a streamed output waits for beyond the start of its hop's frame: 2 S - 1 + Hs + W - S = 1407 (58.6 ms)."""
    return E.TSM_SEARCH - 1 + E.TSM_HOP + E.TSM_WINDOW


def _stream_counts(n_before, n_chunk, rq):
    n_before, n_chunk, rq = int(n_before), int(n_chunk), int(rq)
    if not E.TSM_RATE_MIN <= rq <= E.TSM_RATE_MAX:
        raise ValueError(f"rate {rq} / 65536 is outside the supported range [0.5, 2.0]")
    if n_before < 0 or n_chunk < 0 or n_before + n_chunk > E.TSM_MAX_SAMPLES:
        raise ValueError(f"a stream of {n_before} + {n_chunk} samples: non-negative counts, at most {E.TSM_MAX_SAMPLES} in all")
    return n_before, n_chunk, rq


def stream_frames_done(n, rq):
    """The Python mirror of tt_tss_frames_done: the frames 1 .. done are complete once n samples are in, the k with a_k + 1407 <= n.
    ValueError for what the library answers with -1."""
    n, _, rq = _stream_counts(n, 0, rq)
    look = stream_latency()
    if n < look:
        return 0
    return (((n - look + 1) << 16) - 32768 - 1) // (E.TSM_HOP * rq) + 1


def stream_frames_total(n, rq, flush):
    """The frames that have run after a push that brought the total to n: done(n), or all K - 1 of the clip once it is flushed."""
    if not flush:
        return stream_frames_done(n, rq)
    n, _, rq = _stream_counts(n, 0, rq)
    return -(-max(1, (n * E.TSM_RATE_ONE + rq // 2) // rq) // E.TSM_HOP) if n >= 1 else 0


def _ready_total(n, rq, flush):
    if not flush:
        return stream_frames_done(n, rq) * E.TSM_HOP
    return max(1, (n * E.TSM_RATE_ONE + rq // 2) // rq) if n >= 1 else 0


def stream_ready(n_before, n_chunk, rq, flush):
    """The Python mirror of tt_tss_ready: the outputs a push of n_chunk samples emits on a stream that holds n_before, given it has emitted
    done(n_before) Hs; a flush brings the total to n_out (0 for a stream of no samples).  ValueError for what the library answers with -1."""
    n_before, n_chunk, rq = _stream_counts(n_before, n_chunk, rq)
    return _ready_total(n_before + n_chunk, rq, bool(flush)) - _ready_total(n_before, rq, False)


def stream_offsets(n_before, n_chunk, rq, flush):
    """The chosen offsets a push emits: one per frame it runs, and d_0 = 0 in front of frame 1's."""
    n_before, n_chunk, rq = _stream_counts(n_before, n_chunk, rq)
    k0, k1 = stream_frames_done(n_before, rq) + 1, stream_frames_total(n_before + n_chunk, rq, flush)
    return k1 - k0 + 1 + (k0 == 1) if k1 >= k0 else 0


def stream_options(kwargs):
    """Takes `stream_speaking_rate` and `stream_pitch` out of a streaming call's **kwargs -> (rq_eff, pq): the time-stretch rate and the
    resampling ratio (pq, 65536) behind it, or None (both absent, None, 1.0 / 0: nothing is built, nothing changes).  Validated as
    speaking_rate= and pitch= of tts() are (rate_q, resample.pitch); the messages name the streaming keywords."""
    rate, s = kwargs.pop("stream_speaking_rate", None), kwargs.pop("stream_pitch", None)
    try:
        if rate is not None:
            if isinstance(rate, (bool, str)):
                raise ValueError(f"speaking_rate={rate!r}: a number in [{RATE_RANGE[0]}, {RATE_RANGE[1]}]")
            rate_q(rate)
            rate = None if float(rate) == 1.0 else float(rate)
        if s is not None:
            if isinstance(s, (bool, str)):
                raise ValueError(f"pitch={s!r}: semitones in [{rs.PITCH_RANGE[0]}, {rs.PITCH_RANGE[1]}]")
            rs.pitch(s, rate)
            s = None if float(s) == 0.0 else float(s)
    except ValueError as err:
        raise ValueError("stream_" + str(err).replace("speaking rate ", "speaking_rate=", 1).replace("with speaking_rate=", "with stream_speaking_rate=")
                         .replace("(speaking_rate=", "(stream_speaking_rate=")) from None
    if rate is None and s is None:
        return None
    pq, rq_eff = rs.pitch(0.0 if s is None else s, rate)
    return rq_eff, pq
