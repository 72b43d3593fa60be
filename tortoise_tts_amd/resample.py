"""Host side of the resampler (include/tortoise_mi355x_rs.h, csrc/resample.hip, stages.ResampleStage): the options of a tts() call, the
integer ratios of a rate conversion and of a pitch shift, and the integers that carry a position across."""
import math

from . import engine as E

SAMPLE_RATE = 24000                 # what the engine renders
SAMPLE_RATE_RANGE = (8000, 96000)   # sample_rate= of a tts() call
PITCH_RANGE = (-12.0, 12.0)         # pitch= of a tts() call, semitones


def check_ratio(P, Q):
    """(P, Q) as the device takes it: 1 <= P, Q <= 2^20, 1/8 <= P/Q <= 8, reduced unless Q = 65536.  ValueError otherwise."""
    P, Q = int(P), int(Q)
    if not (1 <= P <= E.RS_MAX_TERM and 1 <= Q <= E.RS_MAX_TERM and P <= E.RS_MAX_RATIO * Q and Q <= E.RS_MAX_RATIO * P):
        raise ValueError(f"resampling ratio {P}/{Q}: both terms must lie in 1 .. {E.RS_MAX_TERM} and the ratio in 1/{E.RS_MAX_RATIO} .. {E.RS_MAX_RATIO}")
    if Q != E.RS_PITCH_ONE and math.gcd(P, Q) != 1:
        raise ValueError(f"resampling ratio {P}/{Q} is not reduced")
    return P, Q


def ratio(from_rate, to_rate):
    """Sample rates in Hz (positive integers) -> (P, Q) = from / to reduced by their gcd: input samples per output sample."""
    if int(from_rate) != from_rate or int(to_rate) != to_rate or from_rate < 1 or to_rate < 1:
        raise ValueError(f"sample rates {from_rate!r} -> {to_rate!r}: positive integers (Hz)")
    g = math.gcd(int(from_rate), int(to_rate))
    return check_ratio(int(from_rate) // g, int(to_rate) // g)


def pitch_ratio(semitones):
    """Semitones (+: up) -> (pq, 65536), pq = round(2^(s/12) * 65536): 16.16 fixed point, not reduced."""
    s = float(semitones)
    if not math.isfinite(s):
        raise ValueError(f"pitch={semitones!r} semitones")
    return check_ratio(int(round(2.0 ** (s / 12.0) * E.RS_PITCH_ONE)), E.RS_PITCH_ONE)


def out_samples(n, P, Q):
    """n_out = ceil(n Q / P) (the header's integer)."""
    return -((-int(n) * int(Q)) // int(P))


def map_sample(s, P, Q, n_out):
    """Where input sample s lies in the output: min(n_out, (s Q + P / 2) / P), integer division."""
    return min(int(n_out), (int(s) * int(Q) + int(P) // 2) // int(P))


def stretch_rq(rq, pq):
    """The time-stretch rate that, followed by a resampling at (pq, 65536), leaves a clip at speaking rate rq / 65536 and pitch ratio
    pq / 65536: rq_eff = round(rq * 65536 / pq)."""
    return (int(rq) * E.RS_PITCH_ONE + int(pq) // 2) // int(pq)


def pitch(semitones, rate=None):
    """Validated (pq, rq_eff) of pitch= and speaking_rate= together.  ValueError for a pitch outside +-12 semitones or a combination whose
    time-stretch rate leaves 0.5 .. 2.0; the message names both."""
    s = float(semitones)
    r = 1.0 if rate is None else float(rate)
    if not PITCH_RANGE[0] <= s <= PITCH_RANGE[1]:  # (NaN fails too)
        raise ValueError(f"pitch={s} semitones is outside the supported range [{PITCH_RANGE[0]}, {PITCH_RANGE[1]}] (speaking_rate={r})")
    pq = pitch_ratio(s)[0]
    rq_eff = stretch_rq(int(round(r * E.TSM_RATE_ONE)), pq)
    if not E.TSM_RATE_MIN <= rq_eff <= E.TSM_RATE_MAX:
        raise ValueError(f"pitch={s} semitones with speaking_rate={r} needs a time-stretch at rate {rq_eff / E.TSM_RATE_ONE:.4f}, outside "
                         f"the supported range [0.5, 2.0]")
    return pq, rq_eff


def sample_rate(rate):
    """Validated sample_rate= -> int Hz.  ValueError unless an integer in 8000 .. 96000."""
    if isinstance(rate, bool) or not isinstance(rate, (int,)) and not (isinstance(rate, float) and rate.is_integer()):
        raise ValueError(f"sample_rate={rate!r}: an integer number of Hz in {SAMPLE_RATE_RANGE[0]} .. {SAMPLE_RATE_RANGE[1]}")
    rate = int(rate)
    if not SAMPLE_RATE_RANGE[0] <= rate <= SAMPLE_RATE_RANGE[1]:
        raise ValueError(f"sample_rate={rate} Hz is outside the supported range {SAMPLE_RATE_RANGE[0]} .. {SAMPLE_RATE_RANGE[1]}")
    return rate


def options(kwargs, speaking_rate=None):
    """Takes `pitch` and `sample_rate` out of a tts() call's **kwargs -> (pitch in semitones or None, sample rate in Hz or None).  None:
    absent, None, pitch 0 or 24000 Hz - nothing is built, nothing changes.  The pitch is validated together with `speaking_rate` (what
    stretch.speaking_rate returned): ValueError where the time-stretch they need together leaves its range."""
    s, sr = kwargs.pop("pitch", None), kwargs.pop("sample_rate", None)
    if s is not None:
        pitch(s, speaking_rate)
        s = None if float(s) == 0.0 else float(s)
    if sr is not None:
        sr = sample_rate(sr)
        sr = None if sr == SAMPLE_RATE else sr
    return s, sr


def half_width(P, Q):
    """H of the header: ceil(Z L 65536 / cq), cq = floor(9 L 65536 Qc / (10 Pc)) with (Pc, Qc) = (P, Q) for P > Q, else (1, 1)."""
    num = E.RS_RHO_NUM * E.RS_PER_ZERO * 65536
    cq = num * int(Q) // (E.RS_RHO_DEN * int(P)) if P > Q else num // E.RS_RHO_DEN
    return -((-(E.RS_ZEROS * E.RS_PER_ZERO * 65536)) // cq)


def stream_latency(P, Q):
    """Input samples a streamed output waits for beyond its own position: H + 1 (include/tortoise_mi355x_rss.h)."""
    return half_width(P, Q) + 1


def _ready_total(n, P, Q, flush):
    have = n if flush else n - stream_latency(P, Q)
    return -((-have * int(Q)) // int(P)) if have > 0 else 0


def stream_ready(n_before, n_chunk, P, Q, flush):
    """The Python mirror of tt_rss_ready: the outputs a push of n_chunk samples emits on a stream that holds n_before, given it has
    emitted ready(n_before) = ceil((n_before - H - 1) Q / P) (0 until n_before > H + 1); a flush brings the total to ceil(n Q / P).
    ValueError for what the library answers with -1."""
    n_before, n_chunk = int(n_before), int(n_chunk)
    P, Q = check_ratio(P, Q)
    if n_before < 0 or n_chunk < 0 or n_before + n_chunk > E.RS_MAX_SAMPLES:
        raise ValueError(f"a stream of {n_before} + {n_chunk} samples: non-negative counts, at most {E.RS_MAX_SAMPLES} in all")
    return _ready_total(n_before + n_chunk, P, Q, bool(flush)) - _ready_total(n_before, P, Q, False)


def stream_options(kwargs):
    """Takes `stream_sample_rate` out of a streaming call's **kwargs -> the rate in Hz, or None (absent, None or 24000: nothing is built,
    nothing changes).  ValueError as for sample_rate=."""
    sr = kwargs.pop("stream_sample_rate", None)
    if sr is None:
        return None
    try:
        sr = sample_rate(sr)
    except ValueError as err:
        raise ValueError("stream_" + str(err)) from None
    return None if sr == SAMPLE_RATE else sr


def refuse_streaming(kwargs, who):
    for k in ("pitch", "sample_rate"):
        if k in kwargs:
            raise ValueError(f"{who}: {k} is not available for streamed audio (the resampler filters across the pieces' borders, and they are "
                             f"cross-faded as they are made); use tts() / tts_many(), or shift_pitch() / resample() the collected clip")
