"""Host side of the speaking-rate control (include/tortoise_mi355x_tsm.h, csrc/tsm.hip, stages.TimeStretchStage): the fixed-point rate, and
the anchors that carry a position in the original clip over to the stretched one; and of its streaming form
(include/tortoise_mi355x_tss.h, csrc/tsm_stream.hip, stages.StreamStretchStage): the frames done and the outputs ready, and the options of a
streaming call; and of a speaking rate that changes inside the clip (include/tortoise_mi355x_tsw.h, csrc/tsm_warp.hip,
stages.WarpStretchStage): the table of segments, its plan from segments, anchors or word timings (RateMap), and its anchors."""
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


# ----------------------------------------------------------------------------------------- a speaking rate that changes inside the clip
# include/tortoise_mi355x_tsw.h, csrc/tsm_warp.hip, stages.WarpStretchStage.  A table is a list of segments (m_i, a_i, rq_i): from output
# sample m_i on, where the input stands at sample a_i, the clip runs at rate rq_i.  Everything here is integers that host and device
# agree on; the functions mirror the library's (csrc/tsm_warp_host.h).
def _advance(length, rq):
    return (length * rq + 32768) >> 16


def table_out_samples(n, table):
    """The Python mirror of tt_tsw_out_samples: n_out of a clip of n samples along `table`, 0 for a table that breaks a rule ((0, 0) start,
    m strictly increasing, rates in range, continuity, a_(S-1) < n)."""
    n, S = int(n), len(table)
    if n < 1 or n > E.TSM_MAX_SAMPLES or S < 1 or S > E.TSW_MAX_SEGMENTS:
        return 0
    if table[0][0] != 0 or table[0][1] != 0:
        return 0
    for i, (m, a, rq) in enumerate(table):
        if not E.TSM_RATE_MIN <= rq <= E.TSM_RATE_MAX:
            return 0
        if i + 1 < S and (table[i + 1][0] <= m or a + _advance(table[i + 1][0] - m, rq) != table[i + 1][1]):
            return 0
    m, a, rq = table[-1]
    if a >= n:
        return 0
    return m + max(1, ((n - a) * E.TSM_RATE_ONE + rq // 2) // rq)


def table_frames(n, table):
    """The Python mirror of tt_tsw_frames: K = ceil(n_out / Hs) + 1, 0 for a table that breaks a rule."""
    n_out = table_out_samples(n, table)
    return -(-n_out // E.TSM_HOP) + 1 if n_out else 0


def table_nominal(k, table):
    """a_k of frame k >= 1 along `table`: a_i + ((((k - 1) Hs - m_i) rq_i + 32768) >> 16), i the last segment with m_i <= (k - 1) Hs."""
    m = (k - 1) * E.TSM_HOP
    i = 0
    while i + 1 < len(table) and table[i + 1][0] <= m:
        i += 1
    return table[i][1] + _advance(m - table[i][0], table[i][2])


def plan(n, starts, rqs):
    """The Python mirror of tt_tsw_plan: input-domain segments (b_i, rq_i), b_0 = 0 < b_1 < .. < b_S = n, each of at least 2 samples ->
    the table.  Every length is measured from the achieved a_i: |a_i - b_i| <= 1.  ValueError for what the library answers with -1."""
    n, S = int(n), len(starts)
    if len(rqs) != S:
        raise ValueError(f"rate map: {S} segment starts with {len(rqs)} rates")
    if n < 1 or n > E.TSM_MAX_SAMPLES:
        raise ValueError(f"rate map: a clip of {n} samples (1 .. {E.TSM_MAX_SAMPLES})")
    if S < 1 or S > E.TSW_MAX_SEGMENTS:
        raise ValueError(f"rate map: {S} segments (1 .. {E.TSW_MAX_SEGMENTS})")
    starts, rqs = [int(b) for b in starts], [int(r) for r in rqs]
    if starts[0] != 0:
        raise ValueError(f"rate map: segment 0 starts at sample {starts[0]}, not at 0")
    for i in range(S):
        end = starts[i + 1] if i + 1 < S else n
        if end - starts[i] < E.TSW_MIN_SEGMENT:
            raise ValueError(f"rate map: segment {i} starts at sample {starts[i]} and ends at {end}: the starts increase, and a segment covers "
                             f"at least {E.TSW_MIN_SEGMENT} samples")
        if not E.TSM_RATE_MIN <= rqs[i] <= E.TSM_RATE_MAX:
            raise ValueError(f"rate map: segment {i}: rate {rqs[i]} / 65536 is outside the supported range [0.5, 2.0]")
    table, m, a = [], 0, 0
    for i in range(S):
        table.append((m, a, rqs[i]))
        if i + 1 < S:
            L = max(1, ((starts[i + 1] - a) * E.TSM_RATE_ONE + rqs[i] // 2) // rqs[i])
            m, a = m + L, a + _advance(L, rqs[i])
    return table


def table_anchors(table, offsets):
    """stretch.anchors along a table: the chosen offsets of a clip's frames -> int64 [K, 2]: (output sample (k - 1) Hs, input sample
    a_k + d_k) of every frame."""
    rows = [(-E.TSM_HOP, -E.TSM_HOP)] + [((k - 1) * E.TSM_HOP, table_nominal(k, table) + int(offsets[k])) for k in range(1, len(offsets))]
    return torch.tensor(rows, dtype=torch.int64)


class RateMap:
    """The speaking rate of a clip of n samples (24 kHz) as it changes inside the clip: input-domain segments (start sample b_i, rate rq_i),
    and the integer table planned from them.  .table [(m_i, a_i, rq_i)], .n_out, .frames are what the device computes with; .starts and
    .rqs what they were planned from.  Build one with from_segments, from_anchors or from_words."""

    def __init__(self, n, starts, rqs):
        self.n, self.starts, self.rqs = int(n), [int(b) for b in starts], [int(r) for r in rqs]
        self.table = plan(self.n, self.starts, self.rqs)
        self.n_out = table_out_samples(self.n, self.table)
        self.frames = table_frames(self.n, self.table)
        assert self.n_out > 0, "a planned table obeys the table's rules"

    def __repr__(self):
        return f"RateMap(n={self.n}, n_out={self.n_out}, segments={[(b, rq / E.TSM_RATE_ONE) for b, rq in zip(self.starts, self.rqs)]})"

    @classmethod
    def from_segments(cls, n, segments):
        """[(start_sample, rate), ...]: from start_sample on (the first one 0) the clip runs at `rate` (0.5 .. 2.0), up to the next start or
        the clip's end.  ValueError names the segment for a rate outside the range, starts that do not increase, a segment under 2 samples
        and more than 64 segments."""
        segments = list(segments)
        rqs = []
        for i, (_, rate) in enumerate(segments):
            try:
                rqs.append(rate_q(rate))
            except (ValueError, TypeError):
                raise ValueError(f"rate map: segment {i}: speaking rate {rate!r} is outside the supported range [{RATE_RANGE[0]}, {RATE_RANGE[1]}]") from None
        return cls(n, [int(b) for b, _ in segments], rqs)

    @classmethod
    def from_anchors(cls, n, anchors):
        """[(src_sample, dst_sample), ...]: input sample src_i is to sound at output sample dst_i; both increase, (0, 0) is implied.  Between
        two anchors the rate is rq_i = round((src_(i+1) - a_i) 65536 / (dst_(i+1) - m_i)), measured from what the plan achieved so far, so
        |m_(i+1) - dst_(i+1)| <= (dst_(i+1) - m_i) / 65536 + 1.  An anchor at src >= n sets the clip's end; behind a last anchor inside
        the clip the rest runs at rate 1.0.  ValueError names the pair whose rate leaves [0.5, 2.0]."""
        n = int(n)
        pts = [(int(s_), int(d)) for s_, d in anchors]
        if pts and pts[0] == (0, 0):
            pts = pts[1:]
        if not pts:
            raise ValueError("rate map: no anchors beyond (0, 0)")
        starts, rqs, m, a = [], [], 0, 0
        prev = (0, 0)
        for j, (src, dst) in enumerate(pts):
            if src <= prev[0] or dst <= prev[1]:
                raise ValueError(f"rate map: anchor ({src}, {dst}) after ({prev[0]}, {prev[1]}): input and output samples both increase")
            if src > n:
                raise ValueError(f"rate map: anchor ({src}, {dst}) lies beyond the clip's {n} samples")
            if src - a < 1 or dst - m < 1:
                raise ValueError(f"rate map: anchors ({prev[0]}, {prev[1]}) -> ({src}, {dst}): too close to place")
            rq = ((src - a) * E.TSM_RATE_ONE * 2 + (dst - m)) // (2 * (dst - m))
            if not E.TSM_RATE_MIN <= rq <= E.TSM_RATE_MAX:
                raise ValueError(f"rate map: anchors ({prev[0]}, {prev[1]}) -> ({src}, {dst}) need rate {rq / E.TSM_RATE_ONE:.4f}, outside the "
                                 f"supported range [{RATE_RANGE[0]}, {RATE_RANGE[1]}]")
            starts.append(prev[0])
            rqs.append(rq)
            if src < n:  # the plan's own step: the next segment starts where this one got to
                L = max(1, ((src - a) * E.TSM_RATE_ONE + rq // 2) // rq)
                m, a = m + L, a + _advance(L, rq)
            elif j + 1 < len(pts):
                raise ValueError(f"rate map: anchor ({pts[j + 1][0]}, {pts[j + 1][1]}) follows the clip's end ({src}, {dst})")
            prev = (src, dst)
        if prev[0] < n:
            starts.append(prev[0])
            rqs.append(E.TSM_RATE_ONE)
        return cls(n, starts, rqs)

    @classmethod
    def from_words(cls, alignment, rates, base=1.0):
        """One rate per word of an align.Alignment (24 kHz): `rates` is a list with one entry per word (None: the base) or a dict
        {word index: rate}.  A word's span is its start to its end; everything else - the pauses, the words without a rate - runs at
        `base`.  A span or a gap under 2 samples owns no segment (it joins the one before it), neighbours at the same rate are one
        segment."""
        words = alignment.words
        if getattr(alignment, "rate", E.TSM_SAMPLE_RATE) != E.TSM_SAMPLE_RATE:
            raise ValueError(f"word_rates: the alignment counts samples at {alignment.rate} Hz; the time-stretch runs at {E.TSM_SAMPLE_RATE}")
        if isinstance(rates, dict):
            for i in rates:
                if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(words):
                    raise ValueError(f"word_rates: word index {i!r} (the text has {len(words)} words: 0 .. {len(words) - 1})")
            per = [rates.get(i) for i in range(len(words))]
        else:
            per = list(rates)
            if len(per) != len(words):
                raise ValueError(f"word_rates: {len(per)} rates for the {len(words)} words of the text")
        rate_q(base)
        raw, at = [(0, float(base))], 0
        for i, ((w, a, b, _), r) in enumerate(zip(words, per)):
            if r is None:
                continue
            try:
                rate_q(r)
            except (ValueError, TypeError):
                raise ValueError(f"word_rates: word {i} ({w!r}): speaking rate {r!r} is outside the supported range [{RATE_RANGE[0]}, {RATE_RANGE[1]}]") from None
            a = max(int(a), at)
            if int(b) - a < E.TSW_MIN_SEGMENT:
                continue
            raw += [(a, float(r)), (int(b), float(base))]
            at = int(b)
        segs = []
        for j, (s_, r) in enumerate(raw):
            end = raw[j + 1][0] if j + 1 < len(raw) else alignment.samples
            if end - s_ < E.TSW_MIN_SEGMENT or (segs and segs[-1][1] == r):
                continue
            segs.append((s_ if segs else 0, r))
        return cls.from_segments(alignment.samples, segs or [(0, float(base))])

    def with_pitch(self, pq):
        """The map of the time-stretch that, followed by a resampling at (pq, 65536), leaves these speaking rates at pitch ratio pq / 65536:
        every segment at round(rq_i 65536 / pq).  ValueError names the segment whose rate leaves [0.5, 2.0]."""
        rqs = [rs.stretch_rq(rq, pq) for rq in self.rqs]
        for i, (rq, eff) in enumerate(zip(self.rqs, rqs)):
            if not E.TSM_RATE_MIN <= eff <= E.TSM_RATE_MAX:
                raise ValueError(f"rate map: segment {i} (speaking rate {rq / E.TSM_RATE_ONE:.4f}) at pitch ratio {pq / E.RS_PITCH_ONE:.4f} needs a "
                                 f"time-stretch at rate {eff / E.TSM_RATE_ONE:.4f}, outside the supported range [0.5, 2.0]")
        return RateMap(self.n, self.starts, rqs)

    def anchors(self, offsets):
        """table_anchors of this map's table."""
        return table_anchors(self.table, offsets)


def rate_map(n, given):
    """What stretch(rate_map=) takes -> a RateMap of a clip of n samples: a RateMap (its n must be the clip's), or a list of
    (start_seconds, rate)."""
    if isinstance(given, RateMap):
        if given.n != int(n):
            raise ValueError(f"stretch: the rate map was made for a clip of {given.n} samples, this one has {int(n)}")
        return given
    try:
        segs = [(int(round(float(t) * E.TSM_SAMPLE_RATE)), r) for t, r in given]
    except (TypeError, ValueError):
        raise ValueError(f"stretch: rate_map={given!r}: a RateMap, or a list of (start_seconds, rate)") from None
    return RateMap.from_segments(n, segs)


def word_rates(kwargs):
    """Takes `word_rates` out of a tts_with_timings call's **kwargs -> None (absent or None) or the list / dict."""
    given = kwargs.pop("word_rates", None)
    if given is not None and not isinstance(given, (list, tuple, dict)):
        raise ValueError(f"word_rates={given!r}: a list with one rate per word (None: the base rate), or a dict {{word index: rate}}")
    return given


def refuse_word_rates(kwargs, who):
    if "word_rates" in kwargs:
        raise ValueError(f"{who}: word_rates is not available here (it needs the finished clip and its word timings); use tts_with_timings()")
