"""Host side of the resampler (include/tortoise_mi355x_rs.h, csrc/resample.hip, stages.ResampleStage): the options of a tts() call, the
integer ratios of a rate conversion and of a pitch shift, and the integers that carry a position across; and of a pitch that changes
inside the clip (include/tortoise_mi355x_rsw.h, csrc/resample_warp.hip, stages.WarpResampleStage): the table of segments, its plan from
segments or word timings (PitchMap), and the chain that keeps every word's duration (warp_chain)."""
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


# ----------------------------------------------------------------------------------------------- a pitch that changes inside the clip
# include/tortoise_mi355x_rsw.h, csrc/resample_warp.hip, stages.WarpResampleStage.  A table is a list of segments (m_i, thi_i, tlo_i, P_i):
# from output sample m_i on, where the input stands at t_i = thi_i 65536 + tlo_i (1 / 65536 sample), the clip is read at P_i / 65536 input
# samples per output sample.  Everything here is integers that host and device agree on; the functions mirror the library's
# (csrc/resample_warp_host.h).
MIN_WORD_SPAN = 4  # samples a word's span or a gap needs to own a segment of a PitchMap.from_words; derived there


def map_out_samples(n, table):
    """The Python mirror of tt_rsw_out_samples: n_out of a clip of n samples along `table`, 0 for a table that breaks a rule ((0, 0) start,
    0 <= tlo < 65536, m strictly increasing, ratios in range, continuity, t_(S-1) < n 65536)."""
    n, S = int(n), len(table)
    if n < 1 or n > E.RS_MAX_SAMPLES or S < 1 or S > E.RSW_MAX_SEGMENTS:
        return 0
    if tuple(table[0][:3]) != (0, 0, 0):
        return 0
    for i, (m, hi, lo, P) in enumerate(table):
        if not E.RSW_P_MIN <= P <= E.RSW_P_MAX or hi < 0 or not 0 <= lo <= 65535:
            return 0
        if i + 1 < S:
            m1, hi1, lo1, _ = table[i + 1]
            if m1 <= m or hi * 65536 + lo + (m1 - m) * P != hi1 * 65536 + lo1:
                return 0
    m, hi, lo, P = table[-1]
    t = hi * 65536 + lo
    if t >= n * 65536:
        return 0
    return m + -((t - n * 65536) // P)


def map_position(m, table):
    """(input index, phase) of output sample m along `table`: pos = t_i + (m - m_i) P_i, i the last segment with m_i <= m -> (pos >> 16,
    pos & 65535)."""
    i = 0
    while i + 1 < len(table) and table[i + 1][0] <= m:
        i += 1
    pos = table[i][1] * 65536 + table[i][2] + (m - table[i][0]) * table[i][3]
    return pos >> 16, pos & 65535


def map_plan(n, starts, pqs):
    """The Python mirror of tt_rsw_plan: input-domain segments (b_i, P_i), b_0 = 0 < b_1 < .. < b_S = n, each of at least 2 samples -> the
    table.  Every length is measured from the achieved t_i: 0 <= t_i - 65536 b_i < P_(i-1).  ValueError for what the library answers
    with -1."""
    n, S = int(n), len(starts)
    if len(pqs) != S:
        raise ValueError(f"pitch map: {S} segment starts with {len(pqs)} ratios")
    if n < 1 or n > E.RS_MAX_SAMPLES:
        raise ValueError(f"pitch map: a clip of {n} samples (1 .. {E.RS_MAX_SAMPLES})")
    if S < 1 or S > E.RSW_MAX_SEGMENTS:
        raise ValueError(f"pitch map: {S} segments (1 .. {E.RSW_MAX_SEGMENTS})")
    starts, pqs = [int(b) for b in starts], [int(p) for p in pqs]
    if starts[0] != 0:
        raise ValueError(f"pitch map: segment 0 starts at sample {starts[0]}, not at 0")
    for i in range(S):
        end = starts[i + 1] if i + 1 < S else n
        if end - starts[i] < E.RSW_MIN_SEGMENT:
            raise ValueError(f"pitch map: segment {i} starts at sample {starts[i]} and ends at {end}: the starts increase, and a segment covers "
                             f"at least {E.RSW_MIN_SEGMENT} samples")
        if not E.RSW_P_MIN <= pqs[i] <= E.RSW_P_MAX:
            raise ValueError(f"pitch map: segment {i}: ratio {pqs[i]} / 65536 is outside the supported range [0.5, 2.0] (+-12 semitones)")
    table, m, t = [], 0, 0
    for i in range(S):
        table.append((m, t >> 16, t & 65535, pqs[i]))
        if i + 1 < S:
            L = max(1, -((t - starts[i + 1] * 65536) // pqs[i]))
            m, t = m + L, t + L * pqs[i]
    return table


def _semitones_q(s, what):
    try:
        s = float(s)
        ok = PITCH_RANGE[0] <= s <= PITCH_RANGE[1]  # (NaN fails too)
    except (TypeError, ValueError):
        ok = False
    if not ok or isinstance(s, bool):
        raise ValueError(f"{what}: pitch {s!r} semitones is outside the supported range [{PITCH_RANGE[0]}, {PITCH_RANGE[1]}]")
    return pitch_ratio(s)[0]


class PitchMap:
    """The pitch of a clip of n samples (24 kHz) as it changes inside the clip: input-domain segments (start sample b_i, ratio pq_i =
    round(2^(s_i / 12) 65536)), and the integer table planned from them.  .table [(m_i, thi_i, tlo_i, P_i)] and .n_out are what the device
    computes with when THIS clip is resampled along the map (which changes every segment's duration by 65536 / pq_i); .starts and .pqs
    what they were planned from.  shift_pitch(pitch_map=) keeps the durations: it plans a time-stretch and a resampling from .starts and
    .pqs (warp_chain).  Build one with from_segments or from_words."""

    def __init__(self, n, starts, pqs):
        self.n, self.starts, self.pqs = int(n), [int(b) for b in starts], [int(p) for p in pqs]
        self.table = map_plan(self.n, self.starts, self.pqs)
        self.n_out = map_out_samples(self.n, self.table)
        assert self.n_out > 0, "a planned table obeys the table's rules"

    def __repr__(self):
        return f"PitchMap(n={self.n}, segments={[(b, round(12 * math.log2(p / E.RS_PITCH_ONE), 3)) for b, p in zip(self.starts, self.pqs)]})"

    @classmethod
    def from_segments(cls, n, segments):
        """[(start_sample, semitones), ...]: from start_sample on (the first one 0) the clip sounds `semitones` higher (+-12), up to the next
        start or the clip's end.  ValueError names the segment for a pitch outside the range, starts that do not increase, a segment under
        2 samples and more than 64 segments."""
        segments = list(segments)
        pqs = [_semitones_q(s, f"pitch map: segment {i}") for i, (_, s) in enumerate(segments)]
        return cls(n, [int(b) for b, _ in segments], pqs)

    @classmethod
    def from_words(cls, alignment, semitones, base=0.0):
        """One pitch per word of an align.Alignment (24 kHz): `semitones` is a list with one entry per word (None: the base) or a dict
        {word index: semitones}.  A word's span is its start to its end; everything else - the pauses, the words without a pitch - sounds
        at `base`.  Neighbours at the same pitch are one segment.  The rules are RateMap.from_words' with one difference: a span or a gap
        under MIN_WORD_SPAN = 4 samples owns no segment (it joins the one before it).  Why 4: the map's segments are first time-stretched,
        at a rate of up to 2.0 (65536 / pq for a pitch alone, rq / pq with word_rates, both held to [0.5, 2.0]), and the resampler's plan
        needs 2 samples of every STRETCHED segment.  The stretch's plan measures a segment from the position it achieved, within one
        sample of the border (|a_i - b_i| <= 1), so a span of 4 counts as at least 3 there and comes out as
        (3 * 65536 + 131072 / 2) / 131072 = 2 samples at rate 2.0; a span of 3 could come out as 1."""
        words = alignment.words
        if getattr(alignment, "rate", SAMPLE_RATE) != SAMPLE_RATE:
            raise ValueError(f"word_pitches: the alignment counts samples at {alignment.rate} Hz; the pitch map runs at {SAMPLE_RATE}")
        if isinstance(semitones, dict):
            for i in semitones:
                if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(words):
                    raise ValueError(f"word_pitches: word index {i!r} (the text has {len(words)} words: 0 .. {len(words) - 1})")
            per = [semitones.get(i) for i in range(len(words))]
        else:
            per = list(semitones)
            if len(per) != len(words):
                raise ValueError(f"word_pitches: {len(per)} pitches for the {len(words)} words of the text")
        base_q = _semitones_q(base, "word_pitches: the base")
        raw, at = [(0, base_q)], 0
        for i, ((w, a, b, _), s) in enumerate(zip(words, per)):
            if s is None:
                continue
            q = _semitones_q(s, f"word_pitches: word {i} ({w!r})")
            a = max(int(a), at)
            if int(b) - a < MIN_WORD_SPAN:
                continue
            raw += [(a, q), (int(b), base_q)]
            at = int(b)
        segs = []
        for j, (s_, q) in enumerate(raw):
            end = raw[j + 1][0] if j + 1 < len(raw) else alignment.samples
            if end - s_ < MIN_WORD_SPAN or (segs and segs[-1][1] == q):
                continue
            segs.append((s_ if segs else 0, q))
        segs = segs or [(0, base_q)]
        return cls(alignment.samples, [b for b, _ in segs], [q for _, q in segs])


def pitch_map(n, given):
    """What shift_pitch(pitch_map=) takes -> a PitchMap of a clip of n samples: a PitchMap (its n must be the clip's), or a list of
    (start_seconds, semitones)."""
    if isinstance(given, PitchMap):
        if given.n != int(n):
            raise ValueError(f"shift_pitch: the pitch map was made for a clip of {given.n} samples, this one has {int(n)}")
        return given
    try:
        segs = [(int(round(float(t) * SAMPLE_RATE)), s) for t, s in given]
    except (TypeError, ValueError):
        raise ValueError(f"shift_pitch: pitch_map={given!r}: a PitchMap, or a list of (start_seconds, semitones)") from None
    return PitchMap.from_segments(n, segs)


def word_pitches(kwargs):
    """Takes `word_pitches` out of a tts_with_timings call's **kwargs -> None (absent or None) or the list / dict."""
    given = kwargs.pop("word_pitches", None)
    if given is not None and not isinstance(given, (list, tuple, dict)):
        raise ValueError(f"word_pitches={given!r}: a list with one pitch in semitones per word (None: the base pitch), or a dict "
                         f"{{word index: semitones}}")
    return given


def refuse_word_pitches(kwargs, who):
    if "word_pitches" in kwargs:
        raise ValueError(f"{who}: word_pitches is not available here (it needs the finished clip and its word timings); use tts_with_timings()")


def refuse_formants(formants, formant_shift, who):
    if formants not in (None, "follow") or formant_shift is not None:
        raise ValueError(f"{who}: formants='keep' / formant_shift= do not go with a pitch that changes inside the clip (the formant stage takes "
                         f"one warp per clip; a warp per segment is not built)")


def merge_maps(n, rate_segments, pitch_segments, name=lambda i, b: f"segment {i}"):
    """Segments over the union of the borders of a rate map and a pitch map of the same clip of n samples: rate_segments [(b, rq)] and
    pitch_segments [(b, pq)], both starting at 0 -> (starts, rqs, pqs), neighbours with the same (rq, pq) joined.  Where the two maps'
    borders leave a piece under MIN_WORD_SPAN samples between them, it owns no segment and joins the one before it (from_words' rule).
    ValueError for more than 64 segments in all and, naming the segment through name(its index, its start sample), for a combination
    whose time-stretch rate stretch_rq(rq_i, pq_i) leaves [0.5, 2.0]."""
    cuts = sorted({int(b) for b, _ in rate_segments} | {int(b) for b, _ in pitch_segments})
    at = lambda segs, b: [v for s_, v in segs if int(s_) <= b][-1]
    merged = []
    for b in cuts:
        rq, pq = int(at(rate_segments, b)), int(at(pitch_segments, b))
        if int(n) - b < MIN_WORD_SPAN and merged:
            continue
        if merged and b - merged[-1][0] < MIN_WORD_SPAN:  # the piece before this border is too short to own a segment
            if len(merged) == 1:
                continue
            merged.pop()
        if merged and merged[-1][1:] == (rq, pq):
            continue
        merged.append((b, rq, pq))
    if len(merged) > E.RSW_MAX_SEGMENTS:
        raise ValueError(f"word_rates and word_pitches together make {len(merged)} segments over the union of their word borders; "
                         f"at most {E.RSW_MAX_SEGMENTS} fit one clip")
    for i, (b, rq, pq) in enumerate(merged):
        eff = stretch_rq(rq, pq)
        if not E.TSM_RATE_MIN <= eff <= E.TSM_RATE_MAX:
            raise ValueError(f"{name(i, b)}: speaking rate {rq / E.TSM_RATE_ONE:.4f} at pitch ratio {pq / E.RS_PITCH_ONE:.4f} needs a "
                             f"time-stretch at rate {eff / E.TSM_RATE_ONE:.4f}, outside the supported range [0.5, 2.0]")
    return [b for b, _, _ in merged], [rq for _, rq, _ in merged], [pq for _, _, pq in merged]


class WarpChain:
    """The two plans that give a clip of n samples the speaking rates rqs and the pitch ratios pqs over the segments `starts`, every
    segment's duration len_i 65536 / rq_i kept: .stretch, the table of ONE tt_tsw_stretch at rq_eff_i = stretch_rq(rq_i, pq_i) (None
    when every rq_eff is 1.0: nothing is stretched), and .resample, the table of ONE tt_rsw_resample whose input-domain borders are the
    stretch table's m_i, at pq_i.  .n_mid and .n_out are the lengths after either; .anchors int64 [S + 1, 2]: (input sample, output
    sample) of every border and of the end."""

    def __init__(self, n, starts, rqs, pqs):
        from . import stretch as tsm
        self.n, self.starts, self.rqs, self.pqs = int(n), [int(b) for b in starts], [int(r) for r in rqs], [int(p) for p in pqs]
        self.rq_effs = [stretch_rq(rq, pq) for rq, pq in zip(self.rqs, self.pqs)]
        for i, (b, e) in enumerate(zip(self.starts, self.starts[1:] + [self.n])):
            if len(self.starts) > 1 and e - b < MIN_WORD_SPAN:
                raise ValueError(f"pitch map: segment {i} starts at sample {b} and ends at {e}: with the durations kept, a segment covers at "
                                 f"least {MIN_WORD_SPAN} samples (PitchMap.from_words)")
        rm = tsm.RateMap(self.n, self.starts, self.rq_effs)
        self.stretch = None if all(r == E.TSM_RATE_ONE for r in self.rq_effs) else rm.table
        self.frames, self.n_mid = rm.frames, rm.n_out
        self.mid_starts = [row[0] for row in rm.table]  # (rate 1.0 throughout: m_i = a_i = b_i, the table is the identity)
        self.resample = map_plan(self.n_mid, self.mid_starts, self.pqs)
        self.n_out = map_out_samples(self.n_mid, self.resample)
        assert self.n_out > 0, "a planned table obeys the table's rules"

    @property
    def anchors(self):
        import torch
        return torch.tensor([(b, row[0]) for b, row in zip(self.starts, self.resample)] + [(self.n, self.n_out)], dtype=torch.int64)

    def ideal(self, i):
        """sum_(j < i) len_j 65536 / rq_j: where border i (i = S: the end) would stand with no rounding, in samples."""
        ends = self.starts[1:] + [self.n]
        return sum((e - b) * E.TSM_RATE_ONE / rq for b, e, rq in list(zip(self.starts, ends, self.rqs))[:i])


def duration_bound(i, ideal):
    """How far border i >= 1 of a WarpChain (i = S: the clip's end) can stand from ideal = sum_(j < i) len_j 65536 / rq_j, in samples:
    ideal / 16384 + 8.01 i + 1.  From the two plans' roundings, with g_j = 65536^2 / (rq_eff_j pq_j) the achieved gain of segment j:
      N_j = (len_j + d_(j+1) - d_j - s_j) g_j + (e_(j+1) - e_j) / pq_j   output samples of segment j, exactly, where
      d_j = a_j - b_j, |d_j| <= 1       the stretch plan's offset at border j (tortoise_mi355x_tsw.h)
      |s_j| <= 1/2                      the rounding of the stretch's advance (or of its last length)
      0 <= e_j < pq_(j-1)               the resampler plan's offset at border j (tortoise_mi355x_rsw.h), e_0 = 0
    - g_j differs from 65536 / rq_j by the rounding of rq_eff_j = round(rq_j 65536 / pq_j): relatively at most
      pq_j / (2 rq_j 65536) / (1 - ...) <= 2^-15 (1 + 2^-14) < 2^-14 for pq / rq <= 4: ideal / 16384 in all, the only term that grows with
      the clip (7 samples in 5 s; a constant pitch=, whose one segment rounds the same way, has it too)
    - (|d_(j+1)| + |d_j| + 1/2) g_j <= 2.5 * 2 (1 + 2^-14) < 5.01 per segment
    - sum_j (e_(j+1) - e_j) / pq_j = e_i / pq_(i-1) + sum_(0 < j < i) e_j (1 / pq_(j-1) - 1 / pq_j): below 1 + 3 (i - 1), as
      e_j / pq_(j-1) < 1 and pq_(j-1) / pq_j <= 4."""
    return ideal / 16384.0 + 8.01 * i + 1.0
