"""The streaming resampler without a GPU (include/tortoise_mi355x_rss.h, tortoise_tts_amd/resample.py, api.py, api_fast.py): the emission
rule against brute force, the reach of a push into the past, an fp64 stream equal to the fp64 whole-clip result index by index, the host
flow of stream_sample_rate= on fakes, and the header's constants and tt_rss_ready where the library is built."""
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_reference as R
from tests import rsstream_reference as S
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_issue_s_ratios_and_the_history():
    assert all(R.ratio_ok(P, Q) for P, Q in S.RATIOS)
    assert max(S.half_width(P, Q) for P, Q in S.RATIOS) == 285 and 2 * 285 + 1 <= S.HIST == E.RSS_HIST
    assert [S.half_width(P, Q) for P, Q in ((1, 2), (3, 2), (3, 1), (8, 1))] == [36, 54, 107, 285]
    assert all(rs.half_width(P, Q) == S.half_width(P, Q) and rs.stream_latency(P, Q) == S.half_width(P, Q) + 1 for P, Q in S.RATIOS)
    # the algorithmic delay: 1.5 ms for up-conversion, 4.5 ms to 8 kHz
    assert round(rs.stream_latency(1, 2) / 24.0, 1) == 1.5 and round(rs.stream_latency(3, 1) / 24.0, 1) == 4.5
    # which ratios have a bank: the common rates do, 320/147 and a pitch ratio do not
    assert [S.bank_fits(P, Q) for P, Q in ((3, 1), (3, 2), (1, 2), (1, 4), (3, 4), (80, 147), (160, 147), (320, 147), (77936, 65536))] == \
        [True] * 7 + [False] * 2


@pytest.mark.parametrize("P,Q", S.RATIOS)
def test_stream_ready_against_brute_force(P, Q):
    H = S.half_width(P, Q)
    worst = 0
    for n in S.LENGTHS:
        for seed in range(3):
            chunks = S.chunking(n, P, Q, 100 * seed + n)
            for flush_with_chunk in (False, True):
                pushes = [(c, False) for c in chunks]
                pushes = pushes[:-1] + [(chunks[-1], True)] if flush_with_chunk else pushes + [(0, True)]
                before, emitted = 0, 0
                for c, flush in pushes:
                    got = rs.stream_ready(before, c, P, Q, flush)
                    want = S.ready_brute(before + c, P, Q, flush) - S.ready_brute(before, P, Q)
                    assert got == want >= 0, (n, P, Q, before, c, flush)
                    if got:  # the earliest tap of this push's outputs: at or after n_prev - (2 H + 1)
                        reach = before - ((emitted * P) // Q - H)
                        assert reach <= 2 * H + 1 <= S.HIST - 5, (n, P, Q, before, c)
                        worst = max(worst, reach)
                    before, emitted = before + c, emitted + got
                assert before == n and emitted == R.out_samples(n, P, Q) == rs.out_samples(n, P, Q)
    assert worst <= 571
    with pytest.raises(ValueError):
        rs.stream_ready(E.RS_MAX_SAMPLES - 5, 6, P, Q, False)
    with pytest.raises(ValueError):
        rs.stream_ready(0, -1, P, Q, False)
    assert rs.stream_ready(E.RS_MAX_SAMPLES - 5, 5, P, Q, True) > 0


def test_stream_ready_refuses_what_the_resampler_refuses():
    for P, Q in ((9, 1), (1, 9), (6, 4), (0, 1)):
        with pytest.raises(ValueError):
            rs.stream_ready(0, 10, P, Q, False)


@pytest.mark.parametrize("P,Q", R.RATIOS + R.EXTREME_RATIOS)
def test_an_fp64_stream_equals_the_fp64_clip_index_by_index(P, Q):
    for n, chunks in ((300, [1] * 300), (37, [37]), (1000, S.chunking(1000, P, Q, 7)), (2000, S.chunking(2000, P, Q, 8) + [0])):
        x = R.clip(n, 3)
        want = R.resample(x, P, Q, bound=False)[0]
        st, got, at = S.Fp64Stream(P, Q), [], 0
        for c in chunks:
            got.append(st.push(x[at:at + c]))
            at += c
        got.append(st.push(x[at:], flush=True))
        got = np.concatenate(got)
        assert at == n and got.shape == want.shape and got.tobytes() == want.tobytes(), (n, P, Q)


def test_stream_options():
    for kw in ({}, {"stream_sample_rate": None}, {"stream_sample_rate": 24000}, {"stream_sample_rate": 24000.0}):
        assert rs.stream_options(kw) is None and kw == {}
    kw = {"stream_sample_rate": 8000, "top_k": 3}
    assert rs.stream_options(kw) == 8000 and kw == {"top_k": 3}
    for bad in (7999, 96001, 16000.5, "16000", True):
        with pytest.raises(ValueError, match="stream_sample_rate"):
            rs.stream_options({"stream_sample_rate": bad})


# ------------------------------------------------------------------------------------------------- host flow on fakes
def _instances(monkeypatch):
    from tests.test_stream_sessions_cpu import _instances as base
    api_fast, make = base(monkeypatch)
    S.FakeStreamResampleStage.made = []
    monkeypatch.setattr(api_fast.stages, "StreamResampleStage", S.FakeStreamResampleStage)
    return api_fast, make


TEXTS = [(list(range(5, 20)), 4, 70, 5), (list(range(3, 12)), 9, 62, 40), (list(range(7, 30)), 11, 66, 4)]  # (text, seed, max_mel_tokens, chunk)


def _whole(pieces, rate):
    x = torch.cat(pieces).numpy()
    return S.whole_hold(x, *rs.ratio(24000, rate))


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_tts_stream_at_another_rate_keeps_the_pieces(monkeypatch, stop):
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    for t, s, m, c in TEXTS:
        kw = dict(max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)
        plain = [p.clone() for p in one.tts_stream(t, **kw)]
        for rate in (None, 24000):
            again = list(one.tts_stream(t, stream_sample_rate=rate, **kw))
            assert len(again) == len(plain) and all(torch.equal(a, b) for a, b in zip(again, plain))
        assert one._stream_stage is None or t is not TEXTS[0][0]  # nothing was built for them
        for rate in (8000, 44100):
            made = len(S.FakeStreamResampleStage.made)
            got = list(one.tts_stream(t, stream_sample_rate=rate, **kw))
            assert len(got) == len(plain) and torch.cat(got).numpy().tobytes() == _whole(plain, rate).tobytes()
            stage = one._stream_stage
            assert len(S.FakeStreamResampleStage.made) == max(made, 1) and stage.max_streams == 1 and not stage.slots  # one stage, slot freed
            assert [f for call in stage.calls[-len(plain):] for _, _, f in call] == [False] * (len(plain) - 1) + [True]
    # a generator that is dropped half way frees its slot
    g = one.tts_stream(TEXTS[0][0], stream_sample_rate=8000, max_mel_tokens=70, use_deterministic_seed=4, stream_chunk_size=5, overlap_wav_len=128)
    next(g)
    assert len(one._stream_stage.slots) == 1
    g.close()
    assert not one._stream_stage.slots


@torch.no_grad()
def test_validation_comes_before_a_slot_is_taken_and_the_old_keywords_stay_refused(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    one, many = make(1), make(2)
    t = TEXTS[0][0]
    for bad in (7000, 16000.5, "8000"):
        with pytest.raises(ValueError, match="stream_sample_rate"):
            next(one.tts_stream(t, stream_sample_rate=bad))
        with pytest.raises(ValueError, match="stream_sample_rate"):
            many.open_stream(t, stream_sample_rate=bad)
        with pytest.raises(ValueError, match="stream_sample_rate"):
            next(many.tts_stream_many([t, t], stream_sample_rate=[8000, bad]))
    with pytest.raises(ValueError, match="3 stream_sample_rate values for 2 texts"):
        next(many.tts_stream_many([t, t], stream_sample_rate=[8000, None, 8000]))
    assert not many._sessions and not S.FakeStreamResampleStage.made
    for fn in (lambda **kw: next(one.tts_stream(t, **kw)), lambda **kw: many.open_stream(t, **kw), lambda **kw: next(many.tts_stream_many([t], **kw))):
        with pytest.raises(ValueError, match="sample_rate is not available for streamed audio"):
            fn(sample_rate=16000)
        with pytest.raises(ValueError, match="sample_rate is not available for streamed audio"):
            fn(sample_rate=16000, stream_sample_rate=16000)
        with pytest.raises(ValueError, match="pitch is not available for streamed audio"):
            fn(pitch=2, stream_sample_rate=16000)
    assert not many._sessions and not S.FakeStreamResampleStage.made


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_sessions_at_their_own_rates(monkeypatch, stop):
    """Three texts on two slots with rates [8000, None, 48000]: the third waits for a slot.  Every text keeps its pieces and flags; a rate's
    pieces concatenate to the whole-clip result, the None one is today's bits; a round's due pieces share one push_many."""
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    kw = dict(max_mel_tokens=66, stream_chunk_size=5, overlap_wav_len=128)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s, _, _ in TEXTS]
    many = make(2, stop)
    rates = [8000, None, 48000]
    got = {}
    for i, wav, done in many.tts_stream_many([t for t, _, _, _ in TEXTS], use_deterministic_seed=[s for _, s, _, _ in TEXTS], stream_sample_rate=rates,
                                             **kw):
        got.setdefault(i, []).append((wav.clone(), done))
    stage = many._stream_stage
    assert len(S.FakeStreamResampleStage.made) == 1 and stage.max_streams == 2 and not stage.slots and not many._sessions
    for i, rate in enumerate(rates):
        assert [d for _, d in got[i]] == [False] * (len(plain[i]) - 1) + [True]
        if rate is None:
            assert all(torch.equal(a, b) for (a, _), b in zip(got[i], plain[i]))
        else:
            assert torch.cat([a for a, _ in got[i]]).numpy().tobytes() == _whole(plain[i], rate).tobytes()
    # two sessions with a rate each and the same schedule: every round is ONE push of two slots
    many = make(2, stop)
    t, s = TEXTS[0][0], TEXTS[0][1]
    for rate in (16000, 44100):
        many.open_stream(t, use_deterministic_seed=s, stream_sample_rate=rate, **kw)
    n = sum(1 for _ in many.stream_pieces())
    calls = many._stream_stage.calls
    assert n == 2 * len(plain[0]) and all(len(c) == 2 for c in calls) and len(calls) == len(plain[0]) and not many._stream_stage.slots


@torch.no_grad()
def test_close_stream_frees_the_resampler_s_slot(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    many = make(2, False)
    t, s, m, c = TEXTS[0]
    kw = dict(max_mel_tokens=m, stream_chunk_size=c, overlap_wav_len=128)
    keep = many.open_stream(t, use_deterministic_seed=s, stream_sample_rate=8000, **kw)
    gone = many.open_stream(t, use_deterministic_seed=s, stream_sample_rate=16000, **kw)
    assert sorted(many._stream_stage.slots) == [0, 1]
    many.close_stream(gone)
    assert sorted(many._stream_stage.slots) == [0]
    late = many.open_stream(t, use_deterministic_seed=s, stream_sample_rate=48000, **kw)  # the freed slot serves the next admission
    assert sorted(many._stream_stage.slots) == [0, 1] and many._stream_stage.slots[1]["Q"] == 2
    out = {}
    for sid, wav, done in many.stream_pieces():
        out.setdefault(sid, []).append(wav)
    assert set(out) == {keep, late} and not many._stream_stage.slots
    one = make(1, False)
    plain = list(one.tts_stream(t, use_deterministic_seed=s, **kw))
    assert torch.cat(out[keep]).numpy().tobytes() == _whole(plain, 8000).tobytes()
    assert torch.cat(out[late]).numpy().tobytes() == _whole(plain, 48000).tobytes()


@torch.no_grad()
def test_open_resampler_on_a_fake(monkeypatch):
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "StreamResampleStage", S.FakeStreamResampleStage)

    class Host(api._Common):
        device = torch.device("cpu")

    h = Host()
    assert h.stream_resampler is None
    x = torch.from_numpy(R.clip(5000, 2))
    with h.open_resampler(44100) as r:
        assert (r.P, r.Q) == (80, 147) and r.latency_seconds == 37 / 24000 and h.stream_resampler.max_streams == 16
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900]), r.push(x[1900:]), r.finish()]
        assert got[0].shape == (0,) and (r.n_in, r.n_out) == (5000, 9188) and r.slot is None
        with pytest.raises(ValueError, match="closed"):
            r.push(x[:4])
    assert torch.cat(got).numpy().tobytes() == S.whole_hold(x.numpy(), 80, 147).tobytes() and not h.stream_resampler.slots
    with pytest.raises(ValueError, match="ratio 12/1"):
        h.open_resampler(2000)
    r = h.open_resampler(16000, from_rate=48000)
    assert (r.P, r.Q) == (3, 1) and r.latency_seconds == 108 / 48000
    r.close()


# ------------------------------------------------------------------------------------------------- the header and the library
def _header():
    return open(os.path.join(ROOT, "include", "tortoise_mi355x_rss.h")).read()


def test_header_constants_equal_engine_constants():
    src = _header()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert (val("TT_RSS_HIST"), val("TT_RSS_MAX_STREAMS"), val("TT_RSS_BANK_MAX"), val("TT_RSS_AUTO_MAX_Q")) == \
        (E.RSS_HIST, E.RSS_MAX_STREAMS, E.RSS_BANK_MAX, E.RSS_AUTO_MAX_Q)
    assert (val("TT_RSS_AUTO"), val("TT_RSS_TABLE"), val("TT_RSS_BANK")) == (E.RSS_AUTO, E.RSS_TABLE, E.RSS_BANK)
    assert "tt_rss_abi_version" in src and E.RSS_ABI_VERSION == 1
    from tortoise_tts_amd import build
    assert "resample_stream.hip" in build.SOURCES and any(h.endswith("tortoise_mi355x_rss.h") for h in build._headers())


@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="the engine library is not built")
def test_tt_rss_ready_equals_stream_ready():
    lib = E.load_library()
    assert lib.tt_rss_abi_version() == E.RSS_ABI_VERSION
    for P, Q in S.RATIOS:
        for n in (1, 37, 300, 5000):
            before = 0
            for c in S.chunking(n, P, Q, n) + [0]:
                for flush in (0, 1):
                    assert lib.tt_rss_ready(before, c, P, Q, flush) == rs.stream_ready(before, c, P, Q, flush)
                before += c
        assert lib.tt_rss_ready(E.RS_MAX_SAMPLES - 5, 5, P, Q, 1) == rs.stream_ready(E.RS_MAX_SAMPLES - 5, 5, P, Q, True)
        assert lib.tt_rss_ready(E.RS_MAX_SAMPLES - 5, 6, P, Q, 0) == -1 and lib.tt_rss_ready(-1, 6, P, Q, 0) == -1 and lib.tt_rss_ready(0, -1, P, Q, 0) == -1
    assert lib.tt_rss_ready(0, 10, 6, 4, 0) == -1 and lib.tt_rss_ready(0, 10, 9, 1, 0) == -1
