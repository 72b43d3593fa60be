"""The streaming time-stretch without a GPU (include/tortoise_mi355x_tss.h, tortoise_tts_amd/stretch.py, api.py, api_fast.py): the closed
forms against brute force and the two safety inequalities, the reach of a stream into its history, an fp64 stream that keeps only a
slot's state equal to the fp64 whole-clip reference, the host flow of stream_speaking_rate= / stream_pitch= on fakes, and the header's
constants and host functions where the library is built."""
import os
import re

import numpy as np
import pytest
import torch

from tests import rsstream_reference as RS
from tests import tsm_reference as T
from tests import tsstream_reference as S
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stretch as tsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants():
    assert S.LOOK == 1407 == E.TSS_LOOK == tsm.stream_latency() and S.REGION == 1663 and S.REGION - 1 <= S.HIST == E.TSS_HIST
    assert round(1000 * tsm.stream_latency() / 24000, 1) == 58.6
    assert (E.TSM_WINDOW, E.TSM_HOP, E.TSM_SEARCH) == (T.W, T.HS, T.SEARCH)


@pytest.mark.parametrize("rq", S.RQS_8)
def test_frames_done_against_brute_force(rq):
    k = np.arange(1, 60)
    assert (np.diff([T.nominal(int(v), rq) for v in k]) >= 0).all()  # a_k does not decrease: the complete frames are a prefix
    for n in range(6000):
        assert tsm.stream_frames_done(n, rq) == S.done_brute(n, rq), (n, rq)
    assert tsm.stream_frames_done(S.LOOK - 1, rq) == 0 and tsm.stream_frames_done(S.LOOK, rq) == 1


@pytest.mark.parametrize("rq", S.RQS_11)
def test_nothing_is_emitted_early(rq):
    """For every n and every final length N >= n: done(n) <= K(N) - 1 and done(n) Hs <= n_out(N).  n_out and K do not decrease in N, so N = n
    is the binding case; both are checked for every n <= 100001.  At most 8 frames are left to a flush."""
    n = np.arange(1, 100002, dtype=np.int64)
    done = np.where(n < S.LOOK, 0, (((n - S.LOOK + 1) << 16) - 32768 - 1) // (T.HS * rq) + 1)
    n_out = np.maximum(1, (n * T.RATE_ONE + rq // 2) // rq)
    K = -(-n_out // T.HS) + 1
    assert (np.diff(n_out) >= 0).all() and (done <= K - 1).all() and (done * T.HS <= n_out).all()
    assert (K - 1 - done).max() <= 8 and ((K - 1 - done).max() == 8) == (rq <= 32769)
    for v in (1, 1406, 1407, 5000, 100001):  # (the vectorised closed form is stream_frames_done's)
        assert done[v - 1] == tsm.stream_frames_done(v, rq) and n_out[v - 1] == T.out_samples(v, rq) and K[v - 1] == T.frames(v, rq)


def test_stream_ready_and_offsets():
    for rq in S.RQS_8:
        for n in S.LENGTHS:
            for seed, (chunks, with_last) in enumerate(S.chunkings(n, n)):
                pushes = [(c, with_last and i == len(chunks) - 1) for i, c in enumerate(chunks)] + ([] if with_last else [(0, True)])
                before = emitted = offsets = 0
                for c, flush in pushes:
                    got = tsm.stream_ready(before, c, rq, flush)
                    assert got == S.ready_total(before + c, rq, flush) - S.ready_total(before, rq, False) >= 0
                    k0, k1 = S.done_brute(before, rq) + 1, S.frames_total(before + c, rq, flush)
                    assert tsm.stream_frames_total(before + c, rq, flush) == k1 >= k0 - 1
                    assert tsm.stream_offsets(before, c, rq, flush) == (k1 - k0 + 1 + (k0 == 1) if k1 >= k0 else 0)
                    before, emitted, offsets = before + c, emitted + got, offsets + tsm.stream_offsets(before, c, rq, flush)
                assert before == n and emitted == T.out_samples(n, rq) and offsets == T.frames(n, rq)
    assert tsm.stream_ready(0, 0, 65536, True) == 0 and tsm.stream_offsets(0, 0, 65536, True) == 0  # a flush of nothing
    assert tsm.stream_ready(E.TSM_MAX_SAMPLES - 5, 5, 32768, True) > 0
    for bad in ((E.TSM_MAX_SAMPLES - 5, 6, 65536), (0, -1, 65536), (-1, 5, 65536), (0, 5, 32767), (0, 5, 131073)):
        with pytest.raises(ValueError):
            tsm.stream_ready(*bad, False)


_reach = []


@pytest.mark.parametrize("rate", S.RATES)
def test_an_fp64_stream_with_a_slot_s_state_equals_the_fp64_clip(rate):
    """Offsets exactly, samples to 1e-12, over the lengths and the chunkings; everything older than the 1664-sample history is NaN."""
    rq = T.rate_q(rate)
    for i, n in enumerate(S.LENGTHS):
        x = T.clip(n, i % 2)
        want = T.stretch(x, rq)
        for chunks, with_last in S.chunkings(n, 100 + i):
            y, off, reach = S.stream_fp64(x, rq, chunks, with_last)
            assert off.shape == want["offsets"].shape and (off == want["offsets"]).all(), (n, rate, chunks[:8])
            assert y.shape == want["y"].shape and np.abs(y - want["y"]).max() < 1e-12, (n, rate, chunks[:8])
            _reach.append(reach)
    assert max(_reach) <= 1662
    if rate == S.RATES[-1]:
        assert max(_reach) >= 1600


def test_the_history_reach_by_brute_force():
    """After a push to n the next frame k' = done(n) + 1 reaches back n - max(a_k' - 256, 0) <= 1662 samples; some n reaches 1662."""
    worst = 0
    for rq in S.RQS_11:
        for n in range(1, 12000):
            k = tsm.stream_frames_done(n, rq) + 1
            reach = n - max(T.nominal(k, rq) - T.SEARCH, 0)
            assert reach <= S.REGION - 1 <= S.HIST, (n, rq)
            worst = max(worst, reach)
    assert worst == 1662


def test_stream_options():
    for kw in ({}, {"stream_speaking_rate": None}, {"stream_speaking_rate": 1.0, "stream_pitch": 0}, {"stream_pitch": None}):
        assert tsm.stream_options(kw) is None and kw == {}
    kw = {"stream_speaking_rate": 1.25, "top_k": 3}
    assert tsm.stream_options(kw) == (81920, 65536) and kw == {"top_k": 3}
    assert tsm.stream_options({"stream_pitch": 3}) == rs.pitch(3)[::-1] == (55109, 77936)
    assert tsm.stream_options({"stream_pitch": 3, "stream_speaking_rate": 1.25}) == rs.pitch(3, 1.25)[::-1]
    for bad in (0.49, 2.01, float("nan"), "1.2", True):
        with pytest.raises(ValueError, match="stream_speaking_rate"):
            tsm.stream_options({"stream_speaking_rate": bad})
    for bad in (12.5, -13, float("nan"), "2"):
        with pytest.raises(ValueError, match="stream_pitch"):
            tsm.stream_options({"stream_pitch": bad})
    with pytest.raises(ValueError, match="stream_pitch=12.0 semitones with stream_speaking_rate=0.9"):  # 0.9 / 2 < 0.5
        tsm.stream_options({"stream_pitch": 12, "stream_speaking_rate": 0.9})


# ------------------------------------------------------------------------------------------------- host flow on fakes
def _instances(monkeypatch):
    from tests.test_stream_sessions_cpu import _instances as base
    api_fast, make = base(monkeypatch)
    RS.FakeStreamResampleStage.made = []
    S.FakeStreamStretchStage.made = []
    monkeypatch.setattr(api_fast.stages, "StreamResampleStage", RS.FakeStreamResampleStage)
    monkeypatch.setattr(api_fast.stages, "StreamStretchStage", S.FakeStreamStretchStage)
    return api_fast, make


TEXTS = [(list(range(5, 20)), 4, 70, 5), (list(range(3, 12)), 9, 62, 40), (list(range(7, 30)), 11, 66, 4)]  # (text, seed, max_mel_tokens, chunk)


def _whole(pieces, rate=None, pitch=None, sample_rate=None):
    """The fakes' whole-clip chain: the stretch at rq_eff, the pitch ratio, the sample rate."""
    x = torch.cat(pieces).numpy()
    plan = tsm.stream_options({"stream_speaking_rate": rate, "stream_pitch": pitch})
    if plan is not None and plan[0] != E.TSM_RATE_ONE:
        x = S.whole_hold(x, plan[0])
    if plan is not None and plan[1] != E.RS_PITCH_ONE:
        x = RS.whole_hold(x, plan[1], E.RS_PITCH_ONE)
    if sample_rate is not None:
        x = RS.whole_hold(x, *rs.ratio(24000, sample_rate))
    return x


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_tts_stream_at_another_speaking_rate_and_pitch_keeps_the_pieces(monkeypatch, stop):
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    for t, s, m, c in TEXTS:
        kw = dict(max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)
        plain = [p.clone() for p in one.tts_stream(t, **kw)]
        for off in ({}, {"stream_speaking_rate": None, "stream_pitch": None}, {"stream_speaking_rate": 1.0, "stream_pitch": 0}):
            again = list(one.tts_stream(t, **off, **kw))
            assert len(again) == len(plain) and all(torch.equal(a, b) for a, b in zip(again, plain))
        if t is TEXTS[0][0]:
            assert one._stretch_stage is None and one._pitch_stage is None and one._stream_stage is None  # nothing was built for them
        for opts in (dict(stream_speaking_rate=1.25), dict(stream_speaking_rate=0.5), dict(stream_pitch=3),
                     dict(stream_speaking_rate=0.8, stream_pitch=-2, stream_sample_rate=16000)):
            got = list(one.tts_stream(t, **opts, **kw))
            want = _whole(plain, opts.get("stream_speaking_rate"), opts.get("stream_pitch"), opts.get("stream_sample_rate"))
            assert len(got) == len(plain) and torch.cat(got).numpy().tobytes() == want.tobytes(), opts
            ts = one._stretch_stage
            assert ts.max_streams == 1 and not ts.slots and len(S.FakeStreamStretchStage.made) == 1  # one stage, slot freed
            assert [f for call in ts.calls[-len(plain):] for _, _, f in call] == [False] * (len(plain) - 1) + [True]
            if "stream_pitch" in opts:
                assert one._pitch_stage is not one._stream_stage and not one._pitch_stage.slots
                # the chain's order: the pitch resampler takes what the stretch emitted, push by push
                assert [n for call in one._pitch_stage.calls[-len(plain):] for _, n, _ in call] == \
                    _emitted(ts.calls[-len(plain):], tsm.stream_options(dict(opts))[0])
            if "stream_sample_rate" in opts:
                assert not one._stream_stage.slots
                assert [f for call in one._stream_stage.calls[-len(plain):] for _, _, f in call] == [False] * (len(plain) - 1) + [True]
    # a generator that is dropped half way frees its slots
    g = one.tts_stream(TEXTS[0][0], stream_speaking_rate=1.25, stream_pitch=2, stream_sample_rate=8000, max_mel_tokens=70, use_deterministic_seed=4,
                       stream_chunk_size=5, overlap_wav_len=128)
    next(g)
    assert len(one._stretch_stage.slots) == len(one._pitch_stage.slots) == len(one._stream_stage.slots) == 1
    g.close()
    assert not one._stretch_stage.slots and not one._pitch_stage.slots and not one._stream_stage.slots


def _emitted(calls, rq):
    """What a stream whose pushes were `calls` (one slot per call) emitted per push."""
    out, before = [], 0
    for (_, n, flush), in calls:
        out.append(tsm.stream_ready(before, n, rq, flush))
        before += n
    return out


@torch.no_grad()
def test_validation_comes_before_a_slot_is_taken_and_the_old_keywords_stay_refused(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    one, many = make(1), make(2)
    t = TEXTS[0][0]
    for name, bad in (("stream_speaking_rate", 2.5), ("stream_speaking_rate", "fast"), ("stream_pitch", 13), ("stream_pitch", float("nan"))):
        with pytest.raises(ValueError, match=name):
            next(one.tts_stream(t, **{name: bad}))
        with pytest.raises(ValueError, match=name):
            many.open_stream(t, **{name: bad})
        with pytest.raises(ValueError, match=name):
            next(many.tts_stream_many([t, t], **{name: [None, bad]}))
    with pytest.raises(ValueError, match="stream_pitch=12.0 semitones with stream_speaking_rate=0.9"):
        many.open_stream(t, stream_pitch=12, stream_speaking_rate=0.9)
    with pytest.raises(ValueError, match="stream_pitch=12.0 semitones with stream_speaking_rate=0.9"):  # per-text values meet per text
        next(many.tts_stream_many([t, t], stream_pitch=[0, 12], stream_speaking_rate=[1.5, 0.9]))
    with pytest.raises(ValueError, match="3 stream_speaking_rate values for 2 texts"):
        next(many.tts_stream_many([t, t], stream_speaking_rate=[0.8, None, 0.8]))
    with pytest.raises(ValueError, match="1 stream_pitch values for 2 texts"):
        next(many.tts_stream_many([t, t], stream_pitch=[2]))
    assert not many._sessions and not S.FakeStreamStretchStage.made and not RS.FakeStreamResampleStage.made
    for fn in (lambda **kw: next(one.tts_stream(t, **kw)), lambda **kw: many.open_stream(t, **kw), lambda **kw: next(many.tts_stream_many([t], **kw))):
        with pytest.raises(ValueError, match="speaking_rate is not available for streamed audio"):
            fn(speaking_rate=1.2)
        with pytest.raises(ValueError, match="speaking_rate is not available for streamed audio"):
            fn(speaking_rate=1.2, stream_speaking_rate=1.2)
        with pytest.raises(ValueError, match="pitch is not available for streamed audio"):
            fn(pitch=2, stream_pitch=2)
        with pytest.raises(ValueError, match="loudness"):
            fn(loudness=-23.0, stream_speaking_rate=1.2)
        with pytest.raises(ValueError, match="trim_silence"):
            fn(trim_silence=True, stream_speaking_rate=1.2)
        with pytest.raises(ValueError, match="max_pause"):
            fn(max_pause=0.3, stream_pitch=1)
    assert not many._sessions and not S.FakeStreamStretchStage.made and not RS.FakeStreamResampleStage.made
    # every stretch slot busy: the refusal takes no row and leaves no slot of the other stages behind
    kw = dict(stream_chunk_size=5, overlap_wav_len=128, max_mel_tokens=70)
    many.open_stream(t, stream_speaking_rate=1.2, **kw)
    many._stretch_stage.slots[1] = dict(many._stretch_stage.slots[0])  # (held by someone else)
    with pytest.raises(RuntimeError, match="time-stretch streams"):
        many.open_stream(t, stream_speaking_rate=0.8, stream_sample_rate=8000, **kw)
    assert len(many._sessions) == 1 and (many._stream_stage is None or not many._stream_stage.slots)


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_sessions_with_their_own_rates_and_pitches(monkeypatch, stop):
    """Three texts on two slots: the third waits for a slot.  Every text keeps its pieces and flags; a chain's pieces concatenate to the
    whole-clip chain, the None one is today's bits; a round's due pieces share ONE push per stage."""
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    kw = dict(max_mel_tokens=66, stream_chunk_size=5, overlap_wav_len=128)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s, _, _ in TEXTS]
    many = make(2, stop)
    rates, pitches, srs = [0.8, None, 1.25], [None, None, 3], [None, None, 16000]
    got = {}
    for i, wav, done in many.tts_stream_many([t for t, _, _, _ in TEXTS], use_deterministic_seed=[s for _, s, _, _ in TEXTS], stream_speaking_rate=rates,
                                             stream_pitch=pitches, stream_sample_rate=srs, **kw):
        got.setdefault(i, []).append((wav.clone(), done))
    assert len(S.FakeStreamStretchStage.made) == 1 and many._stretch_stage.max_streams == 2 and not many._stretch_stage.slots and not many._sessions
    assert len(RS.FakeStreamResampleStage.made) == 2 and not many._pitch_stage.slots and not many._stream_stage.slots
    for i in range(3):
        assert [d for _, d in got[i]] == [False] * (len(plain[i]) - 1) + [True]
        if rates[i] is None:
            assert all(torch.equal(a, b) for (a, _), b in zip(got[i], plain[i]))
        else:
            assert torch.cat([a for a, _ in got[i]]).numpy().tobytes() == _whole(plain[i], rates[i], pitches[i], srs[i]).tobytes()
    # two sessions with a chain each and the same schedule: every round is ONE push of two slots on every stage
    many = make(2, stop)
    t, s = TEXTS[0][0], TEXTS[0][1]
    for rate, pitch in ((1.25, 2), (0.8, -3)):
        many.open_stream(t, use_deterministic_seed=s, stream_speaking_rate=rate, stream_pitch=pitch, stream_sample_rate=16000, **kw)
    n = sum(1 for _ in many.stream_pieces())
    for stage in (many._stretch_stage, many._pitch_stage, many._stream_stage):
        assert n == 2 * len(plain[0]) and all(len(c) == 2 for c in stage.calls) and len(stage.calls) == len(plain[0]) and not stage.slots
    # the flush comes with the extra last piece of a sequence that ends on a buffer boundary
    flags = [[f for _, _, f in c] for c in many._stretch_stage.calls]
    assert flags == [[False, False]] * (len(plain[0]) - 1) + [[True, True]]


@torch.no_grad()
def test_close_stream_frees_every_slot_of_the_session(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    many = make(2, False)
    t, s, m, c = TEXTS[0]
    kw = dict(max_mel_tokens=m, stream_chunk_size=c, overlap_wav_len=128)
    keep = many.open_stream(t, use_deterministic_seed=s, stream_speaking_rate=0.8, **kw)
    gone = many.open_stream(t, use_deterministic_seed=s, stream_speaking_rate=1.25, stream_pitch=2, stream_sample_rate=16000, **kw)
    assert sorted(many._stretch_stage.slots) == [0, 1] and sorted(many._pitch_stage.slots) == [0] and sorted(many._stream_stage.slots) == [0]
    many.close_stream(gone)
    assert sorted(many._stretch_stage.slots) == [0] and not many._pitch_stage.slots and not many._stream_stage.slots
    late = many.open_stream(t, use_deterministic_seed=s, stream_pitch=-2, **kw)  # the freed slots serve the next admission
    assert sorted(many._stretch_stage.slots) == [0, 1] and sorted(many._pitch_stage.slots) == [0]
    out = {}
    for sid, wav, done in many.stream_pieces():
        out.setdefault(sid, []).append(wav)
    assert set(out) == {keep, late} and not many._stretch_stage.slots and not many._pitch_stage.slots
    plain = list(make(1, False).tts_stream(t, use_deterministic_seed=s, **kw))
    assert torch.cat(out[keep]).numpy().tobytes() == _whole(plain, 0.8).tobytes()
    assert torch.cat(out[late]).numpy().tobytes() == _whole(plain, None, -2).tobytes()


@torch.no_grad()
def test_open_stretcher_on_fakes(monkeypatch):
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "StreamResampleStage", RS.FakeStreamResampleStage)
    monkeypatch.setattr(api.stages, "StreamStretchStage", S.FakeStreamStretchStage)

    class Host(api._Common):
        device = torch.device("cpu")

    h = Host()
    assert h.stream_stretcher is None and h.stream_pitch_resampler is None
    x = torch.from_numpy(T.clip(9001, 2))
    with h.open_stretcher(rate=1.25, keep_map=True) as r:
        assert r.rq == 81920 and r.latency_seconds == 1407 / 24000 and h.stream_stretcher.max_streams == 16 and h.stream_pitch_resampler is None
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900]), r.push(x[1900:]), r.finish()]
        assert got[0].shape == (0,) and (r.n_in, r.n_out) == (9001, 7201) and r.slot is None
        assert r.anchors().shape == (T.frames(9001, 81920), 2)
        with pytest.raises(ValueError, match="closed"):
            r.push(x[:4])
    assert torch.cat(got).numpy().tobytes() == S.whole_hold(x.numpy(), 81920).tobytes() and not h.stream_stretcher.slots
    with h.open_stretcher(rate=0.8, pitch=3) as r:
        pq, rq = rs.pitch(3, 0.8)
        assert (r.rq, r.pq) == (rq, pq) and r.latency_seconds > 1407 / 24000
        got = torch.cat([r.push(x[:5000]), r.finish(x[5000:])])
    assert got.numpy().tobytes() == RS.whole_hold(S.whole_hold(x.numpy(), rq), pq, 65536).tobytes()
    assert not h.stream_stretcher.slots and not h.stream_pitch_resampler.slots
    for bad in (dict(rate=2.5), dict(pitch=13), dict(rate=0.9, pitch=12), dict(), dict(rate=1.0, pitch=0)):
        with pytest.raises(ValueError):
            h.open_stretcher(**bad)
    assert not h.stream_stretcher.slots


# ------------------------------------------------------------------------------------------------- the header and the library
def test_header_constants_equal_engine_constants():
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_tss.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert (val("TT_TSS_LOOK"), val("TT_TSS_HIST"), val("TT_TSS_MAX_STREAMS")) == (E.TSS_LOOK, E.TSS_HIST, E.TSS_MAX_STREAMS)
    assert "tt_tss_abi_version" in src and E.TSS_ABI_VERSION == 1
    from tortoise_tts_amd import build
    assert "tsm_stream.hip" in build.SOURCES and any(h.endswith("tortoise_mi355x_tss.h") for h in build._headers())
    steps = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "tsm_steps.h")).read()
    for name in ("tsm_store_region", "tsm_search", "tsm_argmax", "tsm_overlap_add", "tsm_next_template"):  # both kernels are built from the steps
        for f in ("tsm.hip", "tsm_stream.hip"):
            assert name + "(" in open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", f)).read() and name in steps, (name, f)


@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="the engine library is not built")
def test_the_library_s_host_functions_equal_the_mirrors():
    lib = E.load_library()
    assert lib.tt_tss_abi_version() == E.TSS_ABI_VERSION
    for rq in S.RQS_8:
        for n in list(range(0, 6000, 7)) + [E.TSM_MAX_SAMPLES]:
            assert lib.tt_tss_frames_done(n, rq) == tsm.stream_frames_done(n, rq)
        for n in S.LENGTHS:
            before = 0
            for c in list(S.chunkings(n, n))[3][0] + [0]:
                for flush in (0, 1):
                    assert lib.tt_tss_ready(before, c, rq, flush) == tsm.stream_ready(before, c, rq, flush)
                before += c
        assert lib.tt_tss_ready(E.TSM_MAX_SAMPLES - 5, 5, rq, 1) == tsm.stream_ready(E.TSM_MAX_SAMPLES - 5, 5, rq, True)
        assert lib.tt_tss_ready(E.TSM_MAX_SAMPLES - 5, 6, rq, 0) == -1 and lib.tt_tss_ready(-1, 6, rq, 0) == -1 and lib.tt_tss_ready(0, -1, rq, 0) == -1
    assert lib.tt_tss_ready(0, 10, 32767, 0) == -1 and lib.tt_tss_frames_done(10, 131073) == -1 and lib.tt_tss_frames_done(-1, 65536) == -1
