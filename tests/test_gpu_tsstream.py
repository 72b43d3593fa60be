"""The streaming time-stretch on the MI355X (csrc/tsm_stream.hip, include/tortoise_mi355x_tss.h): whatever the chunking, what a stream
emits - samples and chosen offsets - is bit for bit tt_tsm_stretch of the whole clip; every streamed clip also passes the fp64 reference's
protocol (tests/tsm_reference.check: admissible choices, samples inside the derived bound; no tolerance is chosen here); ragged pushes of
16 slots equal streaming alone, slots not named are untouched, nothing is written outside `out` / `offsets`; every refusal leaves the state
as it was; and stream_speaking_rate= / stream_pitch= / open_stretcher end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tsm_reference as T
from tests import tsstream_reference as S
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stages
from tortoise_tts_amd import stretch as tsm

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0    # what every output holds before a push
ISENT = -999   # ... and every offset
PAD = 64       # canaries on either side of `out` and `offsets`

_stages = {}


def stage():
    if "tss" not in _stages:
        _stages["tss"] = stages.StreamStretchStage(16, device=DEV)
    return _stages["tss"]


_whole = {}


def clip_and_whole(n, seed, rq):
    """(x, tt_tsm_stretch of the whole clip: samples and offsets as numpy), computed once."""
    key = (n, seed, rq)
    if key not in _whole:
        if "tsm" not in _stages:
            _stages["tsm"] = stages.TimeStretchStage(12000, max_clips=16, device=DEV)
        x = T.clip(n, seed)
        y, off = _stages["tsm"].stretch_many([torch.from_numpy(x)], [rq])[0]
        _whole[key] = (x, y.cpu().numpy(), off.numpy().astype(np.int32))
    return _whole[key]


def state(st, slot):
    v = [C.c_int() for _ in range(4)]
    E.check(st.lib.tt_tss_state(st.h, slot, *[C.byref(a) for a in v]))
    return tuple(a.value for a in v)  # n_in, m_out, frames, finished


_rq = {}


def opened(st, slot, rq):
    E.check(st.lib.tt_tss_open(st.h, slot, rq))
    _rq[(id(st), slot)] = rq
    return slot


def raw_push(st, items, expect=0, offsets=True):
    """One tt_tss_push of items = [(slot, chunk numpy f32, flush)] with `out` / `offsets` pre-filled with SENT / ISENT and canaries around
    them -> the emitted (samples, offsets) per item (numpy).  expect=-1: the call must be refused (then nothing may have been written)."""
    n = len(items)
    arr = C.c_int * max(n, 1)
    counts, frames = [], []
    for slot, x, flush in items:
        try:
            n_in, _, done, _ = state(st, slot)
            rq = _rq[(id(st), slot)]
            c = st.lib.tt_tss_ready(n_in, len(x), rq, int(flush))
            k1 = tsm.stream_frames_total(n_in + len(x), rq, flush)
            assert done == st.lib.tt_tss_frames_done(n_in, rq)
            k = k1 - done + (done == 0) if k1 > done else 0
        except Exception:
            c = k = 0
        counts.append(max(c, 0)), frames.append(k)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, np.float32) for _, x, _ in items] + [np.zeros(1, np.float32)])).to(DEV)
    y = torch.full((PAD + sum(counts) + PAD,), SENT, device=DEV)
    off = torch.full((PAD + sum(frames) + PAD,), ISENT, device=DEV, dtype=torch.int32)
    rc = st.lib.tt_tss_push(st.h, n, arr(*[s for s, _, _ in items]), arr(*[len(x) for _, x, _ in items]), arr(*[int(f) for _, _, f in items]),
                            E.ptr(audio), y.data_ptr() + 4 * PAD, off.data_ptr() + 4 * PAD if offsets else None, E.stream_ptr())
    y, off = y.cpu().numpy(), off.cpu().numpy()
    assert rc == expect, st.lib.tt_last_error()
    assert (y[:PAD] == SENT).all() and (y[PAD + sum(counts):] == SENT).all()  # nothing beyond the call's outputs
    assert (off[:PAD] == ISENT).all() and (off[PAD + sum(frames):] == ISENT).all()
    if rc:
        assert (y == SENT).all() and (off == ISENT).all()
        return None
    if not offsets:
        assert (off == ISENT).all()
    else:
        assert (off[PAD:PAD + sum(frames)] != ISENT).all()  # every entry of the call's offsets was written
    out, o, f = [], PAD, PAD
    for c, k in zip(counts, frames):
        out.append((y[o:o + c], off[f:f + k]))
        o += c
        f += k
    return out


def stream(st, x, rq, chunks, last_with_flush, slot=0):
    """x in `chunks` through one slot; the flush comes with the last chunk or as a push of its own -> (samples, offsets) (numpy)."""
    opened(st, slot, rq)
    assert sum(chunks) == len(x)
    got, at = [], 0
    for k, c in enumerate(chunks):
        got += raw_push(st, [(slot, x[at:at + c], last_with_flush and k == len(chunks) - 1)])
        at += c
    if not (last_with_flush and chunks):
        got += raw_push(st, [(slot, x[:0], True)])
    n_out = T.out_samples(len(x), rq) if len(x) else 0
    assert state(st, slot) == (len(x), n_out, T.frames(len(x), rq) - 1 if len(x) else 0, 1)
    return np.concatenate([y for y, _ in got]), np.concatenate([o for _, o in got])


def same_bits(a, b):
    return a.shape == b.shape and a.view(np.int32).tobytes() == b.view(np.int32).tobytes()


def same(got, want_y, want_off):
    return same_bits(got[0], want_y) and got[1].dtype == np.int32 and np.array_equal(got[1], want_off)


FAMILY = [(n, T.rate_q(r)) for n in S.LENGTHS for r in S.RATES]
_streamed = []  # (x, rq, y, offsets) of streams the first test ran, for the reference's protocol


def test_chunked_equals_whole_bit_for_bit():
    st = stage()
    done = 0
    for i, (n, rq) in enumerate(FAMILY):
        x, wy, woff = clip_and_whole(n, i % 2, rq)
        for j, (chunks, with_last) in enumerate(S.chunkings(n, 100 + i)):
            got = stream(st, x, rq, chunks, with_last)
            assert same(got, wy, woff), (n, rq, chunks[:8], with_last)
            if j == 3:
                _streamed.append((x, rq) + got)
            done += 1
        if n < S.LOOK:  # nothing is ready before the flush
            opened(st, 0, rq)
            assert raw_push(st, [(0, x, False)])[0][0].shape == (0,) and same(raw_push(st, [(0, x[:0], True)])[0], wy, woff)
    assert done == 4 * len(FAMILY) == 128
    # one sample per push
    x, wy, woff = clip_and_whole(1700, 0, T.RATE_MAX)
    assert same(stream(st, x, T.RATE_MAX, [1] * 1700, False), wy, woff)
    # without the offsets: the same samples, nothing written to `offsets`
    x, wy, woff = clip_and_whole(5000, 1, T.rate_q(0.8))
    opened(st, 3, T.rate_q(0.8))
    a = raw_push(st, [(3, x[:3000], False)], offsets=False)[0][0]
    b = raw_push(st, [(3, x[3000:], True)], offsets=False)[0][0]
    assert same_bits(np.concatenate([a, b]), wy)
    # a flush of nothing: nothing is emitted, the stream is finished
    opened(st, 3, T.RATE_ONE)
    y, off = raw_push(st, [(3, x[:0], True)])[0]
    assert y.shape == (0,) and off.shape == (0,) and state(st, 3) == (0, 0, 0, 1)


def test_every_streamed_clip_passes_the_reference_s_protocol():
    """tests/tsm_reference.check on the device's own offsets: no inadmissible frame, no sample outside its derived bound."""
    if not _streamed:
        test_chunked_equals_whole_bit_for_bit()
    worst_s = worst_y = 0.0
    for x, rq, y, off in _streamed:
        r = T.check(x, rq, y, off)
        assert not r["inadmissible"] and r["bad_samples"] == 0, (len(x), rq, r)
        worst_s, worst_y = max(worst_s, r["score_share"]), max(worst_y, r["y_share"])
    assert len(_streamed) == len(FAMILY)
    print(f"[parity] tt_tss_push: worst share of the fp64 score bound used {worst_s:.3f}, of the sample bound {worst_y:.3f}")


def test_ragged_pushes_of_sixteen_slots_equal_streaming_alone():
    st = stage()
    for s in range(16):
        E.check(st.lib.tt_tss_close(st.h, s))
    rng = np.random.default_rng(5)
    rqs = [T.rate_q(r) for r in S.RATES] * 3 + [32769, 131071, 65536, 100000]
    clips = []
    for s, rq in enumerate(rqs):
        n = int(rng.integers(1, 9000))
        clips.append(clip_and_whole(n, 80 + s, rq) + (list(S.chunkings(n, s))[3][0],))
        opened(st, s, rq)
    at, k, got, first_round = [0] * 16, [0] * 16, [[] for _ in range(16)], True
    while any(k[s] <= len(clips[s][3]) for s in range(16)):
        live = [s for s in range(16) if k[s] <= len(clips[s][3])]
        named = [s for s in live if first_round or rng.random() < 0.6] or live[:1]  # the first push names all sixteen
        first_round = False
        rng.shuffle(named)
        items = []
        for s in named:
            x, _, _, chunks = clips[s]
            c = chunks[k[s]] if k[s] < len(chunks) else 0
            items.append((s, x[at[s]:at[s] + c], k[s] == len(chunks)))  # the flush is a push of its own
        before = {s: state(st, s) for s in live if s not in named}
        for s, yo in zip(named, raw_push(st, items)):
            got[s].append(yo)
            at[s] += len(items[named.index(s)][1])
            k[s] += 1
        assert all(state(st, s) == v for s, v in before.items())  # slots not named: untouched (their bits follow below)
    for s in range(16):
        assert same((np.concatenate([y for y, _ in got[s]]), np.concatenate([o for _, o in got[s]])), clips[s][1], clips[s][2]), (s, rqs[s])
    # a slot that another clip went through reproduces a fresh slot's bits
    x, wy, woff = clip_and_whole(5000, 99, T.rate_q(1.25))
    assert same(stream(st, x, T.rate_q(1.25), list(S.chunkings(5000, 1))[3][0], True, slot=11), wy, woff)
    x, wy, woff = clip_and_whole(3000, 98, T.rate_q(0.5))
    assert same(stream(st, x, T.rate_q(0.5), list(S.chunkings(3000, 2))[2][0], False, slot=11), wy, woff)
    # all-zero input takes d = 0 everywhere and gives +0
    for n, rq in ((5000, T.rate_q(0.8)), (1500, T.RATE_MAX), (1, T.RATE_MIN)):
        y, off = stream(st, np.zeros(n, np.float32), rq, [n // 2, n - n // 2], False)
        assert y.tobytes() == np.zeros(T.out_samples(n, rq), np.float32).tobytes() and not off.any() and len(off) == T.frames(n, rq)


def test_refusals_leave_the_state_as_it_was():
    """Every refused call is followed by the rest of the streams: their bits are those of the whole clips."""
    st = stage()
    for s in range(16):
        E.check(st.lib.tt_tss_close(st.h, s))
    ra, rb = T.rate_q(1.25), T.rate_q(0.5)
    xa, wya, woa = clip_and_whole(9001, 90, ra)
    xb, wyb, wob = clip_and_whole(5000, 91, rb)
    opened(st, 0, ra), opened(st, 1, rb)
    ga, gb = raw_push(st, [(0, xa[:4000], False), (1, xb[:2500], False)])
    opened(st, 2, T.RATE_ONE)
    raw_push(st, [(2, xa[:10], True)])  # slot 2: finished; slot 3: closed
    z = np.zeros(4, np.float32)
    bad = {
        "bad slot": [(16, z, False)], "negative slot": [(-1, z, False)], "duplicate slot": [(0, z, False), (1, z, False), (0, z, False)],
        "closed slot": [(1, z, False), (3, z, False)], "finished slot": [(0, z, False), (2, z, False)], "no stream": [],
    }
    keep = (state(st, 0), state(st, 1), state(st, 2))
    for name, items in bad.items():
        assert raw_push(st, items, expect=-1) is None, name
        assert (state(st, 0), state(st, 1), state(st, 2)) == keep, name
    # a negative length and a chunk that would cross 2^23 samples: refused on the counters alone (no such allocation exists)
    arr, y = C.c_int * 2, torch.full((8,), SENT, device=DEV)
    for n_chunk, what in ((-1, b"a chunk of -1"), (E.TSM_MAX_SAMPLES - 4000 + 1, b"exceed a stream's")):
        assert st.lib.tt_tss_push(st.h, 2, arr(1, 0), arr(0, n_chunk), arr(0, 0), E.ptr(y), E.ptr(y), None, E.stream_ptr()) == -1
        assert what in st.lib.tt_last_error() and (state(st, 0), state(st, 1), state(st, 2)) == keep and (y.cpu() == SENT).all()
    assert st.lib.tt_tss_ready(4000, E.TSM_MAX_SAMPLES - 4000 + 1, ra, 0) == -1 and st.lib.tt_tss_ready(4000, E.TSM_MAX_SAMPLES - 4000, ra, 1) > 0
    # a rate out of range at open: refused, and the open slot it named keeps streaming
    for rq in (0, -1, T.RATE_MIN - 1, T.RATE_MAX + 1):
        assert st.lib.tt_tss_open(st.h, 0, rq) == -1 and b"rate" in st.lib.tt_last_error() and state(st, 0) == keep[0]
        assert st.lib.tt_tss_frames_done(5000, rq) == -1 and st.lib.tt_tss_ready(0, 5000, rq, 0) == -1
    assert st.lib.tt_tss_open(st.h, 16, ra) == -1 and st.lib.tt_tss_open(st.h, -1, ra) == -1 and st.lib.tt_tss_close(st.h, 16) == -1
    for audio, out in ((None, E.ptr(y)), (E.ptr(y), None)):
        assert st.lib.tt_tss_push(st.h, 1, arr(0, 0), arr(1, 0), arr(0, 0), audio, out, None, E.stream_ptr()) == -1
        assert b"null argument" in st.lib.tt_last_error()
    assert st.lib.tt_tss_push(st.h, 1, None, arr(1, 0), arr(0, 0), E.ptr(y), E.ptr(y), None, E.stream_ptr()) == -1
    assert (state(st, 0), state(st, 1), state(st, 2)) == keep and (y.cpu() == SENT).all()
    ga2, gb2 = raw_push(st, [(0, xa[4000:], True), (1, xb[2500:], True)])
    assert same((np.concatenate([ga[0], ga2[0]]), np.concatenate([ga[1], ga2[1]])), wya, woa)
    assert same((np.concatenate([gb[0], gb2[0]]), np.concatenate([gb[1], gb2[1]])), wyb, wob)
    # a finished slot takes a new stream after tt_tss_open
    assert same(stream(st, xb, rb, [5000], True, slot=2), wyb, wob)
    assert st.lib.tt_tss_create(0, C.byref(E.vp())) == -1 and st.lib.tt_tss_create(65, C.byref(E.vp())) == -1
    # the stage's own checks come before the library's
    with pytest.raises(ValueError, match="rate"):
        st.open(T.RATE_MAX + 1)
    with pytest.raises(ValueError, match="not open"):
        st.push_many([(14, torch.zeros(4), False)])


# ------------------------------------------------------------------------------------------------- the API
def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


@torch.no_grad()
def test_open_stretcher_equals_stretch_and_shift_pitch():
    h = _host()
    x = torch.from_numpy(T.clip(9001, 2))
    want, amap = h.stretch_many([x.to(DEV)], rates=1.25, return_map=True)
    with h.open_stretcher(rate=1.25, keep_map=True) as r:
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900].to(DEV)), r.push(x[1900:9000]), r.finish(x[9000:])]
        assert got[0].shape == (0,) and all(g.device.type == "cuda" and g.dtype == torch.float32 for g in got)
        assert (r.n_in, r.n_out) == (9001, 7201) and r.latency_seconds == 1407 / 24000
        assert torch.equal(r.anchors(), amap[0])
    assert torch.equal(torch.cat(got).view(torch.int32), want[0].view(torch.int32)) and not h.stream_stretcher.slots
    want = h.shift_pitch(x.to(DEV), 3)
    with h.open_stretcher(pitch=3) as r:
        got = torch.cat([r.push(x[:2500]), r.push(x[2500:7000]), r.finish(x[7000:])])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not h.stream_stretcher.slots and not h.stream_pitch_resampler.slots
    want = h._at_pitch([x.to(DEV)], 0.8, -2)[0]
    with h.open_stretcher(rate=0.8, pitch=-2) as r:
        got = torch.cat([r.push(x[:5000]), r.finish(x[5000:])])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError, match="rate"):
        h.open_stretcher(rate=3.0)
    with pytest.raises(ValueError):
        h.open_stretcher()


@torch.no_grad()
def test_streams_at_another_speaking_rate_and_pitch_equal_the_whole_clip_chain():
    """Weights, texts and seeds as in tests/test_gpu_hifi_batch.py (max_mel_tokens=64)."""
    from tests.test_gpu_hifi_batch import _fast_instances, _texts
    texts, seeds, cond = _texts(3)
    kw = dict(conditioning_latents=(cond,), max_mel_tokens=64, stream_chunk_size=20)
    one = _fast_instances("bf16", 1)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s in zip(texts, seeds)]
    assert any(len(p) >= 2 for p in plain), "the streams of this test have several pieces"
    got = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_speaking_rate=1.25, **kw))
    want = one.stretch(torch.cat(plain[0]), rate=1.25)
    assert len(got) == len(plain[0]) and torch.equal(torch.cat(got).view(torch.int32), want.view(torch.int32))
    assert one._stretch_stage.max_streams == 1 and not one._stretch_stage.slots and one._pitch_stage is None
    # rate, pitch and sample rate: the whole-clip calls _voiced makes, without loudness
    got = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_speaking_rate=1.25, stream_pitch=3, stream_sample_rate=16000, **kw))
    want = one._voiced([torch.cat(plain[0])], 1.25, 3.0, None, 16000)[0]
    assert len(got) == len(plain[0]) and torch.equal(torch.cat(got).view(torch.int32), want.view(torch.int32))
    assert not one._stretch_stage.slots and not one._pitch_stage.slots and not one._stream_stage.slots
    again = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_speaking_rate=1.0, stream_pitch=0, **kw))
    assert len(again) == len(plain[0]) and all(torch.equal(a, b) for a, b in zip(again, plain[0]))
    # three texts on two slots, values per text (None: today's bits): one text waits for a slot
    many = _fast_instances("bf16", 2)
    rates, pitches = [0.8, None, 1.25], [None, None, -2]
    out = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=seeds, stream_speaking_rate=rates, stream_pitch=pitches, **kw):
        out.setdefault(i, []).append((wav.clone(), done))
    assert many._stretch_stage.max_streams == 2 and not many._stretch_stage.slots and not many._pitch_stage.slots and not many._sessions
    assert many._stream_stage is None
    for i, (rate, pitch) in enumerate(zip(rates, pitches)):
        assert [d for _, d in out[i]] == [False] * (len(plain[i]) - 1) + [True]
        if rate is None and pitch is None:
            assert all(torch.equal(a, b) for (a, _), b in zip(out[i], plain[i]))
        else:
            want = one._voiced([torch.cat(plain[i])], rate, pitch, None, None)[0]
            assert torch.equal(torch.cat([a for a, _ in out[i]]).view(torch.int32), want.view(torch.int32)), (i, rate, pitch)
