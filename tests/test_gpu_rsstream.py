"""The streaming resampler on the MI355X (csrc/resample_stream.hip, include/tortoise_mi355x_rss.h): whatever the chunking, what a stream
emits is bit for bit tt_rs_resample of the whole clip, in the table form and in the bank form; every streamed sample also lies inside the
fp64 reference's derived bound (tests/resample_reference.py; no tolerance is chosen here); ragged pushes of 16 slots equal streaming
alone, slots not named are untouched, nothing is written outside `out`; every refusal leaves the state as it was; and
stream_sample_rate= / open_resampler end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_reference as R
from tests import rsstream_reference as S
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0   # what every output holds before a push
PAD = 64      # canaries on either side of `out`

_src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tortoise_tts_amd", "csrc", "resample_stream.hip")).read()
TILES = {"table": int(re.search(r"kRssTableTile == (\d+)", _src).group(1)), "bank": int(re.search(r"kRssBankTile == (\d+)", _src).group(1))}
FORMS = ("table", "bank")
COMMON = ((3, 1), (3, 2), (1, 2), (80, 147))  # 8, 16, 48 and 44.1 kHz from 24 kHz

_stages = {}


def stage(form):
    if form not in _stages:
        _stages[form] = stages.StreamResampleStage(16, form=form, device=DEV)
    return _stages[form]


_whole = {}


def clip_and_whole(n, seed, P, Q):
    """(x, tt_rs_resample of the whole clip as numpy f32), computed once."""
    key = (n, seed, P, Q)
    if key not in _whole:
        if "rs" not in _stages:
            _stages["rs"] = stages.ResampleStage(8000, max_clips=16, device=DEV)
        x = R.clip(n, seed)
        _whole[key] = (x, _stages["rs"].resample_many([torch.from_numpy(x)], [(P, Q)])[0][0].cpu().numpy())
    return _whole[key]


def state(st, slot):
    v = [C.c_int() for _ in range(4)]
    E.check(st.lib.tt_rss_state(st.h, slot, *[C.byref(a) for a in v]))
    return tuple(a.value for a in v)  # n_in, m_out, finished, form


def raw_open(st, slot, P, Q):
    return st.lib.tt_rss_open(st.h, slot, P, Q, E.stream_ptr())


def raw_push(st, items, expect=0):
    """One tt_rss_push of items = [(slot, chunk numpy f32, flush)] with `out` pre-filled with SENT and canaries around it -> the emitted
    samples per item (numpy).  expect=-1: the call must be refused (then nothing may have been written)."""
    n = len(items)
    arr = C.c_int * max(n, 1)
    counts = []
    for slot, x, flush in items:
        try:
            n_in = state(st, slot)[0]
            c = st.lib.tt_rss_ready(n_in, len(x), *_ratio[(id(st), slot)], int(flush))
        except Exception:
            c = 0
        counts.append(max(c, 0))
    audio = torch.from_numpy(np.concatenate([np.asarray(x, np.float32) for _, x, _ in items] + [np.zeros(1, np.float32)])).to(DEV)
    y = torch.full((PAD + sum(counts) + PAD,), SENT, device=DEV)
    rc = st.lib.tt_rss_push(st.h, n, arr(*[s for s, _, _ in items]), arr(*[len(x) for _, x, _ in items]), arr(*[int(f) for _, _, f in items]),
                            E.ptr(audio), y.data_ptr() + 4 * PAD, E.stream_ptr())
    y = y.cpu().numpy()
    assert rc == expect, st.lib.tt_last_error()
    assert (y[:PAD] == SENT).all() and (y[PAD + sum(counts):] == SENT).all()  # nothing beyond the call's outputs
    if rc:
        assert (y == SENT).all()
        return None
    out, o = [], PAD
    for c in counts:
        out.append(y[o:o + c])
        o += c
    return out


_ratio = {}


def opened(st, slot, P, Q):
    E.check(raw_open(st, slot, P, Q))
    _ratio[(id(st), slot)] = (P, Q)
    return slot


def stream(st, x, P, Q, chunks, last_with_flush, slot=0):
    """x in `chunks` through one slot; the flush comes with the last chunk or as a push of its own -> every output (numpy)."""
    opened(st, slot, P, Q)
    assert sum(chunks) == len(x)
    got, at = [], 0
    for k, c in enumerate(chunks):
        got += raw_push(st, [(slot, x[at:at + c], last_with_flush and k == len(chunks) - 1)])
        at += c
    if not (last_with_flush and chunks):
        got += raw_push(st, [(slot, x[:0], True)])
    assert state(st, slot)[:3] == (len(x), R.out_samples(len(x), P, Q) if len(x) else 0, 1)
    return np.concatenate(got)


def chunkings(n, P, Q):
    H = S.half_width(P, Q)
    yield [n], True                                        # everything in one push, flushed with it
    yield [n], False                                       # ... and flushed by a push of its own
    cyc, left = [], n
    for k in range(10 ** 6):
        if left == 0:
            break
        c = min((1, 37, H, 0, H + 1)[k % 5], left)         # shorter than the history; pushes that emit nothing; zero-length ones between
        cyc.append(c)
        left -= c
    yield cyc, False
    yield S.chunking(n, P, Q, n) + [0], True               # seeded draws; the flush comes with a zero-length last chunk


def same_bits(a, b):
    return a.shape == b.shape and a.view(np.int32).tobytes() == b.view(np.int32).tobytes()


FAMILY = [(n, P, Q) for P, Q in R.RATIOS for n in (1, 2, 37, 300, 5000)] + [(n, P, Q) for P, Q in R.EXTREME_RATIOS for n in (1, 2, 37, 300, 2000)]


@pytest.mark.parametrize("form", FORMS)
def test_chunked_equals_whole_bit_for_bit(form):
    st = stage(form)
    done = 0
    for i, (n, P, Q) in enumerate(FAMILY):
        if form == "bank" and not S.bank_fits(P, Q):
            continue
        x, want = clip_and_whole(n, i, P, Q)
        for chunks, with_last in chunkings(n, P, Q):
            assert same_bits(stream(st, x, P, Q, chunks, with_last), want), (form, n, P, Q, chunks[:8], with_last)
            done += 1
        if n == 300:  # one sample per push
            assert same_bits(stream(st, x, P, Q, [1] * n, False), want), (form, n, P, Q)
        if n < S.half_width(P, Q) + 2:  # nothing is ready before the flush
            opened(st, 0, P, Q)
            assert raw_push(st, [(0, x, False)])[0].shape == (0,) and same_bits(raw_push(st, [(0, x[:0], True)])[0], want)
    assert done >= 100


@pytest.mark.parametrize("form", FORMS)
def test_pushes_that_end_around_a_tile(form):
    """A first push that emits one tile - 1, one tile and one tile + 1 outputs of the form's tile (and twice that), then the rest."""
    st, T = stage(form), TILES[form]
    assert TILES == {"table": 1024, "bank": 256}
    for P, Q in ((3, 2), (3, 1)):  # (downward: every output count is reachable)
        x, want = clip_and_whole(8000, 40, P, Q)
        for count in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
            first = next(c for c in range(1, 8000) if st.lib.tt_rss_ready(0, c, P, Q, 0) == count)
            for with_last in (True, False):
                assert same_bits(stream(st, x, P, Q, [first, 8000 - first], with_last), want), (form, P, Q, count)
        # ... and a clip whose flush brings the total to such a count
        for count in (T - 1, T, T + 1):
            n = next(n for n in range(1, 5000) if R.out_samples(n, P, Q) == count)
            x2, want2 = clip_and_whole(n, 41, P, Q)
            assert same_bits(stream(st, x2, P, Q, [n // 2, n - n // 2], True), want2) and same_bits(stream(st, x2, P, Q, [n], False), want2)


def test_the_bank_form_equals_the_table_form_and_auto_serves_every_ratio():
    tb, bk, au = stage("table"), stage("bank"), stage("auto")
    for i, (P, Q) in enumerate(COMMON + ((160, 147), (1, 4), (3, 4))):
        x = R.clip(3000, 50 + i)
        chunks = S.chunking(3000, P, Q, i)
        opened(tb, 3, P, Q), opened(bk, 5, P, Q)
        at = 0
        for k, c in enumerate(chunks):
            a = raw_push(tb, [(3, x[at:at + c], k == len(chunks) - 1)])[0]
            b = raw_push(bk, [(5, x[at:at + c], k == len(chunks) - 1)])[0]
            assert same_bits(a, b), (P, Q, k)
            at += c
        assert state(tb, 3)[3] == E.RSS_TABLE and state(bk, 5)[3] == E.RSS_BANK
    for P, Q in ((320, 147), (77936, 65536), (55109, 65536)):  # no bank fits: a bank handle refuses at open, AUTO serves them
        assert raw_open(bk, 7, P, Q) == -1 and b"does not fit" in bk.lib.tt_last_error()
        x, want = clip_and_whole(2000, 60, P, Q)
        assert same_bits(stream(au, x, P, Q, S.chunking(2000, P, Q, 3), True), want) and _form_of(au, P, Q) == E.RSS_TABLE
    for P, Q in COMMON:
        x, want = clip_and_whole(2000, 61, P, Q)
        assert same_bits(stream(au, x, P, Q, S.chunking(2000, P, Q, 4), False), want)
        assert _form_of(au, P, Q) == (E.RSS_BANK if Q <= E.RSS_AUTO_MAX_Q else E.RSS_TABLE)


def _form_of(st, P, Q):
    opened(st, 9, P, Q)
    return state(st, 9)[3]


def test_every_streamed_sample_lies_inside_the_fp64_bound():
    """Independent of tt_rs_resample: the reference's own derived bound per sample (the whole-clip kernel uses 0.126 of it)."""
    worst = {}
    for form in FORMS:
        st = stage(form)
        for i, (n, P, Q) in enumerate(((5000, 3, 1), (5000, 3, 2), (3000, 1, 2), (3000, 80, 147), (2000, 8, 1), (700, 1, 8), (3000, 77936, 65536))):
            if form == "bank" and not S.bank_fits(P, Q):
                continue
            x = R.clip(n, 70 + i)
            y, b = R.resample(x, P, Q)
            got = stream(st, x, P, Q, S.chunking(n, P, Q, i), True)
            share = np.abs(got.astype(np.float64) - y) / b
            assert got.shape == y.shape and (share <= 1.0).all(), (form, n, P, Q, int(share.argmax()), float(share.max()))
            worst[form] = max(worst.get(form, 0.0), float(share.max()))
    for form in FORMS:
        print(f"[parity] tt_rss_push {form} form: worst share of the fp64 sample bound used {worst[form]:.3f}")


def test_ragged_pushes_of_sixteen_slots_equal_streaming_alone():
    st = stage("auto")
    ratios = (COMMON + R.RATIOS + R.EXTREME_RATIOS + ((160, 147), (320, 147), (3, 4), (1, 4)))[:16]
    assert len(ratios) == 16
    rng = np.random.default_rng(5)
    clips = []
    for s, (P, Q) in enumerate(ratios):
        n = int(rng.integers(1, 2500)) if (P, Q) not in R.EXTREME_RATIOS else int(rng.integers(1, 900))
        clips.append(clip_and_whole(n, 80 + s, P, Q) + (S.chunking(n, P, Q, s),))
        opened(st, s, P, Q)
    at, k, got, first_round = [0] * 16, [0] * 16, [[] for _ in range(16)], True
    while any(k[s] <= len(clips[s][2]) for s in range(16)):
        live = [s for s in range(16) if k[s] <= len(clips[s][2])]
        named = [s for s in live if first_round or rng.random() < 0.6] or live[:1]  # the first push names all sixteen
        first_round = False
        rng.shuffle(named)
        items = []
        for s in named:
            x, _, chunks = clips[s]
            c = chunks[k[s]] if k[s] < len(chunks) else 0
            items.append((s, x[at[s]:at[s] + c], k[s] == len(chunks)))  # the flush is a push of its own
        before = {s: state(st, s) for s in live if s not in named}
        for s, y in zip(named, raw_push(st, items)):
            got[s].append(y)
            at[s] += len(items[named.index(s)][1])
            k[s] += 1
        assert all(state(st, s) == v for s, v in before.items())  # slots not named: untouched (their bits follow below)
    for s in range(16):
        assert same_bits(np.concatenate(got[s]), clips[s][1]), (s, ratios[s])
    # a slot that another clip went through reproduces a fresh slot's bits
    x, want = clip_and_whole(1500, 99, 80, 147)
    assert same_bits(stream(st, x, 80, 147, S.chunking(1500, 80, 147, 1), True, slot=11), want)
    x, want = clip_and_whole(1500, 98, 3, 1)
    assert same_bits(stream(st, x, 3, 1, S.chunking(1500, 3, 1, 2), False, slot=11), want)
    # all-zero input gives +0
    for form in FORMS:
        for n, P, Q in ((3000, 3, 2), (1025, 1, 2), (1, 8, 1), (1, 1, 8)):
            y = stream(stage(form), np.zeros(n, np.float32), P, Q, [n // 2, n - n // 2], False)
            assert y.tobytes() == np.zeros(R.out_samples(n, P, Q), np.float32).tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_refusals_leave_the_state_as_it_was(form):
    """Every refused call is followed by the rest of the streams: their bits are those of the whole clips."""
    st = stage(form)
    for s in range(16):
        E.check(st.lib.tt_rss_close(st.h, s))
    xa, wa = clip_and_whole(2000, 90, 3, 1)
    xb, wb = clip_and_whole(1500, 91, 1, 2)
    opened(st, 0, 3, 1), opened(st, 1, 1, 2)
    ga, gb = raw_push(st, [(0, xa[:700], False), (1, xb[:400], False)])
    opened(st, 2, 3, 2)
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
    for n_chunk, what in ((-1, b"a chunk of -1"), (E.RS_MAX_SAMPLES - 700 + 1, b"exceed a stream's")):
        assert st.lib.tt_rss_push(st.h, 2, arr(1, 0), arr(0, n_chunk), arr(0, 0), E.ptr(y), E.ptr(y), E.stream_ptr()) == -1
        assert what in st.lib.tt_last_error() and (state(st, 0), state(st, 1), state(st, 2)) == keep and (y.cpu() == SENT).all()
    assert st.lib.tt_rss_ready(700, E.RS_MAX_SAMPLES - 700 + 1, 3, 1, 0) == -1 and st.lib.tt_rss_ready(700, E.RS_MAX_SAMPLES - 700, 3, 1, 1) > 0
    # a bad ratio at open: refused, and the open slot it named keeps streaming
    for P, Q in ((9, 1), (6, 4), (0, 1), (1, 0)):
        assert raw_open(st, 0, P, Q) == -1 and b"ratio" in st.lib.tt_last_error() and state(st, 0) == keep[0]
    assert raw_open(st, 16, 3, 1) == -1 and raw_open(st, -1, 3, 1) == -1 and st.lib.tt_rss_close(st.h, 16) == -1
    assert st.lib.tt_rss_push(st.h, 1, arr(0, 0), arr(1, 0), arr(0, 0), None, E.ptr(y), E.stream_ptr()) == -1 and b"null argument" in st.lib.tt_last_error()
    ga2, gb2 = raw_push(st, [(0, xa[700:], True), (1, xb[400:], True)])
    assert same_bits(np.concatenate([ga, ga2]), wa) and same_bits(np.concatenate([gb, gb2]), wb)
    # a finished slot takes a new stream after tt_rss_open
    assert same_bits(stream(st, xb, 1, 2, [1500], True, slot=2), wb)
    assert stages.StreamResampleStage.FORMS[form] and st.lib.tt_rss_create(0, 0, C.byref(E.vp())) == -1 and st.lib.tt_rss_create(65, 0, C.byref(E.vp())) == -1
    assert st.lib.tt_rss_create(4, 3, C.byref(E.vp())) == -1


# ------------------------------------------------------------------------------------------------- the API
def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


@torch.no_grad()
def test_open_resampler_equals_resample():
    h = _host()
    x = torch.from_numpy(R.clip(5000, 2))
    want = h.resample(x.to(DEV), 44100)
    with h.open_resampler(44100) as r:
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900].to(DEV)), r.push(x[1900:4999]), r.finish(x[4999:])]
        assert got[0].shape == (0,) and all(g.device.type == "cuda" and g.dtype == torch.float32 for g in got)
        assert (r.n_in, r.n_out) == (5000, 9188) and r.latency_seconds == 37 / 24000
    assert torch.equal(torch.cat(got).view(torch.int32), want.view(torch.int32)) and not h.stream_resampler.slots
    # the stage's own schedule (tt_rss_ready through resample.stream_ready) is the library's: push_many returned what the device wrote
    with h.open_resampler(8000) as r:
        assert torch.equal(torch.cat([r.push(x[:2500]), r.finish(x[2500:])]).view(torch.int32), h.resample(x.to(DEV), 8000).view(torch.int32))


@torch.no_grad()
def test_streams_at_another_rate_equal_resampling_the_collected_stream():
    """Weights, texts and seeds as in tests/test_gpu_hifi_batch.py (max_mel_tokens=64)."""
    from tests.test_gpu_hifi_batch import _fast_instances, _texts
    texts, seeds, cond = _texts(3)
    kw = dict(conditioning_latents=(cond,), max_mel_tokens=64, stream_chunk_size=20)
    one = _fast_instances("bf16", 1)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s in zip(texts, seeds)]
    assert any(len(p) >= 2 for p in plain), "the streams of this test have several pieces"
    got = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_sample_rate=16000, **kw))
    want = one.resample(torch.cat(plain[0]), 16000)
    assert len(got) == len(plain[0]) and torch.equal(torch.cat(got).view(torch.int32), want.view(torch.int32))
    assert one._stream_stage.max_streams == 1 and not one._stream_stage.slots
    again = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_sample_rate=24000, **kw))
    assert len(again) == len(plain[0]) and all(torch.equal(a, b) for a, b in zip(again, plain[0]))
    # three texts on two slots, a rate each (None: today's bits): one text waits for a slot
    many = _fast_instances("bf16", 2)
    rates = [8000, None, 48000]
    out = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=seeds, stream_sample_rate=rates, **kw):
        out.setdefault(i, []).append((wav.clone(), done))
    assert many._stream_stage.max_streams == 2 and not many._stream_stage.slots and not many._sessions
    for i, rate in enumerate(rates):
        assert [d for _, d in out[i]] == [False] * (len(plain[i]) - 1) + [True]
        if rate is None:
            assert all(torch.equal(a, b) for (a, _), b in zip(out[i], plain[i]))
        else:
            want = one.resample(torch.cat(plain[i]), rate)
            assert torch.equal(torch.cat([a for a, _ in out[i]]).view(torch.int32), want.view(torch.int32)), (i, rate)
