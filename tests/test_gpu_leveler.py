"""The streaming leveler on the MI355X (csrc/loudness_stream.hip, include/tortoise_mi355x_lvs.h).

  chunking   whatever the chunking, a stream's samples, per-hop trace and readings are byte-identical to one flushed push of the clip.
  ragged     sixteen ragged slots with mixed modes in one push per round are byte-identical to each stream alone, on another handle too.
  anchors    bit for bit against the verified whole-clip code: q_h = tt_loud_measure's hop energies; L_h and the block counts =
             tt_loud_measure of the prefix; FIXED + LOOKAHEAD = tt_loud_normalize(LOOKAHEAD)'s samples at its gain; FIXED + NONE = f32(g x).
  bounds     every q, L, G, gl and y of every shared stream inside the bound tests/leveler_reference.py derives.
  readings   the peaks and the limited count against the device's own output.
  refusals   change nothing, and the stream goes on."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import leveler_reference as V
from tests import loudness_reference as R
from tests.test_gpu_loudness import device_call
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOPS = 64  # the handles hold streams of up to 6.4 s: 153 600 samples

_stages = {}


def stage(max_streams=16):
    if max_streams not in _stages:
        _stages[max_streams] = stages.StreamLevelStage(max_streams, max_hops=HOPS, device=DEV)
    return _stages[max_streams]


def run(st, jobs):
    """jobs = [(x, Options, [(chunk length, flush)])] -> per job dict(y, trace..., gl, read): every round is ONE push of the next chunk of
    every stream that still has one."""
    slots = [st.open(o) for _, o, _ in jobs]
    pos, outs, step = [0] * len(jobs), [[] for _ in jobs], 0
    while True:
        items, who = [], []
        for j, (x, o, chunks) in enumerate(jobs):
            if step < len(chunks):
                c, fl = chunks[step]
                want = V.ready(pos[j], c, o.limit, fl)
                items.append((slots[j], torch.from_numpy(np.array(x[pos[j]:pos[j] + c])), fl))
                who.append((j, c, want))
        if not items:
            break
        for (j, c, want), y in zip(who, st.push_many(items)):
            assert y.shape[0] == want
            outs[j].append(y)
            pos[j] += c
        step += 1
    res = []
    for j, (x, o, chunks) in enumerate(jobs):
        assert pos[j] == len(x)
        rd, tr = st.read(slots[j]), st.trace(slots[j])
        assert rd["n_in"] == rd["n_out"] == len(x) and rd["hops"] == len(x) // V.H
        gl = np.full(rd["hops"] + 2, np.float32(o.gain0), np.float32)
        res.append(dict(y=torch.cat(outs[j]).cpu().numpy(), q=tr["q"], L=tr["lufs"], G=tr["gain_db"], status=tr["status"], blocks_abs=tr["blocks_abs"],
                        blocks_rel=tr["blocks_rel"], read=rd, gl=gl if o.steer == V.FIXED else None))
        st.close(slots[j])
    return res


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("y", "q", "L", "G", "status", "blocks_abs", "blocks_rel")) and a["read"] == b["read"]


def whole(x):
    return [(len(x), True)]


@pytest.fixture(scope="module")
def solo():
    """Every shared stream, ADAPT and FIXED, as one flushed push on its own."""
    st = stage()
    return {(i, fx): run(st, [(x, V.stream_settings(i)[fx], whole(x))])[0] for i, (x, _) in enumerate(V.streams()) for fx in (0, 1)}


CHUNKED = (1, 12, 15, 20, 23, 24, 25, 26, 27, 28, 29)  # n = 2399, 19201, 120000 and every length around the segment, D, history and tile


@pytest.mark.parametrize("fx", (0, 1))
def test_chunk_invariance(solo, fx):
    st, S = stage(), V.streams()
    tried = 0
    x700 = S[1][0][:700]
    jobs = [(i, S[i][0]) for i in CHUNKED] + [(None, x700)]
    for i, x in jobs:
        o = V.stream_settings(i if i is not None else 0)[fx]
        ref = solo[(i, fx)] if i is not None else run(st, [(x, o, whole(x))])[0]
        for name, chunks in V.chunkings(len(x)).items():
            assert sum(c for c, _ in chunks) == len(x) and chunks[-1][1]
            got = run(st, [(x, o, chunks)])[0]
            assert same(got, ref), (len(x), name)
            assert got["y"].view(np.int32).tobytes() == ref["y"].view(np.int32).tobytes()
            tried += 1
    assert tried >= 60


def test_ragged_slots(solo):
    S = V.streams()
    picks = [(i, i % 2) for i in (15, 13, 12, 8, 4, 1, 0, 20, 22, 23, 25, 26, 27, 29, 16, 19)]
    rng = np.random.default_rng(5)
    jobs = []
    for i, fx in picks:
        x, n = S[i][0], len(S[i][0])
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 6))))
        sizes = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
        jobs.append((x, V.stream_settings(i)[fx], [(int(c), k == len(sizes) - 1) for k, c in enumerate(sizes)]))
    for st in (stage(16), stage(23)):
        got = run(st, jobs)
        for (i, fx), g in zip(picks, got):
            assert same(g, solo[(i, fx)]), (i, fx, st.max_streams)


def test_anchor_hop_energies_and_prefix_loudness(solo):
    S = V.streams()
    for i in range(len(R.FAMILY)):
        x = S[i][0]
        w = device_call([(x, -23.0, 1.0)])[0]
        assert solo[(i, 0)]["q"].tobytes() == w["hop_energy"][:len(x) // V.H].tobytes(), len(x)
    checked = 0
    for i in (12, 14, 15):  # 19201, 72000 and 120000 samples: every h >= 3
        x, s = S[i][0], solo[(i, 1)]
        hops = list(range(3, len(x) // V.H))
        for k in range(0, len(hops), 12):
            part = hops[k:k + 12]
            for h, w in zip(part, device_call([(x[:(h + 1) * V.H], -23.0, 1.0) for h in part])):
                assert np.float64(w["lufs"]).tobytes() == s["L"][h].tobytes(), (len(x), h)
                assert (w["blocks_abs"], w["blocks_rel"], w["status"]) == (s["blocks_abs"][h], s["blocks_rel"][h], s["status"][h]), (len(x), h)
                checked += 1
    assert checked == 5 + 27 + 47


def test_anchor_fixed_gain_is_the_whole_clip_limiter():
    st, fam = stage(), R.family_reference()
    done = 0
    for x, T, c, m in fam:
        if m["status"] != R.OK:
            continue
        w = device_call([(x, T, c)], R.LOOKAHEAD)[0]
        g = float(w["gain"])
        got = run(st, [(x, V.Options(V.FIXED, V.LOOKAHEAD, g, T, c), V.chunkings(len(x))["random"])])[0]
        assert got["y"].tobytes() == w["y"].tobytes(), len(x)
        plain = run(st, [(x, V.Options(V.FIXED, V.NONE, g, T, c), V.chunkings(len(x))["random"])])[0]
        assert plain["y"].tobytes() == (np.float32(g) * x).tobytes(), len(x)
        done += 1
    assert done >= 10


def test_bounds(solo):
    S = V.streams()
    worst, lim = {}, 0
    for i, (x, _) in enumerate(S):
        for fx in (0, 1):
            o = V.stream_settings(i)[fx]
            ref = V.stream_reference(i, bool(fx))
            got = dict(solo[(i, fx)])
            if o.steer == V.ADAPT:  # gl_h: the last one is read back; every one shows in y
                got["gl"] = None
                if len(ref["G"]):
                    assert abs(float(np.float32(got["read"]["gain"])) - ref["gl"][-1]) <= ref["glb"][-1]
                    worst["gl"] = max(worst.get("gl", 0.0), V.share(abs(float(np.float32(got["read"]["gain"])) - ref["gl"][-1]), ref["glb"][-1]))
            for k, v in V.verify(got, ref, x, o).items():
                worst[k] = max(worst.get(k, 0.0), v)
            lim += bool(ref["limited"].any())
    assert lim >= 8
    print("[parity] tt_lvs_push: %d streams x 2 settings; worst share of the bound used: " % len(S) + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


def test_readings(solo):
    S = V.streams()
    seen = 0
    for i, (x, _) in enumerate(S):
        for fx in (0, 1):
            o, s, ref = V.stream_settings(i)[fx].f32(), solo[(i, fx)], V.stream_reference(i, bool(fx))
            rd = s["read"]
            assert np.float32(rd["out_peak"]).tobytes() == np.abs(s["y"]).max().tobytes()
            if o.limit == V.NONE:
                assert rd["peak"] == 0.0 and rd["limited"] == 0
                continue
            assert np.float32(rd["peak"]).tobytes() == np.float32(device_call([(x, -23.0, 1.0)])[0]["true_peak"]).tobytes(), len(x)
            # s < 1 surely where the sample differs from g x (FIXED: g is known exactly), never where nothing can limit
            upper = int((~ref["free"]).sum())
            lower = int((s["y"] != np.float32(o.gain0) * x).sum()) if o.steer == V.FIXED else 0
            assert lower <= rd["limited"] <= upper, (len(x), lower, rd["limited"], upper)
            seen += rd["limited"] > 0
    assert seen >= 8


def test_refusals_change_nothing():
    st, lib = stage(), stage().lib
    x = V.streams()[12][0]
    o = V.stream_settings(12)[0]
    ref = run(st, [(x, o, whole(x))])[0]
    a, b, fin = st.open(o), st.open(V.stream_settings(12)[1]), st.open(o)
    st.push_many([(fin, torch.from_numpy(x[:100].copy()), True)])
    y0 = st.push_many([(a, torch.from_numpy(x[:5000].copy()), False)])[0]
    free = [s for s in range(st.max_streams) if s not in st.slots][0]
    arr = lambda *v: (C.c_int * len(v))(*v)
    buf = torch.zeros(200000, device=DEV)

    def state():
        out = []
        for s in (a, b, fin):
            v = [C.c_int() for _ in range(4)]
            E.check(lib.tt_lvs_state(st.h, s, *[C.byref(k) for k in v]))
            out.append(tuple(k.value for k in v))
        return out

    keep = state()
    push = lambda ids, nc, fl: lib.tt_lvs_push(st.h, len(ids), arr(*ids), arr(*nc), arr(*fl), E.ptr(buf), E.ptr(buf[100000:]), E.stream_ptr())
    for ids, nc, fl, what in (((a, fin), (10, 10), (0, 0), b"finished"), ((a, free), (10, 10), (0, 0), b"closed"), ((a, a), (10, 10), (0, 0), b"twice"),
                              ((b, a), (10, -1), (0, 0), b"a chunk of -1"), ((b, a), (10, HOPS * V.H), (0, 0), b"pass the handle's"),
                              ((a, st.max_streams), (10, 10), (0, 0), b"slot")):
        assert push(ids, nc, fl) == -1 and what in lib.tt_last_error() and state() == keep, what
    f = C.c_float
    good = [V.ADAPT, V.LOOKAHEAD, 1.0, -23.0, 0.9, 12.0, 24.0, 3.0, 12.0]
    for at, bad in ((3, math.nan), (3, math.inf), (4, 0.0), (4, -1.0), (4, math.nan), (7, -1.0), (8, -0.5), (5, -1.0), (6, math.nan), (2, 0.0), (0, 2), (1, 2)):
        args = list(good)
        args[at] = bad
        assert lib.tt_lvs_open(st.h, a, *args[:2], *[f(v) for v in args[2:]]) == -1 and state() == keep, (at, bad)
    assert lib.tt_lvs_open(st.h, st.max_streams, *good[:2], *[f(v) for v in good[2:]]) == -1 and lib.tt_lvs_close(st.h, -1) == -1
    assert lib.tt_lvs_create(0, 0, C.byref(E.vp())) == -1 and lib.tt_lvs_create(65, 0, C.byref(E.vp())) == -1
    assert lib.tt_lvs_create(1, E.LVS_MAX_HOPS + 1, C.byref(E.vp())) == -1 and lib.tt_lvs_ready(0, -1, 1, 0) == -1
    with pytest.raises(ValueError):
        st.push_many([(a, torch.zeros(10), False), (a, torch.zeros(10), False)])
    # the rest of the stream goes through
    y1 = st.push_many([(a, torch.from_numpy(x[5000:].copy()), True)])[0]
    assert torch.cat([y0, y1]).cpu().numpy().tobytes() == ref["y"].tobytes()
    assert st.trace(a)["gain_db"].tobytes() == ref["G"].tobytes()
    for s in (a, b, fin):
        st.close(s)
    assert not st.slots


# ------------------------------------------------------------------------------------------------- the API
def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


@torch.no_grad()
def test_open_leveler_equals_level_and_the_stage():
    h = _host()
    x = torch.from_numpy(np.array(V.streams()[15][0]))
    o = V.stream_settings(15)[0]  # ADAPT + LOOKAHEAD at -30 LUFS under -1 dBTP
    want, info = h.level_many([x.to(DEV)], loudness=-30.0, true_peak=-1.0, return_info=True)
    solo = run(stage(), [(x.numpy(), o, whole(x))])[0]
    assert want[0].cpu().numpy().tobytes() == solo["y"].tobytes()  # the API's settings are the stage's
    assert info[0].samples_out == len(x) and info[0].status == "ok" and info[0].limited == solo["read"]["limited"] and info[0].lufs == solo["read"]["lufs"]
    with h.open_leveler(loudness=-30.0, true_peak=-1.0) as r:
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900].to(DEV)), r.push(x[1900:90000]), r.finish(x[90000:])]
        assert got[0].shape == (0,) and all(g.device.type == "cuda" and g.dtype == torch.float32 for g in got)
        assert (r.n_in, r.n_out) == (len(x), len(x)) and r.latency_seconds == 248 / 24000 and r.reading() == info[0]
    assert torch.equal(torch.cat(got).view(torch.int32), want[0].view(torch.int32)) and not h.stream_leveller.slots
    y = h.level(x.reshape(1, -1), gain=-6.0)
    assert y.shape == (1, len(x)) and y.device.type == "cpu" and y.numpy().tobytes() == (np.float32(10.0 ** (-6.0 / 20.0)) * x.numpy()).reshape(1, -1).tobytes()
    with pytest.raises(ValueError):
        h.open_leveler(loudness=-23.0, gain=0.0)
    assert not h.stream_leveller.slots


@torch.no_grad()
def test_streams_at_a_level_equal_level_of_the_plain_stream():
    """Weights, texts and seeds as in tests/test_gpu_hifi_batch.py (max_mel_tokens=64)."""
    from tests.test_gpu_hifi_batch import _fast_instances, _texts
    texts, seeds, cond = _texts(3)
    kw = dict(conditioning_latents=(cond,), max_mel_tokens=64, stream_chunk_size=20)
    one = _fast_instances("bf16", 1)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s in zip(texts, seeds)]
    assert any(len(p) >= 2 for p in plain), "the streams of this test have several pieces"
    assert one._level_stage is None  # no keyword: the stage is never constructed
    again = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_loudness=None, stream_gain=None, **kw))
    assert len(again) == len(plain[0]) and all(torch.equal(a, b) for a, b in zip(again, plain[0])) and one._level_stage is None
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_loudness=-20.0, **kw))
    assert len(got) == len(plain[0]) and eq(torch.cat(got), one.level(torch.cat(plain[0]), loudness=-20.0))
    assert one._level_stage.max_streams == 1 and not one._level_stage.slots
    # the whole chain in the documented order: stretch, pitch, LEVEL, sample rate
    opts = dict(stream_loudness=-18.0, stream_true_peak=-3.0, stream_level=dict(assume=-30.0, rise=6.0))
    got = list(one.tts_stream(texts[0], use_deterministic_seed=seeds[0], stream_speaking_rate=1.25, stream_pitch=3, stream_sample_rate=16000, **opts, **kw))
    mid = one._voiced([torch.cat(plain[0])], 1.25, 3.0, None, None)[0]
    want = one.resample(one.level(mid, loudness=-18.0, true_peak=-3.0, assume=-30.0, rise=6.0), 16000)
    assert len(got) == len(plain[0]) and eq(torch.cat(got), want)
    assert not one._level_stage.slots and not one._stretch_stage.slots and not one._pitch_stage.slots and not one._stream_stage.slots
    # three sessions with different settings: open_stream / stream_pieces, then tts_stream_many with values per text
    many = _fast_instances("bf16", 3)
    settings = [dict(stream_loudness=-16.0), dict(stream_gain=2.0, stream_true_peak=-2.0), dict(stream_loudness=-30.0, stream_limit="none")]
    level_kw = [dict(loudness=-16.0), dict(gain=2.0, true_peak=-2.0), dict(loudness=-30.0, limit="none")]
    sids = [many.open_stream(t, use_deterministic_seed=s, **o, **kw) for t, s, o in zip(texts, seeds, settings)]
    out = {sid: [] for sid in sids}
    for sid, wav, done in many.stream_pieces():
        out[sid].append((wav.clone(), done))
    for i, sid in enumerate(sids):
        assert [d for _, d in out[sid]] == [False] * (len(plain[i]) - 1) + [True]
        assert eq(torch.cat([a for a, _ in out[sid]]), one.level(torch.cat(plain[i]), **level_kw[i])), i
    assert many._level_stage.max_streams == 3 and not many._level_stage.slots and not many._sessions
    res = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=seeds, stream_loudness=[-16.0, None, -30.0], stream_limit=[None, None, "none"], **kw):
        res.setdefault(i, []).append(wav.clone())
    assert eq(torch.cat(res[0]), one.level(torch.cat(plain[0]), loudness=-16.0)) and eq(torch.cat(res[2]), one.level(torch.cat(plain[2]), loudness=-30.0, limit="none"))
    assert all(torch.equal(a, b) for a, b in zip(res[1], plain[1])) and not many._level_stage.slots
    for fn in (lambda **k: next(one.tts_stream(texts[0], **k, **kw)), lambda **k: many.open_stream(texts[0], **k, **kw)):
        with pytest.raises(ValueError, match="loudness is not available for streamed audio"):
            fn(loudness=-23.0)
