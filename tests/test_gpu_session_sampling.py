"""-m gpu: streaming sessions with their own sampling settings (TT_AR_OPT_SESSION_SAMPLING, ArStage(per_session_sampling=True),
api_fast.TextToSpeech(max_streams > 1, per_session_sampling=True)).

The rule is the one of tests/test_gpu_stream_sessions.py, now per session: whatever the other rows sample with, a session's codes and
per-step latents are the bits of the same session streamed alone through a max_batch = 1 handle with ITS settings and seed.  The
scalars are device data: the handle keeps one step graph per combination of optional sampler launches (full-sort sampler, typical mask).
"""
import ctypes as C

import pytest
import torch

from oracle import make_golden_full as GF
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd.config import ARConfig, HifiganConfig
from tests.gpu_util import DTYPES

pytestmark = pytest.mark.gpu
MAXN = 96

# one session each: the defaults, a flat fast-path setting, the full-sort sampler, typical sampling, greedy with a penalty
SETTINGS = [{}, dict(temperature=0.5, top_p=0.95, repetition_penalty=1.0), dict(top_k=0), dict(typical_mass=0.9),
            dict(top_k=1, repetition_penalty=1.3)]


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def sds():
    import bench
    return bench.synthetic_weights()


def _sessions(limits=(70, 25, 60, 50, 40), settings=SETTINGS):
    """Five sessions with different texts, voice latents, seeds, lengths and settings: (admission step, cond, text, seed, tokens, settings)."""
    text, auto, _ = GF.prompt()
    g = torch.Generator().manual_seed(7)
    out = []
    for i, (at, cut, limit) in enumerate(zip([0, 0, 17, 40, None], [55, 30, 44, 20, 38], limits)):
        cond = auto * (1.0 + 0.1 * i) + 0.05 * torch.randn(auto.shape, generator=g)
        out.append((at, cond, text[:, :cut].clone(), 100 + 17 * i, limit, settings[i]))
    return out


def _alone(st, cond, text, seed, limit, settings):
    """The session on today's streaming handle (max_batch = 1) with its own settings: codes [1, n] and its per-step latents [1, n, D]."""
    st.prefill(cond, text)
    last = None
    for c, _fin in st.generate_stream(1, limit, 16, first_chunk=16, seed=seed, **settings):
        last = c.clone()
    return last, st.stream_latents(1, last.shape[1]).clone()


def _run_schedule(st, sessions, slots, events=None, own=True):
    """(As tests/test_gpu_stream_sessions.py, with every session admitted with its own settings unless own=False.)  Admissions at their
    steps, each session up to its own limit, the second one retired when done and its slot reused by the fifth.  Returns {session index:
    (codes, latents)}; `events` collects (session, finished on the device, ended inside the chunk, other sessions still running)."""
    running, results, step, queue = {}, {}, 0, list(range(len(sessions)))
    while queue or running:
        for i in list(queue):
            at = sessions[i][0]
            if (at is not None and at <= step) or (at is None and 1 in results and slots[i] not in running):
                _, cond, text, seed, _, settings = sessions[i]
                st.admit(slots[i], cond, text, seed, **(settings if own else {}))
                running[slots[i]] = i
                queue.remove(i)
        if not running:
            step += 1
            continue
        due = [sessions[i][0] for i in queue if sessions[i][0] is not None]
        n = min([sessions[i][4] - st._n[s] for s, i in running.items()] + [d - step for d in due if d > step] + [7])
        before = {s: st._n[s] for s in running}
        n_total, finished = st.advance(n)
        step += n
        for s, i in list(running.items()):
            if finished[s] or n_total[s] >= sessions[i][4]:
                if events is not None:
                    others = any(not finished[o] and n_total[o] < sessions[j][4] for o, j in running.items() if o != s)
                    events.append((i, finished[s], n_total[s] - before[s] < n, others))
                results[i] = (st.session_codes(s).clone(), st.session_latents(s, n_total[s]).clone())
                st.close(s)
                del running[s]
    return results


def _session_stage(sd, cfg, dt, max_batch=4, per_session_sampling=True):
    return stages.ArStage(sd, cfg, dtype=dt, max_batch=max_batch, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True,
                          per_session_sampling=per_session_sampling)


def _want(sd, cfg, dt, sessions):
    single = stages.ArStage(sd, cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    want = [_alone(single, s[1], s[2], s[3], s[4], s[5]) for s in sessions]
    single.close()
    return want


def _check(want, got):
    for i, (codes, lat) in enumerate(want):
        c, l_ = got[i]
        assert c.shape == codes.shape and torch.equal(c, codes), f"session {i}: codes differ from the max_batch = 1 handle"
        assert torch.equal(l_, lat), f"session {i}: latents differ from the max_batch = 1 handle"


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_mixed_settings_equal_each_session_alone(sds, lib, name, dt, tdt, tol):
    cfg = ARConfig()
    sessions = _sessions()
    want = _want(sds["autoregressive"], cfg, dt, sessions)
    st = _session_stage(sds["autoregressive"], cfg, dt)
    got = _run_schedule(st, sessions, [0, 1, 2, 3, 1])
    _check(want, got)
    captures = st.stat(0)
    assert 1 <= captures <= 4, f"{captures} step-graph captures for at most four launch combinations"
    # the same sessions in other slots and beside other neighbours: the same bits, no new capture
    got2 = _run_schedule(st, sessions, [3, 2, 0, 1, 2])
    for i in range(len(sessions)):
        assert torch.equal(got2[i][0], got[i][0]) and torch.equal(got2[i][1], got[i][1]), f"session {i}: depends on its slot"
    assert st.stat(0) == captures
    st.close()


STOP_BIASES = (3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 7.0)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_session_with_own_settings_stops_mid_chunk(lib, name, dt, tdt, tol):
    """Session 1 samples with the full-sort sampler and stops on its stop token inside a chunk while sessions with other settings keep
    running (the stop logit raised as tests/test_gpu_stream_sessions.py does); its slot is then reused by the fifth session."""
    from tortoise_tts_amd import weights as W
    cfg = ARConfig()
    sessions = _sessions((70, 60, 60, 50, 40), settings=[SETTINGS[3], dict(top_k=0), SETTINGS[1], SETTINGS[0], SETTINGS[4]])
    base = W.synthetic_state_dict(W.ar_manifest(cfg), 1234)
    stop = cfg.stop_mel_token
    for extra in STOP_BIASES:
        sd = dict(base)
        b = sd["mel_head.bias"].clone()
        b[stop] += extra
        sd["mel_head.bias"] = b
        want = _want(sd, cfg, dt, sessions)
        if not (int(want[1][0][0, -1]) == stop and want[1][0].shape[1] < sessions[1][4]):
            continue
        st = _session_stage(sd, cfg, dt)
        events = []
        got = _run_schedule(st, sessions, [0, 1, 2, 3, 1], events)
        st.close()
        ended = {i: (fin, mid, others) for i, fin, mid, others in events}
        if all(ended[1]):
            break
    else:
        pytest.fail(f"no stop-logit raise in {STOP_BIASES} makes session 1 stop inside a chunk beside running sessions")
    assert int(got[1][0][0, -1]) == stop and got[1][0].shape[1] < sessions[1][4]
    _check(want, got)


def _chunk_raw(st, n, entries):
    """tt_ar_generate_chunk with hand-made per-slot entries (what advance() builds from the admissions)."""
    S = st.max_batch
    s = (E.Sampling * S)()
    for r, e in enumerate(entries):
        s[r].temperature, s[r].top_p, s[r].repetition_penalty, s[r].top_k, s[r].typical_mass = e[:5]
        s[r].seed, s[r].row_offset, s[r].exp_noise, s[r].group_seeds = e[5], 0, e[6], None
    n_total, fin = (C.c_int * S)(), (C.c_int * S)()
    E.check(st.lib.tt_ar_generate_chunk(st.h, S, 0, int(n), st.max_new, s, E.ptr(st._codes), n_total, fin, E.stream_ptr()))


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES[:1])
@torch.no_grad()
def test_refusals_leave_running_sessions_unchanged(sds, lib, name, dt, tdt, tol):
    cfg = ARConfig()
    _, cond, text, seed, _, _ = _sessions()[0]
    own = SETTINGS[3]  # typical sampling
    want = _want(sds["autoregressive"], cfg, dt, [(0, cond, text, seed, 48, own)])[0]
    st = _session_stage(sds["autoregressive"], cfg, dt, max_batch=2)
    st.admit(1, cond, text, seed, **own)
    st.advance(20)
    captures = st.stat(0)
    started = st._settings[1]
    # a running slot's settings changed (scalars, or its key)
    for changed in (dict(temperature=0.5), dict(top_k=0)):
        st._settings[1] = stages.session_sampling(**dict(own, **changed))
        with pytest.raises(E.EngineError, match="slot 1: sampling settings differ"):
            st.advance(4)
    st._settings[1] = started
    st._seeds[1] = seed + 1
    with pytest.raises(E.EngineError, match="slot 1: sampling settings differ"):
        st.advance(4)
    st._seeds[1] = seed
    # an invalid value in a pending slot's entry
    st.admit(0, cond, text, seed)
    for bad in ((0.0, 0.8, 2.0, 50, 0.0), (0.8, 0.8, -1.0, 50, 0.0), (0.8, 0.8, 2.0, 50, 1.0)):
        st._settings[0] = bad
        with pytest.raises(E.EngineError, match="slot 0: bad sampling parameters"):
            st.advance(4)
    st._settings[0] = stages.session_sampling()
    st.close(0)
    # an injected exp_noise in the running slot's entry
    noise = torch.ones(1, device="cuda")
    entries = [stages.session_sampling() + (0, None), started + (seed, E.ptr(noise))]
    with pytest.raises(E.EngineError, match="slot 1: exp_noise"):
        _chunk_raw(st, 4, entries)
    # the option itself: twice, on a non-session handle, after an admission
    with pytest.raises(E.EngineError, match="switched on once"):
        st.set_option(E.TT_AR_OPT_SESSION_SAMPLING, 1)
    h = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    with pytest.raises(E.EngineError, match="needs a session handle"):
        h.set_option(E.TT_AR_OPT_SESSION_SAMPLING, 1)
    h.close()
    h = _session_stage(sds["autoregressive"], cfg, dt, max_batch=2, per_session_sampling=False)
    h.admit(0, cond, text, seed)
    with pytest.raises(E.EngineError, match="before the first admission"):
        h.set_option(E.TT_AR_OPT_SESSION_SAMPLING, 1)
    h.close()
    n, fin = st.advance(28)
    assert n[1] == want[0].shape[1] or fin[1]
    assert torch.equal(st.session_codes(1), want[0]) and torch.equal(st.session_latents(1, n[1]), want[1])
    assert st.stat(0) == captures
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_default_settings_match_the_plain_session_handle(sds, lib, name, dt, tdt, tol):
    cfg = ARConfig()
    sessions = _sessions(settings=[{}] * 5)[:4]
    plain = _session_stage(sds["autoregressive"], cfg, dt, per_session_sampling=False)
    want = _run_schedule(plain, sessions, [0, 1, 2, 3], own=False)
    per_step = plain.stat(2)
    plain.close()
    st = _session_stage(sds["autoregressive"], cfg, dt)
    got = _run_schedule(st, sessions, [0, 1, 2, 3])
    assert st.stat(0) == 1 and st.stat(2) == per_step
    for i in range(len(sessions)):
        assert torch.equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]), f"session {i}: differs from the plain session handle"
    st.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@torch.no_grad()
def test_open_stream_and_stream_many_with_own_settings(dtype):
    """api_fast: three staggered sessions with three settings (one typical, one full-sort) give exactly their tts_stream pieces; so does
    tts_stream_many with per-text lists."""
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    a_cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), 1234), "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    sessions = _sessions()[:3]
    own = [dict(), dict(temperature=0.6, top_p=0.9, top_k=0), dict(typical_sampling=True, typical_mass=0.85, repetition_penalty=1.5)]
    kw = dict(stream_chunk_size=20, overlap_wav_len=512)
    one = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True)
    want = [[c.cpu() for c in one.tts_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw, **o)]
            for (_, cond, t, seed, lim, _), o in zip(sessions, own)]
    shared = sessions[0][1]
    want_many = [[c.cpu() for c in one.tts_stream(t, conditioning_latents=(shared,), max_mel_tokens=60, use_deterministic_seed=seed, **kw, **o)]
                 for (_, _, t, seed, _, _), o in zip(sessions, own)]
    del one
    many = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True, max_streams=3, per_session_sampling=True)
    ids, got = {}, {}
    _, cond, t, seed, lim, _ = sessions[0]
    ids[many.open_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw, **own[0])] = 0
    pieces = 0
    for sid, wav, done in many.stream_pieces():
        got.setdefault(ids[sid], []).append(wav.cpu())
        pieces += 1
        if pieces in (1, 2):  # later admissions with other settings, between pieces of the running sessions
            _, cond, t, seed, lim, _ = sessions[pieces]
            ids[many.open_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw, **own[pieces])] = pieces
    for i in range(len(sessions)):
        assert len(got[i]) == len(want[i]), f"session {i}: {len(got[i])} pieces, tts_stream made {len(want[i])}"
        for a, b in zip(got[i], want[i]):
            assert torch.equal(a, b), f"session {i}: a piece differs from tts_stream"
    lists = {name: [o.get(name, d) for o in own] for name, d in
             (("temperature", .8), ("top_p", .8), ("repetition_penalty", 2.0), ("top_k", 50), ("typical_sampling", False), ("typical_mass", .9))}
    got_many = {}
    for i, wav, done in many.tts_stream_many([s[2] for s in sessions], conditioning_latents=(shared,), max_mel_tokens=60,
                                             use_deterministic_seed=[s[3] for s in sessions], **kw, **lists):
        got_many.setdefault(i, []).append(wav.cpu())
    for i in range(len(sessions)):
        assert len(got_many[i]) == len(want_many[i]) and all(torch.equal(a, b) for a, b in zip(got_many[i], want_many[i])), \
            f"tts_stream_many text {i}: pieces differ from tts_stream"
    assert many.ar.stat(0) <= 4
