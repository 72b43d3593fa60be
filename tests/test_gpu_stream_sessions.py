"""-m gpu: several streaming sessions in one decode batch (TT_AR_OPT_SESSIONS, api_fast.TextToSpeech(max_streams > 1)).

Batch independence is the rule: a session's codes and per-step latents do not depend on which other rows run, when they were admitted
or which slot it sits in - and they are the bits of the same session streamed alone through the max_batch = 1 handle of today's
api_fast (same seed).  The graph of the step is captured once for every admission, finish and retirement.
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


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def sds():
    import bench
    return bench.synthetic_weights()


def _sessions(limits=(70, 25, 60, 50, 40)):
    """Five sessions with different texts, voice latents, seeds and lengths: (admission step, cond, text, seed, tokens)."""
    text, auto, _ = GF.prompt()
    g = torch.Generator().manual_seed(7)
    out = []
    for i, (at, cut, limit) in enumerate(zip([0, 0, 17, 40, None], [55, 30, 44, 20, 38], limits)):
        cond = auto * (1.0 + 0.1 * i) + 0.05 * torch.randn(auto.shape, generator=g)
        out.append((at, cond, text[:, :cut].clone(), 100 + 17 * i, limit))
    return out


def _alone(st, cond, text, seed, limit):
    """The session on today's streaming handle (max_batch = 1): codes [1, n] and its per-step latents [1, n, D]."""
    st.prefill(cond, text)
    last = None
    for c, _fin in st.generate_stream(1, limit, 16, first_chunk=16, seed=seed):
        last = c.clone()
    return last, st.stream_latents(1, last.shape[1]).clone()


def _run_schedule(st, sessions, slots, events=None):
    """Drive the session handle: admissions at their steps, each session up to its own limit, the second one retired when done and its
    slot reused by the fifth.  Returns {session index: (codes, latents)}; `events` collects (session, finished on the device, ended
    inside the chunk, other sessions still running after that chunk) for every session that ended."""
    running, results, step, queue = {}, {}, 0, list(range(len(sessions)))
    while queue or running:
        for i in list(queue):
            at = sessions[i][0]
            if (at is not None and at <= step) or (at is None and 1 in results and slots[i] not in running):
                _, cond, text, seed, _ = sessions[i]
                st.admit(slots[i], cond, text, seed)
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


STOP_BIASES = (3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 7.0)  # the seed-1234 stop logit sits ~4.8 below the top one, ~3.5 below the 50th


def _stop_case(cfg, dt, sessions):
    """Weights whose stop token is sampled (tests/test_gpu_stages.py raises its logit the same way).  Of the raises in STOP_BIASES the
    first is taken at which session 1 samples its stop token before its limit, inside a chunk of the schedule, while other sessions keep
    running after that chunk - the row then finishes on the device beside running rows and its slot is reused.  Returns (the sessions
    alone on the max_batch = 1 handle, the session handle's results, the session handle, the schedule's events)."""
    from tortoise_tts_amd import weights as W
    base = W.synthetic_state_dict(W.ar_manifest(cfg), 1234)
    stop = cfg.stop_mel_token
    for extra in STOP_BIASES:
        sd = dict(base)
        b = sd["mel_head.bias"].clone()
        b[stop] += extra
        sd["mel_head.bias"] = b
        single = stages.ArStage(sd, cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
        want = [_alone(single, s[1], s[2], s[3], s[4]) for s in sessions]
        single.close()
        if not (int(want[1][0][0, -1]) == stop and want[1][0].shape[1] < sessions[1][4]):
            continue
        st = stages.ArStage(sd, cfg, dtype=dt, max_batch=4, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True)
        events = []
        got = _run_schedule(st, sessions, [0, 1, 2, 3, 1], events)
        ended = {i: (fin, mid, others) for i, fin, mid, others in events}
        if all(ended[1]):
            return want, got, st, events
        st.close()
    pytest.fail(f"no stop-logit raise in {STOP_BIASES} makes session 1 stop inside a chunk beside running sessions")


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_sessions_are_batch_independent_and_equal_the_single_stream_handle(sds, lib, name, dt, tdt, tol, stop):
    """stop=False: the stop token suppressed, sessions end at their own limits.  stop=True: sessions sample their stop tokens - the row
    finishes on the device (per-row stop detection, SESS_FINISHED, an idle row beside running ones, the stop token counted), inside a
    chunk while others keep running, and its slot is reused by the fifth session."""
    cfg = ARConfig()
    sessions = _sessions((70, 60, 60, 50, 40) if stop else (70, 25, 60, 50, 40))
    if stop:
        want, got, st, events = _stop_case(cfg, dt, sessions)
        assert int(got[1][0][0, -1]) == cfg.stop_mel_token and got[1][0].shape[1] < sessions[1][4]  # the stop token is counted
    else:
        single = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
        want = [_alone(single, s[1], s[2], s[3], s[4]) for s in sessions]
        single.close()
        st = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=4, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True)
        got = _run_schedule(st, sessions, [0, 1, 2, 3, 1])
    assert st.stat(0) == 1, "admissions / retirements re-captured the step graph"
    for i, (codes, lat) in enumerate(want):
        c, l_ = got[i]
        assert c.shape == codes.shape and torch.equal(c, codes), f"session {i}: codes differ from the max_batch = 1 handle"
        assert torch.equal(l_, lat), f"session {i}: latents differ from the max_batch = 1 handle"
    # the same sessions in other slots, and session 2 alone on the handle
    got2 = _run_schedule(st, sessions, [3, 2, 0, 1, 2])
    for i in range(len(sessions)):
        assert torch.equal(got2[i][0], got[i][0]) and torch.equal(got2[i][1], got[i][1]), f"session {i}: depends on its slot"
    _, cond, text, seed, limit = sessions[2]
    alone = _run_schedule(st, [(0, cond, text, seed, limit)], [3])
    assert torch.equal(alone[0][0], got[2][0]) and torch.equal(alone[0][1], got[2][1])
    assert st.stat(0) == 1
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES[:1])
@torch.no_grad()
def test_rejected_admissions_and_calls_leave_running_sessions_unchanged(sds, lib, name, dt, tdt, tol):
    cfg = ARConfig()
    _, cond, text, seed, _ = _sessions()[0]
    single = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    codes, lat = _alone(single, cond, text, seed, 48)
    single.close()
    st = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=2, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True)
    st.admit(1, cond, text, seed)
    st.advance(20)
    with pytest.raises(E.EngineError, match="holds a session"):
        st.admit(1, cond, text, seed)
    with pytest.raises(E.EngineError, match="exceeds capacity"):
        st.admit(0, cond, torch.ones(1, 120, dtype=torch.int32), seed)
    with pytest.raises(E.EngineError, match="differ"):
        st.advance(4, temperature=0.5)
    with pytest.raises(E.EngineError, match="exceed capacity"):
        st.advance(MAXN)
    with pytest.raises(E.EngineError, match="generate_chunk"):
        st.generate(1, 8)
    with pytest.raises(E.EngineError, match="no session"):
        st.close(0)
    n, fin = st.advance(28)
    assert n[1] == codes.shape[1] or fin[1]
    assert torch.equal(st.session_codes(1), codes) and torch.equal(st.session_latents(1, n[1]), lat)
    assert st.stat(0) == 1
    st.close()
    # opting in is refused on handles that do not qualify, and after the first prefill
    for kw in (dict(max_batch=5), dict(max_batch=2, max_groups=1)):
        h = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, **kw)
        with pytest.raises(E.EngineError, match="sessions need"):
            h.set_option(E.TT_AR_OPT_SESSIONS, 1)
        h.close()
    h = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    h.prefill(cond, text)
    with pytest.raises(E.EngineError, match="before the first prefill"):
        h.set_option(E.TT_AR_OPT_SESSIONS, 1)
    h.close()


def _decode_attention_reference(q, kp, vp, k_own, v_own):
    k = torch.cat([kp, k_own], dim=1)
    v = torch.cat([vp, v_own], dim=1)
    w = torch.einsum("hd,hkd->hk", q, k)
    return torch.einsum("hk,hkd->hd", torch.softmax(w, dim=-1), v)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("tgens", [(1, 64, -1, 500), (65, 127, 128, 3), (200, 1, 499, 64)])
def test_per_row_decode_attention_operator(lib, name, dt, tdt, tol, tgens):
    """tt_op_decode_attention_rows: four rows with unequal prefix lengths and 1 .. 500 own keys (-1: a row that does not decode - its output
    row stays untouched) against torch fp32 from the same rounded operands."""
    H, B, tmax, cap = 16, 4, 504, 190
    p1s = [59, 190, 7, 120]
    g = torch.Generator().manual_seed(sum(tgens) + dt)
    q = (torch.randn(B, H, 64, generator=g) * 0.25).to(tdt)
    kp = torch.zeros(B, H * cap * 64, dtype=tdt)
    vp = torch.zeros_like(kp)
    kc = (torch.randn(B, H, tmax, 64, generator=g)).to(tdt)
    vc = (torch.randn(B, H, tmax, 64, generator=g)).to(tdt)
    refs = []
    for b in range(B):
        P1 = p1s[b]
        k_ = torch.randn(H, P1, 64, generator=g).to(tdt)
        v_ = torch.randn(H, P1, 64, generator=g).to(tdt)
        kp[b, :H * P1 * 64] = k_.reshape(-1)
        vp[b, :H * P1 * 64] = v_.reshape(-1)
        t = tgens[b]
        refs.append(None if t < 0 else _decode_attention_reference(q[b].float(), k_.float(), v_.float(), kc[b, :, :t].float(), vc[b, :, :t].float()))
    kc_chunk = kc.reshape(B, H, tmax, 8, 8).permute(0, 1, 3, 2, 4).contiguous()  # [B][H][8 chunks][tmax][8]
    dev = torch.device("cuda")
    q_d, kp_d, vp_d, kc_d, vc_d = (x.to(dev).contiguous() for x in (q, kp, vp, kc_chunk, vc))
    p1_d = torch.tensor(p1s, dtype=torch.int32, device=dev)
    slot_d = torch.tensor([t - 1 if t > 0 else -1 for t in tgens], dtype=torch.int32, device=dev)
    out = torch.full((B, H * 64), 7.0, dtype=tdt, device=dev)
    E.check(lib.tt_op_decode_attention_rows(dt, E.ptr(q_d), E.ptr(kp_d), E.ptr(vp_d), C.c_longlong(H * cap * 64), E.ptr(p1_d), cap, E.ptr(kc_d), E.ptr(vc_d), tmax,
                                            E.ptr(slot_d), E.ptr(out), B, H, None))
    out = out.cpu().float()
    for b in range(B):
        if refs[b] is None:
            assert torch.all(out[b] == 7.0), "a row that does not decode was written"
            continue
        want = refs[b].reshape(-1)
        rel = float((out[b] - want).norm() / want.norm())
        assert rel < tol, f"row {b} (P1={p1s[b]}, {tgens[b]} own keys): rel_l2 {rel:.3e}"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@torch.no_grad()
def test_stream_pieces_equal_tts_stream_per_session(dtype):
    """api_fast.TextToSpeech(max_streams=3): staggered sessions through stream_pieces() give every session exactly its tts_stream pieces."""
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    a_cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), 1234), "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    sessions = _sessions()[:3]
    kw = dict(stream_chunk_size=20, overlap_wav_len=512)
    one = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True)
    want = [[c.cpu() for c in one.tts_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw)]
            for _, cond, t, seed, lim in sessions]
    del one
    many = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True, max_streams=3)
    ids, got = {}, {}
    _, cond, t, seed, lim = sessions[0]
    ids[many.open_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw)] = 0
    pieces = 0
    for sid, wav, done in many.stream_pieces():
        got.setdefault(ids[sid], []).append(wav.cpu())
        pieces += 1
        if pieces in (1, 2):  # later admissions, between pieces of the running sessions
            _, cond, t, seed, lim = sessions[pieces]
            ids[many.open_stream(t, conditioning_latents=(cond,), max_mel_tokens=lim, use_deterministic_seed=seed, **kw)] = pieces
    assert many.ar.stat(0) == 1
    for i in range(len(sessions)):
        assert len(got[i]) == len(want[i]), f"session {i}: {len(got[i])} pieces, tts_stream made {len(want[i])}"
        for a, b in zip(got[i], want[i]):
            assert torch.equal(a, b), f"session {i}: a piece differs from tts_stream"
