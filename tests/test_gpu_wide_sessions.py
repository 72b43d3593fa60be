"""-m gpu: wide session handles (TT_AR_OPT_SESSIONS = 2, ArStage(sessions=True, max_batch=5 .. 16),
api_fast.TextToSpeech(max_streams=2 .. 16, wide_sessions=True)).

The GEMV decode step takes 5 .. 16 rows (csrc/gemv.hip gemv_rows_kernel): output (r, c) of an M-row launch is the bits of output (0, c)
of a 1-row launch on row r alone.  On top of it a session on a 16-row handle computes exactly what it computes alone on the max_batch = 1
handle, whatever the other fifteen rows do, and admissions, finishes and retirements replay one kept step graph.
"""
import math

import pytest
import torch

from oracle import make_golden_full as GF
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd.config import ARConfig, HifiganConfig
from tests.gpu_util import DTYPES, report

pytestmark = pytest.mark.gpu
MAXN = 96
WIDE = 16


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def sds():
    import bench
    return bench.synthetic_weights()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("M", [5, 8, 13, 16])
def test_gemv_rows_equal_their_single_row_launches(lib, name, dt, tdt, tol, M):
    """Every (N, K, epilogue) of the decode step at M = 5 .. 16: row r of the M-row launch is torch.equal to a 1-row launch on row r, and
    every row matches torch fp32 from the same rounded operands within the bars of the <= 4-row operator test."""
    g = torch.Generator().manual_seed(140 + M)
    for (N, K, epi) in ((8196, 1024, 0), (1024, 1024, 1), (1024, 4096, 1), (4096, 1024, 2)):
        A = torch.randn(M, K, generator=g).to(tdt).cuda()
        Wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(tdt).cuda()
        bias = torch.randn(N, generator=g).cuda()
        x0 = torch.randn(M, N, generator=g).cuda()
        o32 = x0.clone()
        ot = torch.zeros(M, N, device="cuda", dtype=tdt)
        E.check(lib.tt_op_gemv(dt, E.ptr(A), E.ptr(Wt), M, N, K, E.ptr(bias), epi, E.ptr(o32), E.ptr(ot), None))
        for r in range(M):
            a1 = A[r:r + 1].contiguous()
            o1 = x0[r:r + 1].clone()
            t1 = torch.zeros(1, N, device="cuda", dtype=tdt)
            E.check(lib.tt_op_gemv(dt, E.ptr(a1), E.ptr(Wt), 1, N, K, E.ptr(bias), epi, E.ptr(o1), E.ptr(t1), None))
            got, want = (ot[r:r + 1], t1) if epi == 2 else (o32[r:r + 1], o1)
            assert torch.equal(got, want), f"gemv {name} M={M} N={N} K={K} epi={epi}: row {r} differs from its 1-row launch"
        torch.cuda.synchronize()
        ref = A.float() @ Wt.float().t() + bias
        if epi == 0:
            report(f"gemv {name} M={M} N={N} K={K} f32 + bias", o32, ref, 2e-5)
        elif epi == 1:
            report(f"gemv {name} M={M} N={N} K={K} residual update", o32, x0 + ref, 2e-5)
        else:
            report(f"gemv {name} M={M} N={N} K={K} bias + gelu -> T", ot.float(), torch.nn.functional.gelu(ref, approximate="tanh"), {"bf16": 4e-3, "f16": 6e-4}[name])
    # the LayerNorm in front of c_fc inside the launch
    x = (torch.randn(M, 1024, generator=g) * 3 + 0.5).cuda()
    gam = (1 + 0.2 * torch.randn(1024, generator=g)).cuda()
    bet = (0.1 * torch.randn(1024, generator=g)).cuda()
    Wt = (torch.randn(4096, 1024, generator=g) / 32).to(tdt).cuda()
    bias = torch.randn(4096, generator=g).cuda()
    ot = torch.zeros(M, 4096, device="cuda", dtype=tdt)
    E.check(lib.tt_op_gemv_ln(dt, E.ptr(x), E.ptr(gam), E.ptr(bet), 1e-5, E.ptr(Wt), M, 4096, E.ptr(bias), E.ptr(ot), None))
    for r in range(M):
        x1 = x[r:r + 1].contiguous()
        t1 = torch.zeros(1, 4096, device="cuda", dtype=tdt)
        E.check(lib.tt_op_gemv_ln(dt, E.ptr(x1), E.ptr(gam), E.ptr(bet), 1e-5, E.ptr(Wt), 1, 4096, E.ptr(bias), E.ptr(t1), None))
        assert torch.equal(ot[r:r + 1], t1), f"gemv {name} M={M} LayerNorm inside: row {r} differs from its 1-row launch"
    torch.cuda.synchronize()
    h = torch.nn.functional.layer_norm(x, (1024,), gam, bet, 1e-5).to(tdt).float()
    report(f"gemv {name} M={M} LayerNorm inside, bias + gelu -> T", ot.float(), torch.nn.functional.gelu(h @ Wt.float().t() + bias, approximate="tanh"), {"bf16": 4e-3, "f16": 6e-4}[name])
    # more than 16 rows is refused
    A = torch.zeros(17, 1024, dtype=tdt, device="cuda")
    Wt = torch.zeros(1024, 1024, dtype=tdt, device="cuda")
    o32 = torch.zeros(17, 1024, device="cuda")
    with pytest.raises(E.EngineError, match="M <= 16"):
        E.check(lib.tt_op_gemv(dt, E.ptr(A), E.ptr(Wt), 17, 1024, 1024, None, 0, E.ptr(o32), None, None))


def _sessions(n=20, settings=None):
    """n sessions with their own texts, voice latents, seeds and lengths: (admission step, cond, text, seed, tokens, settings).  The first
    three start at once (slots 0, 7, 15), the next thirteen fill the handle at staggered steps, the rest wait for a slot."""
    text, auto, _ = GF.prompt()
    g = torch.Generator().manual_seed(11)
    out = []
    for i in range(n):
        at = 0 if i < 3 else (i - 2 if i < WIDE else None)
        cut = 20 + (7 * i) % 37
        cond = auto * (1.0 + 0.03 * i) + 0.05 * torch.randn(auto.shape, generator=g)
        out.append((at, cond, text[:, :cut].clone(), 300 + 13 * i, 30 + (11 * i) % 41, settings[i] if settings else {}))
    return out


def _alone(st, cond, text, seed, limit, settings):
    """The session on the streaming handle of api_fast (max_batch = 1): codes [1, n] and its per-step latents [1, n, D]."""
    st.prefill(cond, text)
    last = None
    for c, _fin in st.generate_stream(1, limit, 16, first_chunk=16, seed=seed, **settings):
        last = c.clone()
    return last, st.stream_latents(1, last.shape[1]).clone()


def _run(st, sessions, own=False):
    """Drive a wide handle: the first three sessions into slots 0, 7 and 15, the others at their step (None: as soon as a slot is free)
    into the slot of the latest session that stopped on the device inside a chunk if one is free, else the lowest free slot; chunks of
    at most 7 tokens.  Returns ({session: (codes, latents)}, events): an event per session that ended -
    (session, slot, finished on the device, ended inside its chunk, others still running after that chunk); used: slot -> its sessions;
    peak: the most sessions running at once."""
    first = {0: 0, 1: 7, 2: 15}
    running, results, events, step, queue, used, peak, pref = {}, {}, [], 0, list(range(len(sessions))), {}, 0, []
    while queue or running:
        for i in list(queue):
            at = sessions[i][0]
            free = [s for s in range(st.max_batch) if s not in running]
            if not free or (at is not None and at > step) or (at is None and any(sessions[j][0] is not None for j in queue)):
                continue
            slot = first.get(i, next((s for s in pref if s in free), free[0]))
            if slot not in free:
                continue
            if slot in pref:
                pref.remove(slot)
            _, cond, text, seed, _, settings = sessions[i]
            st.admit(slot, cond, text, seed, **(settings if own else {}))
            running[slot] = i
            used.setdefault(slot, []).append(i)
            queue.remove(i)
        peak = max(peak, len(running))
        if not running:
            step += 1
            continue
        due = [sessions[i][0] - step for i in queue if sessions[i][0] is not None and sessions[i][0] > step]
        n = min([sessions[i][4] - st._n[s] for s, i in running.items()] + due + [7])
        before = {s: st._n[s] for s in running}
        n_total, finished = st.advance(n)
        step += n
        for s, i in list(running.items()):
            if finished[s] or n_total[s] >= sessions[i][4]:
                others = any(not finished[o] and n_total[o] < sessions[j][4] for o, j in running.items() if o != s)
                events.append((i, s, finished[s], n_total[s] - before[s] < n, others))
                if finished[s] and n_total[s] - before[s] < n:
                    pref.insert(0, s)
                results[i] = (st.session_codes(s).clone(), st.session_latents(s, n_total[s]).clone())
                st.close(s)
                del running[s]
    return results, events, used, peak


def _check(want, got):
    for i, (codes, lat) in enumerate(want):
        c, l_ = got[i]
        assert c.shape == codes.shape and torch.equal(c, codes), f"session {i}: codes differ from the max_batch = 1 handle"
        assert torch.equal(l_, lat), f"session {i}: latents differ from the max_batch = 1 handle"


STOP_BIASES = (4.0, 5.0, 6.0, 7.0)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_sixteen_sessions_equal_the_single_stream_handle(lib, name, dt, tdt, tol):
    """Twenty-four sessions on a 16-row handle with the stop token sampled: the first three in slots 0, 7 and 15, staggered admissions
    until every row runs, sessions that finish on the device inside a chunk beside running rows, and their slots reused by the eight
    sessions that waited.  Every session's codes and latents are the bits of the same session alone on the max_batch = 1 handle; one graph capture."""
    from tortoise_tts_amd import weights as W
    cfg = ARConfig()
    sessions = _sessions(24)
    base = W.synthetic_state_dict(W.ar_manifest(cfg), 1234)
    stop = cfg.stop_mel_token
    for extra in STOP_BIASES:
        sd = dict(base)
        b = sd["mel_head.bias"].clone()
        b[stop] += extra
        sd["mel_head.bias"] = b
        single = stages.ArStage(sd, cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
        want = [_alone(single, *s[1:5], {}) for s in sessions]
        single.close()
        if not any(int(c[0, -1]) == stop and c.shape[1] < s[4] for (c, _), s in zip(want, sessions)):
            continue
        st = stages.ArStage(sd, cfg, dtype=dt, max_batch=WIDE, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True)
        got, events, used, peak = _run(st, sessions)
        reused = {i for s, ids in used.items() if len(ids) > 1 for i in ids[:-1]}
        print(f"[wide] stop raise {extra}: peak {peak}, device finishes {[(i, mid, others) for i, _, fin, mid, others in events if fin]}, reused {sorted(reused)}")
        if peak == WIDE and any(fin and mid and others and i in reused for i, _, fin, mid, others in events):
            break
        st.close()
    else:
        pytest.fail(f"no stop-logit raise in {STOP_BIASES} makes a session stop inside a chunk beside running ones before its slot is reused "
                    "with all sixteen rows running at some point")
    assert peak == WIDE and len(used) == WIDE and max(len(ids) for ids in used.values()) >= 2
    assert st.stat(0) == 1, "admissions / finishes / retirements re-captured the step graph"
    _check(want, got)
    st.close()


SETTINGS16 = [{}, dict(temperature=0.5, top_p=0.95, repetition_penalty=1.0), dict(top_k=0), dict(typical_mass=0.9),
              dict(top_k=1, repetition_penalty=1.3)] + [dict(temperature=0.6 + 0.05 * i, top_k=10 + 15 * i, top_p=0.7 + 0.02 * i) for i in range(11)]


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_sixteen_sessions_keep_their_own_sampling_settings(sds, lib, name, dt, tdt, tol):
    """Sixteen sessions, sixteen settings (a typical-sampling row and a full-sort row among them) on a wide handle with per-session
    sampling: each equals itself alone with its own settings; at most four graph captures."""
    cfg = ARConfig()
    sessions = _sessions(WIDE, SETTINGS16)
    single = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    want = [_alone(single, *s[1:6]) for s in sessions]
    single.close()
    st = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=WIDE, max_text=80, max_new_tokens=MAXN, max_latent_candidates=1, sessions=True,
                        per_session_sampling=True)
    got, _, _, peak = _run(st, sessions, own=True)
    assert peak == WIDE
    assert 1 <= st.stat(0) <= 4
    _check(want, got)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES[:1])
@torch.no_grad()
def test_wide_sessions_are_refused_where_they_do_not_qualify(sds, lib, name, dt, tdt, tol):
    cfg = ARConfig()
    kw = dict(max_text=80, max_new_tokens=MAXN, max_latent_candidates=1)
    for extra in (dict(max_batch=17, max_groups=16, dtype=dt), dict(max_batch=8, max_groups=1, dtype=E.TT_F32), dict(max_batch=8, max_groups=4, dtype=dt)):
        h = stages.ArStage(sds["autoregressive"], cfg, **kw, **extra)
        with pytest.raises(E.EngineError, match="wide sessions need"):
            h.set_option(E.TT_AR_OPT_SESSIONS, 2)
        h.close()
    # value 1 keeps its <= 4-row rule
    h = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=5, max_groups=5, **kw)
    with pytest.raises(E.EngineError, match="sessions need max_batch <= 4"):
        h.set_option(E.TT_AR_OPT_SESSIONS, 1)
    h.close()
    _, cond, text, _, _, _ = _sessions(1)[0]
    h = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=8, max_groups=8, **kw)
    h.prefill(cond, text)
    with pytest.raises(E.EngineError, match="before the first prefill"):
        h.set_option(E.TT_AR_OPT_SESSIONS, 2)
    h.close()
    with pytest.raises(E.EngineError, match="switched on once"):
        st = stages.ArStage(sds["autoregressive"], cfg, dtype=dt, max_batch=8, **kw, sessions=True)
        try:
            st.set_option(E.TT_AR_OPT_SESSIONS, 2)
        finally:
            st.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@torch.no_grad()
def test_tts_stream_many_on_sixteen_streams_equals_tts_stream(dtype):
    """TextToSpeech(max_streams=16, wide_sessions=True).tts_stream_many over 20 texts (four wait for a slot): every text's pieces are
    torch.equal to tts_stream alone on a max_streams=1 instance."""
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    a_cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), 1234), "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    sessions = _sessions()
    texts = [t for _, _, t, _, _, _ in sessions]
    seeds = [s for _, _, _, s, _, _ in sessions]
    cond = sessions[0][1]
    kw = dict(conditioning_latents=(cond,), max_mel_tokens=48, stream_chunk_size=20, overlap_wav_len=512)
    one = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True)
    want = [[c.cpu() for c in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s in zip(texts, seeds)]
    del one
    many = TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=96, kv_cache=True, max_streams=WIDE, wide_sessions=True)
    got = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=seeds, **kw):
        got.setdefault(i, []).append(wav.cpu())
    assert many.ar.stat(0) == 1
    for i in range(len(texts)):
        assert len(got[i]) == len(want[i]), f"text {i}: {len(got[i])} pieces, tts_stream made {len(want[i])}"
        for a, b in zip(got[i], want[i]):
            assert torch.equal(a, b), f"text {i}: a piece differs from tts_stream"
