"""-m gpu: the host driver of the autoregressive stage (csrc/gpt2.hip) - what the other files do not pin.

  * a refused call (chunk capacity, sampling scalars, batch, changed session settings) leaves a running generation resumable: the
    continuation has the bits and the capture count of an uninterrupted run, and the error texts are the ones callers match on;
  * the number of step-graph captures over scripted sequences of calls: one kept graph on an utterance handle (any change of what the
    step bakes in re-captures, a repeated call never does), one per combination of optional sampler launches on a session handle;
  * eager launches equal graph replay on the session path (tests/test_gpu_r5.py has the utterance path);
  * the copy that ends a call fills exactly [rows][min(ldcodes, columns)] of the caller's buffer.

The utterance / chunked cases run the reduced configuration of oracle/make_golden.py (MFMA-shaped step); session handles need the full
width (GEMV-shaped step), with synthetic weights whose stop logit is suppressed so that no row ends early.
"""
import ctypes as C

import pytest
import torch

from oracle import make_golden as G
from oracle import make_golden_full as GF
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ARConfig

pytestmark = pytest.mark.gpu
ERR = "tortoise_mi355x error -1: "
CANARY = -7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return E.init()


@pytest.fixture(scope="module")
def small(lib):
    """Reduced configuration: (cfg, weights with the stop token suppressed, cond, text)."""
    cfg = ARConfig(**G.AR_CFG)
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), cfg)
    return (cfg, sd) + tuple(G.ar_inputs(cfg))


@pytest.fixture(scope="module")
def full(lib):
    """Full width: (cfg, a stage that owns the packed weights, [(cond, text, seed)] for four sessions)."""
    cfg = ARConfig()
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg)
    owner = stages.ArStage(sd, cfg, max_batch=1, max_text=80, max_new_tokens=14, max_latent_candidates=1)
    text, auto, _ = GF.prompt()
    g = torch.Generator().manual_seed(7)
    prompts = [(auto * (1.0 + 0.1 * i) + 0.05 * torch.randn(auto.shape, generator=g), text[:, :cut].clone(), 100 + 17 * i)
               for i, cut in enumerate([55, 30, 44, 20])]
    yield cfg, owner, prompts
    owner.close()


def _small_stage(small, B, new=16, **kw):
    cfg, sd, _, _ = small
    return stages.ArStage(sd, cfg, max_batch=B, max_text=40, max_new_tokens=new, max_latent_candidates=1, **kw)


def _session_stage(full, S, per_session_sampling=False, new=14):
    cfg, owner, _ = full
    return stages.ArStage(None, cfg, max_batch=S, max_text=80, max_new_tokens=new, max_latent_candidates=1, sessions=True,
                          per_session_sampling=per_session_sampling, share_weights_with=owner)


def _sampling(seed=5, top_k=50, typical_mass=0.0, temperature=0.8):
    s = E.Sampling()
    s.temperature, s.top_p, s.repetition_penalty, s.top_k, s.typical_mass = temperature, 0.8, 2.0, top_k, typical_mass
    s.seed, s.row_offset, s.exp_noise, s.group_seeds = seed, 0, None, None
    return s


def _chunk(st, B, first, n, codes, ld=None, **sampling):
    """tt_ar_generate_chunk on a chunked handle with the caller's own buffer -> (tokens so far, finished)."""
    s = _sampling(**sampling)
    total, fin = C.c_int(0), C.c_int(0)
    E.check(st.lib.tt_ar_generate_chunk(st.h, B, int(first), int(n), codes.shape[1] if ld is None else ld, C.byref(s), E.ptr(codes), C.byref(total),
                                        C.byref(fin), E.stream_ptr()))
    return total.value, bool(fin.value)


def _refused(text, call, *args, **kw):
    with pytest.raises(E.EngineError) as err:
        call(*args, **kw)
    print(f"[driver] refused: {err.value}")
    assert str(err.value) == ERR + text


@torch.no_grad()
def test_refused_calls_leave_a_chunked_generation_resumable(small):
    cfg, _, cond, text = small
    B, N = 2, 15
    whole = _small_stage(small, B)
    whole.prefill(cond, text)
    want = torch.empty(B, N, device="cuda", dtype=torch.int32)
    assert _chunk(whole, B, 1, N, want) == (N, False)
    want_lat = whole.stream_latents(B, N).clone()
    want_captures = whole.stat(0)
    whole.close()

    st = _small_stage(small, B)
    st.prefill(cond, text)
    got = torch.empty(B, N, device="cuda", dtype=torch.int32)
    assert _chunk(st, B, 1, 5, got) == (5, False)
    tmax = 24  # 16 + 2 tokens of capacity, rounded up to 8 KV slots
    _refused(f"tt_ar_generate_chunk: 5 + 11 tokens exceed capacity ({N} code columns, {tmax} KV slots)", _chunk, st, B, 0, 11, got)
    _refused("tt_ar_generate: typical_mass 1.5 outside (0, 1) (0 = off)", _chunk, st, B, 0, 5, got, typical_mass=1.5)
    _refused("tt_ar_generate_chunk: no generation of 1 rows to resume", _chunk, st, 1, 0, 5, got)
    assert _chunk(st, B, 0, 5, got) == (10, False)
    assert _chunk(st, B, 0, 5, got) == (15, False)
    assert torch.equal(got, want), "codes after refused calls differ from the uninterrupted run"
    assert torch.equal(st.stream_latents(B, N), want_lat), "latents after refused calls differ from the uninterrupted run"
    print(f"[driver] chunked captures: uninterrupted {want_captures}, interrupted {st.stat(0)}")
    assert st.stat(0) == want_captures == 1 and st.stat(1) == 0
    st.close()


def _admit_all(st, prompts, slots, settings=None):
    for i, slot in enumerate(slots):
        cond, text, seed = prompts[i % len(prompts)]
        st.admit(slot, cond, text, seed + i, **(settings[i] if settings else {}))


@torch.no_grad()
def test_refused_chunk_leaves_sessions_resumable(full):
    _, _, prompts = full
    whole = _session_stage(full, 4, new=16)
    _admit_all(whole, prompts, [0, 2])
    n, fin = whole.advance(15)
    assert n == [15, 0, 15, 0] and not any(fin), (n, fin)
    want = whole._codes.clone()
    want_lat = [whole.session_latents(s, 15).clone() for s in (0, 2)]
    want_captures = whole.stat(0)
    whole.close()

    st = _session_stage(full, 4, new=16)
    _admit_all(st, prompts, [0, 2])
    st.advance(5)
    _refused("tt_ar_generate_chunk: sampling settings differ from those of the running sessions", st.advance, 5, temperature=0.5)
    st.advance(5)
    n, fin = st.advance(5)
    assert n == [15, 0, 15, 0] and not any(fin), (n, fin)
    assert torch.equal(st._codes[[0, 2]], want[[0, 2]]), "session codes after a refused chunk differ from the uninterrupted run"
    for s, lat in zip((0, 2), want_lat):
        assert torch.equal(st.session_latents(s, 15), lat), f"slot {s}: latents after a refused chunk differ from the uninterrupted run"
    print(f"[driver] session captures: uninterrupted {want_captures}, interrupted {st.stat(0)}")
    assert st.stat(0) == want_captures == 1 and st.stat(1) == 0
    st.close()


@torch.no_grad()
def test_capture_counts_of_an_utterance_handle(small):
    """One kept graph: every change of what the step bakes in (sampler scalars, typical mask, groups) re-captures - also the way back -
    and a repeated call (another seed: device data) never does."""
    _, _, cond, text = small
    B, N = 16, 12
    st = _small_stage(small, B, max_groups=2)

    def one():
        st.prefill(cond, text)

    def two():
        st.prefill_group(0, 2, cond, text)
        st.prefill_group(1, 2, cond, text[:, :6].contiguous())

    script = [("default", one, {}), ("top_k 300", one, dict(top_k=300)), ("typical", one, dict(typical_mass=0.9)),
              ("two groups of 8", two, {}), ("default again", one, {})]
    for i, (name, prefill, kw) in enumerate(script):
        for rep in range(2):
            prefill()
            codes, n = st.generate(B, N, seed=3 + rep, **kw)
            assert n == N
            print(f"[driver] utterance handle, {name}, call {rep}: stat(0) = {st.stat(0)}")
            assert st.stat(0) == i + 1, f"{name}, call {rep}: {st.stat(0)} captures, expected {i + 1}"
    assert st.stat(1) == 0
    st.close()


@torch.no_grad()
def test_capture_counts_of_a_wide_session_handle(full):
    """Per-row scalars are device data: one kept graph per combination of optional sampler launches, each captured once."""
    _, _, prompts = full
    st = _session_stage(full, 16, per_session_sampling=True, new=30)  # (slot 0 samples 24 tokens)
    fast, wide, typical = dict(top_k=50), dict(top_k=300), dict(typical_mass=0.9)
    cond, text, seed = prompts[0]
    # (what happens before the advance, the combination it runs, captures after it)
    script = [(lambda: st.admit(0, cond, text, seed, **fast), "fast", 1),
              (lambda: st.admit(1, cond, text, seed + 1, **wide), "fast + full sort", 2),
              (lambda: st.close(1), "fast", 2),
              (lambda: st.admit(2, cond, text, seed + 2, **typical), "fast + typical", 3),
              (lambda: st.admit(1, cond, text, seed + 3, **wide), "fast + full sort + typical", 4),
              (lambda: (st.close(1), st.close(2)), "fast", 4)]
    for before, name, captures in script:
        before()
        for rep in range(2):
            st.advance(2)
            print(f"[driver] wide session handle, {name}, advance {rep}: stat(0) = {st.stat(0)}")
            assert st.stat(0) == captures, f"{name}, advance {rep}: {st.stat(0)} captures, expected {captures}"
    assert st.stat(1) == 0
    st.close()


@pytest.mark.parametrize("S", [4, 16])
@torch.no_grad()
def test_session_eager_launches_equal_graph_replay(full, S):
    _, _, prompts = full
    slots = [0, 2] if S == 4 else [0, 5, 11]
    settings = None if S == 4 else [dict(top_k=50), dict(top_k=300), dict(typical_mass=0.9)]
    runs = []
    for replay in (1, 0):
        E.load_library().tt_graph_replay(replay)
        try:
            st = _session_stage(full, S, per_session_sampling=settings is not None)
            _admit_all(st, prompts, slots, settings)
            seen = [st.advance(n) for n in (4, 3, 5)]
            runs.append((st._codes[slots].clone(), seen, st.stat(0)))
            st.close()
        finally:
            E.load_library().tt_graph_replay(1)
    (codes, seen, captures), (codes_e, seen_e, captures_e) = runs
    assert seen[-1][0] == [12 if s in slots else 0 for s in range(S)]
    assert seen == seen_e, "n_total / finished of eager launches differ from the replayed graph"
    assert torch.equal(codes[:, :12], codes_e[:, :12]), "codes of eager launches differ from the replayed graph"
    assert captures >= 1 and captures_e == 0


def _buffer(rows, ld):
    """[rows + 1][ld] of canaries: the caller's [rows][ld] buffer and one row after it."""
    return torch.full((rows + 1, ld), CANARY, device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("ld", [15, 20])
@torch.no_grad()
def test_finishing_copy_of_a_chunked_generation(small, ld):
    """ldcodes == the tokens asked for in all, and ldcodes beyond them."""
    cfg, _, cond, text = small
    B, stop = 2, cfg.stop_mel_token
    st = _small_stage(small, B)
    st.prefill(cond, text)
    buf = _buffer(B, ld)
    for done, first in ((5, 1), (10, 0), (15, 0)):
        assert _chunk(st, B, first, 5, buf) == (done, False)
        assert bool((buf[:B, :done] != stop).all()) and bool((buf[:B, :done] >= 0).all()), "generated columns"
        assert bool((buf[:B, done:] == stop).all()), "columns beyond what was generated do not hold the stop token"
        assert bool((buf[B] == CANARY).all()), "the row after the caller's buffer was written"
    st.close()


@pytest.mark.parametrize("ld", [10, 20])
@torch.no_grad()
def test_finishing_copy_of_a_session_chunk(full, ld):
    """ldcodes below and above the handle's 16 code columns (14 + 2 tokens of capacity): min(ldcodes, 16) columns are copied."""
    cfg, _, prompts = full
    S, stop, tmax = 4, cfg.stop_mel_token, 16
    st = _session_stage(full, S)
    _admit_all(st, prompts, [1, 3])
    buf = _buffer(S, ld)
    s, gs = st._shared_sampling()
    n_total, fin = (C.c_int * S)(), (C.c_int * S)()
    for done in (3, 6):
        E.check(st.lib.tt_ar_generate_chunk(st.h, S, 0, 3, ld, C.byref(s), E.ptr(buf), n_total, fin, E.stream_ptr()))
        assert list(n_total) == [0, done, 0, done] and not any(fin)
        rows = buf[[1, 3]]
        assert bool((rows[:, :done] != stop).all()) and bool((rows[:, :done] >= 0).all()), "generated columns"
        assert bool((rows[:, done:min(ld, tmax)] == stop).all()), "columns beyond what was generated do not hold the stop token"
        assert bool((buf[S] == CANARY).all()), "the row after the caller's buffer was written"
    st.close()
