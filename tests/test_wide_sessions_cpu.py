"""CPU checks of the host side of wide session handles (api_fast.TextToSpeech(max_streams=2 .. 16, wide_sessions=True)) on oracle-backed
stand-ins of the session stage: sixteen slots, admissions as sessions end, close_stream, per-text lists, and the refusals.  The engine's
side - a session on a 16-row handle equals the same session alone - is tests/test_gpu_wide_sessions.py."""
import pytest
import torch

from tests import fake_stages
from tests.test_session_sampling_cpu import PerSessionArStage


class WideSessionArStage(PerSessionArStage):
    """The per-session stand-in with up to 16 rows, recording the stages the instance builds."""
    made = []

    def __init__(self, *a, max_batch=256, sessions=False, **kw):
        WideSessionArStage.made.append(dict(max_batch=max_batch, sessions=sessions))
        if not sessions:
            PerSessionArStage.__init__(self, *a, max_batch=max_batch, sessions=False, **kw)
            return
        assert max_batch <= 16
        PerSessionArStage.__init__(self, *a, max_batch=1, sessions=True, **kw)
        self.max_batch = max_batch
        self.rows = [None] * max_batch


def _instances(monkeypatch):
    from oracle import make_golden as G
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api_fast
    monkeypatch.setattr(api_fast.stages, "ArStage", WideSessionArStage)
    monkeypatch.setattr(api_fast.E, "require_gpu", lambda device=None: torch.device("cpu"))
    a_cfg = ARConfig(**G.AR_CFG)
    h_cfg = HifiganConfig(in_channels=a_cfg.model_dim, cond_channels=a_cfg.model_dim, upsample_initial_channel=64)
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.AR_SEED),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), seed=43),
           "rlg_auto": W.synthetic_state_dict(W.rlg_manifest(a_cfg.model_dim), seed=G.RLG_SEED, gain=3.0)}

    def make(max_streams, **kw):
        return api_fast.TextToSpeech(state_dicts=sds, configs={"ar": a_cfg, "hifigan": h_cfg}, max_mel_tokens=80, max_text_tokens=40,
                                     kv_cache=True, max_streams=max_streams, **kw)
    return api_fast, make


TEXTS = [list(range(2 + i % 5, 12 + (3 * i) % 17)) for i in range(19)]
KW = dict(max_mel_tokens=24, stream_chunk_size=8, overlap_wav_len=128)


def _alone(make, texts, seeds, settings=None):
    one = make(1)
    return [list(one.tts_stream(t, use_deterministic_seed=s, **KW, **(settings[i] if settings else {}))) for i, (t, s) in enumerate(zip(texts, seeds))]


@torch.no_grad()
def test_sixteen_streams_serve_more_texts_than_slots(monkeypatch):
    """tts_stream_many over 19 texts on 16 slots: the stage is a 16-row session stage, three texts wait and take the slots of sessions
    that ended, and every text's pieces equal its tts_stream pieces."""
    api_fast, make = _instances(monkeypatch)
    seeds = [40 + i for i in range(len(TEXTS))]
    want = _alone(make, TEXTS, seeds)
    WideSessionArStage.made = []
    many = make(16, wide_sessions=True)
    assert WideSessionArStage.made == [dict(max_batch=16, sessions=True)]
    got = {}
    for i, wav, done in many.tts_stream_many(TEXTS, use_deterministic_seed=seeds, **KW):
        got.setdefault(i, []).append(wav)
    # the first sixteen texts are admitted into the sixteen slots before the first piece; the others reuse slots
    assert [slot for slot, _, _ in many.ar.admits][:16] == list(range(16)) and len(many.ar.admits) == len(TEXTS)
    for i in range(len(TEXTS)):
        assert len(got[i]) == len(want[i]) and all(torch.equal(a, b) for a, b in zip(got[i], want[i])), f"text {i}: pieces differ"
    assert not many._sessions


@torch.no_grad()
def test_sixteen_open_streams_close_and_admit_between_pieces(monkeypatch):
    """open_stream fills all sixteen slots, a seventeenth is refused as busy; close_stream frees a slot that the next open_stream takes
    between pieces; the remaining sessions keep their pieces."""
    api_fast, make = _instances(monkeypatch)
    seeds = [60 + i for i in range(17)]
    want = _alone(make, TEXTS[:17], seeds)
    many = make(16, wide_sessions=True)
    ids = {many.open_stream(TEXTS[i], use_deterministic_seed=seeds[i], **KW): i for i in range(16)}
    with pytest.raises(RuntimeError, match="busy"):
        many.open_stream(TEXTS[16], use_deterministic_seed=seeds[16], **KW)
    closed = next(sid for sid, i in ids.items() if i == 5)
    got = {}
    for sid, wav, done in many.stream_pieces():
        got.setdefault(ids[sid], []).append(wav)
        if closed is not None and ids[sid] != 5:
            many.close_stream(closed)
            ids[many.open_stream(TEXTS[16], use_deterministic_seed=seeds[16], **KW)] = 16
            closed = None
    assert closed is None and not many._sessions
    assert len(got.get(5, [])) < len(want[5])
    for i in [i for i in range(17) if i != 5]:
        assert len(got[i]) == len(want[i]) and all(torch.equal(a, b) for a, b in zip(got[i], want[i])), f"session {i}: pieces differ"


@torch.no_grad()
def test_per_text_settings_reach_sixteen_sessions(monkeypatch):
    """per_session_sampling on sixteen streams: per-text lists of settings reach their own sessions and each text equals tts_stream with
    its own settings."""
    api_fast, make = _instances(monkeypatch)
    texts, seeds = TEXTS[:16], [80 + i for i in range(16)]
    temps = [0.5 + 0.05 * i for i in range(16)]
    top_k = [0 if i == 3 else 10 + i for i in range(16)]
    settings = [dict(temperature=t, top_k=k) for t, k in zip(temps, top_k)]
    want = _alone(make, texts, seeds, settings)
    many = make(16, wide_sessions=True, per_session_sampling=True)
    got = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=seeds, temperature=temps, top_k=top_k, **KW):
        got.setdefault(i, []).append(wav)
    seen = {seed: (s["temperature"], s["top_k"]) for _, seed, s in many.ar.admits}
    assert seen == {s: (t, k) for s, t, k in zip(seeds, temps, top_k)}
    for i in range(16):
        assert len(got[i]) == len(want[i]) and all(torch.equal(a, b) for a, b in zip(got[i], want[i])), f"text {i}: pieces differ"


def test_stream_counts_are_refused_outside_their_range(monkeypatch):
    """wide_sessions=True: 2 .. 16 streams; without it 1 .. 4, and the message points to the flag."""
    api_fast, make = _instances(monkeypatch)
    with pytest.raises(ValueError, match="max_streams"):
        make(17, wide_sessions=True)
    with pytest.raises(ValueError, match="max_streams"):
        make(1, wide_sessions=True)
    with pytest.raises(ValueError, match="max_streams=5 .*wide_sessions=True"):
        make(5)
    WideSessionArStage.made = []
    make(5, wide_sessions=True)
    make(3, wide_sessions=True)
    assert WideSessionArStage.made == [dict(max_batch=5, sessions=True), dict(max_batch=3, sessions=True)]
