"""CPU checks of the host side of per-session sampling settings (api_fast.TextToSpeech(max_streams > 1, per_session_sampling=True),
ArStage(per_session_sampling=True)) on an oracle-backed stand-in of the session stage defined here.  The engine's contract - a session
computes what it computes alone with its own settings (tests/test_gpu_session_sampling.py) - is how the stand-in produces its codes; what
is checked here is that every session's settings reach its own row, and the refusals."""
import os
import re

import pytest
import torch

from tests import fake_stages
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

NAMES = ("temperature", "top_p", "repetition_penalty", "top_k", "typical_mass")


class PerSessionArStage:
    """Session stage stand-in: every row is a single-stream stand-in of its own.  With per_session_sampling each row samples with the
    settings it was admitted with; without it, with the settings advance() passes (which must not change while a row that sampled runs)."""
    made = []

    def __init__(self, sd, cfg, device="cpu", dtype=0, max_batch=256, max_text=402, max_new_tokens=500, max_latent_candidates=4,
                 share_weights_with=None, kv_cache=True, max_groups=1, sessions=False, per_session_sampling=False):
        PerSessionArStage.made.append(dict(sessions=sessions, per_session_sampling=per_session_sampling))
        if not sessions:
            self.__class__ = fake_stages.FakeArStage
            fake_stages.FakeArStage.__init__(self, sd, cfg, device, dtype, max_batch=max_batch, max_text=max_text, max_new_tokens=max_new_tokens,
                                             max_latent_candidates=max_latent_candidates, share_weights_with=share_weights_with,
                                             kv_cache=kv_cache, max_groups=max_groups)
            return
        assert max_batch <= 4
        self.args = (sd, cfg, device, dtype, kv_cache)
        self.cfg, self.max_batch, self.max_new = cfg, max_batch, max_new_tokens
        self.per_session_sampling = per_session_sampling
        self.rows = [None] * max_batch
        self.admits = []
        self.scalars = None

    def admit(self, slot, cond, text, seed, **settings):
        if self.per_session_sampling:
            own = dict(zip(NAMES, stages.session_sampling(**settings)))
        else:
            assert not settings, "settings passed to admit() on a stage without per_session_sampling"
            own = None
        assert self.rows[slot] is None, "admission into an occupied slot"
        sd, cfg, device, dtype, kv_cache = self.args
        row = fake_stages.FakeArStage(sd, cfg, device, dtype, max_batch=1, kv_cache=kv_cache)
        row.prefill(cond, text)
        self.rows[slot] = {"stage": row, "seed": seed, "n": 0, "codes": None, "settings": own}
        self.admits.append((slot, seed, own))

    def advance(self, n, **scalars):
        if self.per_session_sampling:
            assert not scalars, "scalars passed to advance() on a per-session stage"
        running = [r for r in self.rows if r is not None and not r.get("finished")]
        if not self.per_session_sampling:
            if any(r["codes"] is not None for r in running):
                assert scalars == self.scalars, "the sampling settings of the running sessions changed"
            self.scalars = scalars
        for r in running:
            if r["codes"] is None:
                own = r["settings"] if self.per_session_sampling else scalars
                r["codes"], _ = r["stage"].generate(1, self.max_new, seed=r["seed"], **own)
            total = r["codes"].shape[1]
            r["n"] = min(r["n"] + n, total)
            r["finished"] = r["n"] == total and int(r["codes"][0, -1]) == self.cfg.stop_mel_token
        return ([0 if r is None else r["n"] for r in self.rows], [r is not None and bool(r.get("finished")) for r in self.rows])

    def session_codes(self, slot):
        r = self.rows[slot]
        return r["codes"][:, :r["n"]]

    def session_latents(self, slot, n):
        return self.rows[slot]["stage"].stream_latents(1, n)

    def stat(self, which):
        return 1

    def close(self, slot=None):
        if slot is not None:
            assert self.rows[slot] is not None
            self.rows[slot] = None


def _instances(monkeypatch):
    from oracle import make_golden as G
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api_fast
    monkeypatch.setattr(api_fast.stages, "ArStage", PerSessionArStage)
    monkeypatch.setattr(api_fast.E, "require_gpu", lambda device=None: torch.device("cpu"))
    a_cfg = ARConfig(**G.AR_CFG)
    h_cfg = HifiganConfig(in_channels=a_cfg.model_dim, cond_channels=a_cfg.model_dim, upsample_initial_channel=64)
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.AR_SEED),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), seed=43),
           "rlg_auto": W.synthetic_state_dict(W.rlg_manifest(a_cfg.model_dim), seed=G.RLG_SEED, gain=3.0)}

    def make(max_streams, per_session_sampling=False):
        return api_fast.TextToSpeech(state_dicts=sds, configs={"ar": a_cfg, "hifigan": h_cfg}, max_mel_tokens=80, max_text_tokens=40,
                                     kv_cache=True, max_streams=max_streams, per_session_sampling=per_session_sampling)
    return api_fast, make


TEXT = list(range(5, 20))
OWN = [dict(temperature=0.7), dict(temperature=0.9, top_p=0.95, top_k=0), dict(repetition_penalty=1.2, typical_sampling=True, typical_mass=0.8)]
KW = dict(max_mel_tokens=50, stream_chunk_size=10, overlap_wav_len=128)


@torch.no_grad()
def test_differing_settings_are_accepted_per_session_and_refused_otherwise(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    one = make(1)
    want = [list(one.tts_stream(TEXT, use_deterministic_seed=3 + i, **KW, **o)) for i, o in enumerate(OWN)]
    PerSessionArStage.made = []
    many = make(3, per_session_sampling=True)
    assert PerSessionArStage.made[-1] == dict(sessions=True, per_session_sampling=True)
    ids = {many.open_stream(TEXT, use_deterministic_seed=3 + i, **KW, **o): i for i, o in enumerate(OWN)}
    got = {}
    for sid, wav, done in many.stream_pieces():
        got.setdefault(ids[sid], []).append(wav)
    for i in range(len(OWN)):
        assert len(got[i]) == len(want[i]) and all(torch.equal(a, b) for a, b in zip(got[i], want[i])), f"session {i}: pieces differ"
    assert [s for _, _, s in many.ar.admits] == [dict(temperature=0.7, top_p=0.8, repetition_penalty=2.0, top_k=50, typical_mass=0.0),
                                                 dict(temperature=0.9, top_p=0.95, repetition_penalty=2.0, top_k=0, typical_mass=0.0),
                                                 dict(temperature=0.8, top_p=0.8, repetition_penalty=1.2, top_k=50, typical_mass=0.8)]
    # a default instance keeps refusing them, and builds its stage exactly as before
    PerSessionArStage.made = []
    default = make(3)
    assert PerSessionArStage.made[-1] == dict(sessions=True, per_session_sampling=False)
    default.open_stream(TEXT, use_deterministic_seed=3, **KW, **OWN[0])
    with pytest.raises(ValueError, match="sampling settings"):
        default.open_stream(TEXT, use_deterministic_seed=4, **KW, **OWN[1])


@torch.no_grad()
def test_invalid_settings_raise_before_a_slot_is_taken(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    many = make(2, per_session_sampling=True)
    for bad in (dict(temperature=0.0), dict(top_p=-0.5), dict(repetition_penalty=0.0), dict(typical_sampling=True, typical_mass=1.0)):
        with pytest.raises(ValueError):
            many.open_stream(TEXT, use_deterministic_seed=1, **KW, **bad)
        assert not many._sessions and many.ar.rows == [None, None] and not many.ar.admits
    many.open_stream(TEXT, use_deterministic_seed=1, **KW)
    assert len(many._sessions) == 1


@torch.no_grad()
def test_stream_many_lists_reach_their_sessions(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    many = make(2, per_session_sampling=True)
    texts = [TEXT, TEXT[:9], TEXT[3:]]
    out = {}
    for i, wav, done in many.tts_stream_many(texts, use_deterministic_seed=[5, 6, 7], temperature=[0.5, 0.8, 1.1], top_k=[50, 0, 7],
                                             typical_sampling=[False, True, False], typical_mass=[0.9, 0.6, 0.9], **KW):
        out.setdefault(i, []).append(wav)
    seen = {seed: s for _, seed, s in many.ar.admits}
    assert seen == {5: dict(temperature=0.5, top_p=0.8, repetition_penalty=2.0, top_k=50, typical_mass=0.0),
                    6: dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=0, typical_mass=0.6),
                    7: dict(temperature=1.1, top_p=0.8, repetition_penalty=2.0, top_k=7, typical_mass=0.0)}
    one = make(1)
    for i, (t, seed, o) in enumerate(zip(texts, [5, 6, 7], [dict(temperature=0.5), dict(top_k=0, typical_sampling=True, typical_mass=0.6),
                                                          dict(temperature=1.1, top_k=7)])):
        ref = list(one.tts_stream(t, use_deterministic_seed=seed, **KW, **o))
        assert len(out[i]) == len(ref) and all(torch.equal(a, b) for a, b in zip(out[i], ref)), f"text {i}: pieces differ"
    with pytest.raises(ValueError, match="3 temperature values for 2 texts"):
        list(many.tts_stream_many(texts[:2], temperature=[0.5, 0.8, 1.1], **KW))
    default = make(2)
    with pytest.raises(ValueError, match="per_session_sampling"):
        list(default.tts_stream_many(texts, temperature=[0.5, 0.8, 1.1], **KW))
    assert not default._sessions


def test_per_session_sampling_needs_several_streams(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    with pytest.raises(ValueError, match="max_streams"):
        make(1, per_session_sampling=True)


def test_stage_refusals_without_a_gpu():
    with pytest.raises(ValueError, match="sessions=True"):
        stages.ArStage(None, per_session_sampling=True)
    assert stages.session_sampling() == (0.8, 0.8, 2.0, 50, 0.0)
    for bad in (dict(temperature=-1.0), dict(top_p=0.0), dict(repetition_penalty=float("nan")), dict(typical_mass=-0.1)):
        with pytest.raises(ValueError):
            stages.session_sampling(**bad)


def test_option_constant_matches_the_header():
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "tortoise_mi355x.h")).read()
    m = re.search(r"^#define\s+TT_AR_OPT_SESSION_SAMPLING\s+(\d+)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == E.TT_AR_OPT_SESSION_SAMPLING == 7
