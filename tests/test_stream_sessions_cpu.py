"""CPU checks of the host side of several streaming sessions in one decode batch (api_fast.TextToSpeech(max_streams > 1): open_stream,
stream_pieces, tts_stream_many) on oracle-backed stand-ins of the session stage.  The engine's contract - a session's codes and latents
equal the same session streamed alone (tests/test_gpu_stream_sessions.py) - is how the stand-in produces them; what is checked here is
the piece schedule, admissions between pieces, slot reuse and the refusals."""
import pytest
import torch

from tests import fake_stages


class RecordingArStage(fake_stages.FakeArStage):
    """The single-stream stand-in, recording how the instance builds and calls its stage."""
    made = []

    def __init__(self, *a, **kw):
        RecordingArStage.made.append(kw)
        self.calls = []
        super().__init__(*a, **kw)

    def prefill(self, *a):
        self.calls.append("prefill")
        return super().prefill(*a)

    def generate_stream(self, *a, **kw):
        self.calls.append("generate_stream")
        return super().generate_stream(*a, **kw)

    def stream_latents(self, *a):
        self.calls.append("stream_latents")
        return super().stream_latents(*a)


class FakeSessionArStage:
    """Session stage stand-in: every row is a single-stream stand-in of its own; advance() hands out its tokens n at a time and reports
    a row finished when it reaches a sampled stop token, as the engine does."""

    def __init__(self, sd, cfg, device="cpu", dtype=0, max_batch=256, max_text=402, max_new_tokens=500, max_latent_candidates=4,
                 share_weights_with=None, kv_cache=True, max_groups=1, sessions=False):
        if not sessions:
            self.__class__ = RecordingArStage
            RecordingArStage.__init__(self, sd, cfg, device, dtype, max_batch=max_batch, max_text=max_text, max_new_tokens=max_new_tokens,
                                      max_latent_candidates=max_latent_candidates, share_weights_with=share_weights_with, kv_cache=kv_cache,
                                      max_groups=max_groups)
            return
        assert max_batch <= 4
        self.args = (sd, cfg, device, dtype, kv_cache)
        self.cfg, self.max_batch, self.max_new = cfg, max_batch, max_new_tokens
        self.rows = [None] * max_batch
        self.scalars = None
        self.advances = []

    def admit(self, slot, cond, text, seed):
        assert self.rows[slot] is None, "admission into an occupied slot"
        sd, cfg, device, dtype, kv_cache = self.args
        row = fake_stages.FakeArStage(sd, cfg, device, dtype, max_batch=1, kv_cache=kv_cache)
        row.prefill(cond, text)
        self.rows[slot] = {"stage": row, "seed": seed, "n": 0, "codes": None}

    def advance(self, n, **scalars):
        assert n >= 1
        running = [r for r in self.rows if r is not None and not r.get("finished")]
        if any(r["codes"] is not None for r in running):
            assert scalars == self.scalars, "the sampling settings of the running sessions changed"
        self.scalars = scalars
        self.advances.append(n)
        for r in running:
            if r["codes"] is None:
                r["codes"], _ = r["stage"].generate(1, self.max_new, seed=r["seed"], **scalars)
            total = r["codes"].shape[1]
            assert r["n"] + n <= self.max_new
            r["n"] = min(r["n"] + n, total)
            r["finished"] = r["n"] == total and int(r["codes"][0, -1]) == self.cfg.stop_mel_token
        return ([0 if r is None else r["n"] for r in self.rows], [r is not None and bool(r.get("finished")) for r in self.rows])

    def session_codes(self, slot):
        r = self.rows[slot]
        return r["codes"][:, :r["n"]]

    def session_latents(self, slot, n):
        return self.rows[slot]["stage"].stream_latents(1, n)

    def latents(self, cond, text, codes, stream_positions=False):
        return fake_stages.FakeArStage.latents(self.rows[0]["stage"], cond, text, codes, stream_positions)

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
    monkeypatch.setattr(api_fast.stages, "ArStage", FakeSessionArStage)
    monkeypatch.setattr(api_fast.E, "require_gpu", lambda device=None: torch.device("cpu"))
    a_cfg = ARConfig(**G.AR_CFG)
    h_cfg = HifiganConfig(in_channels=a_cfg.model_dim, cond_channels=a_cfg.model_dim, upsample_initial_channel=64)
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.AR_SEED),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), seed=43),
           "rlg_auto": W.synthetic_state_dict(W.rlg_manifest(a_cfg.model_dim), seed=G.RLG_SEED, gain=3.0)}
    sds_nostop = dict(sds, autoregressive=W.suppress_stop_token(sds["autoregressive"], a_cfg))

    def make(max_streams, stop=True):
        return api_fast.TextToSpeech(state_dicts=sds if stop else sds_nostop, configs={"ar": a_cfg, "hifigan": h_cfg}, max_mel_tokens=80,
                                     max_text_tokens=40, kv_cache=True, max_streams=max_streams)
    return api_fast, make


# (text, seed, max_mel_tokens, stream_chunk_size): a boundary-ending sequence (70 = 60 + 2 x 5), a session cut short by its own limit, an
# odd limit, a longer one
SESSIONS = [(list(range(5, 20)), 4, 70, 5), (list(range(3, 12)), 9, 62, 40), (list(range(7, 30)), 11, 66, 4), (list(range(2, 9)), 13, 75, 7)]


def _single_pieces(make, stop):
    one = make(1, stop)
    return [[c.clone() for c in one.tts_stream(t, max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)]
            for t, s, m, c in SESSIONS]


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_stream_pieces_follow_tts_stream_per_session(monkeypatch, stop):
    """Two slots, four sessions: the third and fourth are admitted between pieces (staggered) and reuse the slots of sessions that ended;
    every session's pieces equal its tts_stream pieces, including the extra piece of a sequence that ends on a buffer boundary.
    stop=True: sampled stop tokens end sequences early."""
    api_fast, make = _instances(monkeypatch)
    want = _single_pieces(make, stop)
    many = make(2, stop)
    ids, got = {}, {}

    def admit(i):
        t, s, m, c = SESSIONS[i]
        ids[many.open_stream(t, max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)] = i

    admit(0)
    nxt = 1
    for sid, wav, done in many.stream_pieces():
        got.setdefault(ids[sid], []).append((wav.clone(), done))
        if nxt < len(SESSIONS) and len(many._sessions) < 2:
            admit(nxt)
            nxt += 1
    assert nxt == len(SESSIONS) and not many._sessions
    for i in range(len(SESSIONS)):
        assert [d for _, d in got[i]] == [False] * (len(want[i]) - 1) + [True], f"session {i}: done flags"
        assert len(got[i]) == len(want[i]) and all(torch.equal(a, b) for (a, _), b in zip(got[i], want[i])), f"session {i}: pieces differ"
    if not stop:  # the 70-token session ends on a buffer boundary: tts_stream's extra piece is the withheld overlap window
        assert len(want[0]) == 4 and want[0][-1].shape[0] == 128
    # no session overshoots: every advance is at most the distance of some session to its next piece boundary
    assert max(many.ar.advances) <= 60
    # tts_stream_many: the same pieces, by index into the texts
    many2 = make(3, stop)
    out = {}
    for i, wav, done in many2.tts_stream_many([t for t, _, _, _ in SESSIONS[:2]], max_mel_tokens=62, use_deterministic_seed=[4, 9], stream_chunk_size=40,
                                              overlap_wav_len=128):
        out.setdefault(i, []).append(wav)
    one = make(1, stop)
    for i, (t, s, _, _) in enumerate(SESSIONS[:2]):
        ref = list(one.tts_stream(t, max_mel_tokens=62, use_deterministic_seed=s, stream_chunk_size=40, overlap_wav_len=128))
        assert len(out[i]) == len(ref) and all(torch.equal(a, b) for a, b in zip(out[i], ref))


@torch.no_grad()
def test_open_stream_refusals(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    many = make(2)
    t = list(range(5, 20))
    many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=1, temperature=0.7)
    with pytest.raises(ValueError, match="sampling settings"):
        many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=2, temperature=0.8)
    with pytest.raises(ValueError, match="sampling settings"):
        many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=2, temperature=0.7, top_k=20)
    with pytest.raises(ValueError, match="exp_noise"):
        many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=2, temperature=0.7, exp_noise=torch.ones(1))
    many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=2, temperature=0.7)
    with pytest.raises(RuntimeError, match="busy"):
        many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=3, temperature=0.7)
    with pytest.raises(NotImplementedError, match="max_streams"):
        list(many.tts_stream(t))
    with pytest.raises(ValueError, match="max_streams"):
        make(5)
    assert sum(1 for _ in many.stream_pieces()) >= 2 and not many._sessions
    # once every session has ended, other settings are accepted
    many.open_stream(t, max_mel_tokens=40, use_deterministic_seed=3, temperature=0.9)
    one = make(1)
    with pytest.raises(NotImplementedError, match="max_streams"):
        one.open_stream(t)


@torch.no_grad()
def test_single_stream_instance_keeps_its_stage_and_calls(monkeypatch):
    """max_streams=1 (the default) builds today's max_batch = 1 handle without sessions and streams through the same stage calls."""
    api_fast, make = _instances(monkeypatch)
    RecordingArStage.made = []
    one = make(1)
    assert RecordingArStage.made[-1]["max_batch"] == 1 and not RecordingArStage.made[-1].get("sessions", False)
    list(one.tts_stream(list(range(5, 20)), max_mel_tokens=70, use_deterministic_seed=4, stream_chunk_size=5, overlap_wav_len=128))
    assert one.ar.calls[:2] == ["prefill", "generate_stream"] and set(one.ar.calls[2:]) == {"stream_latents"}


@torch.no_grad()
def test_close_stream_retires_a_session_and_frees_its_slot(monkeypatch):
    """close_stream(sid) - a client that went away: the session emits nothing more, its slot takes the next session, and the session
    that kept running still gets exactly its tts_stream pieces."""
    api_fast, make = _instances(monkeypatch)
    want = _single_pieces(make, False)
    many = make(2, False)
    t0, s0, m0, c0 = SESSIONS[0]
    t1, s1, m1, c1 = SESSIONS[1]
    keep = many.open_stream(t0, max_mel_tokens=m0, use_deterministic_seed=s0, stream_chunk_size=c0, overlap_wav_len=128)
    gone = many.open_stream(t1, max_mel_tokens=m1, use_deterministic_seed=s1, stream_chunk_size=c1, overlap_wav_len=128)
    got, late = [], None
    for sid, wav, done in many.stream_pieces():
        assert sid != gone, "a closed session still produced a piece"
        if sid == keep:
            got.append(wav.clone())
            if len(got) == 1:
                many.close_stream(gone)
                with pytest.raises(KeyError):
                    many.close_stream(gone)
                t, s, m, c = SESSIONS[2]
                late = many.open_stream(t, max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)
    assert late is not None and len(got) == len(want[0]) and all(torch.equal(a, b) for a, b in zip(got, want[0]))
