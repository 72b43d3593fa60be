"""CPU checks of the speaking-rate control: the fp64 reference of the WSOLA time-stretch against itself, its integers against the built
library's, the header against its Python mirror, and the host flow (stretch / stretch_many / speaking_rate=) on a reference-backed
stand-in of the device stage.  The kernel is tests/test_gpu_tsm.py."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import tsm_reference as T
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stretch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- the reference
def test_rate_one_is_the_identity():
    for n in (1, 767, 5000):
        x = T.clip(n, 3)
        r = T.stretch(x, T.RATE_ONE)
        assert not r["offsets"].any() and len(r["y"]) == n
        assert np.abs(r["y"] - x).max() <= 4 * 2.0 ** -53 * np.abs(x).max()


def test_window_sums_to_one():
    w = T.window()
    assert w.shape == (T.W,) and w[0] == 0 and np.abs(w[:T.HS] + w[T.HS:] - 1).max() <= 2.0 ** -51
    assert T.W == 2 * T.HS


def test_integers_at_the_edge_lengths():
    for n in T.LENGTHS + (2, 383, 384, 385, 24000 * 30, E.TSM_MAX_SAMPLES):
        for rq in [T.rate_q(r) for r in T.RATES] + [T.RATE_MIN, T.RATE_MAX, T.RATE_ONE, 52429, 98765]:
            n_out, K = T.out_samples(n, rq), T.frames(n, rq)
            assert n_out == max(1, int(Fraction(n * 65536, rq) + Fraction(1, 2)))  # round half up of n / rate
            assert K == -(-n_out // T.HS) + 1 and (K - 2) * T.HS < n_out <= (K - 1) * T.HS  # the hops cover the output, none is idle
            assert T.nominal(1, rq) == 0 and T.nominal(K - 1, rq) == ((K - 2) * T.HS * rq + 32768) // 65536
            assert stretch.nominal(K - 1, rq) == T.nominal(K - 1, rq)
    assert T.out_samples(1, T.RATE_MAX) == 1 and T.frames(1, T.RATE_MAX) == 2
    assert T.out_samples(768, T.RATE_MIN) == 1536 and T.frames(768, T.RATE_MIN) == 5
    assert [T.rate_q(r) for r in T.RATES] == [32768, 52429, 81920, 131072]


def test_ties_take_the_smallest_offset_and_the_negative_one():
    s = np.zeros(2 * T.SEARCH)
    assert T.pick(s) == 0
    s[T.SEARCH - 3] = s[T.SEARCH + 3] = s[T.SEARCH + 7] = 1.0
    assert T.pick(s) == -3
    s[T.SEARCH + 2] = 1.0
    assert T.pick(s) == 2
    r = T.stretch(np.zeros(2000, dtype=np.float32), T.rate_q(0.8))
    assert not r["offsets"].any() and not r["y"].any()


def test_bounds_come_from_the_format():
    assert T.U == 2.0 ** -24 and T.EPS == 1e-20
    x = T.clip(5000, 0)
    s, b = T.frame_scores(x, T.rate_q(1.25), 3, 200)
    assert s.shape == b.shape == (512,) and (b >= np.abs(s) * (T.W * T.U / 2 + 4 * T.U)).all()
    assert (b <= (T.W * T.U + T.W * T.U / 2 + 4 * T.U) * np.linalg.norm(T.take(x.astype(np.float64), 200 + T.HS, T.W)) * 1.0000001).all()  # Cauchy-Schwarz
    y, yb = T.overlap_add(x, T.RATE_ONE, np.zeros(T.frames(5000, T.RATE_ONE), dtype=np.int32))
    assert np.allclose(yb, 4 * T.U * np.abs(x), rtol=1e-12, atol=0)  # both frames carry the same sample at rate 1: |w1 x| + |w2 x| = |x|


def test_the_unambiguous_share_of_the_family():
    fam = T.family_reference()
    assert len(fam) == len(T.LENGTHS) * len(T.RATES) * len(T.SEEDS) == 72
    clear = [bool(r["unambiguous"].all()) for _, _, r in fam]
    assert sum(clear) >= 0.4 * len(fam), sum(clear)
    for (x, rq, r) in fam:
        assert len(r["y"]) == T.out_samples(len(x), rq) and len(r["offsets"]) == T.frames(len(x), rq)


def test_an_f32_emulation_passes_the_protocol():
    """Steps 1 - 3 on an f32 run of the algorithm with another summation order than the device's."""
    exact = 0
    for x, rq, r in T.family_reference():
        y, offsets = T.emulate_f32(x, rq)
        c = T.check(x, rq, y, offsets)
        assert not c["inadmissible"] and not c["bad_samples"], (len(x), rq, c)
        if r["unambiguous"].all():
            assert np.array_equal(offsets, r["offsets"]), (len(x), rq)
            exact += 1
    assert exact >= 0.4 * len(T.FAMILY)
    # the check does see a wrong choice and a wrong sample
    x, rq, r = [f for f in T.family_reference() if len(f[0]) == 5000 and f[2]["unambiguous"].all()][0]
    off = r["offsets"].copy()
    off[2] += 5
    assert T.check(x, rq, T.overlap_add(x, rq, off)[0], off)["inadmissible"][0] == 2  # (later frames were chosen for another history)
    y = r["y"].copy()
    y[100] += 1e-5
    assert T.check(x, rq, y, r["offsets"])["bad_samples"] == 1
    assert not T.admissible(x, rq, 2, int(T.positions(rq, r["offsets"])[1]), int(off[2]))
    assert T.admissible(x, rq, 2, int(T.positions(rq, r["offsets"])[1]), int(r["offsets"][2]))


# ----------------------------------------------------------------------------------------- ABI
def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def test_tsm_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_tsm.h")
    assert set(names) == set(E._TSM_PROTOS) == {"tt_tsm_abi_version", "tt_tsm_create", "tt_tsm_destroy", "tt_tsm_out_samples", "tt_tsm_frames",
                                                "tt_tsm_stretch"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_tsm_abi_version() == 1 == E.TSM_ABI_VERSION
    assert lib.tt_ctc_abi_version() == 1 and lib.tt_abi_version() == 6  # the other headers are untouched
    assert not [n for n in declared_symbols() if n.startswith("tt_tsm")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_tsm.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_TSM_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    mirror = dict(TT_TSM_WINDOW=E.TSM_WINDOW, TT_TSM_HOP=E.TSM_HOP, TT_TSM_SEARCH=E.TSM_SEARCH, TT_TSM_RATE_ONE=E.TSM_RATE_ONE,
                  TT_TSM_RATE_MIN=E.TSM_RATE_MIN, TT_TSM_RATE_MAX=E.TSM_RATE_MAX, TT_TSM_SAMPLE_RATE=E.TSM_SAMPLE_RATE,
                  TT_TSM_MAX_SAMPLES=E.TSM_MAX_SAMPLES, TT_TSM_MAX_CLIPS=E.TSM_MAX_CLIPS, TT_TSM_OK=E.TSM_OK, TT_TSM_EMPTY=E.TSM_EMPTY,
                  TT_TSM_REFUSED=E.TSM_REFUSED)
    assert defines == mirror
    assert (T.W, T.HS, T.SEARCH, T.RATE_ONE, T.RATE_MIN, T.RATE_MAX, T.SAMPLE_RATE) == \
        (E.TSM_WINDOW, E.TSM_HOP, E.TSM_SEARCH, E.TSM_RATE_ONE, E.TSM_RATE_MIN, E.TSM_RATE_MAX, E.TSM_SAMPLE_RATE)
    h = E.vp()
    for bad in ((0, 1), (E.TSM_MAX_SAMPLES + 1, 1), (100, 0), (100, E.TSM_MAX_CLIPS + 1)):
        assert lib.tt_tsm_create(*bad, C.byref(h)) == -1 and b"tt_tsm_create" in lib.tt_last_error()
    assert lib.tt_tsm_stretch(None, 1, None, None, None, None, None, None, None, None, None) == -1 and b"tt_tsm_stretch" in lib.tt_last_error()
    rc = lib.tt_tsm_create(1000, 2, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_tsm_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())
        with pytest.raises(E.EngineError):
            E.check(rc)


def test_library_integers_equal_the_reference():
    lib = _lib()
    rng = np.random.default_rng(5)
    cases = [(n, T.rate_q(r)) for n in T.LENGTHS for r in T.RATES]
    cases += [(int(n), int(rq)) for n, rq in zip(rng.integers(1, E.TSM_MAX_SAMPLES + 1, 200), rng.integers(T.RATE_MIN, T.RATE_MAX + 1, 200))]
    cases += [(E.TSM_MAX_SAMPLES, T.RATE_MIN), (E.TSM_MAX_SAMPLES, T.RATE_MAX), (1, T.RATE_MIN), (1, T.RATE_MAX)]
    for n, rq in cases:
        assert (lib.tt_tsm_out_samples(n, rq), lib.tt_tsm_frames(n, rq)) == (T.out_samples(n, rq), T.frames(n, rq)), (n, rq)
    for n, rq in ((0, 65536), (-1, 65536), (E.TSM_MAX_SAMPLES + 1, 65536), (100, T.RATE_MIN - 1), (100, T.RATE_MAX + 1), (100, 0)):
        assert lib.tt_tsm_out_samples(n, rq) == 0 == lib.tt_tsm_frames(n, rq)


# ----------------------------------------------------------------------------------------- host flow
class ReferenceStretchStage:
    """stages.TimeStretchStage backed by tests/tsm_reference.py."""
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceStretchStage.made.append(max_samples)

    def stretch_many(self, clips, rqs):
        ReferenceStretchStage.calls.append(len(clips))
        out = []
        for x, rq in zip(clips, rqs):
            assert x.dim() == 1 and x.shape[0] <= self.max_samples
            r = T.stretch(x.numpy(), rq)
            out.append((torch.from_numpy(r["y"]).float(), torch.from_numpy(r["offsets"])))
        return out

    def close(self):
        pass


def _install(monkeypatch):
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "TimeStretchStage", ReferenceStretchStage)
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []
    return api


def _tts(monkeypatch, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup, voice_latents
    api = _install(monkeypatch)
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, **kw)
    call = dict(conditioning_latents=voice_latents(cfgs), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
                use_deterministic_seed=7, verbose=False)
    return t, call


def _ref(clip, rate):
    return torch.from_numpy(T.stretch(clip.reshape(-1).numpy(), T.rate_q(rate))["y"]).float().reshape(clip.shape[:-1] + (-1,))


@torch.no_grad()
def test_stretch_and_stretch_many(monkeypatch):
    from tests.test_api_flow_cpu import HELLO
    t, _ = _tts(monkeypatch)
    x = torch.from_numpy(T.clip(5000, 0))
    for shape in ((5000,), (1, 5000), (1, 1, 5000)):
        y = t.stretch(x.reshape(shape), rate=1.25)
        assert y.shape == shape[:-1] + (4000,) and y.dtype == torch.float32 and y.device == x.device
        assert torch.equal(y.reshape(-1), _ref(x, 1.25))
    assert ReferenceStretchStage.made == [30 * 24000] and ReferenceStretchStage.calls == [1, 1, 1]
    # a duration: exactly the samples the library's integer gives for the rate it implies
    d = t.stretch(x, duration=0.3)
    rq = stretch.rate_q(5000 / (0.3 * 24000))
    assert d.shape == (T.out_samples(5000, rq),) and abs(d.shape[0] - 7200) <= 1
    # several clips, a rate each, ONE call; the anchors
    clips = [x, torch.from_numpy(T.clip(769, 1)).reshape(1, -1), torch.from_numpy(T.clip(300, 1))]
    ReferenceStretchStage.calls = []
    out, maps = t.stretch_many(clips, rates=[0.8, 2.0, 0.5], return_map=True)
    assert ReferenceStretchStage.calls == [3] and [tuple(o.shape) for o in out] == [(6250,), (1, 385), (600,)]
    for o, c, r, m in zip(out, clips, (0.8, 2.0, 0.5), maps):
        ref = T.stretch(c.reshape(-1).numpy(), T.rate_q(r))
        assert torch.equal(o, _ref(c, r))
        assert m.dtype == torch.int64 and m.shape == (len(ref["offsets"]), 2)
        assert m[:, 0].tolist() == [(k - 1) * T.HS for k in range(len(m))] and m[:, 1].tolist() == T.positions(T.rate_q(r), ref["offsets"]).tolist()
    assert torch.equal(t.stretch_many(clips, rates=0.8)[2], _ref(clips[2], 0.8))
    assert torch.equal(t.stretch_many(clips, durations=[0.25, 0.03, 0.02])[1], t.stretch(clips[1], duration=0.03))
    # a longer clip than the stage was built for: it is built again, larger
    t.stretch(torch.zeros(30 * 24000 + 1), rate=2.0)
    assert ReferenceStretchStage.made == [30 * 24000, 30 * 24000 + 1]
    # refusals
    for bad in (0.49, 2.01, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
            t.stretch(x, rate=bad)
    with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
        t.stretch(x, duration=1.0)  # 5000 samples cannot last a second
    with pytest.raises(ValueError, match="positive"):
        t.stretch(x, duration=0.0)
    with pytest.raises(ValueError, match="exactly one"):
        t.stretch(x, rate=1.25, duration=0.2)
    with pytest.raises(ValueError, match="exactly one"):
        t.stretch(x)
    with pytest.raises(ValueError, match="3 clips with 2 rates"):
        t.stretch_many(clips, rates=[1.0, 1.5])
    with pytest.raises(ValueError, match="expected"):
        t.stretch(torch.zeros(2, 100), rate=1.5)
    with pytest.raises(ValueError, match="expected"):
        t.stretch(torch.zeros(0), rate=1.5)
    with pytest.raises(ValueError, match="exceeds"):
        t.stretch(torch.zeros(1, E.TSM_MAX_SAMPLES + 1), rate=1.5)


@torch.no_grad()
def test_speaking_rate_on_tts(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    t, kw = _tts(monkeypatch)
    plain = t.tts(HELLO_THERE, **kw)
    # None and exactly 1.0: no stage, no call, today's bits
    assert torch.equal(t.tts(HELLO_THERE, speaking_rate=None, **kw), plain) and torch.equal(t.tts(HELLO_THERE, speaking_rate=1.0, **kw), plain)
    assert torch.equal(t.tts_many([HELLO_THERE], speaking_rate=1.0, **kw)[0], plain)
    assert t.stretcher is None and ReferenceStretchStage.made == [] and ReferenceStretchStage.calls == [] and "stretch_s" not in t.timings
    fast = t.tts(HELLO_THERE, speaking_rate=1.25, **kw)
    assert ReferenceStretchStage.calls == [1] and "stretch_s" in t.timings and "diffusion_s" in t.timings
    assert fast.shape == (1, 1, T.out_samples(plain.shape[-1], 81920)) and torch.equal(fast, _ref(plain, 1.25))
    preset = t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **kw)
    assert torch.equal(t.tts_with_preset(HELLO_THERE, preset="ultra_fast", speaking_rate=1.25, **kw), _ref(preset, 1.25))
    # k winners: one call for all of them
    two = t.tts(HELLO_THERE, k=2, **kw)
    ReferenceStretchStage.calls = []
    slow, state = t.tts(HELLO_THERE, k=2, speaking_rate=0.8, return_deterministic_state=True, **kw)
    assert ReferenceStretchStage.calls == [2] and state[0] == 7
    assert all(torch.equal(a, _ref(b, 0.8)) for a, b in zip(slow, two))
    # tts_many: one call for the texts
    many = t.tts_many([HELLO_THERE, HELLO], **kw)
    ReferenceStretchStage.calls = []
    many_fast = t.tts_many([HELLO_THERE, HELLO], speaking_rate=2.0, **kw)
    assert ReferenceStretchStage.calls == [2] and all(torch.equal(a, _ref(b, 2.0)) for a, b in zip(many_fast, many)) and "stretch_s" in t.timings
    for bad in (0.3, 2.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
            t.tts(HELLO_THERE, speaking_rate=bad, **kw)
        with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
            t.tts_many([HELLO_THERE], speaking_rate=bad, **kw)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (other unknown kwargs are refused as before)
        t.tts(HELLO_THERE, speaking_speed=1.2, **kw)


@torch.no_grad()
def test_timings_and_long_form_follow_the_stretched_clip(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tortoise_tts_amd import longform
    t, m = CC._flow(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "TimeStretchStage", ReferenceStretchStage)
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []
    from tests.test_api_flow_cpu import voice_latents, small_setup
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    plain = t.tts("hello there", **kw)
    res, al = t.tts_with_timings("hello there", speaking_rate=0.8, **kw)
    assert torch.equal(res, _ref(plain, 0.8)) and al.samples == res.shape[-1] and al == CC._expected(m, res, "hello there")


@torch.no_grad()
def test_long_form_passes_the_rate_on(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    from tortoise_tts_amd import longform
    t, kw = _tts(monkeypatch, candidate_sharding=False)
    kw = dict(conditioning_latents=kw["conditioning_latents"], num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, seed=5,
              texts_are_chunks=True, preset="ultra_fast")
    _, clips = longform.read_long_form(t, [HELLO_THERE, HELLO], **kw)
    _, fast = longform.read_long_form(t, [HELLO_THERE, HELLO], speaking_rate=1.25, **kw)
    assert sum(ReferenceStretchStage.calls) == 2 and all(torch.equal(a, _ref(b, 1.25)) for a, b in zip(fast, clips))


@torch.no_grad()
def test_fast_path_rate_and_streaming_refusals(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    monkeypatch.setattr(api_fast.stages, "TimeStretchStage", ReferenceStretchStage)
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []
    one = make(1)
    kw = dict(max_mel_tokens=24, use_deterministic_seed=41)
    plain = one.tts(TEXTS[0], **kw)
    assert torch.equal(one.tts(TEXTS[0], speaking_rate=1.0, **kw), plain) and torch.equal(one.tts(TEXTS[0], speaking_rate=None, **kw), plain)
    assert ReferenceStretchStage.made == [] and one.stretcher is None
    assert torch.equal(one.tts(TEXTS[0], speaking_rate=1.5, **kw), _ref(plain, 1.5)) and ReferenceStretchStage.calls == [1]
    both = one.tts_many(TEXTS[:2], **kw)
    ReferenceStretchStage.calls = []
    assert all(torch.equal(a, _ref(b, 0.5)) for a, b in zip(one.tts_many(TEXTS[:2], speaking_rate=0.5, **kw), both))
    assert ReferenceStretchStage.calls == [2]
    with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
        one.tts(TEXTS[0], speaking_rate=3.0, **kw)
    # streamed audio is cross-faded piece by piece: no rate there
    with pytest.raises(ValueError, match="speaking_rate is not available"):
        next(one.tts_stream(TEXTS[0], speaking_rate=1.5, **KW))
    many = make(3)
    with pytest.raises(ValueError, match="speaking_rate is not available"):
        many.open_stream(TEXTS[0], speaking_rate=1.5, **KW)
    with pytest.raises(ValueError, match="speaking_rate is not available"):
        next(many.tts_stream_many(TEXTS[:2], speaking_rate=1.5, **KW))
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.TimeStretchStage)  # (no handle: the checks come before any device work)
    st.h = None
    st.max_samples, st.max_clips = 1000, 16
    with pytest.raises(ValueError, match="1001 samples"):
        st.stretch_many([torch.zeros(1001)], [65536])
    with pytest.raises(ValueError, match="at least one sample"):
        st.stretch_many([torch.zeros(0)], [65536])
    with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
        st.stretch_many([torch.zeros(10)], [131073])
    with pytest.raises(ValueError, match="2 clips with 1 rates"):
        st.stretch_many([torch.zeros(10), torch.zeros(10)], [65536])
