"""The arbitrary-ratio resampler without a GPU: the fp64 reference against first principles, the integers against exact rational arithmetic,
the header against its Python mirror, and the host flow (pitch=, sample_rate=, resample, shift_pitch) on reference-backed stages."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import resample_reference as R
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = R.RHO_NUM / R.RHO_DEN


# ----------------------------------------------------------------------------------------- the reference against first principles
def _interior(y, P, Q):
    """The outputs none of whose taps reaches beyond the clip: H + 2 input samples from either end, in output samples."""
    edge = -(-(R.half_width(R.cutoff_q(P, Q)) + 2) * Q // P) + 1
    assert len(y) > 4 * edge
    return edge, len(y) - edge


def _tone(n, f, phase=0.3):
    return np.cos(2 * np.pi * f * np.arange(n) + phase).astype(np.float32)


def _fit(y, m, f):
    """Least squares of y[m] on a tone of frequency f (cycles per sample) -> (amplitude, the fitted tone)."""
    A = np.stack([np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)], axis=1)
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    return float(np.hypot(*coef)), A @ coef


def _db(v):
    return 20 * math.log10(max(v, 1e-300))


@pytest.mark.parametrize("P,Q", R.RATIOS)
def test_pass_band_is_flat_and_clean(P, Q):
    """Tones at 0.1, 0.4 and 0.8 of rho times the narrower Nyquist: gain within +-0.001 dB, everything else in the output <= -100 dB."""
    n = 4096
    for share in (0.1, 0.4, 0.8):
        f = share * RHO * 0.5 * min(1.0, Q / P)  # cycles per input sample
        y, _ = R.resample(_tone(n, f), P, Q, bound=False)
        a, b = _interior(y, P, Q)
        m = np.arange(a, b)
        amp, fit = _fit(y[a:b], m, f * P / Q)
        rest = y[a:b] - fit
        gain_db, rest_db = _db(amp), _db(np.sqrt(np.mean(rest ** 2)) / (amp / math.sqrt(2)))
        print(f"{P}/{Q} tone at {share} rho: gain {gain_db:+.2e} dB, rest {rest_db:.1f} dB")
        assert abs(gain_db) <= 0.001 and rest_db <= -100.0


# a tone above the output's Nyquist frequency exists in the input only below the input's own: the ratios that convert downwards, and of the
# two frequencies those that the input can hold (1.5x the output Nyquist of 3/2 is the input Nyquist itself: still a sequence, +1 -1 +1 ...)
STOP_CASES = [(P, Q, k) for P, Q in R.RATIOS for k in (1.1, 1.5) if k * Q <= P]


def test_stop_band_cases_are_the_downward_ratios():
    assert STOP_CASES == [(3, 2, 1.1), (3, 2, 1.5), (3, 1, 1.1), (3, 1, 1.5), (77936, 65536, 1.1)]


@pytest.mark.parametrize("P,Q,k", STOP_CASES)
def test_tones_beyond_the_output_nyquist_are_removed(P, Q, k):
    n = 4096
    x = _tone(n, k * 0.5 * Q / P)
    y, _ = R.resample(x, P, Q, bound=False)
    a, b = _interior(y, P, Q)
    level = _db(np.sqrt(np.mean(y[a:b] ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print(f"{P}/{Q} tone at {k} x the output Nyquist: {level:.1f} dB")
    assert level <= -100.0


def test_table_and_constants():
    tab = R.table()
    assert len(tab) == E.RS_TABLE == 16385 and tab[0] == 1.0 and np.all(tab == tab.astype(np.float32))
    assert np.all(np.abs(tab[R.L::R.L]) < 1e-7)  # the zero crossings of the sinc
    # I0 by its series against numpy's
    for x in (0.0, 0.5, 3.0, 10.0):
        assert abs(R.i0(x) / float(np.i0(x)) - 1) < 1e-14
    # the half-widths the header names
    assert R.half_width(R.cutoff_q(1, 2)) == 36 and R.half_width(R.cutoff_q(8, 1)) == 285
    assert R.cutoff_q(1, 1) == 30198988 and R.cutoff_q(3, 1) == 30198988 * 10 // 30 + 0 == int(Fraction(9 * 512 * 65536, 30))
    for P, Q in R.RATIOS + R.EXTREME_RATIOS:
        c = Fraction(9, 10) * min(Fraction(1), Fraction(Q, P))
        assert R.cutoff_q(P, Q) == math.floor(c * R.L * 65536) and R.half_width(R.cutoff_q(P, Q)) >= math.ceil(R.Z / c)
        assert R.cutoff_f32(P, Q) == float(np.float32(float(c))) or abs(R.cutoff_f32(P, Q) / float(c) - 1) < 2.0 ** -23


def test_bound_comes_from_the_format():
    """One tap on one sample: the bound is gamma_3-and-gamma_N of |h x|, nothing else."""
    x = np.zeros(200, dtype=np.float32)
    x[100] = 1.0
    y, b = R.resample(x, 1, 1)
    N = 2 * 36 + 2
    h = abs(y[100])  # the centre tap: a = 0, so |a dt| = 0 and |v| = tab[0] = 1
    assert h == R.cutoff_f32(1, 1) and abs(b[100] - (R.gamma(3) * h * (1 + R.gamma(N)) + h * R.gamma(N) + N * 2.0 ** -149)) < 1e-20
    assert np.all(b[:60] == N * 2.0 ** -149) and np.all(y[:60] == 0)  # no tap reaches the impulse
    assert R.resample(np.zeros(50, dtype=np.float32), 3, 2)[0].tolist() == [0.0] * 34


# ----------------------------------------------------------------------------------------- integers
def test_integers_against_exact_rationals():
    rng = np.random.default_rng(3)
    cases = [(n, P, Q) for n in R.LENGTHS + (1023, 1024, 1025, E.RS_MAX_SAMPLES) for P, Q in R.RATIOS + R.EXTREME_RATIOS]
    for _ in range(200):
        Q = int(rng.integers(1, E.RS_MAX_TERM + 1))
        P = int(rng.integers(max(1, -(-Q // 8)), min(E.RS_MAX_TERM, 8 * Q) + 1))
        g = math.gcd(P, Q)
        cases.append((int(rng.integers(1, E.RS_MAX_SAMPLES + 1)), P // g, Q // g))
    for n, P, Q in cases:
        n_out = math.ceil(Fraction(n * Q, P))
        assert rs.out_samples(n, P, Q) == R.out_samples(n, P, Q) == n_out, (n, P, Q)
        for s in (0, 1, n // 3, n - 1, n):
            want = min(n_out, math.floor(Fraction(s * Q + P // 2, P)))
            assert rs.map_sample(s, P, Q, n_out) == R.map_sample(s, P, Q, n_out) == want
            assert abs(want - Fraction(s * Q, P)) <= 1  # (within one output sample of the exact position; the end is clamped)
    assert rs.ratio(24000, 8000) == (3, 1) and rs.ratio(24000, 16000) == (3, 2) and rs.ratio(24000, 44100) == (80, 147)
    assert rs.ratio(24000, 48000) == (1, 2) and rs.ratio(44100, 22050) == (2, 1) and rs.ratio(24000, 96000) == (1, 4)
    for bad in ((24000, 2000), (1000, 24000), (24000, 0), (24000.5, 8000), (-1, 8000)):
        with pytest.raises(ValueError):
            rs.ratio(*bad)
    with pytest.raises(ValueError, match="not reduced"):
        rs.check_ratio(6, 4)
    assert rs.check_ratio(98304, 65536) == (98304, 65536)  # (a pitch ratio stays 16.16)


def test_pitch_ratio_and_the_composition_with_the_rate():
    for s in np.linspace(-12, 12, 97):
        pq, Q = rs.pitch_ratio(float(s))
        assert Q == 65536 and abs(pq - 2.0 ** (s / 12) * 65536) <= 0.5
    assert rs.pitch_ratio(0) == (65536, 65536) and rs.pitch_ratio(12) == (131072, 65536) and rs.pitch_ratio(-12) == (32768, 65536)
    assert rs.pitch_ratio(3) == (77936, 65536) and rs.pitch_ratio(-3) == (55109, 65536)  # (two of the reference's six ratios)
    # rq_eff = round(rq 65536 / pq), and the clip keeps its duration to within the rounding of the two lengths
    for s, rate in ((3, None), (-3, None), (12, None), (-12, None), (5, 1.25), (-7, 0.8), (2.5, 2.0), (-2.5, 0.5)):
        pq, rq_eff = rs.pitch(s, rate)
        rq = int(round((rate or 1.0) * 65536))
        assert rq_eff == math.floor(Fraction(rq * 65536, pq) + Fraction(1, 2)) and 32768 <= rq_eff <= 131072
        n = 24000
        n1 = max(1, (n * 65536 + rq_eff // 2) // rq_eff)
        n2 = rs.out_samples(n1, pq, 65536)
        # |n1 - n 65536 / rq_eff| <= 1/2, the resampler rounds up (< 1), and rq_eff is within 1/2 of rq 65536 / pq
        exact = Fraction(n * 65536, rq)
        slack = Fraction(1, 2) * Fraction(65536, pq) + 1 + exact * Fraction(1, 2 * rq_eff - 1)
        assert abs(n2 - exact) <= slack and slack < 3
    for s, rate, both in ((12.5, None, "12.5"), (-13, 1.0, "-13"), (float("nan"), None, "nan"), (12, 0.9, "0.9"), (-12, 1.2, "1.2"), (7, 0.7, "0.7")):
        with pytest.raises(ValueError, match="pitch=.*speaking_rate=") as e:
            rs.pitch(s, rate)
        assert both in str(e.value)
    # options: what is taken out of the kwargs, and the defaults that build nothing
    kw = dict(pitch=0, sample_rate=24000, top_k=5)
    assert rs.options(kw) == (None, None) and kw == dict(top_k=5)
    assert rs.options(dict(pitch=None, sample_rate=None)) == (None, None) and rs.options({}) == (None, None)
    assert rs.options(dict(pitch=-2, sample_rate=8000)) == (-2.0, 8000) and rs.options(dict(sample_rate=44100.0)) == (None, 44100)
    for bad in (7999, 96001, 22050.5, "16000", True):
        with pytest.raises(ValueError, match="sample_rate="):
            rs.options(dict(sample_rate=bad))
    with pytest.raises(ValueError, match="pitch=12.0 semitones with speaking_rate=0.9"):
        rs.options(dict(pitch=12), 0.9)


# ----------------------------------------------------------------------------------------- ABI
def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def test_rs_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_rs.h")
    assert set(names) == set(E._RS_PROTOS) == {"tt_rs_abi_version", "tt_rs_create", "tt_rs_destroy", "tt_rs_out_samples", "tt_rs_resample"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_rs_abi_version() == 1 == E.RS_ABI_VERSION
    assert lib.tt_tsm_abi_version() == 1 and lib.tt_loud_abi_version() == 1 and lib.tt_abi_version() == 6  # the other headers are untouched
    assert not [n for n in declared_symbols() if n.startswith("tt_rs")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_rs.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_RS_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    mirror = dict(TT_RS_ZEROS=E.RS_ZEROS, TT_RS_PER_ZERO=E.RS_PER_ZERO, TT_RS_TABLE=E.RS_TABLE, TT_RS_BETA=E.RS_BETA, TT_RS_RHO_NUM=E.RS_RHO_NUM,
                  TT_RS_RHO_DEN=E.RS_RHO_DEN, TT_RS_PITCH_ONE=E.RS_PITCH_ONE, TT_RS_MAX_TERM=E.RS_MAX_TERM, TT_RS_MAX_RATIO=E.RS_MAX_RATIO,
                  TT_RS_MAX_SAMPLES=E.RS_MAX_SAMPLES, TT_RS_MAX_CLIPS=E.RS_MAX_CLIPS, TT_RS_OK=E.RS_OK, TT_RS_EMPTY=E.RS_EMPTY,
                  TT_RS_REFUSED=E.RS_REFUSED)
    assert defines == mirror
    assert (R.Z, R.L, R.TABLE, R.BETA, R.RHO_NUM, R.RHO_DEN, R.PITCH_ONE, R.MAX_TERM, R.MAX_RATIO, R.MAX_SAMPLES) == \
        (E.RS_ZEROS, E.RS_PER_ZERO, E.RS_TABLE, E.RS_BETA, E.RS_RHO_NUM, E.RS_RHO_DEN, E.RS_PITCH_ONE, E.RS_MAX_TERM, E.RS_MAX_RATIO, E.RS_MAX_SAMPLES)
    assert E.RS_PITCH_ONE == E.TSM_RATE_ONE and rs.SAMPLE_RATE == E.TSM_SAMPLE_RATE == E.LOUD_SAMPLE_RATE
    h = E.vp()
    for bad in ((0, 1), (E.RS_MAX_SAMPLES + 1, 1), (100, 0), (100, E.RS_MAX_CLIPS + 1)):
        assert lib.tt_rs_create(*bad, C.byref(h)) == -1 and b"tt_rs_create" in lib.tt_last_error()
    assert lib.tt_rs_resample(None, 1, None, None, None, None, None, None, None, None, None) == -1 and b"tt_rs_resample" in lib.tt_last_error()
    rc = lib.tt_rs_create(1000, 2, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_rs_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())
        with pytest.raises(E.EngineError):
            E.check(rc)


def test_library_integers_equal_the_reference():
    lib = _lib()
    rng = np.random.default_rng(5)
    cases = [(n, P, Q) for n in R.LENGTHS + (E.RS_MAX_SAMPLES,) for P, Q in R.RATIOS + R.EXTREME_RATIOS]
    for _ in range(200):
        Q = int(rng.integers(1, E.RS_MAX_TERM + 1))
        P = int(rng.integers(max(1, -(-Q // 8)), min(E.RS_MAX_TERM, 8 * Q) + 1))
        cases.append((int(rng.integers(1, E.RS_MAX_SAMPLES + 1)), P, Q))  # (reduced or not)
    for n, P, Q in cases:
        assert lib.tt_rs_out_samples(n, P, Q) == (R.out_samples(n, P, Q) if R.ratio_ok(P, Q) else 0), (n, P, Q)
    for n, P, Q in ((0, 1, 1), (-1, 1, 1), (E.RS_MAX_SAMPLES + 1, 1, 1), (100, 0, 1), (100, 1, 0), (100, 9, 1), (100, 1, 9), (100, 6, 4),
                    (100, E.RS_MAX_TERM + 1, E.RS_MAX_TERM), (100, -3, 2)):
        assert lib.tt_rs_out_samples(n, P, Q) == 0
    assert lib.tt_rs_out_samples(100, 98304, 65536) == 67  # (not reduced, but a 16.16 pitch ratio)


# ----------------------------------------------------------------------------------------- host flow
class ReferenceResampleStage:
    """stages.ResampleStage backed by tests/resample_reference.py."""
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceResampleStage.made.append(max_samples)

    def resample_many(self, clips, ratios):
        ReferenceResampleStage.calls.append([tuple(r) for r in ratios])
        out = []
        for x, (P, Q) in zip(clips, ratios):
            assert x.dim() == 1 and x.shape[0] <= self.max_samples and P != Q
            y = torch.from_numpy(R.resample(x.numpy(), P, Q, bound=False)[0]).float()
            out.append((y, float(y.abs().max())))
        return out

    def close(self):
        pass


def _ref(clip, P, Q):
    y = R.resample(clip.reshape(-1).numpy(), P, Q, bound=False)[0]
    return torch.from_numpy(y).float().reshape(clip.shape[:-1] + (-1,))


def _install(monkeypatch, api):
    from tests.test_loudness_cpu import ReferenceLoudnessStage
    from tests.test_tsm_cpu import ReferenceStretchStage
    monkeypatch.setattr(api.stages, "ResampleStage", ReferenceResampleStage)
    monkeypatch.setattr(api.stages, "LoudnessStage", ReferenceLoudnessStage)
    monkeypatch.setattr(api.stages, "TimeStretchStage", ReferenceStretchStage)
    ReferenceResampleStage.made, ReferenceResampleStage.calls = [], []
    ReferenceLoudnessStage.made, ReferenceLoudnessStage.calls = [], []
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []
    return ReferenceStretchStage, ReferenceLoudnessStage


def _tts(monkeypatch, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup, voice_latents
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, **kw)
    call = dict(conditioning_latents=voice_latents(cfgs), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
                use_deterministic_seed=7, verbose=False)
    return t, call


def _stretched(clip, rq):
    from tests import tsm_reference as T
    return torch.from_numpy(T.stretch(clip.reshape(-1).numpy(), rq)["y"]).float().reshape(clip.shape[:-1] + (-1,))


def _pitched(clip, s, rate=None):
    pq, rq_eff = rs.pitch(s, rate)
    return _ref(clip if rq_eff == 65536 else _stretched(clip, rq_eff), pq, 65536)


@torch.no_grad()
def test_resample_and_shift_pitch(monkeypatch):
    from tests.test_tsm_cpu import ReferenceStretchStage
    t, _ = _tts(monkeypatch)
    x = torch.from_numpy(R.clip(5000, 0))
    for shape in ((5000,), (1, 5000), (1, 1, 5000)):
        y = t.resample(x.reshape(shape), 16000)
        assert y.shape == shape[:-1] + (3334,) and y.dtype == torch.float32 and torch.equal(y.reshape(-1), _ref(x, 3, 2))
    assert ReferenceResampleStage.made == [30 * 24000] and ReferenceResampleStage.calls == [[(3, 2)]] * 3
    # several clips, rates each, ONE call; a voice clip 44.1 -> 22.05 kHz; the peaks; the same rate is no call and the same clip
    clips = [x, torch.from_numpy(R.clip(1000, 1)).reshape(1, -1), torch.from_numpy(R.clip(37, 2)), x[:100]]
    ReferenceResampleStage.calls = []
    out, peaks = t.resample_many(clips, [8000, 44100, 22050, 24000], from_rates=[24000, 24000, 44100, 24000], return_info=True)
    assert ReferenceResampleStage.calls == [[(3, 1), (80, 147), (2, 1)]]
    assert [tuple(o.shape) for o in out] == [(1667,), (1, 1838), (19,), (100,)] and out[3] is clips[3]
    assert all(torch.equal(o, _ref(c, *r)) for o, c, r in zip(out, clips, ((3, 1), (80, 147), (2, 1))))
    assert peaks == [float(o.abs().max()) for o in out]
    assert t.resample_many([], 16000) == [] and t.resample_many([], 16000, return_info=True) == ([], [])
    # pitch: ONE stretch and ONE resampling for all clips; the duration stays to within the rounding; 0 is the clip itself
    ReferenceResampleStage.calls, ReferenceStretchStage.calls = [], []
    up, down, same = t.shift_pitch_many([x, x.reshape(1, -1), x], [3, -3, 0])
    assert ReferenceStretchStage.calls == [2] and ReferenceResampleStage.calls == [[(77936, 65536), (55109, 65536)]] and same is x
    assert torch.equal(up, _pitched(x, 3)) and torch.equal(down.reshape(-1), _pitched(x, -3)) and down.dim() == 2
    assert abs(up.shape[-1] - 5000) <= 2 and abs(down.shape[-1] - 5000) <= 2
    assert torch.equal(t.shift_pitch(x, 3), up)
    # a longer clip than the stage was built for: it is built again, larger
    t.resample(torch.zeros(30 * 24000 + 1), 48000)
    assert ReferenceResampleStage.made == [30 * 24000, 30 * 24000 + 1]
    with pytest.raises(ValueError, match="ratio 12/1"):
        t.resample(x, 2000)
    with pytest.raises(ValueError, match="positive integers"):
        t.resample(x, 16000.5)
    with pytest.raises(ValueError, match="pitch=13.0 semitones is outside"):
        t.shift_pitch(x, 13)
    with pytest.raises(ValueError, match="3 clips with 2 target rates"):
        t.resample_many(clips[:3], [8000, 16000])
    with pytest.raises(ValueError, match="2 clips with 3 pitches"):
        t.shift_pitch_many(clips[:2], [1, 2, 3])
    with pytest.raises(ValueError, match="expected"):
        t.resample(torch.zeros(2, 100), 16000)
    with pytest.raises(ValueError, match="exceeds"):
        t.resample(torch.zeros(1, E.RS_MAX_SAMPLES + 1), 16000)


@torch.no_grad()
def test_pitch_and_sample_rate_on_tts_and_tts_many(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    from tests.test_loudness_cpu import _ref as levelled
    t, kw = _tts(monkeypatch)
    S, Lv = _install(monkeypatch, __import__("tortoise_tts_amd.api", fromlist=["api"]))
    plain = t.tts(HELLO_THERE, **kw)
    # None, 0 semitones and 24000 Hz: no stage, no call, today's bits
    assert torch.equal(t.tts(HELLO_THERE, pitch=None, sample_rate=None, **kw), plain) and torch.equal(t.tts(HELLO_THERE, pitch=0, sample_rate=24000, **kw), plain)
    assert torch.equal(t.tts_many([HELLO_THERE], pitch=0.0, sample_rate=24000, **kw)[0], plain)
    assert t.resampler is None and t.stretcher is None and ReferenceResampleStage.made == [] and ReferenceResampleStage.calls == [] and S.calls == []
    assert "pitch_s" not in t.timings and "resample_s" not in t.timings
    up = t.tts(HELLO_THERE, pitch=3, **kw)
    assert S.calls == [1] and ReferenceResampleStage.calls == [[(77936, 65536)]] and "pitch_s" in t.timings and "stretch_s" in t.timings
    assert torch.equal(up, _pitched(plain, 3)) and abs(up.shape[-1] - plain.shape[-1]) <= 2 and "diffusion_s" in t.timings
    tel = t.tts(HELLO_THERE, sample_rate=8000, **kw)
    assert torch.equal(tel, _ref(plain, 3, 1)) and tel.shape == (1, 1, rs.out_samples(plain.shape[-1], 3, 1)) and "resample_s" in t.timings
    assert t.resample_info == [float(tel.abs().max())]
    preset = t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **kw)
    assert torch.equal(t.tts_with_preset(HELLO_THERE, preset="ultra_fast", pitch=-3, sample_rate=48000, **kw), _ref(_pitched(preset, -3), 1, 2))
    # everything at once, k winners: ONE stretch at rq_eff, ONE resampling by pq, the level at 24 kHz, the sample rate last
    two = t.tts(HELLO_THERE, k=2, **kw)
    ReferenceResampleStage.calls, S.calls, Lv.calls = [], [], []
    both, state = t.tts(HELLO_THERE, k=2, speaking_rate=1.25, pitch=2, loudness=-19, sample_rate=16000, return_deterministic_state=True, **kw)
    pq, rq_eff = rs.pitch(2, 1.25)
    assert rq_eff == (81920 * 65536 + pq // 2) // pq and state[0] == 7
    assert S.calls == [2] and Lv.calls == [("normalize", 2)] and ReferenceResampleStage.calls == [[(pq, 65536)] * 2, [(3, 2)] * 2]
    assert all(torch.equal(a, _ref(levelled(_pitched(b, 2, 1.25), -19.0), 3, 2)) for a, b in zip(both, two))
    # a pitch that undoes the rate: rq_eff = 65536 is not stretched at all
    S.calls = []
    pq = rs.pitch_ratio(4)[0]
    assert rs.pitch(4, pq / 65536) == (pq, 65536) and torch.equal(t.tts(HELLO_THERE, pitch=4, speaking_rate=pq / 65536, **kw), _ref(plain, pq, 65536))
    assert S.calls == []
    # tts_many: one call per stage for the texts
    many = t.tts_many([HELLO_THERE, HELLO], **kw)
    ReferenceResampleStage.calls, S.calls = [], []
    got = t.tts_many([HELLO_THERE, HELLO], pitch=-3, sample_rate=44100, **kw)
    assert S.calls == [2] and ReferenceResampleStage.calls == [[(55109, 65536)] * 2, [(80, 147)] * 2]
    assert all(torch.equal(a, _ref(_pitched(b, -3), 80, 147)) for a, b in zip(got, many)) and len(t.resample_info) == 2
    for call in (lambda **k: t.tts(HELLO_THERE, **k, **kw), lambda **k: t.tts_many([HELLO_THERE], **k, **kw)):
        with pytest.raises(ValueError, match="pitch=13.0 semitones is outside"):
            call(pitch=13)
        with pytest.raises(ValueError, match="pitch=12.0 semitones with speaking_rate=0.9"):
            call(pitch=12, speaking_rate=0.9)
        with pytest.raises(ValueError, match="sample_rate=4000 Hz is outside"):
            call(sample_rate=4000)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (other unknown kwargs are refused as before)
        t.tts(HELLO_THERE, samplerate=16000, **kw)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):
        t.tts(HELLO_THERE, pitch_shift=2, **kw)


@torch.no_grad()
def test_the_order_is_redaction_rate_pitch_level_sample_rate(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    from tests.test_redaction_cpu import _flow_tts
    t, _ = _flow_tts(monkeypatch)
    from tortoise_tts_amd import api
    S, Lv = _install(monkeypatch, api)
    order = []
    redact = t._redact_clips
    t._redact_clips = lambda wavs, text: (order.append("redact"), redact(wavs, text))[1]
    monkeypatch.setattr(S, "stretch_many", lambda self, clips, rqs, f=S.stretch_many: (order.append(("stretch", list(rqs))), f(self, clips, rqs))[1])
    monkeypatch.setattr(Lv, "normalize_many", lambda self, *a, f=Lv.normalize_many: (order.append("level"), f(self, *a))[1])
    monkeypatch.setattr(ReferenceResampleStage, "resample_many",
                        lambda self, clips, ratios, f=ReferenceResampleStage.resample_many: (order.append(("resample", list(ratios))), f(self, clips, ratios))[1])
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    t.tts("[I am so sad,] hello there", speaking_rate=1.25, pitch=-2, loudness=-23, sample_rate=8000, **kw)
    pq, rq_eff = rs.pitch(-2, 1.25)
    assert order == ["redact", ("stretch", [rq_eff]), ("resample", [(pq, 65536)]), "level", ("resample", [(3, 1)])]
    assert all(k in t.timings for k in ("redact_s", "stretch_s", "pitch_s", "level_s", "resample_s"))


@torch.no_grad()
def test_timings_count_samples_of_the_returned_audio(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_api_flow_cpu import voice_latents, small_setup
    from tortoise_tts_amd import align, longform
    t, m = CC._flow(monkeypatch, candidate_sharding=False)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    plain, al0 = t.tts_with_timings("hello there", **kw)
    assert al0.rate == 24000 and al0.seconds() == al0.seconds(24000) and ReferenceResampleStage.made == []
    res, al = t.tts_with_timings("hello there", sample_rate=16000, **kw)
    n_out = res.shape[-1]
    assert torch.equal(res, _ref(plain, 3, 2)) and al.samples == n_out == rs.out_samples(plain.shape[-1], 3, 2) and al.rate == 16000
    f = lambda s: min(n_out, (s * 2 + 1) // 3)
    assert [w[:3] for w in al.words] == [(w, f(a), f(b)) for w, a, b, _ in al0.words] and al.words[-1][2] > 0
    assert [c[:3] for c in al.chars] == [(c, f(a), f(b)) for c, a, b, _ in al0.chars]
    assert al.seconds() == [(w, a / 16000, b / 16000, c) for w, a, b, c in al.words]
    for (_, a0, b0, _), (_, a1, b1, _) in zip(al0.seconds(), al.seconds()):  # the same moments, to within one 16 kHz sample
        assert abs(a0 - a1) <= 1 / 16000 and abs(b0 - b1) <= 1 / 16000
    assert al.to_srt() == al.to_srt(rate=16000) != al.to_srt(rate=24000)
    # with the pitch: aligned on the shifted 24 kHz clip, then converted
    (res2, state), al2 = t.tts_with_timings("hello there", pitch=3, sample_rate=8000, return_deterministic_state=True, **kw)
    shifted = _pitched(plain, 3)
    assert torch.equal(res2, _ref(shifted, 3, 1)) and state[0] == 7 and al2.rate == 8000 and al2.samples == res2.shape[-1]
    want = align.resample_alignment(CC._expected(m, shifted, "hello there"), 8000, res2.shape[-1])
    assert CC._same(al2, want)
    # long-form: every chunk converted in ONE call, after the alignment; the merged alignment carries the rate
    lkw = dict(conditioning_latents=kw["conditioning_latents"], num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, seed=5,
               texts_are_chunks=True, preset="ultra_fast")
    full0, clips0 = longform.read_long_form(t, ["hello there", "hello"], **lkw)
    ReferenceResampleStage.calls = []
    full, clips = longform.read_long_form(t, ["hello there", "hello"], sample_rate=48000, **lkw)
    assert ReferenceResampleStage.calls == [[(1, 2)] * 2] and all(torch.equal(a, _ref(b, 1, 2)) for a, b in zip(clips, clips0))
    assert torch.equal(full, torch.cat([c.squeeze(0) for c in clips], dim=-1)) and full.shape[-1] == 2 * full0.shape[-1]
    _, lal0 = longform.read_long_form(t, ["hello there", "hello"], return_timings=True, **lkw)
    lfull, lal = longform.read_long_form(t, ["hello there", "hello"], return_timings=True, sample_rate=48000, **lkw)
    assert torch.equal(lfull, full) and lal.rate == 48000 and lal0.rate == 24000 and lal.samples == full.shape[-1]
    assert [w[:3] for w in lal.words] == [(w, 2 * a, 2 * b) for w, a, b, _ in lal0.words]
    assert [s[1:3] for s in lal.seconds()] == [s[1:3] for s in lal0.seconds()]
    # the pitch goes to the chunks' calls
    ReferenceResampleStage.calls = []
    _, pclips = longform.read_long_form(t, ["hello there", "hello"], pitch=3, **lkw)
    assert all(torch.equal(a, _pitched(b, 3)) for a, b in zip(pclips, clips0))


@torch.no_grad()
def test_fast_path_and_streaming_refusals(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    S, Lv = _install(monkeypatch, api_fast)
    one = make(1)
    kw = dict(max_mel_tokens=24, use_deterministic_seed=41)
    plain = one.tts(TEXTS[0], **kw)
    assert torch.equal(one.tts(TEXTS[0], pitch=0, sample_rate=24000, **kw), plain) and ReferenceResampleStage.made == [] and one.resampler is None
    assert torch.equal(one.tts(TEXTS[0], pitch=3, sample_rate=16000, **kw), _ref(_pitched(plain, 3), 3, 2))
    assert S.calls == [1] and ReferenceResampleStage.calls == [[(77936, 65536)], [(3, 2)]]
    both = one.tts_many(TEXTS[:2], **kw)
    ReferenceResampleStage.calls, S.calls = [], []
    got = one.tts_many(TEXTS[:2], speaking_rate=0.8, pitch=-3, sample_rate=8000, **kw)
    pq, rq_eff = rs.pitch(-3, 0.8)
    assert S.calls == [2] and ReferenceResampleStage.calls == [[(pq, 65536)] * 2, [(3, 1)] * 2]
    assert all(torch.equal(a, _ref(_pitched(b, -3, 0.8), 3, 1)) for a, b in zip(got, both))
    with pytest.raises(ValueError, match="pitch=-12.0 semitones with speaking_rate=1.2"):
        one.tts(TEXTS[0], pitch=-12, speaking_rate=1.2, **kw)
    # no pitch and no rate conversion on streamed audio
    with pytest.raises(ValueError, match="tts_stream: pitch is not available for streamed audio"):
        next(one.tts_stream(TEXTS[0], pitch=2, **KW))
    with pytest.raises(ValueError, match="tts_stream: sample_rate is not available for streamed audio"):
        next(one.tts_stream(TEXTS[0], sample_rate=16000, **KW))
    many = make(3)
    with pytest.raises(ValueError, match="open_stream: sample_rate is not available"):
        many.open_stream(TEXTS[0], sample_rate=8000, **KW)
    with pytest.raises(ValueError, match="tts_stream_many: pitch is not available"):
        next(many.tts_stream_many(TEXTS[:2], pitch=-1, **KW))
    with pytest.raises(ValueError, match="speaking_rate is not available"):  # (the existing refusals keep their words)
        many.open_stream(TEXTS[0], speaking_rate=1.2, **KW)
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.ResampleStage)  # (no handle: the checks come before any device work)
    st.h, st.lib = None, _lib()
    st.max_samples, st.max_clips = 1000, 16
    with pytest.raises(ValueError, match="1001 samples"):
        st.resample_many([torch.zeros(1001)], [(3, 2)])
    with pytest.raises(ValueError, match="at least one sample"):
        st.resample_many([torch.zeros(0)], [(3, 2)])
    with pytest.raises(ValueError, match="ratio 6/4"):
        st.resample_many([torch.zeros(10)], [(6, 4)])
    with pytest.raises(ValueError, match="ratio 9/1"):
        st.resample_many([torch.zeros(10)], [(9, 1)])
    with pytest.raises(ValueError, match="2 clips with 1 ratios"):
        st.resample_many([torch.zeros(10), torch.zeros(10)], [(3, 2)])
