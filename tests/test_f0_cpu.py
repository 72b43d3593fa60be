"""The F0 tracker without a GPU: the fp64 reference (tests/f0_reference.py) against known signals, its bounds against an f32 emulation, the
host code (tortoise_tts_amd/pitch.py, the library's plain host functions, csrc/f0_host.h under the sanitizers) and the host flow of
f0() / shift_pitch(to_hz=) / tts(pitch_hz=) on a stage backed by the reference (tests/f0_fake.py).

Measured with this reference (and asserted at twice the reading; the factor covers the seed, not the method): worst error against the true
F0 over the inner frames of the harmonic family 0.369 cents at 40 dB SNR and 3.62 cents at 20 dB, every frame voiced, lags 49 .. 385;
3 of 1200 frames ambiguous; the sequential f32 emulation of d reads 0.034 of its bound; the 100 -> 200 Hz glide is followed to within
21.7 cents of the instantaneous frequency at the frame's time."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from tests import f0_reference as R
from tortoise_tts_amd import align
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import pitch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST_CENTS = {40.0: 0.3692, 20.0: 3.6237}  # read with this reference; asserted at twice
GLIDE_CENTS = 21.70


# ----------------------------------------------------------------------------------------- the reference on known signals
def test_reference_recovers_the_true_f0_on_the_family():
    worst = {snr: 0.0 for snr in R.FAMILY_SNR}
    lags = []
    for f0, snr, x, tr in R.family():
        inner = R.inner_frames(len(x))
        assert len(inner) == 45 and tr["voiced"][inner].all()  # (a frame that hangs over the clip's end into the zeros need not be)
        worst[snr] = max(worst[snr], max(abs(R.cents(tr["f0"][f], f0)) for f in inner))
        lags += [int(tr["lag"][f]) for f in inner]
    print(f"[f0] reference on the family: worst error {worst[40.0]:.4f} cents at 40 dB, {worst[20.0]:.4f} cents at 20 dB; lags {min(lags)} .. {max(lags)}")
    for snr in R.FAMILY_SNR:
        assert worst[snr] <= 2.0 * WORST_CENTS[snr]
    assert 48 <= min(lags) and max(lags) <= 400 and len(R.family()) == 24


def test_ambiguous_share_of_the_family_is_small():
    frames = sum(len(tr["lag"]) for *_, tr in R.family())
    amb = sum(int(tr["ambiguous"].sum()) for *_, tr in R.family())
    print(f"[f0] ambiguous frames of the family: {amb} of {frames}")
    assert frames == 1200 and amb <= 0.05 * frames


def test_bounds_are_what_the_header_says():
    assert R.G_D == pytest.approx(962 * 2.0 ** -24, rel=1e-4) and R.E_DP == pytest.approx(1.1469e-4, rel=1e-3) and R.E_DP > 2 * R.G_D
    _, _, x, tr = R.family()[5]
    assert (tr["dprime_bound"][:, 0] == 0).all() and (tr["dprime_bound"][:, 1:] == R.E_DP * tr["dprime"][:, 1:]).all()
    v = tr["voiced"]
    assert (tr["f0_bound"][v] > 0).all() and (tr["f0_bound"][v] < 0.01).all() and (tr["aper_bound"] > 0).all()


def test_a_sequential_f32_sum_stays_inside_the_bound():
    worst = 0.0
    for k in (3, 10, 21):
        X = R.windows(R.family()[k][2])
        d, d32 = R.difference(X), R.difference_f32_sequential(X).astype(np.float64)
        m = d[:, 1:] > 0
        worst = max(worst, float(np.max(np.abs(d32[:, 1:][m] - d[:, 1:][m]) / (R.G_D * d[:, 1:][m]))))
        assert (d32[:, 1:][~m] == 0).all()
    print(f"[f0] sequential f32 emulation of d: worst |err| / bound {worst:.4f}")
    assert worst <= 1.0


def test_noise_and_silence_have_no_voiced_frame():
    rng = np.random.default_rng(5)
    tr = R.track((0.1 * rng.standard_normal(12000)).astype(np.float32))
    assert not tr["voiced"].any() and (tr["f0"] == 0).all() and tr["aper"].min() > 0.5
    tr = R.track(np.zeros(12000, np.float32))
    assert not tr["voiced"].any() and (tr["dprime"] == 1.0).all() and (tr["lag"] == 48).all() and not tr["ambiguous"].any()
    assert (tr["dprime_bound"] == 0).all()
    # a loud tone under a floor above it: periodic, and unvoiced
    x = R.harmonic(150.0, n=6000)
    assert R.track(x)["voiced"][R.inner_frames(6000)].all() and not R.track(x, floor_e=1e6)["voiced"].any()


def test_a_missing_fundamental_reads_the_fundamental():
    t = np.arange(12000) / R.SR
    x = (0.1 * sum(np.sin(2 * np.pi * 110.0 * h * t + 0.3 * h) for h in range(2, 7))).astype(np.float32)
    tr = R.track(x)
    inner = R.inner_frames(len(x))
    assert tr["voiced"][inner].all() and max(abs(R.cents(tr["f0"][f], 110.0)) for f in inner) < 1.0


def test_a_glide_is_followed():
    t = np.arange(12000) / R.SR
    ph = 2 * np.pi * (100.0 * t + 100.0 * t * t)  # f(t) = 100 + 200 t
    x = sum(np.sin((h + 1) * ph) / (h + 1) for h in range(8))
    x = (0.25 * x / np.sqrt(np.mean(x * x))).astype(np.float32)
    tr = R.track(x)
    inner = R.inner_frames(len(x))
    worst = max(abs(R.cents(tr["f0"][f], 100.0 + 200.0 * f * R.H / R.SR)) for f in inner)
    print(f"[f0] 100 -> 200 Hz glide: worst error against the instantaneous frequency at the frame's time {worst:.2f} cents")
    assert tr["voiced"][inner].all() and worst <= 2.0 * GLIDE_CENTS
    assert np.all(np.diff(tr["f0"][inner]) > 0)


# ----------------------------------------------------------------------------------------- host code
def _lib():
    return E.load_library()


def test_constants_and_plain_host_functions():
    text = open(os.path.join(ROOT, "include", "tortoise_mi355x_f0.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (define("TT_F0_HOP"), define("TT_F0_WINDOW"), define("TT_F0_LEAD"), define("TT_F0_LAG_MIN"), define("TT_F0_LAG_MAX")) == \
        (E.F0_HOP, E.F0_WINDOW, E.F0_LEAD, E.F0_LAG_MIN, E.F0_LAG_MAX) == (R.H, R.W, R.LEAD, R.LAG_MIN, R.LAG_MAX)
    assert (define("TT_F0_MAX_SAMPLES"), define("TT_F0_MAX_CLIPS"), define("TT_F0_SAMPLE_RATE")) == (E.F0_MAX_SAMPLES, E.F0_MAX_CLIPS, E.F0_SAMPLE_RATE)
    assert (define("TT_F0_OK"), define("TT_F0_EMPTY"), define("TT_F0_REFUSED")) == (E.F0_OK, E.F0_EMPTY, E.F0_REFUSED)
    lib = _lib()
    assert lib.tt_f0_abi_version() == E.F0_ABI_VERSION == 1 and lib.tt_op_f0_group() == 4
    for n in (1, 239, 240, 241, 719, 720, 721, 959, 960, 961, 1919, 1920, 1921, 12000, E.F0_MAX_SAMPLES):
        assert lib.tt_f0_frames(n) == P.frames(n) == R.frames(n)
    assert lib.tt_f0_frames(0) == 0 and lib.tt_f0_frames(-5) == 0 and lib.tt_f0_frames(E.F0_MAX_SAMPLES + 1) == 0
    lo, hi = C.c_int(-7), C.c_int(-7)
    for hz in range(50, 1001):  # every integer frequency, as either end
        assert lib.tt_f0_lags(float(hz), 1000.0, lo, hi) == 0 and (lo.value, hi.value) == P.lags(hz, 1000) == (24, 24000 // hz)
        assert lib.tt_f0_lags(50.0, float(hz), lo, hi) == 0 and (lo.value, hi.value) == P.lags(50, hz) == (-(-24000 // hz), 480)
    assert P.lags(60, 500) == (48, 400) and P.lags(62.5, 490) == (49, 384)
    for bad in ((49.9, 500), (60, 1000.5), (500, 60), (999, 999)):
        assert lib.tt_f0_lags(float(bad[0]), float(bad[1]), lo, hi) == -1 and b"tt_f0_lags" in lib.tt_last_error()
        with pytest.raises(ValueError, match="fmin="):
            P.lags(*bad)
    assert lib.tt_f0_lags(60.0, 500.0, None, hi) == -1 and b"null argument" in lib.tt_last_error()
    h = E.vp()
    assert lib.tt_f0_create(0, 1, h) == -1 and b"max_samples 0 (1 .. 8388608)" in lib.tt_last_error() and not h
    assert lib.tt_f0_create(100, 0, h) == -1 and b"max_clips 0 (1 .. 64)" in lib.tt_last_error()
    assert lib.tt_f0_create(100, 1, None) == -1 and b"null argument" in lib.tt_last_error()


def test_options_are_validated():
    p = P.params()
    assert p == P.Params(48, 400, 0.15, 960 * 10.0 ** -5.0) and P.params(fmin=50, fmax=1000, threshold=0, floor_db=0) == P.Params(24, 480, 0.0, 960.0)
    for kw, what in ((dict(fmin=49), "fmin=49"), (dict(fmax=1001), "fmax=1001"), (dict(fmin=300, fmax=200), "fmin=300"), (dict(threshold=-0.1), "threshold=-0.1"),
                     (dict(threshold=2.5), "threshold=2.5"), (dict(threshold=float("nan")), "threshold=nan"), (dict(floor_db=1), "floor_db=1"),
                     (dict(floor_db=-300), "floor_db=-300"), (dict(fmin="60"), "fmin='60'"), (dict(fmax=True), "fmax=True")):
        with pytest.raises(ValueError, match=re.escape(what)):
            P.params(**kw)
    assert P.target_hz("to_hz", 180) == 180.0
    for bad in (49.9, 1000.1, float("nan"), "180", None):
        with pytest.raises(ValueError, match="to_hz="):
            P.target_hz("to_hz", bad)
    # the keyword of a tts() call
    kw = dict(pitch_hz=180, other=1)
    assert P.options(kw) == 180.0 and kw == dict(other=1) and P.options({}) is None and P.options(dict(pitch_hz=None)) is None
    with pytest.raises(ValueError, match="tts: pitch_hz= .an absolute pitch. goes with neither pitch= nor word_pitches="):
        P.options(dict(pitch_hz=180), 2.0)
    with pytest.raises(ValueError, match="goes with neither"):
        P.options(dict(pitch_hz=180, word_pitches=[1]))
    with pytest.raises(ValueError, match="pitch_hz=20"):
        P.options(dict(pitch_hz=20))
    assert P.formant_keywords(dict(formants="keep", formant_lifter_ms=2, k=1)) == dict(formants="keep", formant_lifter_ms=2)
    # the shift
    assert P.shift_to(150.0, 300.0) == (12.0, False) and P.shift_to(200.0, 100.0) == (-12.0, False)
    s, c = P.shift_to(150.0, 180.0)
    assert s == pytest.approx(3.1564, abs=1e-4) and not c
    with pytest.warns(UserWarning, match=r"clip 2: 100.0 Hz -> 250 Hz is \+15.86 semitones.*clamped to \+12"):
        assert P.shift_to(100.0, 250.0, clip=2) == (12.0, True)
    with pytest.warns(UserWarning, match="clamped to -12"):
        assert P.shift_to(400.0, 100.0, "tts") == (-12.0, True)
    with pytest.warns(UserWarning, match="fewer than 10 voiced frames.*returned as it is"):
        assert P.shift_to(None, 180.0) == (0.0, False)
    # the refusals, in the house wording
    for f, who, what in ((P.refuse_streaming, "tts_stream", "for streamed audio"), (P.refuse_long_form, "read_long_form", "for a reading"),
                         (P.refuse_sharded, "tts", "on a sharded job")):
        f({}, who)
        with pytest.raises(ValueError, match=f"{who}: pitch_hz is not available {what}"):
            f(dict(pitch_hz=180), who)


def test_f0track():
    hz = np.zeros(30, np.float32)
    hz[5:25] = np.linspace(100, 200, 20)
    tr = P.F0Track(hz, np.full(30, 0.1), np.full(30, 100), samples=7200)
    assert len(tr) == 30 and tr.hop_seconds == 0.01 and tr.voiced.sum() == 20 and tr.times()[3] == pytest.approx(0.03)
    assert tr.median_hz() == pytest.approx(150.0, abs=1e-3) and tr.median_hz(min_voiced=21) is None
    st = tr.semitones(100.0)
    assert np.isnan(st[0]) and st[5] == pytest.approx(0.0, abs=1e-6) and st[24] == pytest.approx(12.0, abs=1e-5)
    want = 12 * math.log2(np.percentile(hz[5:25].astype(np.float64), 95) / np.percentile(hz[5:25].astype(np.float64), 5))
    assert tr.range_semitones() == pytest.approx(want) and tr.range_semitones(0, 100) == pytest.approx(12.0, abs=1e-5)
    assert tr.range_semitones(min_voiced=21) is None
    assert tr.at(0.0) == 0.0 and tr.at(0.05) == pytest.approx(100.0) and tr.at(0.054) == pytest.approx(100.0) and tr.at(0.056) == hz[6]
    for bad in (-0.01, 0.296, float("nan")):
        with pytest.raises(ValueError, match="seconds=|outside the clip"):
            tr.at(bad)
    with pytest.raises(ValueError, match="percentiles"):
        tr.range_semitones(60, 40)
    with pytest.raises(ValueError, match="must be one"):
        P.F0Track(hz, np.zeros(3), np.zeros(30))
    few = P.F0Track(np.array([0, 120, 0], np.float32), np.zeros(3), np.zeros(3))
    assert few.median_hz() is None and few.median_hz(min_voiced=1) == 120.0
    # one median per word of an Alignment; a word with no voiced frame, and one with an empty span, read None
    al = align.Alignment("a b c d", [], [("a", 1200, 2400, 1.0), ("b", 2400, 2400, float("nan")), ("c", 3600, 6000, 1.0), ("d", 6240, 7200, 1.0)], 0.0, 7200)
    got = tr.for_words(al)
    assert got[0] == pytest.approx(float(np.median(hz[5:10]))) and got[1] is None and got[2] == pytest.approx(float(np.median(hz[15:25]))) and got[3] is None
    assert repr(al) == repr(align.Alignment("a b c d", [], list(al.words), 0.0, 7200))  # Alignment itself does not change
    half = align.Alignment("a", [], [("a", 600, 1200, 1.0)], 0.0, 3600, rate=12000)     # positions at another rate: the same times
    assert tr.for_words(half) == [got[0]]


# ----------------------------------------------------------------------------------------- host flow on the reference stage
def _host(monkeypatch):
    from tests import f0_fake
    from tests.test_resample_cpu import ReferenceResampleStage, _tts
    from tests.test_tsm_cpu import ReferenceStretchStage
    t, kw = _tts(monkeypatch)
    from tortoise_tts_amd import api
    F = f0_fake.install(monkeypatch, api)
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []
    ReferenceResampleStage.made, ReferenceResampleStage.calls = [], []
    return t, kw, F, ReferenceStretchStage, ReferenceResampleStage


def _tone(hz, n=4800, seed=1):
    return torch.from_numpy(R.harmonic(hz, n=n, seed=seed).copy())


@torch.no_grad()
def test_f0_and_shift_pitch_to_hz(monkeypatch):
    t, _, F, St, Rs = _host(monkeypatch)
    x = _tone(150.0)
    for shape in ((4800,), (1, 4800), (1, 1, 4800)):
        tr = t.f0(x.reshape(shape))
        assert isinstance(tr, P.F0Track) and len(tr) == 20 and tr.samples == 4800 and abs(R.cents(tr.median_hz(), 150.0)) < 2.0
    assert F.calls == [1, 1, 1] and F.made == [30 * 24000] and t.f0_many([]) == [] and F.calls == [1, 1, 1]
    ref = R.track(x.numpy(), 48, 400, 0.15, 960e-5)
    assert tr.hz.tobytes() == ref["f0"].astype(np.float32).tobytes() and (tr.lag == ref["lag"]).all()
    assert t.f0(x, fmin=100, fmax=200, threshold=0.1, floor_db=-60).lag.min() >= 120
    with pytest.raises(ValueError, match="fmin=20"):
        t.f0(x, fmin=20)
    with pytest.raises(ValueError, match="f0: clip 0 of shape"):
        t.f0(torch.zeros(2, 100))
    # to_hz: ONE measurement for all clips, then the path of semitones= with a shift per clip
    F.calls, St.calls, Rs.calls = [], [], []
    y, info = t.shift_pitch(x, to_hz=180.0, return_info=True)
    med = tr.median_hz()
    assert info["measured_hz"] == med and info["semitones"] == 12 * math.log2(180.0 / med) and not info["clamped"] and info["peak"] == float(y.abs().max())
    assert torch.equal(y, t.shift_pitch(x, info["semitones"])) and t.pitch_info[0]["measured_hz"] == med and F.calls == [1]
    assert abs(R.cents(t.f0(y).median_hz(), 180.0)) < 5.0
    clips = [x, _tone(220.0, 3600, 2).reshape(1, -1), torch.zeros(3000)]
    F.calls, St.calls = [], []
    with pytest.warns(UserWarning, match="shift_pitch: clip 2: fewer than 10 voiced frames"):
        out, infos = t.shift_pitch_many(clips, to_hz=[180.0, 200.0, 180.0], return_info=True)
    assert F.calls == [3] and len(St.calls) == 1  # one measurement, one stretch call for the clips that move
    assert out[2] is clips[2] and infos[2] == dict(measured_hz=None, semitones=0.0, clamped=False, peak=0.0)  # no median: bit for bit
    assert torch.equal(out[0], y) and out[1].shape[0] == 1 and torch.equal(out[1], t.shift_pitch(clips[1], infos[1]["semitones"]))
    # a shift beyond +-12 is clamped, with a warning
    with pytest.warns(UserWarning, match=r"shift_pitch: 150\.\d Hz -> 400 Hz is \+16\.\d+ semitones.*clamped to \+12"):
        up, info = t.shift_pitch(x, to_hz=400.0, return_info=True)
    assert info["clamped"] and info["semitones"] == 12.0 and torch.equal(up, t.shift_pitch(x, 12))


@torch.no_grad()
def test_exactly_one_of_semitones_pitch_map_to_hz(monkeypatch):
    t, _, F, _, _ = _host(monkeypatch)
    x = _tone(150.0)
    for kw in (dict(), dict(semitones=2, to_hz=180.0), dict(pitch_map=[(0, 1)], to_hz=180.0), dict(semitones=2, pitch_map=[(0, 1)], to_hz=180.0)):
        with pytest.raises(ValueError, match="exactly one of semitones and pitch_map, or to_hz"):
            t.shift_pitch(x, **kw)
    with pytest.raises(ValueError, match="return_map=True goes with pitch_map"):
        t.shift_pitch(x, to_hz=180.0, return_map=True)
    with pytest.raises(ValueError, match="to_hz=1200"):
        t.shift_pitch(x, to_hz=1200.0)
    with pytest.raises(ValueError, match="2 clips with 3 target pitches"):
        t.shift_pitch_many([x, x], to_hz=[100.0, 120.0, 140.0])
    with pytest.raises(ValueError, match="formants='loud'"):
        t.shift_pitch(x, to_hz=180.0, formants="loud")
    assert F.calls == []  # every refusal comes before the measurement
    assert torch.equal(t.shift_pitch(x, 2), t.shift_pitch_many([x], 2)[0])  # the positional form of today


@torch.no_grad()
def test_pitch_hz_on_tts(monkeypatch):
    from tests.test_api_flow_cpu import HELLO_THERE
    t, kw, F, St, Rs = _host(monkeypatch)
    plain = t.tts(HELLO_THERE, **kw)
    assert torch.equal(t.tts(HELLO_THERE, pitch_hz=None, **kw), plain) and F.made == [] and t.f0_stage is None and t.pitch_info is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the fake stages' clip may have no median, or one far away)
        got = t.tts(HELLO_THERE, pitch_hz=180.0, **kw)
        info = t.pitch_info
        want = t.shift_pitch_many([plain], to_hz=180.0)[0]
    assert torch.equal(got, want) and F.calls == [1, 1] and len(info) == 1 and set(info[0]) >= {"measured_hz", "semitones", "clamped"}
    assert "f0_s" in t.timings
    # several winners: ONE measurement
    F.calls = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        two = t.tts(HELLO_THERE, k=2, pitch_hz=180.0, **kw)
        both = t.tts_many([HELLO_THERE, HELLO_THERE[:6]], pitch_hz=200.0, **kw)
    assert len(two) == 2 and F.calls[0] == 2 and len(both) == 2 and F.calls[-1] == 2
    assert torch.equal(t.tts(HELLO_THERE, **kw), plain)  # without the keyword, today's bits
    # exclusive with the relative forms; validated before anything renders
    for bad, what in ((dict(pitch_hz=180.0, pitch=2), "goes with neither pitch= nor word_pitches="), (dict(pitch_hz=20.0), "pitch_hz=20"),
                      (dict(pitch_hz="high"), "pitch_hz='high'")):
        with pytest.raises(ValueError, match=what):
            t.tts(HELLO_THERE, **bad, **kw)
        with pytest.raises(ValueError, match=what):
            t.tts_many([HELLO_THERE], **bad, **kw)
        with pytest.raises(ValueError, match=what):
            t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **bad, **kw)


@torch.no_grad()
def test_refusals_on_readings_streams_and_shards(monkeypatch):
    from tortoise_tts_amd import longform
    with pytest.raises(ValueError, match="read_long_form: pitch_hz is not available for a reading"):
        longform.read_long_form(None, "hello there", pitch_hz=180.0)
    from tests.test_resample_cpu import _install
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    from tests import f0_fake
    api_fast, make = _instances(monkeypatch)
    _install(monkeypatch, api_fast)
    F = f0_fake.install(monkeypatch, api_fast)
    one = make(1)
    kw = dict(max_mel_tokens=24, use_deterministic_seed=41)
    plain = one.tts(TEXTS[0], **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = one.tts(TEXTS[0], pitch_hz=180.0, **kw)
        assert torch.equal(got, one.shift_pitch_many([plain], to_hz=180.0)[0]) and F.calls == [1, 1]
        many = one.tts_many(TEXTS[:2], pitch_hz=180.0, **kw)
    assert len(many) == 2 and F.calls[-1] == 2 and torch.equal(one.tts(TEXTS[0], **kw), plain)
    with pytest.raises(ValueError, match="tts_stream: pitch_hz is not available for streamed audio"):
        next(one.tts_stream(TEXTS[0], pitch_hz=180.0, **KW))
    wide = make(3)
    with pytest.raises(ValueError, match="open_stream: pitch_hz is not available for streamed audio"):
        wide.open_stream(TEXTS[0], pitch_hz=180.0, **KW)
    with pytest.raises(ValueError, match="tts_stream_many: pitch_hz is not available for streamed audio"):
        next(wide.tts_stream_many(TEXTS[:2], pitch_hz=180.0, **KW))
    assert not wide._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.F0Stage)  # (no handle: the checks come before any device work)
    st.h, st.lib = None, _lib()
    st.max_samples, st.max_clips = 1000, 16
    with pytest.raises(ValueError, match="1001 samples exceed the F0 stage's capacity"):
        st.track_many([torch.zeros(1001)], [P.params()])
    with pytest.raises(ValueError, match="at least one sample"):
        st.track_many([torch.zeros(0)], [P.params()])
    with pytest.raises(ValueError, match="2 clips with 1 parameter sets"):
        st.track_many([torch.zeros(10), torch.zeros(10)], [P.params()])


# ----------------------------------------------------------------------------------------- the host code under the sanitizers
def test_host_check_builds_and_passes_under_the_sanitizers(tmp_path):
    """csrc/checks/f0_host_check.cpp: a stand-alone program (its own main) over f0_host.h, compiled with ASan + UBSan and run on the CPU -
    the frame counts at every border, the lags of every integer frequency, every refusal."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    src = os.path.join(ROOT, "tortoise_tts_amd", "csrc", "checks", "f0_host_check.cpp")
    exe = str(tmp_path / "f0_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "f0_host_check: ok" in r.stdout, r.stdout + r.stderr
