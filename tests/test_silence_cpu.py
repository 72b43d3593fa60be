"""The silence stage without a GPU: the reference against first principles, the device's closed-form labelling against bridge-then-dilate,
the cut arithmetic, the options and every refusal, the header against its Python mirror, and the host flow (trim_silence=, max_pause=, trim,
speech_regions, read_long_form(pause=)) on a reference-backed stage."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import silence_reference as R
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import silence as sil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- the reference against first principles
def test_energies_are_exact_and_the_band_comes_from_the_format():
    x = R.build([("s", 700), ("l", 333), ("z", 100)], 3)
    e = R.energies(x)
    assert len(e) == R.frames(len(x)) == 5
    for f in range(len(e)):
        exact = sum(Fraction(float(v)) ** 2 for v in x[f * R.HOP:f * R.HOP + R.FRAME])
        assert abs(Fraction(float(e[f])) - exact) <= Fraction(2.0 ** -53) * exact  # rounded once
    # the device's order of operations, in f64: inside the band, and the band is gamma_(K+1) with K = 4 S + 3 = 483
    q = []
    for s in range(R.slots(len(x))):
        acc = 0.0
        for v in x[s * R.S:(s + 1) * R.S].astype(np.float64):
            acc = acc + v * v  # (v * v is exact in f64, so this is the FMA's single rounding)
        q.append(acc)
    q += [0.0] * 4
    dev = np.array([((q[2 * f] + q[2 * f + 1]) + q[2 * f + 2]) + q[2 * f + 3] for f in range(len(e))])
    assert (np.abs(dev - e) <= R.band(e)).all() and R.K_OPS == 483
    assert R.band(np.array([1.0]))[0] == 484 * 2.0 ** -53 / (1 - 484 * 2.0 ** -53)


def test_a_frame_at_its_threshold_is_reported_undecided():
    e = np.array([1.0, 1e-4, 1e-4 * (1 + 2e-14), 1e-4 * (1 - 2e-14), 1e-4 * (1 + 1e-9), 0.0, 2e-4, 0.5e-4])
    active, undecided, E_ = R.activity(e, 1e-4, 0.0)
    assert E_ == 1.0 and undecided.tolist() == [False, True, True, True, False, False, False, False]
    assert active.tolist()[4:] == [True, False, True, False] and active[0]
    # the floor: exact, so only the energy's own band counts
    active, undecided, _ = R.activity(np.array([1.0, 0.25, 0.25 * (1 + 2e-14), 0.3]), 1e-4, 0.25)
    assert undecided.tolist() == [False, True, True, False] and active.tolist() == [True, False, True, True]
    # all-zero audio: no frame is active and none is undecided
    active, undecided, E_ = R.activity(np.zeros(4), 1e-4, 0.0)
    assert E_ == 0.0 and not active.any() and not undecided.any()


def test_closed_form_equals_bridge_then_dilate():
    rng = np.random.default_rng(11)
    for _ in range(3000):
        F = int(rng.integers(1, 60))
        flags = (rng.random(F) < rng.choice([0.05, 0.2, 0.5, 0.9])).tolist()
        min_sil, pad = int(rng.integers(0, 12)), int(rng.integers(0, 8))
        assert R.label_closed(flags, min_sil, pad) == R.label(flags, min_sil, pad), (flags, min_sil, pad)
    assert R.label([False] * 5, 3, 2) == [False] * 5
    assert R.label([0, 0, 1, 0, 0, 0, 1, 0, 0, 0], 4, 0) == [False, False] + [True] * 5 + [False] * 3   # a gap of 3 < 4 is bridged
    assert R.label([0, 0, 1, 0, 0, 0, 1, 0, 0, 0], 3, 0) == [bool(v) for v in [0, 0, 1, 0, 0, 0, 1, 0, 0, 0]]
    assert R.label([0, 0, 0, 1, 0, 0, 0], 0, 2) == [False, True, True, True, True, True, False]
    assert R.regions([True, True, False, True], 900) == [(0, 480), (720, 900)] and R.regions([False] * 3, 700) == []


def test_the_cut_keeps_exactly_max_pause():
    for M in (R.X, R.X + 1, 121, 240, 2279, 2280, 2281, 7200, 7201):
        M1, M2 = R.cut_lengths(M)
        assert M1 + M2 - R.X == M and M1 >= R.X and M2 >= R.X and M1 - M2 in (0, 1)
        for G in (M + R.X - 1, M + R.X, M + R.X + 1, M + 5000):
            a, b = 1000, 1000 + G  # a pause [a, b) between two regions
            n = b + 700
            segs, n_out, D0, Dt = R.plan(n, [(0, a), (b, n)], -1, -1, M)
            if G < M + R.X:
                assert segs == [(0, 0, n)] and n_out == n
                continue
            assert M1 + M2 <= G  # the kept head and tail do not overlap in the input
            assert segs == [(0, 0, a + M1), (a + M1, b - M2 + R.X, n - (b - M2 + R.X))] and n_out == n - (G - M) and (D0, Dt) == (0, 0)
            assert R.map_sample(b, segs) - R.map_sample(a, segs) == M  # exactly max_pause between the two regions
            x = np.arange(1, n + 1, dtype=np.float32)
            y, bound, ops = R.render(x, segs, n_out, 0, 0)
            m = a + M1 - R.X  # the cross-fade: head x[m + j] -> tail x[b - M2 + j]
            assert (ops[m:m + R.X] == 3).all() and ops.sum() == 3 * R.X and (bound[ops == 0] == 0).all()
            j = np.arange(R.X)
            w = (2 * j + 1) / 240.0
            assert np.allclose(y[m:m + R.X], (1 - w) * x[m + j] + w * x[b - M2 + j], rtol=1e-15)
            assert (y[:m] == x[:m]).all() and (y[m + R.X:] == x[b - M2 + R.X:]).all()
            y32, _ = R.trim_f32(x, (0.0, 0.0, 0, 0, -1, -1, -1))
            assert y32.tobytes() == x.tobytes()


def test_edges_and_fades():
    x = R.build([("z", 3000), ("s", 3000), ("z", 3000)], 5)
    r = R.trim(x, R.params(lead=1200, trail=600))
    assert r["regions"] == [(1440, 7200)] and (r["D0"], r["Dt"]) == (240, 1200) and r["segments"] == [(0, 240, 7560)] and r["status"] == R.OK
    assert (r["ops"][:R.X] == 2).all() and (r["ops"][-R.X:] == 2).all() and r["ops"][R.X:-R.X].sum() == 0
    y32, _ = R.trim_f32(x, R.params(lead=1200, trail=600))
    assert (np.abs(y32 - r["y"]) <= r["bound"]).all() and y32[R.X:-R.X].tobytes() == x[240 + R.X:7800 - R.X].tobytes()
    # a gap that is not longer than what may stay is left alone, and -1 leaves it alone whatever its length
    assert R.trim(x, R.params(lead=1440, trail=1800))["status"] == R.UNCHANGED
    assert R.trim(x, R.params(lead=1439, trail=1800))["D0"] == 1 and R.trim(x, R.params(lead=-1, trail=-1))["status"] == R.UNCHANGED
    r = R.trim(x, R.params(lead=0, trail=0))
    assert r["n_out"] == 7200 - 1440 and r["segments"] == [(0, 1440, 5760)]
    # silent: unchanged, never emptied
    z = np.zeros(5000, np.float32)
    r = R.trim(z, R.params(lead=0, trail=0, max_pause=120))
    assert r["status"] == R.SILENT and r["n_out"] == 5000 and r["regions"] == [] and r["segments"] == [(0, 0, 5000)] and not r["y"].any()
    assert R.trim(np.zeros(0, np.float32), R.params())["status"] == R.EMPTY
    for bad in (dict(max_pause=119), dict(max_pause=0), dict(lead=-2), dict(min_sil=-1), dict(pad=6001), dict(trail=R.MAX_SAMPLES + 1)):
        assert R.trim(x, R.params(**bad))["status"] == R.REFUSED, bad


def test_map_sample():
    segs = [(0, 240, 10740), (10740, 11940, 9660)]  # 240 dropped at the start, 960 cut from a pause, the end dropped after 21600
    n_out = 20400
    for s, want in ((0, 0), (239, 0), (240, 0), (241, 1), (10979, 10739), (10980, 10740), (11500, 10740), (11940, 10740), (11941, 10741),
                    (21599, 20399), (21600, 20400), (23999, 20400)):
        assert sil.map_sample(s, segs) == R.map_sample(s, segs) == want, s
    rng = np.random.default_rng(2)
    x = R.build([p for _ in range(6) for p in (("s", 1300), ("z", 1900))], 1)
    r = R.trim(x, R.params(pad=1, min_sil=2, max_pause=600, lead=100, trail=50))
    assert len(r["segments"]) == 6
    prev = -1
    for s in sorted(rng.integers(0, len(x), 300).tolist()) + [len(x) - 1]:
        m = sil.map_sample(s, r["segments"])
        assert m == R.map_sample(s, r["segments"]) and prev <= m <= r["n_out"]  # monotone, inside the output
        prev = m
    assert sil.pauses(r["regions"], len(x)) == [(b, a) for (_, b), (a, _) in zip(r["regions"], r["regions"][1:])]


# ----------------------------------------------------------------------------------------- options
def test_options_and_every_refusal():
    assert sil.params() == sil.Params(1e-4, 480 * 1e-7, 10, 5, 1200, 2400, -1) == sil.Params(*R.params())
    p = sil.params(lead=None, trail=0, max_pause=0.3, top_db=30, floor_db=-60, min_silence=0.25, pad=0)
    assert p == sil.Params(10.0 ** -3.0, 480 * 10.0 ** -6.0, 25, 0, -1, 0, 7200)
    assert sil.params(max_pause=0.005).max_pause == 120 and sil.params(min_silence=0.004).min_sil == 0 and sil.params(pad=0.015).pad == 2
    assert sil.params(lead=0.00002).lead == 0 and sil.params(lead=1 / 24000).lead == 1  # round(s * 24000)
    for bad, word in ((dict(max_pause=0.004), "max_pause"), (dict(max_pause=0), "max_pause"), (dict(max_pause=-1), "max_pause"),
                      (dict(lead=-0.1), "lead"), (dict(trail=float("nan")), "trail"), (dict(trail="0.1"), "trail"), (dict(lead=True), "lead"),
                      (dict(lead=350), "lead"), (dict(top_db=0), "top_db"), (dict(top_db=121), "top_db"), (dict(top_db=None), "top_db"),
                      (dict(floor_db=1), "floor_db"), (dict(floor_db=-201), "floor_db"), (dict(min_silence=-0.01), "min_silence"),
                      (dict(min_silence=61), "min_silence"), (dict(pad=None), "pad"), (dict(pad=60.5), "pad")):
        with pytest.raises(ValueError, match=word + "="):
            sil.params(**bad)
    # what is taken out of a call's kwargs, and the defaults that build nothing
    kw = dict(trim_silence=None, max_pause=None, top_k=5)
    assert sil.options(kw) is None and kw == dict(top_k=5)
    assert sil.options({}) is None and sil.options(dict(trim_silence=False)) is None
    assert sil.options(dict(trim_silence=True)) == sil.params()
    assert sil.options(dict(trim_silence=True, max_pause=0.3)) == sil.params(max_pause=0.3)
    assert sil.options(dict(max_pause=0.3)) == sil.params(lead=None, trail=None, max_pause=0.3)  # only the pauses: the ends are left alone
    assert sil.options(dict(trim_silence=dict(lead=0, pad=0.02, max_pause=1.0))) == sil.params(lead=0, pad=0.02, max_pause=1.0)
    assert sil.options(dict(trim_silence=dict(max_pause=1.0), max_pause=0.5)) == sil.params(max_pause=0.5)  # the keyword takes the dict's place
    with pytest.raises(ValueError, match="unknown options \\['leed'\\]"):
        sil.options(dict(trim_silence=dict(leed=0)))
    with pytest.raises(ValueError, match="trim_silence=0.5"):
        sil.options(dict(trim_silence=0.5))
    with pytest.raises(ValueError, match="max_pause=0.001"):
        sil.options(dict(trim_silence=True, max_pause=0.001))
    # read_long_form(pause=): both ends cut to the speech, the rest as given
    kw = dict(trim_silence=dict(pad=0.02, lead=0.3), max_pause=0.4)
    assert sil.for_long_form(kw, 0.25) == 6000 and kw == dict(trim_silence=dict(pad=0.02, lead=0.0, trail=0.0), max_pause=0.4)
    assert sil.options(kw) == sil.params(pad=0.02, lead=0, trail=0, max_pause=0.4)
    kw = {}
    assert sil.for_long_form(kw, 0) == 0 and sil.options(kw) == sil.params(lead=0, trail=0)
    kw = dict(trim_silence=True)
    assert sil.for_long_form(kw, 1.5) == 36000 and sil.options(kw) == sil.params(lead=0, trail=0)
    for bad in (-0.5, float("inf"), "1", 400):
        with pytest.raises(ValueError, match="pause="):
            sil.for_long_form({}, bad)
    with pytest.raises(ValueError, match="max_pause=0.001"):
        sil.for_long_form(dict(max_pause=0.001), 0.5)
    for who in ("tts_stream", "open_stream", "tts_stream_many"):
        for k in ("trim_silence", "max_pause"):
            with pytest.raises(ValueError, match=f"{who}: {k} is not available for streamed audio"):
                sil.refuse_streaming({k: None}, who)
    sil.refuse_streaming(dict(top_k=3), "tts_stream")
    assert sil.frames(241) == 2 and sil.max_regions(241) == 1 and sil.max_regions(481) == 2


# ----------------------------------------------------------------------------------------- ABI
def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def test_sil_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_sil.h")
    assert set(names) == set(E._SIL_PROTOS) == {"tt_sil_abi_version", "tt_sil_create", "tt_sil_destroy", "tt_sil_frames", "tt_sil_max_regions",
                                                "tt_sil_find", "tt_sil_trim"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_sil_abi_version() == 1 == E.SIL_ABI_VERSION
    # the other headers are untouched
    assert lib.tt_rs_abi_version() == 1 and lib.tt_tsm_abi_version() == 1 and lib.tt_loud_abi_version() == 1 and lib.tt_abi_version() == 6
    assert not [n for n in declared_symbols() if n.startswith("tt_sil")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_sil.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_SIL_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    mirror = dict(TT_SIL_SLOT=E.SIL_SLOT, TT_SIL_HOP=E.SIL_HOP, TT_SIL_FRAME=E.SIL_FRAME, TT_SIL_FADE=E.SIL_FADE, TT_SIL_SAMPLE_RATE=E.SIL_SAMPLE_RATE,
                  TT_SIL_MAX_SAMPLES=E.SIL_MAX_SAMPLES, TT_SIL_MAX_CLIPS=E.SIL_MAX_CLIPS, TT_SIL_MAX_FRAMES_PARAM=E.SIL_MAX_FRAMES_PARAM,
                  TT_SIL_OK=E.SIL_OK, TT_SIL_UNCHANGED=E.SIL_UNCHANGED, TT_SIL_SILENT=E.SIL_SILENT, TT_SIL_EMPTY=E.SIL_EMPTY,
                  TT_SIL_REFUSED=E.SIL_REFUSED)
    assert defines == mirror
    assert (R.S, R.HOP, R.FRAME, R.X, R.SAMPLE_RATE, R.MAX_SAMPLES, R.MAX_CLIPS, R.MAX_FRAMES_PARAM) == \
        (E.SIL_SLOT, E.SIL_HOP, E.SIL_FRAME, E.SIL_FADE, E.SIL_SAMPLE_RATE, E.SIL_MAX_SAMPLES, E.SIL_MAX_CLIPS, E.SIL_MAX_FRAMES_PARAM)
    assert (E.SIL_SLOT, E.SIL_HOP, E.SIL_FRAME, E.SIL_FADE, E.SIL_MAX_SAMPLES, E.SIL_MAX_CLIPS) == (120, 240, 480, 120, 2 ** 23, 64)
    assert (R.OK, R.UNCHANGED, R.SILENT, R.EMPTY, R.REFUSED) == (E.SIL_OK, E.SIL_UNCHANGED, E.SIL_SILENT, E.SIL_EMPTY, E.SIL_REFUSED)
    assert sil.SAMPLE_RATE == E.SIL_SAMPLE_RATE == E.TSM_SAMPLE_RATE == E.LOUD_SAMPLE_RATE and sil.FRAMES_PER_SECOND * E.SIL_HOP == sil.SAMPLE_RATE
    h = E.vp()
    for bad in ((0, 1), (E.SIL_MAX_SAMPLES + 1, 1), (100, 0), (100, E.SIL_MAX_CLIPS + 1)):
        assert lib.tt_sil_create(*bad, C.byref(h)) == -1 and b"tt_sil_create" in lib.tt_last_error()
    assert lib.tt_sil_find(*([None, 1] + [None] * 12)) == -1 and b"tt_sil_find" in lib.tt_last_error()
    assert lib.tt_sil_trim(*([None, 1] + [None] * 15)) == -1 and b"tt_sil_trim" in lib.tt_last_error()
    rc = lib.tt_sil_create(1000, 2, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_sil_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())
        with pytest.raises(E.EngineError):
            E.check(rc)


def test_library_integers_equal_the_reference():
    lib = _lib()
    rng = np.random.default_rng(5)
    for n in [1, 119, 120, 121, 239, 240, 241, 479, 480, 481, 5000, 24000, E.SIL_MAX_SAMPLES] + rng.integers(1, E.SIL_MAX_SAMPLES + 1, 200).tolist():
        assert lib.tt_sil_frames(n) == R.frames(n) == sil.frames(n) == math.ceil(Fraction(n, 240)), n
        assert lib.tt_sil_max_regions(n) == R.max_regions(n) == sil.max_regions(n) == math.ceil(Fraction(R.frames(n), 2)), n
    for n in (0, -1, E.SIL_MAX_SAMPLES + 1):
        assert lib.tt_sil_frames(n) == 0 and lib.tt_sil_max_regions(n) == 0
    # no labelling has more regions than that: speech and silence alternate frame by frame
    for F in (1, 2, 3, 8, 9):
        assert len(R.regions([f % 2 == 0 for f in range(F)], F * 240)) == R.max_regions(F * 240)


# ----------------------------------------------------------------------------------------- host flow
class ReferenceSilenceStage:
    """stages.SilenceStage backed by tests/silence_reference.py."""
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceSilenceStage.made.append(max_samples)

    def find_many(self, clips, params, energies=False):
        ReferenceSilenceStage.calls.append(("find", [tuple(p) for p in params]))
        out = []
        for x, p in zip(clips, params):
            assert x.dim() == 1 and 1 <= x.shape[0] <= self.max_samples
            r = R.analyse(x.numpy(), tuple(p))
            out.append(dict(status=R.SILENT if r["status"] == R.SILENT else R.OK, peak=r["E"], regions=r["regions"]))
        return out

    def trim_many(self, clips, params):
        ReferenceSilenceStage.calls.append(("trim", [tuple(p) for p in params]))
        out = []
        for x, p in zip(clips, params):
            assert x.dim() == 1 and 1 <= x.shape[0] <= self.max_samples
            y, r = R.trim_f32(x.numpy(), tuple(p))
            out.append((torch.from_numpy(y), dict(status=r["status"], peak=r["E"], regions=r["regions"], segments=r["segments"])))
        return out

    def close(self):
        pass


def _ref(clip, p):
    y = R.trim_f32(clip.reshape(-1).numpy(), tuple(p))[0]
    return torch.from_numpy(y).reshape(clip.shape[:-1] + (-1,))


def _install(monkeypatch, api):
    from tests.test_resample_cpu import ReferenceResampleStage
    from tests.test_resample_cpu import _install as install_rest
    S, Lv = install_rest(monkeypatch, api)
    monkeypatch.setattr(api.stages, "SilenceStage", ReferenceSilenceStage)
    ReferenceSilenceStage.made, ReferenceSilenceStage.calls = [], []
    return S, Lv, ReferenceResampleStage


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


# what the flow tests trim with: the small models' clips are noise, so the detection is set where it finds several regions in them
LOOSE = dict(top_db=3.0, min_silence=0.0, pad=0.0, lead=0.0, trail=0.0)


def _speechy(n, seed):
    return torch.from_numpy(R.build([("z", 3000), ("s", n), ("z", 5000), ("s", 2000), ("l", 3000)], seed))


@torch.no_grad()
def test_trim_and_speech_regions(monkeypatch):
    t, _ = _tts(monkeypatch)
    x = _speechy(4000, 0)
    n = x.shape[0]
    p = sil.params(max_pause=0.05)
    want = _ref(x, p)
    for shape in ((n,), (1, n), (1, 1, n)):
        y = t.trim(x.reshape(shape), max_pause=0.05)
        assert y.shape == shape[:-1] + (want.shape[-1],) and y.dtype == torch.float32 and torch.equal(y.reshape(-1), want)
    assert ReferenceSilenceStage.made == [30 * 24000] and ReferenceSilenceStage.calls == [("trim", [tuple(p)])] * 3 and want.shape[-1] < n
    assert t.silence_info[0]["status"] == "ok" and t.silence_info[0]["removed_s"] == (n - want.shape[-1]) / 24000
    # several clips in ONE call; the map; a silent clip comes back as it is
    clips = [x, _speechy(2500, 1).reshape(1, -1), torch.zeros(700), x[3000:3100]]
    ReferenceSilenceStage.calls = []
    out, maps = t.trim_many(clips, lead=0.01, trail=None, max_pause=0.02, pad=0.02, return_map=True)
    q = sil.params(lead=0.01, trail=None, max_pause=0.02, pad=0.02)
    assert ReferenceSilenceStage.calls == [("trim", [tuple(q)] * 4)]
    assert all(torch.equal(o, _ref(c, q)) and o.shape[:-1] == c.shape[:-1] for o, c in zip(out, clips))
    assert [i["status"] for i in t.silence_info] == ["ok", "ok", "silent", "unchanged"] and torch.equal(out[2], clips[2]) and torch.equal(out[3], clips[3])
    assert maps[0] == R.trim(x.numpy(), tuple(q))["segments"] and len(maps[0]) == 2 and maps[2] == [(0, 0, 700)]
    assert t.trim_many([]) == [] and t.trim_many([], return_map=True) == ([], [])
    regions, pauses = t.speech_regions(x)
    r = R.analyse(x.numpy(), R.params())
    assert regions == r["regions"] and len(regions) == 2 and pauses == [(regions[0][1], regions[1][0])]
    assert ReferenceSilenceStage.calls[-1] == ("find", [tuple(sil.params(lead=None, trail=None))])
    both = t.speech_regions_many([x, torch.zeros(1, 500)], pad=0.0)
    assert both[0][0] == R.analyse(x.numpy(), R.params(pad=0))["regions"] and both[1] == ([], []) and t.speech_regions_many([]) == []
    # a longer clip than the stage was built for: it is built again, larger
    t.trim(torch.zeros(30 * 24000 + 1))
    assert ReferenceSilenceStage.made == [30 * 24000, 30 * 24000 + 1]
    with pytest.raises(ValueError, match="max_pause=0.001"):
        t.trim(x, max_pause=0.001)
    with pytest.raises(ValueError, match="top_db=0"):
        t.speech_regions(x, top_db=0)
    with pytest.raises(ValueError, match="expected"):
        t.trim(torch.zeros(2, 100))
    with pytest.raises(ValueError, match="exceeds"):
        t.trim(torch.zeros(1, E.SIL_MAX_SAMPLES + 1))


@torch.no_grad()
def test_trim_silence_and_max_pause_on_tts_and_tts_many(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    from tests.test_loudness_cpu import _ref as levelled
    from tests.test_resample_cpu import _pitched, _ref as resampled
    from tortoise_tts_amd import resample as rs
    t, kw = _tts(monkeypatch)
    S, Lv, Rs = _install(monkeypatch, __import__("tortoise_tts_amd.api", fromlist=["api"]))
    plain = t.tts(HELLO_THERE, **kw)
    # None and False: no stage, no call, today's bits
    assert torch.equal(t.tts(HELLO_THERE, trim_silence=None, max_pause=None, **kw), plain) and torch.equal(t.tts(HELLO_THERE, trim_silence=False, **kw), plain)
    assert torch.equal(t.tts_many([HELLO_THERE], trim_silence=None, **kw)[0], plain)
    assert t.silencer is None and ReferenceSilenceStage.made == [] and ReferenceSilenceStage.calls == [] and "silence_s" not in t.timings
    loose = sil.from_option(dict(LOOSE, max_pause=0.005))
    got = t.tts(HELLO_THERE, trim_silence=LOOSE, max_pause=0.005, **kw)
    assert ReferenceSilenceStage.calls == [("trim", [tuple(loose)])] and "silence_s" in t.timings and "diffusion_s" in t.timings
    assert torch.equal(got, _ref(plain, loose)) and got.shape[-1] < plain.shape[-1] and got.shape[:-1] == plain.shape[:-1]
    assert t.silence_info[0]["status"] == "ok" and t.silence_info[0]["removed_s"] == (plain.shape[-1] - got.shape[-1]) / 24000
    assert torch.equal(t.tts(HELLO_THERE, trim_silence=True, **kw), _ref(plain, sil.params()))
    assert torch.equal(t.tts(HELLO_THERE, max_pause=0.01, **kw), _ref(plain, sil.params(lead=None, trail=None, max_pause=0.01)))
    preset = t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **kw)
    assert torch.equal(t.tts_with_preset(HELLO_THERE, preset="ultra_fast", trim_silence=LOOSE, **kw), _ref(preset, sil.from_option(LOOSE)))
    # everything at once, k winners: rate and pitch -> pauses -> level -> sample rate, ONE call per stage
    two = t.tts(HELLO_THERE, k=2, **kw)
    ReferenceSilenceStage.calls, Rs.calls, S.calls, Lv.calls = [], [], [], []
    both, state = t.tts(HELLO_THERE, k=2, speaking_rate=1.25, pitch=2, trim_silence=LOOSE, max_pause=0.005, loudness=-19, sample_rate=16000,
                        return_deterministic_state=True, **kw)
    pq, _ = rs.pitch(2, 1.25)
    assert state[0] == 7 and S.calls == [2] and Lv.calls == [("normalize", 2)] and Rs.calls == [[(pq, 65536)] * 2, [(3, 2)] * 2]
    assert ReferenceSilenceStage.calls == [("trim", [tuple(loose)] * 2)] and len(t.silence_info) == 2
    assert all(torch.equal(a, resampled(levelled(_ref(_pitched(b, 2, 1.25), loose), -19.0), 3, 2)) for a, b in zip(both, two))
    # tts_many: one call for the texts
    many = t.tts_many([HELLO_THERE, HELLO], **kw)
    ReferenceSilenceStage.calls = []
    got = t.tts_many([HELLO_THERE, HELLO], trim_silence=LOOSE, **kw)
    assert ReferenceSilenceStage.calls == [("trim", [tuple(sil.from_option(LOOSE))] * 2)]
    assert all(torch.equal(a, _ref(b, sil.from_option(LOOSE))) for a, b in zip(got, many)) and len(t.silence_info) == 2
    for call in (lambda **k: t.tts(HELLO_THERE, **k, **kw), lambda **k: t.tts_many([HELLO_THERE], **k, **kw)):
        with pytest.raises(ValueError, match="max_pause=0.001"):
            call(max_pause=0.001)
        with pytest.raises(ValueError, match="unknown options"):
            call(trim_silence=dict(tail=0.1))
        with pytest.raises(ValueError, match="trim_silence='yes'"):
            call(trim_silence="yes")
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (other unknown kwargs are refused as before)
        t.tts(HELLO_THERE, trim=True, **kw)


@torch.no_grad()
def test_the_order_is_redaction_rate_pitch_pauses_level_sample_rate(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    from tests.test_redaction_cpu import _flow_tts
    from tortoise_tts_amd import resample as rs
    t, _ = _flow_tts(monkeypatch)
    from tortoise_tts_amd import api
    S, Lv, Rs = _install(monkeypatch, api)
    order = []
    redact = t._redact_clips
    t._redact_clips = lambda wavs, text: (order.append("redact"), redact(wavs, text))[1]
    monkeypatch.setattr(S, "stretch_many", lambda self, clips, rqs, f=S.stretch_many: (order.append("stretch"), f(self, clips, rqs))[1])
    monkeypatch.setattr(Lv, "normalize_many", lambda self, *a, f=Lv.normalize_many: (order.append("level"), f(self, *a))[1])
    monkeypatch.setattr(Rs, "resample_many", lambda self, clips, ratios, f=Rs.resample_many: (order.append(("resample", list(ratios))), f(self, clips, ratios))[1])
    monkeypatch.setattr(ReferenceSilenceStage, "trim_many",
                        lambda self, clips, params, f=ReferenceSilenceStage.trim_many: (order.append("pauses"), f(self, clips, params))[1])
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    t.tts("[I am so sad,] hello there", speaking_rate=1.25, pitch=-2, trim_silence=True, loudness=-23, sample_rate=8000, **kw)
    pq, _ = rs.pitch(-2, 1.25)
    assert order == ["redact", "stretch", ("resample", [(pq, 65536)]), "pauses", "level", ("resample", [(3, 1)])]
    assert all(k in t.timings for k in ("redact_s", "stretch_s", "pitch_s", "silence_s", "level_s", "resample_s"))


@torch.no_grad()
def test_timings_and_long_form_pause(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_api_flow_cpu import voice_latents, small_setup
    from tortoise_tts_amd import longform
    t, m = CC._flow(monkeypatch, candidate_sharding=False)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    # tts_with_timings aligns what tts() returns: the trimmed clip
    plain, _ = t.tts_with_timings("hello there", **kw)
    res, al = t.tts_with_timings("hello there", trim_silence=LOOSE, **kw)
    assert torch.equal(res, _ref(plain, sil.from_option(LOOSE))) and al.samples == res.shape[-1] < plain.shape[-1]
    assert CC._same(al, CC._expected(m, res, "hello there"))
    # long-form
    lkw = dict(conditioning_latents=kw["conditioning_latents"], num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, seed=5,
               texts_are_chunks=True, preset="ultra_fast")
    texts = ["hello there", "hello", "hello there"]
    full0, clips0 = longform.read_long_form(t, texts, **lkw)
    assert ReferenceSilenceStage.calls == [("trim", [tuple(sil.from_option(LOOSE))])]  # (only the call above: pause=None builds nothing)
    again, _ = longform.read_long_form(t, texts, pause=None, **lkw)
    assert torch.equal(again, full0) and len(ReferenceSilenceStage.calls) == 1
    gap = 3000
    inner = dict(top_db=3.0, min_silence=0.0, pad=0.0, max_pause=0.005)
    p = sil.from_option(dict(inner, lead=0.0, trail=0.0))
    full, parts = longform.read_long_form(t, texts, pause=0.125, trim_silence=dict(inner, lead=0.3, trail=0.3), **lkw)
    assert torch.equal(full, torch.cat([c.squeeze(0) for c in parts], dim=-1)) and len(parts) == 3
    assert all(c == ("trim", [tuple(p)]) for c in ReferenceSilenceStage.calls[1:]) and len(ReferenceSilenceStage.calls) == 4
    speech = []
    for j, (part, c0) in enumerate(zip(parts, clips0)):
        r = R.trim(c0.reshape(-1).numpy(), tuple(p))
        body = part if j == 2 else part[..., :-gap]
        assert torch.equal(body, _ref(c0, p)) and (j == 2 or not part[..., -gap:].any()) and part.shape[-1] == r["n_out"] + (gap if j < 2 else 0)
        # the chunk was cut to its speech: it begins where its first region begins and ends where its last one ends
        assert r["status"] == R.OK and r["D0"] == r["regions"][0][0] and r["Dt"] == c0.shape[-1] - r["regions"][-1][1]
        first, last = sil.map_sample(r["regions"][0][0], r["segments"]), sil.map_sample(r["regions"][-1][1], r["segments"])
        assert first == 0 and last == r["n_out"]
        speech.append((first, last))
    # so between the last speech region of one chunk and the first of the next lie exactly round(pause * 24000) samples
    off = np.concatenate(([0], np.cumsum([c.shape[-1] for c in parts])))
    for j in range(2):
        assert (off[j + 1] + speech[j + 1][0]) - (off[j] + speech[j][1]) == gap == round(0.125 * 24000)
    # the pause with the timings: aligned on the parts as joined
    # pause= alone: the default detection, only the ends
    ReferenceSilenceStage.calls = []
    full1, parts1 = longform.read_long_form(t, texts, pause=0.5, **lkw)
    assert all(c == ("trim", [tuple(sil.params(lead=0, trail=0))]) for c in ReferenceSilenceStage.calls) and len(ReferenceSilenceStage.calls) == 3
    assert not parts1[0][..., -12000:].any() and torch.equal(full1, torch.cat([c.squeeze(0) for c in parts1], dim=-1))
    # the pause with the timings: the chunks are aligned with the pause in place, and the merged alignment covers the parts as joined
    lfull, lal = longform.read_long_form(t, texts, pause=0.5, return_timings=True, **lkw)
    assert torch.equal(lfull, full1) and lal.samples == full1.shape[-1]
    with pytest.raises(ValueError, match="pause=-1"):
        longform.read_long_form(t, texts, pause=-1, **lkw)


@torch.no_grad()
def test_fast_path_and_streaming_refusals(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    _install(monkeypatch, api_fast)
    one = make(1)
    kw = dict(max_mel_tokens=24, use_deterministic_seed=41)
    plain = one.tts(TEXTS[0], **kw)
    assert torch.equal(one.tts(TEXTS[0], trim_silence=None, max_pause=None, **kw), plain) and ReferenceSilenceStage.made == [] and one.silencer is None
    p = sil.from_option(LOOSE)
    assert torch.equal(one.tts(TEXTS[0], trim_silence=LOOSE, **kw), _ref(plain, p)) and ReferenceSilenceStage.calls == [("trim", [tuple(p)])]
    both = one.tts_many(TEXTS[:2], **kw)
    ReferenceSilenceStage.calls = []
    got = one.tts_many(TEXTS[:2], trim_silence=LOOSE, max_pause=0.005, **kw)
    q = sil.from_option(LOOSE, 0.005)
    assert ReferenceSilenceStage.calls == [("trim", [tuple(q)] * 2)] and all(torch.equal(a, _ref(b, q)) for a, b in zip(got, both))
    # no pause shaping on streamed audio
    with pytest.raises(ValueError, match="tts_stream: trim_silence is not available for streamed audio"):
        next(one.tts_stream(TEXTS[0], trim_silence=True, **KW))
    with pytest.raises(ValueError, match="tts_stream: max_pause is not available for streamed audio"):
        next(one.tts_stream(TEXTS[0], max_pause=0.3, **KW))
    many = make(3)
    with pytest.raises(ValueError, match="open_stream: max_pause is not available"):
        many.open_stream(TEXTS[0], max_pause=0.3, **KW)
    with pytest.raises(ValueError, match="tts_stream_many: trim_silence is not available"):
        next(many.tts_stream_many(TEXTS[:2], trim_silence=True, **KW))
    with pytest.raises(ValueError, match="sample_rate is not available"):  # (the existing refusals keep their words)
        many.open_stream(TEXTS[0], sample_rate=8000, **KW)
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.SilenceStage)  # (no handle: the checks come before any device work)
    st.h, st.lib = None, _lib()
    st.max_samples, st.max_clips = 1000, 16
    p = sil.params()
    for call in (st.trim_many, st.find_many):
        with pytest.raises(ValueError, match="1001 samples"):
            call([torch.zeros(1001)], [p])
        with pytest.raises(ValueError, match="at least one sample"):
            call([torch.zeros(0)], [p])
        with pytest.raises(ValueError, match="2 clips with 1 parameter sets"):
            call([torch.zeros(10), torch.zeros(10)], [p])
