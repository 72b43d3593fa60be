"""CPU-only checks of the device mel front-end (include/tortoise_mi355x_mel.h, csrc/melfront.hip): the C-ABI is exported and mirrored, the
host tables (pack.py) are the DFT / filter banks / resampler taps the torch path uses, the fp64 reference of tests/melfront_reference.py
agrees with audio.MelFrontEnd within its own bound, and the mel_front_end= option of the TextToSpeech classes is wired as documented."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import melfront_reference as R
from tortoise_tts_amd import audio, engine as E, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "tortoise_mi355x_mel.h"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


@pytest.fixture(scope="module")
def tables():
    g = torch.Generator().manual_seed(3)
    norms = -(2.0 + 6.0 * torch.rand(80, generator=g))  # U(-8, -2), like the released mel_norms: all negative
    return norms, pack.melfront_tables(norms)


# ------------------------------------------------------------------------------------------------------------------ C-ABI
def test_every_declared_symbol_is_exported_and_mirrored(lib):
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(tt_mel_[a-z0-9_]+)\s*\(", src)))
    assert len(names) >= 11, names
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert set(names) == set(E._MEL_PROTOS), set(names) ^ set(E._MEL_PROTOS)
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
    # the main boundary did not grow
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read(), flags=re.S)
    assert not re.findall(r"\btt_mel_", main)


def test_struct_mirrors_match(lib):
    assert lib.tt_mel_abi_version() == 1
    for i, st in enumerate(E.MEL_STRUCTS):
        assert C.sizeof(st) == lib.tt_mel_struct_size(i), st.__name__
    assert lib.tt_mel_struct_size(len(E.MEL_STRUCTS)) == 0
    # field by field: a reordered field keeps the size
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    for cname, mirror in (("tt_mel_config", E.MelConfig), ("tt_mel_tables", E.MelTables)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [re.match(r"^(?:const\s+)?\w+\s*\**\s*(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert declared == [f[0] for f in mirror._fields_], cname
    assert int(re.search(r"#define TT_MEL_MAX_CLIPS (\d+)", src).group(1)) == E.MEL_MAX_CLIPS


def _config(**kw):
    c = E.MelConfig()
    c.n_fft, c.hop, c.n_mels, c.bins_pad, c.power, c.clamp_input = 1024, 256, 80, 544, 2, 0
    c.floor, c.max_samples, c.max_clips = 1e-5, 4096, 2
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_create_checks_its_arguments_before_any_device_work(lib):
    """Refused configurations name the offending field through tt_last_error, on any machine."""
    t = E.MelTables()
    t.basis, t.fb = 256, 256  # (never dereferenced on the host)
    h = E.vp()
    for kw, word in ((dict(hop=255), b"hop"), (dict(bins_pad=513), b"bins_pad"), (dict(power=3), b"power"), (dict(n_mels=129), b"n_mels"),
                     (dict(max_clips=17), b"max_clips"), (dict(max_samples=512), b"max_samples"), (dict(floor=0.0), b"floor")):
        c = _config(**kw)
        assert lib.tt_mel_create(C.byref(c), C.byref(t), C.byref(h)) == -1, kw
        assert word in lib.tt_last_error(), (kw, lib.tt_last_error())
    assert lib.tt_mel_create(C.byref(_config()), C.byref(E.MelTables()), C.byref(h)) == -1 and b"null table" in lib.tt_last_error()
    assert lib.tt_mel_resampler_create(256, 147, 147, 7, 1000, C.byref(h)) == -1 and b"147" in lib.tt_last_error()
    assert lib.tt_mel_resampler_create(None, 147, 160, 7, 1000, C.byref(h)) == -1


def test_create_fails_loudly_without_gpu(lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    t = E.MelTables()
    t.basis, t.fb = 256, 256
    h = E.vp()
    rc = lib.tt_mel_create(C.byref(_config()), C.byref(t), C.byref(h))
    assert rc != 0 and not h
    msg = lib.tt_last_error().lower()
    assert b"hip" in msg or b"device" in msg, msg
    with pytest.raises(E.EngineError):
        E.check(rc)
    assert lib.tt_mel_resampler_create(256, 147, 160, 7, 1000, C.byref(h)) != 0 and not h


# ------------------------------------------------------------------------------------------------------------------ host tables
def test_basis_is_the_windowed_dft_of_torch_stft():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g, dtype=torch.float64)
    basis = pack.stft_basis()
    assert basis.dtype == torch.float64 and basis.shape == (1024, 2 * pack.MEL_BINS_PAD)
    fr = R.padded_frames(x, 1024, 256)
    got = (fr @ basis).reshape(fr.shape[0], pack.MEL_BINS_PAD, 2)
    want = torch.stft(x, n_fft=1024, hop_length=256, win_length=1024, window=torch.hann_window(1024, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True)  # [513][17]
    assert want.shape == (513, 1 + 4096 // 256)
    assert (got[:, :513, 0] - want.real.t()).abs().max() <= 1e-9
    assert (got[:, :513, 1] - want.imag.t()).abs().max() <= 1e-9
    assert not got[:, 513:].any()


def test_padded_filterbanks_and_scale(tables):
    norms, t = tables
    for name, args in (("fb_auto", (22050, 1024, 80, 0.0, 8000.0, True)), ("fb_diff", (24000, 1024, 100, 0.0, 12000.0, False))):
        fb = audio.mel_filterbank(*args[:5], htk=args[5])
        assert t[name].dtype == torch.float32 and t[name].shape == (fb.shape[0], pack.MEL_BINS_PAD)
        assert torch.equal(t[name][:, :513], fb)
        assert not t[name][:, 513:].any()
    assert t["basis"].dtype == torch.float32 and torch.equal(t["basis"], pack.stft_basis().float())
    assert torch.equal(t["scale_auto"], (1.0 / norms.double()).float())


def test_resampler_taps_match_the_oracle_and_the_aligner(tables):
    from oracle import audio_oracle
    from tortoise_tts_amd import align
    k, width, orig, new = audio_oracle.resample_kernel(147, 160)
    taps, w = audio.resample_taps(147, 160)
    assert (w, taps.shape) == (width, (160, 161)) and (orig, new) == (147, 160)
    assert np.abs(taps.numpy() - k).max() <= 1e-12
    assert torch.equal(tables[1]["taps"], taps.float()) and tables[1]["width"] == 7
    # 3 -> 2: the aligner builds its [2][23] kernel with the same formula in f32 (the waveform's dtype there), so the two agree to f32 rounding
    t32, w32 = audio.resample_taps(3, 2)
    a = align.resample_taps()
    assert t32.shape == a.shape == (2, 23) and w32 == 10
    assert (t32 - a.double()).abs().max() <= 4 * 2.0 ** -24
    # the torch path still resamples with these taps, bit for bit what it computed before the formula moved
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3000, generator=g)
    ref = audio_oracle.resample(x[0].numpy(), 22050, 24000)
    got = audio.resample_sinc(x, 22050, 24000)
    assert got.shape == (1, len(ref)) and np.abs(got[0].numpy() - ref).max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("n", R.LENGTHS)
def test_reference_agrees_with_the_torch_front_end(tables, n):
    """Pins the fp64 reference to audio.MelFrontEnd, which tests/test_audio_frontend.py pins to the reference's own classes.  MelFrontEnd
    pads or cuts every clip to the product lengths, so that is what the reference is given."""
    norms, t = tables
    fe = audio.MelFrontEnd(mel_norms=norms)
    clip = R.probe_signal(n, seed=n)
    auto_in = audio.pad_or_truncate(clip, audio.AUTO_COND_SAMPLES)
    ra = R.mel_reference(auto_in, t["basis"], t["fb_auto"], t["scale_auto"], 1024, 256, power=2, clamp=False)
    got = fe.auto_mel(clip, start=0)[0]
    assert got.shape == ra.mel.shape == (80, 517)
    ratio, i = R.worst_ratio(got, ra.mel, ra.e_log)
    print(f"[melfront] torch auto mel vs fp64, n={n}: worst |err| / e_log = {ratio:.3f} (max e_log {float(ra.e_log.max()):.2e})")
    assert ratio <= 1.0, (n, ratio, divmod(i, 517))
    diff_in = audio.pad_or_truncate(audio.resample_sinc(clip.reshape(1, -1), 22050, 24000), audio.DIFF_COND_SAMPLES)[0]
    rd = R.mel_reference(diff_in, t["basis"], t["fb_diff"], None, 1024, 256, power=1, clamp=True)
    got = fe.diffusion_mel(clip)[0]
    assert got.shape == rd.mel.shape == (100, 401)
    ratio, i = R.worst_ratio(got, rd.mel, rd.e_log)
    print(f"[melfront] torch diffusion mel vs fp64, n={n}: worst |err| / e_log = {ratio:.3f} (max e_log {float(rd.e_log.max()):.2e})")
    assert ratio <= 1.0, (n, ratio, divmod(i, 401))


def test_reference_catches_the_usual_mistakes(tables):
    """A wrong window, a frame off by one, a swapped bin and a missing clamp each miss the reference by far more than the bound."""
    norms, t = tables
    x = R.probe_signal(4096, seed=7) * 6.0  # (samples beyond +-1: the clamp matters)
    ref = R.mel_reference(x, t["basis"], t["fb_diff"], None, 1024, 256, power=1, clamp=True)
    assert float(ref.e_log.max()) <= 3e-3

    def miss(r):
        return float(((r.mel - ref.mel).abs() - ref.e_log).max())
    assert miss(R.mel_reference(x, t["basis"], t["fb_diff"], None, 1024, 256, power=1, clamp=False)) > 1e-1
    rect = pack.stft_basis().reshape(1024, -1, 2) / (0.5 - 0.5 * torch.cos(torch.arange(1024, dtype=torch.float64) * (2 * math.pi / 1024))).clamp(min=1e-30)[:, None, None]
    assert miss(R.mel_reference(x, rect.reshape(1024, -1).float(), t["fb_diff"], None, 1024, 256, power=1, clamp=True)) > 1e-1
    assert miss(R.mel_reference(torch.roll(x, 256), t["basis"], t["fb_diff"], None, 1024, 256, power=1, clamp=True)) > 1e-1
    swapped = t["fb_diff"].clone()
    swapped[:, [40, 41]] = swapped[:, [41, 40]]
    assert miss(R.mel_reference(x, t["basis"], swapped, None, 1024, 256, power=1, clamp=True)) > 1e-1


# ------------------------------------------------------------------------------------------------------------------ API wiring
class FakeMelFrontStage:
    """Stand-in for stages.MelFrontStage: the torch front-end behind the stage's interface, counting the calls."""
    instances = []

    def __init__(self, models_dir=None, mel_norms=None, device="cpu", **kw):
        self.fe = audio.MelFrontEnd(mel_norms=torch.ones(80) if mel_norms is None else mel_norms)
        self.many_calls, self.auto_many_calls = [], []
        FakeMelFrontStage.instances.append(self)

    def many(self, clips):
        self.many_calls.append(len(clips))
        return [self.fe(c) for c in clips]

    def auto_many(self, clips):
        self.auto_many_calls.append(len(clips))
        return [self.fe.auto_mel(c) for c in clips]


def _tts(monkeypatch, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "MelFrontStage", FakeMelFrontStage)
    FakeMelFrontStage.instances = []
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=16, **kw)
    t._cfgs = cfgs
    return t


def test_unknown_mel_front_end_is_refused(monkeypatch):
    with pytest.raises(ValueError, match="mel_front_end"):
        _tts(monkeypatch, mel_front_end="nonsense")
    assert _tts(monkeypatch).mel_front_end_kind == "torch"
    from tortoise_tts_amd import api_fast, stages
    with pytest.raises(ValueError, match="mel_front_end"):
        api_fast.TextToSpeech(mel_front_end="nonsense", device="cpu")
    with pytest.raises(ValueError):
        stages.mel_front_end_kind(None)


@torch.no_grad()
def test_device_option_builds_all_mels_in_one_call_and_passes_pairs_through(monkeypatch):
    g = torch.Generator().manual_seed(5)
    clips = [torch.randn(1, n, generator=g).clamp(-1, 1) * 0.2 for n in (30000, 45000, 20000)]
    fe = audio.MelFrontEnd(mel_norms=torch.ones(80))
    pair = fe(clips[1])
    tts = _tts(monkeypatch, mel_front_end="device")
    a, d, am, dm = tts.get_conditioning_latents(clips, return_mels=True)
    stage = tts.mel_front_end
    assert isinstance(stage, FakeMelFrontStage) and stage.many_calls == [3] and len(FakeMelFrontStage.instances) == 1
    assert am.shape == (1, 3, 80, 517) and dm.shape == (1, 3, 100, 401)
    # same mels as the torch path gives for these clips (the stand-in IS the torch front-end), hence the same latents
    ref = _tts(monkeypatch)
    ref.mel_front_end = fe
    a2, d2, am2, dm2 = ref.get_conditioning_latents(clips, return_mels=True)
    assert torch.equal(am, am2) and torch.equal(dm, dm2) and torch.equal(a, a2) and torch.equal(d, d2)
    # a ready pair between two waveforms: untouched, and only the two waveforms reach the stage, in order
    marked = (pair[0] + 1.0, pair[1] - 1.0)
    _, _, am3, dm3 = tts.get_conditioning_latents([clips[0], marked, clips[2]], return_mels=True)
    assert stage.many_calls == [3, 2]
    assert torch.equal(am3[:, 1], marked[0]) and torch.equal(dm3[:, 1], marked[1])
    assert torch.equal(am3[:, 0], am[:, 0]) and torch.equal(am3[:, 2], am[:, 2]) and torch.equal(dm3[:, 2], dm[:, 2])
    # pairs only: the stage is not consulted at all
    tts.get_conditioning_latents([marked])
    assert stage.many_calls == [3, 2]


@pytest.mark.parametrize("n,draws", [(132300, 0), (140000, 1)])
def test_both_paths_draw_the_same_random_numbers(monkeypatch, n, draws):
    """The crop start of a clip longer than 132300 samples is the only torch.randint draw, on either path (stages.MelFrontStage keeps
    the host half of audio.MelFrontEnd): the state of the caller's generator afterwards is the same."""
    from tortoise_tts_amd import stages
    clip = R.probe_signal(n, seed=1).reshape(1, -1)
    calls = []
    real = torch.randint
    monkeypatch.setattr(torch, "randint", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    torch.manual_seed(11)
    audio.MelFrontEnd(mel_norms=torch.ones(80)).auto_mel(clip)
    state_torch, n_torch = torch.get_rng_state(), len(calls)
    st = stages.MelFrontStage.__new__(stages.MelFrontStage)  # (the host half alone: no handle is made)
    st.auto_samples, st.device = audio.AUTO_COND_SAMPLES, torch.device("cpu")
    st.h_auto = st.h_diff = st.h_rs = None
    torch.manual_seed(11)
    prepared = st._auto_clip(clip)
    assert len(calls) - n_torch == n_torch == draws
    assert torch.equal(torch.get_rng_state(), state_torch)
    assert prepared.shape == (audio.AUTO_COND_SAMPLES,)
    if draws:
        torch.manual_seed(11)
        s = int(real(0, n - audio.AUTO_COND_SAMPLES + 1, (1,)))
        assert torch.equal(prepared, clip[0, s:s + audio.AUTO_COND_SAMPLES])
