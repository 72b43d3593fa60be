"""-m gpu: the device mel front-end (csrc/melfront.hip) through its C-ABI (include/tortoise_mi355x_mel.h) against the fp64 reference and the
element-wise bounds of tests/melfront_reference.py: spectrum and log mel of both product configurations at the hop / frame-count edges and
the product lengths, the clamp, the resampler, ragged batches bit-identical to solo runs, and the stage / API wiring."""
import ctypes as C
import functools
import math

import pytest
import torch

from oracle import make_golden as G
from tests import melfront_reference as R
from tortoise_tts_amd import audio, engine as E, pack, stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, VocoderConfig

pytestmark = pytest.mark.gpu

N_FFT, HOP, BINS, BINS_PAD = pack.MEL_N_FFT, pack.MEL_HOP, pack.MEL_N_FFT // 2 + 1, pack.MEL_BINS_PAD
MAX_SAMPLES, MAX_CLIPS = 132300, 4
# name -> (n_mels, power, clamp, filter bank, scale)
CONFIGS = {"auto": (80, 2, 0, "fb_auto", "scale_auto"), "diffusion": (100, 1, 1, "fb_diff", None)}


def mel_norms():
    g = torch.Generator().manual_seed(3)
    return -(2.0 + 6.0 * torch.rand(80, generator=g))  # U(-8, -2): the division matters


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def tabs():
    host = pack.melfront_tables(mel_norms())
    dev = {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in host.items()}
    return host, dev


@pytest.fixture(scope="module")
def handles(lib, tabs):
    host, dev = tabs
    hs = {}
    for name, (n_mels, power, clamp, fb, scale) in CONFIGS.items():
        c = E.MelConfig()
        c.n_fft, c.hop, c.n_mels, c.bins_pad, c.power, c.clamp_input = N_FFT, HOP, n_mels, BINS_PAD, power, clamp
        c.floor, c.max_samples, c.max_clips = R.FLOOR, MAX_SAMPLES, MAX_CLIPS
        t = E.MelTables()
        t.basis, t.fb, t.scale = E.ptr(dev["basis"]), E.ptr(dev[fb]), E.ptr(dev[scale]) if scale else None
        h = E.vp()
        E.check(lib.tt_mel_create(C.byref(c), C.byref(t), C.byref(h)))
        hs[name] = h
    yield hs
    for h in hs.values():
        lib.tt_mel_destroy(h)


def _call(lib, fn, h, wav, offs, lens, out, ooffs):
    k = len(lens)
    return fn(h, E.ptr(wav), (C.c_longlong * k)(*offs), (C.c_int * k)(*lens), k, E.ptr(out), (C.c_longlong * k)(*ooffs), E.stream_ptr())


def run_clips(lib, h, n_mels, clips, spectrum=False, gap=0):
    """clips (host f32 vectors) in one call, `gap` + c unused elements in front of clip c in the input and the output buffer
    -> one [n_mels][T] (or [T][BINS_PAD]) device tensor per clip"""
    offs, ooffs, lens, a, b = [], [], [], 0, 0
    for c, x in enumerate(clips):
        a, b = a + (gap + c if gap else 0), b + (gap + c if gap else 0)
        T = lib.tt_mel_frames(h, x.shape[0])
        assert T == 1 + x.shape[0] // HOP
        offs.append(a); ooffs.append(b); lens.append(x.shape[0])
        a, b = a + x.shape[0], b + T * (BINS_PAD if spectrum else n_mels)
    wav = torch.full((a,), 1.0e3, dtype=torch.float32)  # (anything read from a gap would show)
    for o, x in zip(offs, clips):
        wav[o:o + x.shape[0]] = x
    wav = wav.cuda()
    out = torch.full((b,), float("nan"), device="cuda", dtype=torch.float32)
    E.check(_call(lib, lib.tt_mel_spectrum if spectrum else lib.tt_mel_run, h, wav, offs, lens, out, ooffs))
    torch.cuda.synchronize()
    res = []
    for o, n in zip(ooffs, lens):
        T = 1 + n // HOP
        res.append(out[o:o + T * BINS_PAD].reshape(T, BINS_PAD) if spectrum else out[o:o + T * n_mels].reshape(n_mels, T))
    if gap:  # nothing written outside the clips' own outputs
        keep = torch.ones(b, dtype=torch.bool, device="cuda")
        for o, r in zip(ooffs, res):
            keep[o:o + r.numel()] = False
        assert torch.isnan(out[keep]).all()
    return res


@functools.lru_cache(maxsize=None)
def reference(name, n):
    host = pack.melfront_tables(mel_norms())
    n_mels, power, clamp, fb, scale = CONFIGS[name]
    x = R.probe_signal(n, seed=n)
    return x, R.mel_reference(x, host["basis"], host[fb], host[scale] if scale else None, N_FFT, HOP, power=power, clamp=bool(clamp))


@pytest.mark.parametrize("n", R.LENGTHS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_spectrum_and_log_mel_against_fp64(lib, handles, name, n):
    n_mels = CONFIGS[name][0]
    x, ref = reference(name, n)
    T = 1 + n // HOP
    assert ref.frames == T and ref.floor_fraction <= 0.5, (ref.frames, ref.floor_fraction)
    spec = run_clips(lib, handles[name], n_mels, [x], spectrum=True)[0]
    assert spec.shape == (T, BINS_PAD) and not spec[:, BINS:].any()
    rs, i = R.worst_ratio(spec[:, :BINS], ref.spec, ref.e_spec)
    mel = run_clips(lib, handles[name], n_mels, [x])[0]
    assert mel.shape == (n_mels, T)
    rm, j = R.worst_ratio(mel, ref.mel, ref.e_log)
    print(f"[melfront] {name} n={n} T={T}: spectrum worst |err| / bound = {rs:.3f} at (t, bin) = {divmod(i, BINS)}; log mel {rm:.3f} at (mel, t) = "
          f"{divmod(j, T)}; max e_log {float(ref.e_log.max()):.2e}; at the floor {ref.floor_fraction:.1%}")
    assert rs <= 1.0, (name, n, rs, divmod(i, BINS))
    assert rm <= 1.0, (name, n, rm, divmod(j, T))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_silence_gives_the_floor_exactly(lib, handles, tabs, name):
    """An all-zero clip: every element is logf(floor) times scale[m] in one f32 multiplication, with nothing from the spectrum in it.
    logf's last bit is the device library's (it is faithful, not correctly rounded), so logf(floor) may be either f32 neighbour of the
    fp64 value - but the same one everywhere."""
    n_mels, _, _, _, scale = CONFIGS[name]
    mel = run_clips(lib, handles[name], n_mels, [torch.zeros(4096)])[0].cpu()
    assert mel.shape == (n_mels, 17)
    exact = math.log(float(torch.tensor(R.FLOOR, dtype=torch.float32)))
    near = torch.tensor(exact, dtype=torch.float64).float()
    cands = {float(near), float(torch.nextafter(near, torch.tensor(0.0))), float(torch.nextafter(near, torch.tensor(-100.0)))}
    cands = [c for c in cands if abs(c - exact) < 2.0 ** -20]  # within one f32 spacing at 11.5
    print(f"[melfront] {name} silence: got {mel[0, 0].item()!r}; fp64 log(floor) = {exact!r}, f32 candidates {sorted(cands)}")
    hits = []
    for c in cands:
        want = torch.full((n_mels,), c, dtype=torch.float32)
        if scale:
            want = want * tabs[0][scale]  # one f32 multiplication
        hits.append(torch.equal(mel, want[:, None].expand(n_mels, 17).contiguous()))
    assert sum(hits) == 1, hits


def test_bad_clips_are_refused_not_faulted(lib, handles):
    h = handles["auto"]
    wav = torch.zeros(8192, device="cuda")
    out = torch.zeros(80 * 40, device="cuda")
    for lens, word in (([512], b"reflect"), ([4096, 512], b"clip 1"), ([MAX_SAMPLES + 1], b"handle takes"), ([600] * (MAX_CLIPS + 1), b"clips")):
        k = len(lens)
        assert _call(lib, lib.tt_mel_run, h, wav, [0] * k, lens, out, [0] * k) == -1, lens
        assert word in lib.tt_last_error(), (lens, lib.tt_last_error())
        assert _call(lib, lib.tt_mel_spectrum, h, wav, [0] * k, lens, out, [0] * k) == -1, lens
    assert _call(lib, lib.tt_mel_run, h, wav, [-1], [4096], out, [0]) == -1
    assert lib.tt_mel_run(h, None, (C.c_longlong * 1)(0), (C.c_int * 1)(4096), 1, E.ptr(out), (C.c_longlong * 1)(0), None) == -1
    torch.cuda.synchronize()


def test_clamp_is_live(lib, handles, tabs):
    host = tabs[0]
    x = R.probe_signal(4096, seed=5)
    x[5::7] = 1.7
    x[3::11] = -1.7
    mel = run_clips(lib, handles["diffusion"], 100, [x])[0]
    clamped = R.mel_reference(x, host["basis"], host["fb_diff"], None, N_FFT, HOP, power=1, clamp=True)
    plain = R.mel_reference(x, host["basis"], host["fb_diff"], None, N_FFT, HOP, power=1, clamp=False)
    r, _ = R.worst_ratio(mel, clamped.mel, clamped.e_log)
    r2, _ = R.worst_ratio(mel, plain.mel, plain.e_log)
    print(f"[melfront] clamp: worst |err| / bound {r:.3f} against the clamped reference, {r2:.1f} against the unclamped one")
    assert r <= 1.0 and r2 > 1.0


@pytest.mark.parametrize("orig,new,lengths", [(147, 160, (1, 146, 147, 148, 161, 1000, 22050)), (2, 1, (1001,)), (3, 2, (1001,))])
def test_resampler_against_fp64(lib, orig, new, lengths):
    taps64, width = audio.resample_taps(orig, new)
    taps = taps64.float()
    tdev = taps.cuda().contiguous()
    h = E.vp()
    E.check(lib.tt_mel_resampler_create(E.ptr(tdev), orig, new, width, max(lengths), C.byref(h)))
    try:
        for n in lengths:
            x = R.probe_signal(n, seed=n + 1)
            ref, bound = R.resample_reference(x, taps, orig, new, width)
            m = lib.tt_mel_resampled_length(h, n)
            assert m == math.ceil(new * n / orig) == ref.shape[0]
            out = torch.full((m + 64,), float("nan"), device="cuda")
            E.check(lib.tt_mel_resample(h, E.ptr(x.cuda()), n, E.ptr(out), E.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.isnan(out[m:]).all(), "wrote past the output"
            r, i = R.worst_ratio(out[:m], ref, bound)
            print(f"[melfront] resample {orig}->{new} n={n}: worst |err| / bound = {r:.3f} at {i}")
            assert r <= 1.0, (orig, new, n, r, i)
        assert lib.tt_mel_resample(h, E.ptr(tdev), max(lengths) + 1, E.ptr(tdev), None) == -1 and b"samples" in lib.tt_last_error()
    finally:
        lib.tt_mel_resampler_destroy(h)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ragged_batch_is_bit_identical_to_solo_runs(lib, handles, name):
    n_mels = CONFIGS[name][0]
    clips = [R.probe_signal(n, seed=10 + n) for n in (513, 4096, 1025, 132300)]
    for spectrum in (False, True):
        batch = run_clips(lib, handles[name], n_mels, clips, spectrum=spectrum, gap=3)  # clips at offsets 3, 3 + 513 + 4, ...: not aligned
        for x, got in zip(clips, batch):
            solo = run_clips(lib, handles[name], n_mels, [x], spectrum=spectrum)[0]
            assert torch.equal(got, solo), (name, spectrum, x.shape[0])


@pytest.fixture(scope="module")
def stage():
    st = stages.MelFrontStage(mel_norms=mel_norms())
    yield st
    st.close()


@torch.no_grad()
def test_stage_call_equals_many(stage):
    clips = [R.probe_signal(n, seed=n).reshape(1, -1) for n in (50000, 132300, 9000)]
    many = stage.many(clips)
    assert [tuple(a.shape) for a, _ in many] == [(1, 80, 517)] * 3 and [tuple(d.shape) for _, d in many] == [(1, 100, 401)] * 3
    for c, (am, dm) in zip(clips, many):
        a1, d1 = stage(c)
        assert torch.equal(a1, am) and torch.equal(d1, dm)
        assert torch.equal(stage.auto_mel(c), am) and torch.equal(stage.diffusion_mel(c), dm)
    assert all(torch.equal(a, am) for a, (am, _) in zip(stage.auto_many(clips), many))
    # the stage's resampler cuts a long clip where output 102400 stops reading: the values of resampling all of it
    long = R.probe_signal(140000, seed=2)
    ref, bound = R.resample_reference(long, stage.t["taps"], 147, 160, 7)
    got = stage._diff_clip(long)
    assert got.shape == (audio.DIFF_COND_SAMPLES,)
    assert R.worst_ratio(got, ref[:audio.DIFF_COND_SAMPLES], bound[:audio.DIFF_COND_SAMPLES])[0] <= 1.0


@torch.no_grad()
def test_api_device_front_end(stage):
    """TextToSpeech(mel_front_end="device").get_conditioning_latents: the stage's own mels, the conditioning stage's latents of exactly
    those mels, the torch path's shapes, and values within the two paths' bounds against fp64."""
    from tortoise_tts_amd.api import TextToSpeech
    ar, clvp, diff = ARConfig(**G.AR_CFG), CLVPConfig(**G.CLVP_CFG), DiffusionConfig(**G.DIFF_CFG)
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(ar), seed=G.COND_SEED),
           "clvp": W.synthetic_state_dict(W.clvp_manifest(clvp), seed=G.CLVP_SEED),
           "diffusion": W.synthetic_state_dict(W.diffusion_manifest(diff), seed=G.COND_SEED + 1),
           "vocoder": W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(VocoderConfig()), seed=G.VOC_SEED))}
    kw = dict(state_dicts=sds, configs={"ar": ar, "clvp": clvp, "diffusion": diff}, max_candidates=8, max_mel_tokens=32)
    norms = mel_norms()
    c1, c2 = R.probe_signal(50000, seed=21).reshape(1, -1), R.probe_signal(140000, seed=22).reshape(1, -1)  # c2: a random crop start is drawn
    dev = TextToSpeech(mel_front_end="device", **kw)
    dev.mel_front_end = stage  # (synthetic mel_norms: data/mel_norms.pth may be absent on the test machine)
    torch.manual_seed(4)
    a, d, am, dm = dev.get_conditioning_latents([c1, c2], return_mels=True)
    torch.manual_seed(4)
    own = stage.many([c1, c2])
    assert torch.equal(am, torch.stack([p[0] for p in own], dim=1)) and torch.equal(dm, torch.stack([p[1] for p in own], dim=1))
    assert torch.equal(a, dev.conditioning.auto_latent([p[0] for p in own])) and torch.equal(d, dev.conditioning.diffusion_latent([p[1] for p in own]))
    ref = TextToSpeech(**kw)
    assert ref.mel_front_end_kind == "torch"
    ref.mel_front_end = audio.MelFrontEnd(mel_norms=norms)
    torch.manual_seed(4)
    a2, d2, am2, dm2 = ref.get_conditioning_latents([c1, c2], return_mels=True)
    assert isinstance(ref.mel_front_end, audio.MelFrontEnd)
    assert (a.shape, d.shape, am.shape, dm.shape) == (a2.shape, d2.shape, am2.shape, dm2.shape)
    assert am.shape == (1, 2, 80, 517) and dm.shape == (1, 2, 100, 401)
    # fp64 references of what each path was given: the padded / cropped 22.05 kHz clip, and the torch path's resampled clip
    torch.manual_seed(4)
    s = int(torch.randint(0, c2.shape[1] - audio.AUTO_COND_SAMPLES + 1, (1,)))
    host = pack.melfront_tables(norms)
    for j, x in enumerate((audio.pad_or_truncate(c1[0], audio.AUTO_COND_SAMPLES), c2[0, s:s + audio.AUTO_COND_SAMPLES])):
        r = R.mel_reference(x, host["basis"], host["fb_auto"], host["scale_auto"], N_FFT, HOP, power=2, clamp=False)
        for what, m in (("device", am), ("torch", am2)):
            ratio = R.worst_ratio(m[0, j], r.mel, r.e_log)[0]
            print(f"[melfront] api auto mel clip {j} {what}: worst |err| / e_log = {ratio:.3f}")
            assert ratio <= 1.0, (what, j, ratio)
        assert bool(((am[0, j] - am2[0, j]).abs().cpu().double() <= 2 * r.e_log).all())
    for j, c in enumerate((c1, c2)):
        x = audio.pad_or_truncate(audio.resample_sinc(c.cuda(), 22050, 24000), audio.DIFF_COND_SAMPLES)[0].cpu()
        r = R.mel_reference(x, host["basis"], host["fb_diff"], None, N_FFT, HOP, power=1, clamp=True)
        ratio = R.worst_ratio(dm2[0, j], r.mel, r.e_log)[0]
        gap = float(((dm[0, j] - dm2[0, j]).abs().cpu().double() / (2 * r.e_log)).max())
        print(f"[melfront] api diffusion mel clip {j}: torch worst |err| / e_log = {ratio:.3f}; |device - torch| / (2 e_log) = {gap:.3f}")
        assert ratio <= 1.0 and gap <= 1.0, (j, ratio, gap)
    for t in (dev, ref):
        for st in (t.ar, t.clvp, t.diffusion, t.vocoder, t.conditioning):
            st.close()
