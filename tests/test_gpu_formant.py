"""-m gpu: the formant correction (csrc/formant.hip) through its C-ABI (include/tortoise_mi355x_fmt.h) and the staged operator entries
(include/tortoise_mi355x_test.h) against the fp64 reference and the element-wise bounds of tests/formant_reference.py: log magnitudes, log
gains from the device's log magnitudes, output from the device's spectrum and gains, then end to end; zeros, clips whose bins reach delta,
ragged batches bit-identical to solo runs, refusals that write nothing, and the stage / API wiring."""
import ctypes as C
import functools

import pytest
import torch

from tests import formant_reference as R
from tests.melfront_reference import probe_signal
from tortoise_tts_amd import engine as E, formant as fmt, stages

pytestmark = pytest.mark.gpu

N, H, B, BP = fmt.N_FFT, fmt.HOP, fmt.BINS, fmt.BINS_PAD
Q = 48
LENGTHS = (513, 1024, 1279, 1280, 4096, 24000)
WARPS = (2.0 ** (4 / 12.0), 2.0 ** (7 / 12.0), 0.5, 2.0, 1.0)
GAINS_DB = (24.0, 6.0)
MAX_SAMPLES, MAX_CLIPS = 24000, 16
CANARY = 777.0


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def tabs():
    host = fmt.tables(Q, list(WARPS))
    return host, {k: v.cuda().contiguous() for k, v in host.items()}, R.Tables(host, N, H)


@pytest.fixture(scope="module")
def handles(lib, tabs):
    _, dev, _ = tabs
    hs = {}
    for db in GAINS_DB:
        c = E.FmtConfig()
        c.n_fft, c.hop, c.bins_pad, c.q, c.max_gain_db, c.max_samples, c.max_clips, c.n_warps = N, H, BP, Q, db, MAX_SAMPLES, MAX_CLIPS, len(WARPS)
        t = E.FmtTables()
        t.basis, t.inverse, t.cepstrum, t.warps = (E.ptr(dev[k]) for k in ("basis", "inverse", "cepstrum", "warps"))
        h = E.vp()
        E.check(lib.tt_fmt_create(C.byref(c), C.byref(t), C.byref(h)))
        hs[db] = h
    yield hs
    for h in hs.values():
        lib.tt_fmt_destroy(h)


@functools.lru_cache(maxsize=None)
def clip(n):
    return probe_signal(n, seed=n % 7, sr=24000.0)


def layout(lens, gap=0):
    offs, soffs, a, b = [], [], 0, 0
    for c, n in enumerate(lens):
        a, b = a + (gap + c if gap else 0), b + (4 * (gap + c) if gap else 0)
        offs.append(a); soffs.append(b)
        a, b = a + n, b + (1 + n // H) * BP
    return offs, soffs, a, b


def run(lib, h, clips, warps, staged=False, gap=0):
    """clips (host f32 vectors) in one call -> per clip out [n] (and spectrum [T][2 BP], logmag [T][BP], gains [T][BP]) as host tensors"""
    k, lens = len(clips), [int(x.shape[0]) for x in clips]
    offs, soffs, a, b = layout(lens, gap)
    wav = torch.full((a,), 1.0e3, dtype=torch.float32)  # (anything read from a gap would show)
    for o, x in zip(offs, clips):
        wav[o:o + x.shape[0]] = x
    wav = wav.cuda()
    out = torch.full((a,), CANARY, device="cuda", dtype=torch.float32)
    ll, ii, wi = (C.c_longlong * k)(*offs), (C.c_int * k)(*lens), (C.c_int * k)(*warps)
    if not staged:
        E.check(lib.tt_fmt_run(h, E.ptr(wav), ll, ii, wi, k, E.ptr(out), ll, E.stream_ptr()))
        st = None
    else:
        st = [torch.full((2 * b,), CANARY, device="cuda"), torch.full((b,), CANARY, device="cuda"), torch.full((b,), CANARY, device="cuda")]
        E.check(lib.tt_op_fmt_run(h, E.ptr(wav), ll, ii, wi, k, E.ptr(out), ll, E.ptr(st[0]), E.ptr(st[1]), E.ptr(st[2]), (C.c_longlong * k)(*soffs),
                                  E.stream_ptr()))
    torch.cuda.synchronize()
    o = out.cpu()
    used = torch.zeros(a, dtype=torch.bool)
    res = []
    for c, (of, n) in enumerate(zip(offs, lens)):
        used[of:of + n] = True
        r = dict(out=o[of:of + n].clone())
        if st is not None:
            T, so = 1 + n // H, soffs[c]
            r["spec"] = st[0][2 * so:2 * so + 2 * T * BP].cpu().reshape(T, BP, 2)
            r["logmag"] = st[1][so:so + T * BP].cpu().reshape(T, BP)
            r["gains"] = st[2][so:so + T * BP].cpu().reshape(T, BP)
        res.append(r)
    assert bool((o[~used] == CANARY).all()), "written outside the clips"
    return res, st, soffs


def synth(lib, h, st, soffs, lens):
    k = len(lens)
    offs, _, a, _ = layout(lens)
    out = torch.full((a,), CANARY, device="cuda", dtype=torch.float32)
    E.check(lib.tt_op_fmt_synth(h, E.ptr(st[0]), E.ptr(st[2]), (C.c_longlong * k)(*soffs), (C.c_int * k)(*lens), k, E.ptr(out),
                                (C.c_longlong * k)(*offs), E.stream_ptr()))
    torch.cuda.synchronize()
    return [out[o:o + n].cpu() for o, n in zip(offs, lens)]


def staged_checks(name, x, d, tb, wi, db, worst, end_to_end=True):
    """the four comparisons of one clip's device results `d`; `worst`: stage -> (ratio, what)"""
    n, lim = int(x.shape[0]), R.gain_limit(db)
    r = R.formant_reference(x, tb, wi, lim)
    T = r.L.shape[0]
    assert all(torch.isfinite(d[k]).all() for k in d), name
    assert not d["spec"][:, B:].any() and not d["gains"][:, B:].any()  # zero tables beyond n_fft / 2
    ratios = {}
    ratios["log magnitude"] = R.worst_ratio(d["logmag"][:, :B], r.L, r.e_L)
    # log gains: the reference starts from the DEVICE's log magnitudes
    g_ref, _, e_g = R.log_gain(d["logmag"][:, :B].double(), tb, wi, lim)
    ratios["log gain"] = R.worst_ratio(d["gains"][:, :B], g_ref, e_g)
    if lim > 0:
        assert float(d["gains"].abs().max()) <= lim
    # output: the reference starts from the DEVICE's spectrum and gains
    o_ref, e_o = R.synthesis(d["spec"][:, :B, 0].double(), d["spec"][:, :B, 1].double(), d["gains"][:, :B].double(), tb, n)
    ratios["output"] = R.worst_ratio(d["out"], o_ref, e_o)
    if end_to_end:
        ratios["end to end"] = R.worst_ratio(d["out"], r.out, r.e_out)
    for stage, (ratio, at) in ratios.items():
        print(f"{name} T {T}: {stage} worst |err| / bound {ratio:.3f} at element {at}")
        if ratio > worst.get(stage, (0.0, ""))[0]:
            worst[stage] = (ratio, f"{name} element {at}")
        assert ratio <= 1.0, (name, stage, ratio, at)
    return r


def test_staged_against_fp64(lib, handles, tabs):
    _, _, tb = tabs
    worst = {}
    for db in GAINS_DB:
        for n in LENGTHS:
            warps = range(len(WARPS)) if n in (513, 4096) or db == 6.0 else (0, 3)  # (every warp at two lengths and under the tight clamp)
            for wi in warps:
                if db == 6.0 and n not in (1279, 24000):
                    continue
                res, st, soffs = run(lib, handles[db], [clip(n)], [wi], staged=True)
                r = staged_checks(f"n {n} warp {WARPS[wi]:.4f} clamp {db:g} dB", clip(n), res[0], tb, wi, db, worst)
                if WARPS[wi] == 1.0:
                    assert not res[0]["gains"].any()  # D = 0: the gains are exactly zero and the clip is reconstructed
                if db == 6.0 and WARPS[wi] in (0.5, 2.0):
                    assert float(res[0]["gains"].abs().max()) == R.gain_limit(6.0)  # the clamp engages
                # steps 5 to 7 alone from the same spectrum and gains: the same bits
                again = synth(lib, handles[db], st, soffs, [n])[0]
                assert torch.equal(again.view(torch.int32), res[0]["out"].view(torch.int32))
    for stage, (ratio, what) in worst.items():
        print(f"worst {stage}: {ratio:.3f} ({what})")


def test_the_spectrum_is_melfronts_to_the_bit(lib, handles, tabs):
    """csrc/stft_steps.h restates the staging and the MFMA loop that csrc/melfront.hip keeps inline: this ties the two.  mel_stft_kernel hands
    out only re^2 + im^2 (one f32 expression, which the compiler may contract either way round), so its value must be a correctly rounded
    f32 of that expression evaluated exactly on fmt_stft_kernel's re and im - in one and the same form for every element."""
    from fractions import Fraction
    import numpy as np
    _, dev, _ = tabs
    c = E.MelConfig()
    c.n_fft, c.hop, c.n_mels, c.bins_pad, c.power, c.clamp_input, c.floor, c.max_samples, c.max_clips = N, H, 1, BP, 2, 0, 1e-5, MAX_SAMPLES, 1
    fb = torch.zeros(1, BP, device="cuda")
    t = E.MelTables()
    t.basis, t.fb, t.scale = E.ptr(dev["basis"]), E.ptr(fb), None
    mel = E.vp()
    E.check(lib.tt_mel_create(C.byref(c), C.byref(t), C.byref(mel)))
    try:
        for n in (1279, 4096):
            x = clip(n)
            T = 1 + n // H
            spec = torch.full((T * BP,), CANARY, device="cuda")
            xd = x.cuda()
            E.check(lib.tt_mel_spectrum(mel, E.ptr(xd), (C.c_longlong * 1)(0), (C.c_int * 1)(n), 1, E.ptr(spec), (C.c_longlong * 1)(0), E.stream_ptr()))
            torch.cuda.synchronize()
            p2 = spec.cpu().reshape(T, BP)[:, :B].numpy().reshape(-1)
            ours = run(lib, handles[24.0], [x], [4], staged=True)[0][0]["spec"][:, :B]
            re, im = ours[..., 0].numpy().reshape(-1), ours[..., 1].numpy().reshape(-1)
            rr, ii = re * re, im * im  # (numpy f32: each product rounded once)
            up, down = np.nextafter(p2, np.float32(np.inf)), np.nextafter(p2, np.float32(-np.inf))
            F = lambda v: Fraction(float(v))
            forms = {"fma(re, re, im im)": lambda k: F(re[k]) ** 2 + F(ii[k]), "fma(im, im, re re)": lambda k: F(rr[k]) + F(im[k]) ** 2,
                     "re re + im im": lambda k: F(rr[k]) + F(ii[k])}
            fits = {}
            for name, exact in forms.items():
                bad = 0
                for k in range(p2.shape[0]):
                    e = exact(k)
                    d = abs(F(p2[k]) - e)
                    bad += not (d <= abs(F(up[k]) - e) and d <= abs(F(down[k]) - e))
                fits[name] = bad
            print(f"n {n}: elements of melfront's power spectrum that are no rounding of the form: {fits}")
            assert min(fits.values()) == 0, (n, fits)
    finally:
        lib.tt_mel_destroy(mel)


def test_zeros_and_clips_whose_bins_reach_delta(lib, handles, tabs):
    _, _, tb = tabs
    h = handles[24.0]
    z = run(lib, h, [torch.zeros(1279)], [0], staged=True)[0][0]
    assert not z["out"].any() and not z["spec"].any() and torch.isfinite(z["gains"]).all()
    worst = {}
    half = clip(4096).clone()
    half[:2048] = 0.0
    for name, x in (("clean vowel", R.vowel(4096, 150.0, (700.0, 1200.0), noise=0.0)), ("silent first half", half)):
        for wi in (0, 2):
            res, _, _ = run(lib, h, [x], [wi], staged=True)
            staged_checks(f"{name} warp {WARPS[wi]:.4f}", x, res[0], tb, wi, 24.0, worst, end_to_end=False)


def test_ragged_batches_equal_the_solo_calls(lib, handles):
    h = handles[24.0]
    lens = [513, 24000, 1024, 1279, 1280, 4096, 777, 2048, 513, 5000, 1025, 3000, 600, 12000, 1300, 4097]
    wis = [c % len(WARPS) for c in range(16)]
    clips = [clip(n) for n in lens]
    solo = [run(lib, h, [x], [w])[0][0]["out"] for x, w in zip(clips, wis)]
    for k, gap in ((16, 3), (2, 0), (1, 5)):
        got, _, _ = run(lib, h, clips[:k], wis[:k], gap=gap)
        for c in range(k):
            assert torch.equal(got[c]["out"].view(torch.int32), solo[c].view(torch.int32)), (k, c, lens[c])
    # the operator entry makes the boundary's bits
    got, _, _ = run(lib, h, clips[:3], wis[:3], staged=True)
    assert all(torch.equal(got[c]["out"].view(torch.int32), solo[c].view(torch.int32)) for c in range(3))


def test_every_refusal_writes_nothing(lib, handles):
    h = handles[24.0]
    good = clip(1279)
    wav = torch.cat([good, good, good]).cuda()
    out = torch.full((3 * 1279,), CANARY, device="cuda")
    L3, I3 = C.c_longlong * 3, C.c_int * 3
    offs = L3(0, 1279, 2558)
    ok = dict(h=h, wav=E.ptr(wav), offs=offs, lens=I3(1279, 1279, 1279), wi=I3(0, 1, 2), k=3, out=E.ptr(out), ooffs=offs)
    call = lambda **kw: (lambda a: lib.tt_fmt_run(a["h"], a["wav"], a["offs"], a["lens"], a["wi"], a["k"], a["out"], a["ooffs"], E.stream_ptr()))(dict(ok, **kw))
    for bad, words in ((dict(lens=I3(1279, 512, 1279)), b"clip 1 has 512 samples"), (dict(lens=I3(1279, MAX_SAMPLES + 1, 1279)), b"the handle takes"),
                       (dict(wi=I3(0, len(WARPS), 2)), b"asks for warp"), (dict(wi=I3(0, -1, 2)), b"asks for warp"), (dict(k=0), b"0 clips"),
                       (dict(k=MAX_CLIPS + 1), b"17 clips"), (dict(wav=None), b"null"), (dict(out=None), b"null"), (dict(wi=None), b"null"),
                       (dict(offs=L3(0, -1, 2558)), b"negative offset"), (dict(h=None), b"null")):
        assert call(**bad) == -1 and words in lib.tt_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == CANARY).any())


@torch.no_grad()
def test_stage_and_clip_entries_equal_the_pieces(lib, handles):
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device("cuda")

    host = Host()
    x = clip(24000)
    a4 = 2.0 ** (4 / 12.0)
    st = stages.FormantStage(MAX_SAMPLES)
    direct = run(lib, handles[24.0], [x], [0])[0][0]["out"]
    y = st.correct_many([x], [a4])[0]
    assert y.device.type == "cuda" and torch.equal(y.cpu().view(torch.int32), direct.view(torch.int32))
    # more warps than the table has slots, and more clips than one call takes: every clip the bits of its solo call
    alphas = [2.0 ** ((s - 10) / 12.0) for s in range(21) if s != 10]
    many = st.correct_many([clip(1279)] * 20, alphas)
    again = st.correct_many([clip(1279)] * 2, [alphas[0], alphas[19]])
    assert torch.equal(many[0], again[0]) and torch.equal(many[19], again[1]) and len(st.slots) == 16
    st.close()
    # the clip entries of the API
    got = host.shift_formants(x.reshape(1, 1, -1), -4)  # formants down by 4 semitones: warp 2^(4/12)
    assert got.shape == (1, 1, 24000) and got.device.type == "cpu" and torch.equal(got.reshape(-1).view(torch.int32), direct.view(torch.int32))
    assert host.shift_formants(x, 0) is x and (host.formant_stage.max_samples, host.formant_stage.max_clips) == (24000, 1)  # sized from the batch
    three = host.shift_formants_many([x[:5000], x, x[:600]], -4)  # a larger batch: rebuilt, never smaller, the same bits
    assert (host.formant_stage.max_samples, host.formant_stage.max_clips) == (24000, 3) and torch.equal(three[1].view(torch.int32), direct.view(torch.int32))
    up = host.shift_pitch(x, 4)
    kept = host.shift_pitch(x, 4, formants="keep")
    want = host.load_formant().correct_many([up], [a4])[0].cpu()
    assert kept.shape == up.shape and torch.equal(kept, want) and not torch.equal(kept, up)
    assert torch.equal(host.shift_pitch(x, 4, formants="follow"), up)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    return TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)


@torch.no_grad()
def test_formants_on_tts_equal_the_chain_on_the_clip(tts):
    import bench
    text = bench.synthetic_prompt()[0].tolist()
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts(text, **kw)
    again = tts.tts(text, formants="keep", formant_shift=None, **kw)
    assert torch.equal(again, plain) and tts.formant_stage is None and "formant_s" not in tts.timings  # today's bits, no stage
    up = tts.tts(text, pitch=4, **kw)
    got = tts.tts(text, pitch=4, formants="keep", **kw)
    assert tts.timings["formant_s"] > 0
    want = tts.shift_pitch(plain, 4, formants="keep")
    assert got.shape == up.shape == want.shape and torch.equal(got, want) and torch.isfinite(got).all() and not torch.equal(got, up)
    assert torch.equal(tts.tts(text, formant_shift=3, **kw), tts.shift_formants(plain, 3))
