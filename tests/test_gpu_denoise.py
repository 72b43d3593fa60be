"""-m gpu: the spectral-subtraction denoiser (csrc/denoise.hip) through its C-ABI (include/tortoise_mi355x_nr.h) and the staged operator
entry (include/tortoise_mi355x_test.h) against the fp64 reference and the element-wise bounds of tests/denoise_reference.py: spectrum and
power on every cell, the noise floor BIT FOR BIT against a sort of the device's own power (both forms of the select) and inside the interval
bound, the region mean, the gains, G |spectrum| and the output; ragged batches bit-identical to solo runs, short clips copied, refusals that
write nothing, the clip entries of the API and the voice-cloning path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import denoise_reference as R
from tortoise_tts_amd import denoise as nr, engine as E, stages

pytestmark = pytest.mark.gpu

N, H, B, BP = R.N, R.H, R.B, R.BP
REG = E.NR_REG_FRAMES
MAX_SAMPLES, MAX_CLIPS = REG * H + 255, 16  # a clip of REG + 1 frames, the first the register form does not hold
CANARY = 777.0
U = R.U


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def tb():
    return R.tables()


@pytest.fixture(scope="module")
def handle(lib):
    tabs = {k: v.cuda().contiguous() for k, v in nr.tables().items()}
    c = E.NrConfig()
    c.n_fft, c.hop, c.bins_pad, c.max_samples, c.max_clips = N, H, BP, MAX_SAMPLES, MAX_CLIPS
    t = E.NrTables()
    t.basis, t.inverse = E.ptr(tabs["basis"]), E.ptr(tabs["inverse"])
    h = E.vp()
    E.check(lib.tt_nr_create(C.byref(c), C.byref(t), C.byref(h)))
    yield h
    lib.tt_nr_destroy(h)


@functools.lru_cache(maxsize=None)
def family():
    return R.family()


@functools.lru_cache(maxsize=None)
def hiss(n):
    """seeded noise of n samples with a slow swell: every bin's column has T distinct values"""
    g = torch.Generator().manual_seed(7000 + n % 997)
    x = torch.randn(n, generator=g) * 0.05
    return x * (1.0 + 0.5 * torch.sin(torch.arange(n) * (2 * np.pi / 9000.0)))


def layout(lens, gap=0):
    offs, soffs, a, b = [], [], 0, 0
    for c, n in enumerate(lens):
        a, b = a + (gap + c if gap else 0), b + (gap + c if gap else 0)
        offs.append(a); soffs.append(b)
        a, b = a + n, b + (1 + n // H) * BP
    return offs, soffs, a, b


def run(lib, h, clips, regions, p, staged=False, gap=0):
    """clips (host f32 vectors) in one call -> per clip dict(out [n], floor [BP], status) and, staged, spec [T][BP][2], power [T][BP] (put
    back the usual way round) and gains [T][BP], as host tensors"""
    k, lens = len(clips), [int(x.shape[0]) for x in clips]
    offs, soffs, a, b = layout(lens, gap)
    wav = torch.full((a,), 1.0e3, dtype=torch.float32)  # (anything read from a gap would show)
    for o, x in zip(offs, clips):
        wav[o:o + x.shape[0]] = x
    wav = wav.cuda()
    out = torch.full((a,), CANARY, device="cuda", dtype=torch.float32)
    floor = torch.full((k, BP), CANARY, device="cuda", dtype=torch.float32)
    status = (C.c_int * k)(*([-7] * k))
    ll, ii = (C.c_longlong * k)(*offs), (C.c_int * k)(*lens)
    first, count = (C.c_int * k)(*[r[0] for r in regions]), (C.c_int * k)(*[r[1] for r in regions])
    cp = nr.c_params(p)
    st = None
    if not staged:
        E.check(lib.tt_nr_run(h, E.ptr(wav), ll, ii, first, count, C.byref(cp), k, E.ptr(out), ll, E.ptr(floor), status, E.stream_ptr()))
    else:
        st = [torch.full((2 * b,), CANARY, device="cuda"), torch.full((b,), CANARY, device="cuda"), torch.full((b,), CANARY, device="cuda")]
        E.check(lib.tt_op_nr_run(h, E.ptr(wav), ll, ii, first, count, C.byref(cp), k, E.ptr(out), ll, E.ptr(floor), status, E.ptr(st[0]), E.ptr(st[1]),
                                 E.ptr(st[2]), (C.c_longlong * k)(*soffs), E.stream_ptr()))
    torch.cuda.synchronize()
    o, fl = out.cpu(), floor.cpu()
    used = torch.zeros(a, dtype=torch.bool)
    res = []
    for c, (of, n) in enumerate(zip(offs, lens)):
        used[of:of + n] = True
        r = dict(out=o[of:of + n].clone(), floor=fl[c].clone(), status=int(status[c]))
        if st is not None and r["status"] == E.NR_OK:
            T, so = 1 + n // H, soffs[c]
            r["spec"] = st[0][2 * so:2 * so + 2 * T * BP].cpu().reshape(T, BP, 2)
            r["power"] = st[1][so:so + T * BP].cpu().reshape(BP, T).t().contiguous()
            r["gains"] = st[2][so:so + T * BP].cpu().reshape(T, BP)
        res.append(r)
    assert bool((o[~used] == CANARY).all()), "written outside the clips"
    return res


def bits(t):
    return t.contiguous().view(torch.int32)


def sorted_floor(power, k, c):
    """f32(sort(P[:, b])[k] * c) of every bin from the device's own power [T][BP], numpy f32: one product, rounded once"""
    col = np.sort(power.numpy(), axis=0)[k]
    return torch.from_numpy((col.astype(np.float32) * np.float32(c)).astype(np.float32))


def inside(x, lo, hi):
    x = x.double()
    return bool(((x >= lo) & (x <= hi)).all()), float(torch.maximum(lo - x, x - hi).max())


def staged_checks(name, x, d, tb, p, region=(0, 0)):
    """every comparison of one clip's device results `d` with the fp64 reference"""
    n = int(x.shape[0])
    r = R.denoise_reference(x, tb, p, region)
    T = r.P.shape[0]
    assert d["status"] == E.NR_OK and all(torch.isfinite(d[k]).all() for k in ("out", "floor", "spec", "power", "gains")), name
    assert not d["spec"][:, B:].any() and not d["power"][:, B:].any() and not d["gains"][:, B:].any() and not d["floor"][B:].any()  # the padding
    re, im, P, G = d["spec"][:, :B, 0].double(), d["spec"][:, :B, 1].double(), d["power"][:, :B], d["gains"][:, :B]
    ratios = {"re": R.FR.worst_ratio(re, r.re, r.e_re), "im": R.FR.worst_ratio(im, r.im, r.e_im), "power": R.FR.worst_ratio(P, r.P, r.e_P)}
    # the power is the expression as written, from the device's own spectrum: two products and one add, each rounded (numpy f32)
    sp = d["spec"][:, :B].numpy()
    assert np.array_equal((sp[..., 0] * sp[..., 0] + sp[..., 1] * sp[..., 1]).view(np.int32), P.numpy().view(np.int32)), name
    par = R.Par(p)
    if region[1]:  # the mean of the device's own power over the region, within gamma_m (+ the division)
        m = P[region[0]:region[0] + region[1]].double().mean(0)
        ratios["region mean"] = R.FR.worst_ratio(d["floor"][:B], m, (R.gamma(region[1]) + 2 * U) * m + R.TINY)
    else:  # bit for bit the k-th element of the device's own column sorted, times c
        assert torch.equal(bits(d["floor"][:B]), bits(sorted_floor(P, r.k, par.c))), name
    ok, over = inside(d["floor"][:B], r.S_lo, r.S_hi)
    assert ok, (name, "floor outside its interval by", over)
    # gains: every resolved cell inside its interval; G |spectrum| on EVERY cell
    res = ~r.unresolved
    ok, over = inside(G[res], r.G_lo[res], r.G_hi[res])
    assert ok, (name, "gain outside its interval by", over)
    assert float(G.min()) >= par.g_min and float(G.max()) <= 1.0
    lo, hi = R.magnitude_interval(r)
    ok, over = inside(G.double() * (re * re + im * im).sqrt(), lo, hi)
    assert ok, (name, "G |spectrum| outside its interval by", over)
    # the gain from the device's OWN power and floor: the arithmetic of steps 3 and 4 alone
    g_lo, g_hi = R.gain_interval(P.double(), P.double(), d["floor"][:B].double(), d["floor"][:B].double(), par)
    ok, over = inside(G, g_lo, g_hi)
    assert ok, (name, "gain from the device's power outside its rounding bound by", over)
    # output: from the device's spectrum and gains, then end to end
    o_ref, e_o = R.synthesis(re, im, G.double(), tb, n)
    ratios["output"] = R.FR.worst_ratio(d["out"], o_ref, e_o)
    ratios["end to end"] = R.FR.worst_ratio(d["out"], r.out, r.e_out)
    for stage, (ratio, at) in ratios.items():
        print(f"{name} T {T}: {stage} worst |err| / bound {ratio:.3f} at element {at}")
        assert ratio <= 1.0, (name, stage, ratio, at)
    print(f"{name} T {T}: {int(r.unresolved.sum())} of {r.unresolved.numel()} gain cells unresolved")
    return r


def test_family_against_fp64(lib, handle, tb):
    fam = family()
    other = nr.params(reduction_db=30.0, beta=1.0, quantile=0.5, smooth_frames=0, smooth_bins=4)
    for name, x in fam.items():
        if name == "short":
            continue
        for p in (nr.params(), other) if name in ("white 0 dB", "pink 10 dB", "all ties", "noise only") else (nr.params(),):
            d = run(lib, handle, [x], [(0, 0)], p, staged=True)[0]
            r = staged_checks(f"{name} (q {p.quantile}, Rt {p.smooth_frames}, Rb {p.smooth_bins})", x, d, tb, p)
            if name in ("zero pauses", "clean vowel"):
                assert not d["floor"].any()  # digital silence in more than q of the frames: a floor of exactly 0, nothing removed
                assert float((d["out"] - x).abs().max()) <= 4e-6
            if name == "all ties":
                assert bool((d["power"] == d["power"][0:1]).all())  # every frame the same bits: a column of ties
    # region mode: the noise-only head of the gated clip, and a region in the middle of a noisy one
    x, head = R.gated_noisy()
    reg = nr.region_frames((0.0, head), x.shape[0], R.SR)
    staged_checks("zero pauses, region", x, run(lib, handle, [x], [reg], nr.params(), staged=True)[0], tb, nr.params(), reg)
    x = fam["pink 10 dB"]
    reg = nr.region_frames((1.0, 1.2), x.shape[0], R.SR)
    staged_checks("pink 10 dB, region", x, run(lib, handle, [x], [reg], nr.params(), staged=True)[0], tb, nr.params(), reg)


SELECT_FRAMES = (31, 32, 33, 63, 64, 65, REG - 1, REG, REG + 1)


def test_the_floor_is_the_kth_of_the_sorted_column_bit_for_bit_in_both_forms(lib, handle):
    """every clip and bin, q = 0.01 / 0.2 / 0.5, the register form and the form of long clips (forced on the short ones by the switch; the
    clip of REG + 1 frames takes it by itself), n mod 256 = 0 and 255, a column of ties"""
    lens = [(T - 1) * H + (255 if i % 2 else 0) for i, T in enumerate(SELECT_FRAMES)]
    clips = [hiss(n) for n in lens] + [family()["all ties"], family()["white 0 dB"]]
    regions = [(0, 0)] * len(clips)
    floors = {}
    for form in (0, 1):
        prev = lib.ttx_kernel_variant(E.TTX_NR_SELECT_LONG, form)
        try:
            for q in (0.01, 0.2, 0.5):
                p = nr.params(quantile=q)
                res = run(lib, handle, clips, regions, p, staged=True)
                for x, d in zip(clips, res):
                    T = 1 + x.shape[0] // H
                    if T < E.NR_MIN_FRAMES:
                        assert d["status"] == E.NR_SHORT and torch.equal(bits(d["out"]), bits(x)) and not d["floor"].any()
                        continue
                    want = sorted_floor(d["power"], nr.rank(p.quantile_num, T), R.f32(p.quantile_scale))
                    assert d["status"] == E.NR_OK and torch.equal(bits(d["floor"]), bits(want)), (form, q, T)
                    assert float(d["floor"][:B].min()) > 0.0 or x is clips[-2]
                floors[form, q] = torch.stack([d["floor"] for d in res])
        finally:
            lib.ttx_kernel_variant(E.TTX_NR_SELECT_LONG, prev)
    for q in (0.01, 0.2, 0.5):
        assert torch.equal(bits(floors[0, q]), bits(floors[1, q]))
    assert not torch.equal(floors[0, 0.01], floors[0, 0.5])


def test_ragged_batches_equal_the_solo_calls(lib, handle):
    p = nr.params()
    lens = [8192, 24000, 513, 12033, 8191, 30000, 9000, 16384, 2048, 50000, 8447, 21000, 7935, 40001, 12000, 262399]
    regions = [(0, 0), (10, 20), (0, 0), (0, 0), (2, 8), (0, 0), (0, 36), (30, 35), (0, 9), (100, 64), (0, 0), (0, 0), (0, 0), (5, 100), (0, 0), (0, 0)]
    clips = [hiss(n) for n in lens]
    solo = [run(lib, handle, [x], [r], p)[0] for x, r in zip(clips, regions)]
    assert [s["status"] for s in solo] == [E.NR_OK, E.NR_OK, E.NR_SHORT, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK, E.NR_OK,
                                           E.NR_SHORT, E.NR_OK, E.NR_OK, E.NR_OK]
    for c in (2, 12):  # short clips in auto mode: copied bit for bit, a floor of zeros
        assert torch.equal(bits(solo[c]["out"]), bits(clips[c])) and not solo[c]["floor"].any()
    assert not torch.equal(solo[0]["out"], clips[0])
    for k, gap in ((16, 3), (2, 0), (5, 5)):
        got = run(lib, handle, clips[:k], regions[:k], p, gap=gap)
        for c in range(k):
            assert got[c]["status"] == solo[c]["status"], (k, c)
            assert torch.equal(bits(got[c]["out"]), bits(solo[c]["out"])) and torch.equal(bits(got[c]["floor"]), bits(solo[c]["floor"])), (k, c, lens[c])
    # the operator entry makes the boundary's bits
    got = run(lib, handle, clips[:4], regions[:4], p, staged=True)
    assert all(torch.equal(bits(got[c]["out"]), bits(solo[c]["out"])) and torch.equal(bits(got[c]["floor"]), bits(solo[c]["floor"])) for c in range(4))


def test_every_refusal_writes_nothing(lib, handle):
    good = hiss(12000)
    wav = torch.cat([good, good, good]).cuda()
    out = torch.full((3 * 12000,), CANARY, device="cuda")
    floor = torch.full((3, BP), CANARY, device="cuda")
    status = (C.c_int * 3)(-7, -7, -7)
    L3, I3 = C.c_longlong * 3, C.c_int * 3
    offs = L3(0, 12000, 24000)
    par = lambda **kw: nr.c_params(nr.params()._replace(**kw))
    ok = dict(h=handle, wav=E.ptr(wav), offs=offs, lens=I3(12000, 12000, 12000), first=I3(0, 5, 0), count=I3(0, 8, 0), p=par(), k=3, out=E.ptr(out), ooffs=offs,
              floor=E.ptr(floor), status=status)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tt_nr_run(a["h"], a["wav"], a["offs"], a["lens"], a["first"], a["count"], C.byref(a["p"]) if a["p"] is not None else None, a["k"], a["out"],
                             a["ooffs"], a["floor"], a["status"], E.stream_ptr())
    for bad, words in ((dict(lens=I3(12000, 512, 12000)), b"clip 1 has 512 samples"), (dict(lens=I3(12000, MAX_SAMPLES + 1, 12000)), b"the handle takes"),
                       (dict(count=I3(0, 7, 0)), b"at least TT_NR_MIN_REGION"), (dict(count=I3(0, -1, 0)), b"noise region of -1 frames"),
                       (dict(first=I3(0, 40, 0)), b"not inside the clip"), (dict(first=I3(0, -1, 0)), b"not inside the clip"),
                       (dict(count=I3(0, 48, 0), first=I3(0, 0, 0)), b"not inside the clip"), (dict(k=0), b"0 clips"), (dict(k=MAX_CLIPS + 1), b"17 clips"),
                       (dict(wav=None), b"null"), (dict(out=None), b"null"), (dict(floor=None), b"null"), (dict(status=None), b"null"), (dict(p=None), b"null"),
                       (dict(first=None), b"null"), (dict(offs=L3(0, -1, 24000)), b"negative offset"), (dict(h=None), b"null"),
                       (dict(p=par(quantile_num=99)), b"quantile_num"), (dict(p=par(quantile_num=5001)), b"quantile_num"),
                       (dict(p=par(quantile_scale=0.0)), b"quantile_scale"), (dict(p=par(quantile_scale=float("inf"))), b"quantile_scale"),
                       (dict(p=par(beta=0.5)), b"beta"), (dict(p=par(beta=4.5)), b"beta"), (dict(p=par(g_min=1.0)), b"g_min"), (dict(p=par(g_min=0.001)), b"g_min"),
                       (dict(p=par(smooth_frames=5)), b"smooth_frames"), (dict(p=par(smooth_bins=-1)), b"smooth_bins")):
        assert call(**bad) == -1 and words in lib.tt_last_error(), (bad, lib.tt_last_error())
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((floor == CANARY).all()) and list(status) == [-7, -7, -7]
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == CANARY).any()) and not bool((floor == CANARY).any()) and list(status) == [E.NR_OK] * 3


@torch.no_grad()
def test_stage_and_clip_entries_equal_the_pieces(lib, handle):
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device("cuda")

    host = Host()
    fam = family()
    x, short = fam["pink 0 dB"], fam["short"]
    p = nr.params()
    direct = run(lib, handle, [x], [(0, 0)], p)[0]
    st = stages.DenoiseStage(30000, max_clips=2)
    (y, d), (ys, ds), (yr, dr) = st.denoise_many([x, short, x], [(0, 0), (0, 0), (0, 18)], p)  # three clips through a handle of two: two calls
    assert y.device.type == "cuda" and torch.equal(bits(y.cpu()), bits(direct["out"])) and torch.equal(bits(d["floor"]), bits(direct["floor"][:B]))
    assert d["status"] == E.NR_OK and ds["status"] == E.NR_SHORT and torch.equal(ys.cpu(), short) and d["floor"].shape == (B,)
    assert torch.equal(bits(yr.cpu()), bits(run(lib, handle, [x], [(0, 18)], p)[0]["out"]))
    st.close()
    # the clip entries of the API: shape and device of what came in, the info, nothing built for reduction_db=0
    assert host.denoise(x, reduction_db=0) is x and host.denoiser is None
    got, info = host.denoise(x.reshape(1, 1, -1), return_info=True)
    assert got.shape == (1, 1, x.shape[0]) and got.device.type == "cpu" and torch.equal(bits(got.reshape(-1)), bits(direct["out"]))
    assert info["status"] == "ok" and info["noise_floor"].shape == (B,) and torch.equal(bits(info["noise_floor"]), bits(direct["floor"][:B]))
    assert info["mean_attenuation_db"] > 1.0 and -40.0 < info["noise_dbfs"] < 0.0
    xd = x.cuda().reshape(1, -1)
    outs, infos = host.denoise_many([xd, short, x], noise=[None, None, (0.0, 0.2)], return_info=True)
    assert outs[0].shape == (1, x.shape[0]) and outs[0].device.type == "cuda" and torch.equal(bits(outs[0].cpu().reshape(-1)), bits(direct["out"]))
    assert [i["status"] for i in infos] == ["ok", "short", "ok"] and torch.equal(outs[1], short) and torch.equal(bits(outs[2]), bits(yr.cpu()))
    assert host.denoiser.max_samples == api.DENOISER_SECONDS * nr.VOICE_SAMPLE_RATE
    # what the feature is for: the noise of the pauses goes down by about reduction_db, the vowel stays
    clip, clean, noise, active, pause = R.noisy(144000, 10.0, 1)
    out = host.denoise(clip).double()
    att = R.db(float(clip.double()[pause].pow(2).sum() / out[pause].pow(2).sum()))
    gain = R.db(float(noise[active].pow(2).sum() / (out - clean)[active].pow(2).sum()))
    print(f"white 10 dB on the device: pause attenuation {att:.2f} dB, active SNR +{gain:.2f} dB")
    assert att >= nr.DEFAULTS["reduction_db"] - 1.0 and gain >= 3.0


@torch.no_grad()
def test_voice_clips_are_cleaned_before_the_conditioning_encoders():
    from oracle import make_golden as G
    from tortoise_tts_amd import audio, weights as W
    from tortoise_tts_amd.api import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, VocoderConfig
    ar, clvp, diff = ARConfig(**G.AR_CFG), CLVPConfig(**G.CLVP_CFG), DiffusionConfig(**G.DIFF_CFG)
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(ar), seed=G.COND_SEED),
           "clvp": W.synthetic_state_dict(W.clvp_manifest(clvp), seed=G.CLVP_SEED),
           "diffusion": W.synthetic_state_dict(W.diffusion_manifest(diff), seed=G.COND_SEED + 1),
           "vocoder": W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(VocoderConfig()), seed=G.VOC_SEED))}
    kw = dict(state_dicts=sds, configs={"ar": ar, "clvp": clvp, "diffusion": diff}, max_candidates=8, max_mel_tokens=32)
    fam = family()
    clips = [fam["white 0 dB"].reshape(1, -1), fam["pink 10 dB"].reshape(1, -1)]
    fe = audio.MelFrontEnd(mel_norms=torch.ones(80))
    plain = TextToSpeech(**kw)
    plain.mel_front_end = fe
    a0, d0 = plain.get_conditioning_latents(clips)
    assert plain.denoiser is None  # the default builds nothing
    tts = TextToSpeech(denoise_voice_samples=True, **kw)
    tts.mel_front_end = fe
    a, d = tts.get_conditioning_latents(clips)
    cleaned = plain.denoise_many(clips, sample_rate=nr.VOICE_SAMPLE_RATE)
    a1, d1 = plain.get_conditioning_latents(cleaned)
    assert torch.equal(a, a1) and torch.equal(d, d1) and not torch.equal(a, a0) and cleaned[0].shape == clips[0].shape
    a2, d2 = tts.get_conditioning_latents(clips, denoise=None)  # the keyword overrides the constructor: today's latents, bit for bit
    assert torch.equal(a2, a0) and torch.equal(d2, d0)
    a3, _ = plain.get_conditioning_latents(clips, denoise=True)
    assert torch.equal(a3, a)


def test_tt_fmt_run_still_makes_the_parent_commits_bytes(lib):
    """The STFT, inverse and overlap-add kernels of csrc/formant.hip moved to csrc/stft_kernels.h, which csrc/denoise.hip shares.
    tests/golden/formant_parent_digests.json holds the sha256 of every tt_fmt_run output of formant's test family (lengths x warps x clamps
    of tests/test_gpu_formant.py) as the PARENT commit's build made them on an MI355X (scripts/denoise_time.py --against ... --digests;
    profiles/r30_denoise.txt has the run): this build must make the same bytes."""
    import hashlib
    import json
    import os
    from tests.melfront_reference import probe_signal
    from tortoise_tts_amd import formant as fmt
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "formant_parent_digests.json")))
    Q, lengths, warps, clamps = 48, (513, 1024, 1279, 1280, 4096, 24000), (2.0 ** (4 / 12.0), 2.0 ** (7 / 12.0), 0.5, 2.0, 1.0), (24.0, 6.0)
    assert len(want) == len(lengths) * len(warps) * len(clamps)
    tabs = {k: v.cuda().contiguous() for k, v in fmt.tables(Q, list(warps)).items()}
    for db in clamps:
        c = E.FmtConfig()
        c.n_fft, c.hop, c.bins_pad, c.q, c.max_gain_db, c.max_samples, c.max_clips, c.n_warps = fmt.N_FFT, fmt.HOP, fmt.BINS_PAD, Q, db, 24000, 1, len(warps)
        t = E.FmtTables()
        t.basis, t.inverse, t.cepstrum, t.warps = (E.ptr(tabs[k]) for k in ("basis", "inverse", "cepstrum", "warps"))
        h = E.vp()
        E.check(lib.tt_fmt_create(C.byref(c), C.byref(t), C.byref(h)))
        try:
            for n in lengths:
                wav = probe_signal(n, seed=n % 7, sr=24000.0).cuda()
                for wi in range(len(warps)):
                    y = torch.full((n,), -7.0, device="cuda")
                    E.check(lib.tt_fmt_run(h, E.ptr(wav), (C.c_longlong * 1)(0), (C.c_int * 1)(n), (C.c_int * 1)(wi), 1, E.ptr(y), (C.c_longlong * 1)(0), E.stream_ptr()))
                    torch.cuda.synchronize()
                    assert hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest() == want["%d,%d,%g" % (n, wi, db)], (n, wi, db)
        finally:
            lib.tt_fmt_destroy(h)
