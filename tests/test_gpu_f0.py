"""The F0 tracker on the MI355X (csrc/f0.hip, include/tortoise_mi355x_f0.h) against the fp64 reference of tests/f0_reference.py.

  1. the harmonic family: d' of every frame and lag inside its bound, lag and the voiced flag equal on every frame the reference calls
     unambiguous, aper and f0 inside their bounds there, at most 5 % of the frames skipped (the worst share of each bound is printed);
  2. clip lengths at every border of the hops and of the kernel's frame group; 3. a ragged batch of 16 bit-identical to solo calls;
  4. the parameter edges; 5. a clip that is not OK gets its status and nothing else; 6. the argument checks;
  7. the interface: shift_pitch(semitones=) moves the measured median by what it says, shift_pitch(to_hz=) lands on the target,
     tts(pitch_hz=) is shift_pitch_many(to_hz=) of the plain clips, and tts without the keyword returns today's bits.
Every clip is at most 12000 samples (50 frames, thirteen workgroups)."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import f0_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import pitch as P
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7
MAX_SAMPLES = 12000
DEFAULT = ((48, 400), (0.15, R.W * 1e-5))  # fmin 60, fmax 500, threshold 0.15, floor -50 dB

_stage = []


def stage():
    if not _stage:
        _stage.append(stages.F0Stage(MAX_SAMPLES, max_clips=16, device=DEV))
    return _stage[0]


def device_track(clips, pars=None, thrs=None, slices=None, dprime=False):
    """One tt_f0_track call (the test entry with dprime=True) over clips = [x f32 [n]] with every output pre-filled with SENT -> per clip
    the raw status, n_voiced, lag, f0, aper (SENT where the call wrote nothing).  pars / thrs: (lo, hi) / (thr, floor_e) per clip, passed
    as they are; slices: per clip the entries of its frame slice where they are not tt_f0_frames(n)."""
    st, n = stage(), len(clips)
    pars = pars or [DEFAULT[0]] * n
    thrs = thrs or [DEFAULT[1]] * n
    slices = [R.frames(len(x)) if s is None else s for s, x in zip(slices or [None] * n, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x in clips]))).astype(np.int32)
    fo = np.concatenate(([0], np.cumsum(slices))).astype(np.int32)
    Fs = int(fo[-1])
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x in clips] + [np.zeros(1, np.float32)])).to(DEV)
    io_d, fo_d = torch.from_numpy(io).to(DEV), torch.from_numpy(fo).to(DEV)
    par = torch.tensor(pars, dtype=torch.int32, device=DEV).reshape(-1)
    thr = torch.tensor(thrs, dtype=torch.float64, device=DEV).reshape(-1)
    lag = torch.full((Fs + 1,), SENT, dtype=torch.int32, device=DEV)
    f0 = torch.full((Fs + 1,), float(SENT), device=DEV)
    aper = torch.full((Fs + 1,), float(SENT), device=DEV)
    nv = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    status = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    args = (st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(par), E.ptr(thr), E.ptr(fo_d), E.ptr(lag), E.ptr(f0), E.ptr(aper), E.ptr(nv), E.ptr(status))
    dp = None
    if dprime:
        dp = torch.full(((Fs + 1) * (R.T + 1),), float(SENT), dtype=torch.float64, device=DEV)
        E.check(st.lib.tt_op_f0_track(*args, E.ptr(dp), E.stream_ptr()))
        dp = dp.cpu().numpy().reshape(Fs + 1, R.T + 1)
        assert (dp[Fs] == SENT).all()
    else:
        E.check(st.lib.tt_f0_track(*args, E.stream_ptr()))
    lag, f0, aper, nv, status = (t.cpu().numpy() for t in (lag, f0, aper, nv, status))
    assert lag[Fs] == SENT and f0[Fs] == SENT and aper[Fs] == SENT  # nothing beyond the batch
    out = []
    for i in range(n):
        a, b = int(fo[i]), int(fo[i + 1])
        d = dict(status=int(status[i]), n_voiced=nv[i:i + 1], lag=lag[a:b], f0=f0[a:b], aper=aper[a:b])
        if dprime:
            d["dprime"] = dp[a:b]
        out.append(d)
    return out


def untouched(r):
    return (r["lag"] == SENT).all() and (r["f0"] == SENT).all() and (r["aper"] == SENT).all() and r["n_voiced"][0] == SENT


def same(a, b):
    return a["status"] == b["status"] and all(a[k].tobytes() == b[k].tobytes() for k in ("n_voiced", "lag", "f0", "aper"))


class Worst:
    """The worst |err| / bound of each quantity, and the frames compared and skipped."""

    def __init__(self):
        self.share = dict(dprime=0.0, aper=0.0, f0=0.0)
        self.frames = self.skipped = 0

    def clip(self, got, ref):
        F = len(ref["lag"])
        assert got["status"] == E.F0_OK and got["lag"].shape == (F,)
        if "dprime" in got:
            err, bound = np.abs(got["dprime"] - ref["dprime"]), ref["dprime_bound"]
            assert (err <= bound).all(), f"d' outside its bound: worst {np.max(err - bound)} over"
            assert (got["dprime"][bound == 0] == ref["dprime"][bound == 0]).all()
            self.share["dprime"] = max(self.share["dprime"], float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        ok = ~ref["ambiguous"]
        self.frames += F
        self.skipped += int(F - ok.sum())
        assert (got["lag"][ok] == ref["lag"][ok]).all(), (got["lag"], ref["lag"], ok)
        assert ((got["f0"] > 0)[ok] == ref["voiced"][ok]).all()
        assert (got["lag"] >= 24).all() and (got["lag"] <= 480).all() and int(got["n_voiced"][0]) == int((got["f0"] > 0).sum())
        for key in ("aper", "f0"):
            err, bound = np.abs(got[key].astype(np.float64) - ref[key])[ok], ref[key + "_bound"][ok]
            assert (err <= bound).all(), f"{key} outside its bound: {err[err > bound]} against {bound[err > bound]}"
            self.share[key] = max(self.share[key], float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))

    def report(self, what):
        print(f"[f0] {what}: {self.frames} frames, {self.skipped} skipped as ambiguous; worst |err| / bound: "
              + ", ".join(f"{k} {v:.4f}" for k, v in self.share.items()))


@pytest.fixture(scope="module")
def solo():
    return [device_track([x], dprime=True)[0] for _, _, x, _ in R.family()]


# ----------------------------------------------------------------------------------------- 1. the family against the reference
def test_family_agrees_with_the_reference(solo):
    w = Worst()
    for got, (_, _, _, ref) in zip(solo, R.family()):
        w.clip(got, ref)
    w.report("harmonic family")
    assert w.frames == 1200 and w.skipped <= 0.05 * w.frames


# ----------------------------------------------------------------------------------------- 2. lengths and borders
def lengths():
    G = 4  # the kernel's frame group; test_the_frame_group_is_the_one_the_lengths_were_chosen_for checks it
    return [1, 239, 240, 241, 719, 720, 721, G * 240 - 1, G * 240, G * 240 + 1, 500, 2 * G * 240 + 100]


def test_the_frame_group_is_the_one_the_lengths_were_chosen_for():
    assert stage().lib.tt_op_f0_group() == 4 and R.frames(4 * 240 + 1) == 5 and R.frames(2 * 4 * 240 + 100) == 9  # a last group of one frame


def test_every_length_alone():
    x = R.harmonic(150.0, n=MAX_SAMPLES, snr_db=40.0, seed=11)
    w = Worst()
    for n in lengths():
        w.clip(device_track([x[:n]], dprime=True)[0], R.track(x[:n]))
    w.report("lengths " + ", ".join(str(n) for n in lengths()))
    assert w.skipped < w.frames


# ----------------------------------------------------------------------------------------- 3. ragged batches
def test_a_ragged_batch_of_16_is_bit_identical_to_solo():
    fam = R.family()
    rng = np.random.default_rng(3)
    clips, pars, thrs = [], [], []
    for i in range(14):
        x = fam[(5 * i) % len(fam)][2]
        clips.append(x[:int(rng.integers(1, MAX_SAMPLES + 1))] if i % 3 else x)
        lo = int(rng.integers(24, 200))
        pars.append((lo, int(rng.integers(lo, 481))))
        thrs.append((float(rng.uniform(0.05, 0.5)), float(10.0 ** rng.uniform(-6, 1))))
    clips.insert(4, np.zeros(0, np.float32))           # an empty clip
    pars.insert(4, DEFAULT[0]); thrs.insert(4, DEFAULT[1])
    clips.insert(9, np.zeros(3001, np.float32))        # digital silence
    pars.insert(9, DEFAULT[0]); thrs.insert(9, DEFAULT[1])
    batch = device_track(clips, pars, thrs)
    assert len(batch) == 16
    for i, (x, p, t, got) in enumerate(zip(clips, pars, thrs, batch)):
        alone = device_track([x], [p], [t])[0]
        assert same(got, alone), i
        if len(x) == 0:
            assert got["status"] == E.F0_EMPTY and got["n_voiced"][0] == SENT
        else:
            assert got["status"] == E.F0_OK
    assert int(batch[9]["n_voiced"][0]) == 0 and (batch[9]["f0"] == 0).all() and (batch[9]["aper"] == 1).all() and (batch[9]["lag"] == 48).all()
    # the stage's own call: the same bits
    st = stage()
    live = [i for i in range(16) if len(clips[i])]
    res = st.track_many([torch.from_numpy(np.array(clips[i])) for i in live], [P.Params(*pars[i], *thrs[i]) for i in live])
    for i, r in zip(live, res):
        assert r["lag"].tobytes() == batch[i]["lag"].tobytes() and r["f0"].tobytes() == batch[i]["f0"].tobytes()
        assert r["aper"].tobytes() == batch[i]["aper"].tobytes() and r["n_voiced"] == int(batch[i]["n_voiced"][0])


# ----------------------------------------------------------------------------------------- 4. parameter edges
def test_parameter_edges():
    x = R.harmonic(150.0, n=6000, snr_db=40.0, seed=12)
    big = 1e6
    cases = [((160, 160), DEFAULT[1]), ((24, 480), DEFAULT[1]), ((48, 400), (0.0, DEFAULT[1][1])), ((48, 400), (2.0, DEFAULT[1][1])),
             ((48, 400), (0.15, big)), ((480, 480), (2.0, 0.0)), ((24, 24), (0.0, 0.0))]
    batch = device_track([x] * len(cases), [c[0] for c in cases], [c[1] for c in cases], dprime=True)
    w = Worst()
    for got, (par, thr) in zip(batch, cases):
        ref = R.track(x, par[0], par[1], thr[0], thr[1])
        w.clip(got, ref)
        assert (got["lag"] >= par[0]).all() and (got["lag"] <= par[1]).all()
    w.report("parameter edges")
    assert (batch[0]["lag"] == 160).all()                                             # lo = hi
    assert (batch[2]["f0"] == 0).all() and int(batch[2]["n_voiced"][0]) == 0          # thr = 0: never voiced, the lag is the argmin
    ref = R.track(x, 48, 400, 0.0, DEFAULT[1][1])
    inner = [f for f in R.inner_frames(len(x)) if not ref["ambiguous"][f]]
    assert inner and all(batch[2]["lag"][f] == 48 + int(np.argmin(ref["dprime"][f, 48:401])) for f in inner)
    d48 = batch[3]["dprime"][:, 48]                                                   # thr = 2: t0 = lo unless d'(lo) = 2 exactly
    assert (d48 < 2.0).all() and (batch[3]["f0"][np.array(R.inner_frames(len(x)))] > 0).all()
    assert (batch[4]["f0"] == 0).all() and int(batch[4]["n_voiced"][0]) == 0          # a floor above every frame
    full = device_track([x], [(48, 400)], [DEFAULT[1]])[0]
    assert (batch[4]["lag"] == full["lag"]).all() and batch[4]["aper"].tobytes() == full["aper"].tobytes()  # the floor changes the flag alone


# ----------------------------------------------------------------------------------------- 5. refusals
BAD = {
    "lo below 24": dict(par=(23, 400)), "hi above 480": dict(par=(48, 481)), "lo above hi": dict(par=(300, 299)),
    "thr below 0": dict(thr=(-0.01, 0.01)), "thr above 2": dict(thr=(2.01, 0.01)), "thr not a number": dict(thr=(math.nan, 0.01)),
    "floor negative": dict(thr=(0.15, -1e-9)), "floor infinite": dict(thr=(0.15, math.inf)), "floor not a number": dict(thr=(0.15, math.nan)),
    "over max_samples": dict(n=MAX_SAMPLES + 1), "frame slice too short": dict(slice_less=1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_clip_that_is_not_ok_gets_its_status_and_nothing_else(name, solo):
    fam, bad = R.family(), BAD[name]
    x = R.harmonic(200.0, n=bad.get("n", 5000), snr_db=40.0, seed=13)
    sl = R.frames(len(x)) - bad.get("slice_less", 0)
    batch = device_track([fam[2][2], x, fam[7][2]], [DEFAULT[0], bad.get("par", DEFAULT[0]), DEFAULT[0]],
                         [DEFAULT[1], bad.get("thr", DEFAULT[1]), DEFAULT[1]], [None, sl, None])
    assert batch[1]["status"] == E.F0_REFUSED and untouched(batch[1])
    for got, k in ((batch[0], 2), (batch[2], 7)):
        assert same(got, {key: solo[k][key] for key in ("status", "n_voiced", "lag", "f0", "aper")})


# ----------------------------------------------------------------------------------------- 6. argument checks
def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    ok = lambda n, a=E.ptr(y): st.lib.tt_f0_track(st.h, n, a, E.ptr(i), E.ptr(i), E.ptr(d), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(y), E.ptr(i), E.ptr(i),
                                                  E.stream_ptr())
    for n in (0, 17):
        assert ok(n) == -1 and b"clips (1 .. 16)" in st.lib.tt_last_error()
    assert ok(1, None) == -1 and b"null argument" in st.lib.tt_last_error()
    assert st.lib.tt_op_f0_track(st.h, 1, E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(d), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(y), E.ptr(i), E.ptr(i), None,
                                 E.stream_ptr()) == -1
    h = E.vp()
    assert st.lib.tt_f0_create(E.F0_MAX_SAMPLES + 1, 1, h) == -1 and b"max_samples" in st.lib.tt_last_error()
    assert st.lib.tt_f0_create(100, 65, h) == -1 and b"max_clips 65 (1 .. 64)" in st.lib.tt_last_error()
    with pytest.raises(ValueError, match="exceed the F0 stage's capacity"):
        st.track_many([torch.zeros(MAX_SAMPLES + 1)], [P.params()])
    with pytest.raises(ValueError, match="at least one sample"):
        st.track_many([torch.zeros(0)], [P.params()])


# ----------------------------------------------------------------------------------------- 7. the interface
def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


def _median(track):
    v = track["f0"][track["f0"] > 0]
    return float(np.median(v))


@torch.no_grad()
def test_shift_pitch_moves_the_measured_median_by_what_it_says():
    h = _host()
    x = R.harmonic(150.0, n=MAX_SAMPLES, snr_db=None, seed=14)
    xt = torch.from_numpy(x.copy())
    tr_x = h.f0(xt)
    assert isinstance(tr_x, P.F0Track) and len(tr_x) == 50 and abs(R.cents(tr_x.median_hz(), 150.0)) < 1.0
    ref_x = _median(R.track(x))
    for s in (-5, 3, 7):
        y = h.shift_pitch(xt, semitones=s)
        ref_err = abs(R.cents(_median(R.track(y.numpy())), ref_x) - 100.0 * s)  # the reference's own error on the same two clips
        dev_err = abs(R.cents(h.f0(y).median_hz(), tr_x.median_hz()) - 100.0 * s)
        print(f"[f0] shift_pitch({s:+d}): the measured median moved by {s:+d} semitones to within {dev_err:.4f} cents (reference {ref_err:.4f})")
        assert dev_err <= 2.0 * ref_err
    y, info = h.shift_pitch(xt, to_hz=180.0, return_info=True)
    ref_err = abs(R.cents(_median(R.track(y.numpy())), 180.0))
    dev_err = abs(R.cents(h.f0(y).median_hz(), 180.0))
    print(f"[f0] shift_pitch(to_hz=180): lands within {dev_err:.4f} cents (reference {ref_err:.4f}); measured {info['measured_hz']:.3f} Hz")
    assert dev_err <= 2.0 * ref_err
    assert info["measured_hz"] == tr_x.median_hz() and not info["clamped"] and abs(info["semitones"] - 12 * math.log2(180 / tr_x.median_hz())) < 1e-12
    assert h.pitch_info == [info] and h.f0_stage.max_samples == 30 * 24000 and h.f0_stage.max_clips == 16
    # clips on the device, a target each; the same bits as the semitones the readings give
    out, infos = h.shift_pitch_many([xt.to(DEV).reshape(1, 1, -1), xt[:6000]], to_hz=[180.0, 120.0], return_info=True)
    assert out[0].device.type == "cuda" and out[0].shape[:2] == (1, 1) and torch.equal(out[0].cpu().reshape(-1).view(torch.int32), y.view(torch.int32))
    want = h.shift_pitch_many([xt[:6000]], [infos[1]["semitones"]])[0]
    assert torch.equal(out[1].view(torch.int32), want.view(torch.int32))


@pytest.fixture(scope="module")
def tts():
    import bench
    from tests.test_gpu_ctc import _IdsTokenizer
    from tortoise_tts_amd.api import TextToSpeech
    t = TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)
    t._tokenizer = _IdsTokenizer(bench.synthetic_prompt()[0].tolist())
    return t


@torch.no_grad()
def test_pitch_hz_on_tts(tts):
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts("hello there", **kw)
    assert tts.f0_stage is None and tts.pitch_info is None  # without the keyword nothing is built
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a synthetic checkpoint's clip may have no median: it is then returned as it is, with a warning)
        at = tts.tts("hello there", pitch_hz=180.0, **kw)
        info = tts.pitch_info
        want, winfo = tts.shift_pitch_many([plain], to_hz=180.0, return_info=True)
    assert torch.equal(at.view(torch.int32), want[0].view(torch.int32)) and len(info) == 1
    assert info[0]["measured_hz"] == winfo[0]["measured_hz"] and info[0]["semitones"] == winfo[0]["semitones"] and "f0_s" in tts.timings
    print(f"[f0] tts(pitch_hz=180) on the synthetic checkpoint: measured {info[0]['measured_hz']} Hz, shift {info[0]['semitones']:+.3f} semitones")
    again = tts.tts("hello there", **kw)
    assert torch.equal(again.view(torch.int32), plain.view(torch.int32))  # without the keyword, today's bits
    with pytest.raises(ValueError, match="goes with neither pitch= nor word_pitches="):
        tts.tts("hello there", pitch_hz=180.0, pitch=2, **kw)
