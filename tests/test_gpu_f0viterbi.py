"""The Viterbi F0 path on the MI355X (csrc/f0_viterbi.hip, include/tortoise_mi355x_f0v.h) against the fp64 reference of tests/f0v_reference.py.

  1. the path kernel alone (tt_op_f0v_path) on 300 seeded candidate tables: state, lag, n_voiced and the cost bit for bit;
  2. the candidate kernel alone (tt_op_f0v_candidates) on the family: lag sets equal on every frame whose set is not in doubt, dp and the
     candidates' f0 inside their bounds (the worst share of each bound is printed);
  3. end to end (tt_f0v_track) on every unambiguous clip: lag and voicing on every frame, state where the set is not in doubt, f0 and aper
     inside their bounds, |cost - ref| <= B; the planted clips beside tt_f0_track; shift_pitch(to_hz=, f0_smooth=True);
  4. lengths at every border; 5. a ragged batch of 16 bit-identical to solo calls; 6. refusals; 7. smooth=None is tt_f0_track's bits.
Every clip is at most 12000 samples."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import f0_reference as R
from tests import f0v_reference as V
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import pitch as P
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7
MAX_SAMPLES = 12000          # 50 frames a clip ...
PATH_SAMPLES = 500 * 240     # ... and a handle of 500 frames for the path kernel's tables
PAR, THR = (48, 400), (0.15, R.W * 1e-5)

_stages = {}


def stage(max_samples=MAX_SAMPLES):
    if max_samples not in _stages:
        _stages[max_samples] = stages.F0ViterbiStage(max_samples, max_clips=16, device=DEV)
    return _stages[max_samples]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype)).reshape(-1)).to(DEV)


def _outputs(Fs, n):
    return dict(lag=torch.full((Fs + 1,), SENT, dtype=torch.int32, device=DEV), f0=torch.full((Fs + 1,), float(SENT), device=DEV),
                aper=torch.full((Fs + 1,), float(SENT), device=DEV), state=torch.full((Fs + 1,), SENT, dtype=torch.int32, device=DEV),
                n_voiced=torch.full((n,), SENT, dtype=torch.int32, device=DEV), cost=torch.full((n,), float(SENT), dtype=torch.float64, device=DEV),
                status=torch.full((n,), SENT, dtype=torch.int32, device=DEV))


def _cut(o, fo, n):
    Fs = int(fo[-1])
    h = {k: v.cpu().numpy() for k, v in o.items()}
    assert h["lag"][Fs] == SENT and h["f0"][Fs] == SENT and h["aper"][Fs] == SENT and h["state"][Fs] == SENT  # nothing beyond the batch
    return [dict(status=int(h["status"][i]), n_voiced=h["n_voiced"][i:i + 1], cost=h["cost"][i:i + 1],
                 **{k: h[k][int(fo[i]):int(fo[i + 1])] for k in ("lag", "f0", "aper", "state")}) for i in range(n)]


def device_path(tabs, pars=None, costs=None, frames=None, slices=None, st=None):
    """One tt_op_f0v_path call over tabs = [(lag i32 [F, 8], dp f64 [F, 8], f0 f32 [F, 8])], every output pre-filled with SENT."""
    st, n = st or stage(PATH_SAMPLES), len(tabs)
    frames = [len(t[0]) for t in tabs] if frames is None else frames
    slices = [len(t[0]) for t in tabs] if slices is None else slices
    fo = np.concatenate(([0], np.cumsum(slices))).astype(np.int32)
    lag = np.zeros((int(fo[-1]) + 1, 8), np.int32)
    dp, f0 = np.zeros(lag.shape), np.zeros(lag.shape, np.float32)
    for i, t in enumerate(tabs):
        k = min(len(t[0]), int(fo[i + 1] - fo[i]))
        lag[fo[i]:fo[i] + k], dp[fo[i]:fo[i] + k], f0[fo[i]:fo[i] + k] = t[0][:k], t[1][:k], t[2][:k]
    o = _outputs(int(fo[-1]), n)
    a = [_dev(frames, np.int32), _dev(pars or [PAR] * n, np.int32), _dev(costs or [V.COSTS] * n, np.float64), _dev(fo, np.int32), _dev(lag, np.int32),
         _dev(dp, np.float64), _dev(f0, np.float32)]
    E.check(st.lib.tt_op_f0v_path(st.h, n, *[E.ptr(t) for t in a], E.ptr(o["lag"]), E.ptr(o["f0"]), E.ptr(o["aper"]), E.ptr(o["state"]),
                                  E.ptr(o["n_voiced"]), E.ptr(o["cost"]), E.ptr(o["status"]), E.stream_ptr()))
    return _cut(o, fo, n)


def _audio(clips):
    io = np.concatenate(([0], np.cumsum([len(x) for x in clips]))).astype(np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x in clips] + [np.zeros(1, np.float32)])).to(DEV)
    return audio, io


def device_candidates(clips, pars=None, thrs=None):
    """One tt_op_f0v_candidates call -> per clip (status, lag [F, 8], dp [F, 8], f0 [F, 8]), SENT where nothing was written."""
    st, n = stage(), len(clips)
    audio, io = _audio(clips)
    fo = np.concatenate(([0], np.cumsum([R.frames(len(x)) for x in clips]))).astype(np.int32)
    Fs = int(fo[-1])
    lag = torch.full(((Fs + 1) * 8,), SENT, dtype=torch.int32, device=DEV)
    dp = torch.full(((Fs + 1) * 8,), float(SENT), dtype=torch.float64, device=DEV)
    f0 = torch.full(((Fs + 1) * 8,), float(SENT), device=DEV)
    status = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    a = [audio, _dev(io, np.int32), _dev(pars or [PAR] * n, np.int32), _dev(thrs or [THR] * n, np.float64), _dev(fo, np.int32)]
    E.check(st.lib.tt_op_f0v_candidates(st.h, n, *[E.ptr(t) for t in a], E.ptr(lag), E.ptr(dp), E.ptr(f0), E.ptr(status), E.stream_ptr()))
    lag, dp, f0 = lag.cpu().numpy().reshape(-1, 8), dp.cpu().numpy().reshape(-1, 8), f0.cpu().numpy().reshape(-1, 8)
    assert (lag[Fs] == SENT).all() and (dp[Fs] == SENT).all()
    status = status.cpu().numpy()
    return [(int(status[i]), lag[fo[i]:fo[i + 1]], dp[fo[i]:fo[i + 1]], f0[fo[i]:fo[i + 1]]) for i in range(n)]


def device_track(clips, pars=None, thrs=None, costs=None, slices=None, n_clips=None):
    """One tt_f0v_track call, every output pre-filled with SENT -> per clip status, n_voiced, cost, lag, f0, aper, state."""
    st, n = stage(), len(clips)
    audio, io = _audio(clips)
    slices = [R.frames(len(x)) if s is None else s for s, x in zip(slices or [None] * n, clips)]
    fo = np.concatenate(([0], np.cumsum(slices))).astype(np.int32)
    o = _outputs(int(fo[-1]), n)
    a = [audio, _dev(io, np.int32), _dev(pars or [PAR] * n, np.int32), _dev(thrs or [THR] * n, np.float64), _dev(costs or [V.COSTS] * n, np.float64),
         _dev(fo, np.int32)]
    rc = st.lib.tt_f0v_track(st.h, n if n_clips is None else n_clips, *[E.ptr(t) for t in a], E.ptr(o["lag"]), E.ptr(o["f0"]), E.ptr(o["aper"]),
                             E.ptr(o["state"]), E.ptr(o["n_voiced"]), E.ptr(o["cost"]), E.ptr(o["status"]), E.stream_ptr())
    if n_clips is not None:
        return rc, _cut(o, fo, n)
    E.check(rc)
    return _cut(o, fo, n)


def untouched(r):
    return all((r[k] == SENT).all() for k in ("lag", "f0", "aper", "state", "n_voiced", "cost"))


def same(a, b):
    return a["status"] == b["status"] and all(a[k].tobytes() == b[k].tobytes() for k in ("n_voiced", "cost", "lag", "f0", "aper", "state"))


# ----------------------------------------------------------------------------------------- 1. the path kernel, exact
def random_tables(rng, F):
    """Candidate tables of F frames: k of 0 .. 7 candidates a frame by ascending lag, planted ties (dp on a grid of 1 / 8, lags that are
    powers of two: every cost is then exact), runs of frames with no candidate at all, and some pick in slot 7."""
    lag, dp, f0 = np.zeros((F, 8), np.int32), np.zeros((F, 8)), np.zeros((F, 8), np.float32)
    grid = rng.random() < 0.4
    t = 0
    while t < F:
        run = int(rng.integers(1, 6))
        empty = rng.random() < 0.15
        for f in range(t, min(F, t + run)):
            k = 0 if empty else int(rng.integers(0, 8))
            pool = np.array([32, 64, 128, 256]) if grid else np.arange(24, 481)
            k = min(k, len(pool))
            lags = np.sort(rng.choice(pool, size=k, replace=False))
            lag[f, :k] = lags
            dp[f, :k] = rng.integers(0, 5, size=k) / 8.0 if grid else rng.uniform(0.0, 1.2, size=k)
            f0[f, :k] = 24000.0 / lags
            lag[f, 7], dp[f, 7] = int(rng.integers(24, 481)), float(rng.uniform(0.2, 2.0))
        t += run
    return lag, dp, f0


def check_path(got, tab, lo, costs):
    lag, dp, f0 = tab
    state, cost = V.viterbi_tables(lag, dp, lo, costs)
    F = len(lag)
    assert got["status"] == E.F0_OK
    assert (got["state"] == state).all(), (got["state"], state)
    assert (got["lag"] == lag[np.arange(F), state]).all()
    assert got["cost"].view(np.int64)[0] == np.array([cost]).view(np.int64)[0], (got["cost"][0], cost)  # bit for bit
    assert int(got["n_voiced"][0]) == int((state != 7).sum())
    assert got["aper"].tobytes() == dp[np.arange(F), state].astype(np.float32).tobytes()
    assert got["f0"].tobytes() == np.where(state == 7, 0, f0[np.arange(F), state]).astype(np.float32).tobytes()


def test_path_kernel_is_the_reference_bit_for_bit():
    rng = np.random.default_rng(28)
    sizes = [1, 2, 3, 63, 64, 65, 500]
    tabs, pars, costs = [], [], []
    for i in range(300):
        tabs.append(random_tables(rng, sizes[i % len(sizes)]))
        pars.append((int(rng.choice([24, 32, 48])), 480))
        kind = i % 4  # the defaults; all zero (a tie at every step); a grid of 1 / 8 (exact sums: ties between unlike paths); anything
        costs.append(V.COSTS if kind == 0 else (0.0, 0.0, 0.0, 0.0) if kind == 1 else tuple(float(v) / 8.0 for v in rng.integers(0, 4, size=4))
                     if kind == 2 else tuple(float(v) for v in rng.uniform(0, 0.5, size=4)))
    assert {len(t[0]) for t in tabs} == set(sizes)
    for a in range(0, 300, 16):
        got = device_path(tabs[a:a + 16], pars[a:a + 16], costs[a:a + 16])
        for g, t, p, c in zip(got, tabs[a:a + 16], pars[a:a + 16], costs[a:a + 16]):
            check_path(g, t, p[0], c)


def test_path_kernel_hand_cases():
    """F = 1; every state absent but 7; a tie at every step with a state missing in the middle."""
    def tab(F):
        lag = np.zeros((F, 8), np.int32)
        lag[:, 7] = 48
        return lag, np.zeros((F, 8)), np.zeros((F, 8), np.float32)
    one = tab(1)
    one[0][0, :2], one[1][0, :2] = (100, 200), (0.05, 0.02)
    none = tab(4)
    tie = tab(5)
    tie[0][:, :3] = (100, 200, 300)
    tie[0][1, 0] = tie[0][3, 0] = 0
    got = device_path([one, none, tie], costs=[V.COSTS, (0.01, 0.35, 0.14, 0.25), (0.0, 0.0, 0.0, 0.0)])
    assert got[0]["state"].tolist() == [1] and got[0]["cost"][0] == 0.02 + 0.01 * (V.L2[200] - V.L2[48]) and got[0]["lag"].tolist() == [200]
    assert got[1]["state"].tolist() == [7] * 4 and got[1]["cost"][0] == 1.0 and int(got[1]["n_voiced"][0]) == 0 and got[1]["lag"].tolist() == [48] * 4
    assert got[2]["state"].tolist() == [0, 1, 0, 1, 0] and got[2]["cost"][0] == 0.0 and got[2]["lag"].tolist() == [100, 200, 100, 200, 100]


# ----------------------------------------------------------------------------------------- 2. the candidate kernel
@functools.lru_cache(maxsize=None)
def extras():
    """Two clips for the frames the family does not have: a constant (power above the floor, d' = 1 throughout: no dip) and a clean tone whose
    period of 55 samples has exactly 7 multiples in [48, 400]."""
    out = []
    for name, x in (("constant", np.full(2400, 0.1, np.float32)), ("436.4 Hz", R.harmonic(24000.0 / 55.0, n=6000, seed=41))):
        out.append((name, None, False, x, V.track_smooth(x)))
    return out


@pytest.fixture(scope="module")
def fam_candidates():
    fam = V.family() + extras()
    out = []
    for a in range(0, len(fam), 16):
        out += device_candidates([f[3] for f in fam[a:a + 16]], thrs=[(f[4]["thr"], f[4]["floor_e"]) for f in fam[a:a + 16]])
    return out


def test_candidates_agree_with_the_reference(fam_candidates):
    worst = dict(dp=0.0, f0=0.0)
    seen = dict(more=0, seven=0, none=0, floor=0)
    frames = skipped = 0
    for (status, lag, dp, f0), (name, _, _, x, ref) in zip(fam_candidates, V.family() + extras()):
        pl = ref["plain"]
        assert status == E.F0_OK and lag.shape == (len(pl["lag"]), 8), name
        for f in range(len(lag)):
            frames += 1
            assert lag[f, 7] == pl["lag"][f] or pl["ambiguous"][f]  # slot 7: tt_f0_track's own pick
            assert f0[f, 7] == 0 and (lag[f, :7][lag[f, :7] > 0] >= 48).all() and (lag[f, :7] <= 400).all()
            k = int((lag[f, :7] > 0).sum())
            assert (lag[f, :k] > 0).all() and (np.diff(lag[f, :k]) > 0).all() and (lag[f, k:7] == 0).all()  # ascending, the absent ones last
            for s in range(k):  # whatever was kept: d' of that lag inside the bound of the reference's d'
                l = lag[f, s]
                err, b = abs(dp[f, s] - pl["dprime"][f, l]), pl["dprime_bound"][f, l]
                assert err <= b, (name, f, l)
                worst["dp"] = max(worst["dp"], err / b if b > 0 else 0.0)
            if ref["cand_ambiguous"][f]:
                skipped += 1
                continue
            want = ref["cands"][f]
            n_dips = int(V.dip_flags(pl["dprime"][f], 48, 400).sum()) if pl["power"][f] >= THR[1] else -1
            seen["more"] += n_dips > 7
            seen["seven"] += n_dips == 7
            seen["none"] += n_dips == 0
            seen["floor"] += n_dips == -1
            assert lag[f, :k].tolist() == [l for l, _ in want], (name, f)
            for s in range(k):
                b = ref["cand_f0_bound"][f][s]
                if b is not None:
                    err = abs(float(f0[f, s]) - ref["cand_f0"][f][s])
                    assert err <= b, (name, f, s, err, b)
                    worst["f0"] = max(worst["f0"], err / b)
    print(f"[f0v] candidates of the family: {frames} frames, {skipped} skipped (set in doubt); worst |err| / bound: dp {worst['dp']:.4f}, "
          f"f0 {worst['f0']:.4f}; frames with more than 7 dips {seen['more']}, exactly 7 {seen['seven']}, none {seen['none']}, below the floor {seen['floor']}")
    assert all(v > 0 for v in seen.values()), seen


# ----------------------------------------------------------------------------------------- 3. end to end
@pytest.fixture(scope="module")
def fam_tracks():
    fam = V.family()
    out = []
    for a in range(0, len(fam), 16):  # (every clip at the threshold its reference track was made with: 0.05 for the octave-below pair)
        out += device_track([f[3] for f in fam[a:a + 16]], thrs=[(f[4]["thr"], f[4]["floor_e"]) for f in fam[a:a + 16]])
    return out


def test_track_agrees_on_every_unambiguous_clip(fam_tracks):
    worst = dict(f0=0.0, aper=0.0, cost=0.0)
    clips = 0
    for got, (name, _, _, x, ref) in zip(fam_tracks, V.family()):
        assert got["status"] == E.F0_OK and int(got["n_voiced"][0]) == int((got["state"] != 7).sum()), name
        assert ((got["f0"] > 0) == (got["state"] != 7)).all()
        if ref["unambiguous"]:
            clips += 1
            compare_clip(got, ref, worst)
    print(f"[f0v] end to end: {clips} unambiguous clips of {len(fam_tracks)}; worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert clips >= 0.9 * len(fam_tracks)  # (the cap of tests/test_f0v_cpu.py)


PLANTED = ("above 150", "above 220", "below 150", "below 220")  # (by name: the family is computed when a test first asks for it)


def named(name):
    """(index in the family, its entry)."""
    return next((i, f) for i, f in enumerate(V.family()) if f[0] == name)


@pytest.mark.parametrize("planted", PLANTED)
def test_planted_clips_jump_plain_and_not_smoothed(planted, fam_tracks):
    """tt_f0_track and tt_f0v_track of the same clip at the same parameters (the octave-below pair at threshold 0.05, f0v_reference.planted_below)."""
    from tests.test_gpu_f0 import device_track as plain_track
    i, (name, _, is_planted, x, ref) = named(planted)
    assert is_planted
    plain = plain_track([x], thrs=[(ref["thr"], ref["floor_e"])])[0]
    pj, sj = V.octave_jumps(plain["f0"]), V.octave_jumps(fam_tracks[i]["f0"])
    print(f"[f0v] {name}: tt_f0_track {pj} jumps, tt_f0v_track {sj}")
    assert pj >= 2 and sj == 0


@torch.no_grad()
def test_shift_pitch_to_hz_smoothed_lands_where_the_reference_says():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    x = named(PLANTED[0])[1][3]
    xt = torch.from_numpy(x.copy())
    y, info = h.shift_pitch(xt, to_hz=180.0, f0_smooth=True, return_info=True)
    ref_in = V.track_smooth(x)
    med = float(np.median(ref_in["f0"][ref_in["f0"] > 0]))
    assert abs(R.cents(info["measured_hz"], med)) < 0.01 and h.f0_path_stage is not None and h.f0_stage is None
    ref_out = V.track_smooth(y.numpy())
    ref_err = abs(R.cents(float(np.median(ref_out["f0"][ref_out["f0"] > 0])), 180.0))
    dev_err = abs(R.cents(h.f0(y, smooth=True).median_hz(), 180.0))
    print(f"[f0v] shift_pitch(to_hz=180, f0_smooth=True) on a planted clip: lands within {dev_err:.4f} cents (reference {ref_err:.4f})")
    assert dev_err <= 2.0 * ref_err
    tr = h.f0(xt, smooth=True)
    assert tr.smoothed and tr.octave_jumps() == 0 and tr.state.shape == tr.hz.shape and tr.path_cost > 0
    with pytest.raises(ValueError, match="f0_smooth= smooths the measurement of to_hz="):
        h.shift_pitch(xt, 2.0, f0_smooth=True)


# ----------------------------------------------------------------------------------------- 4. lengths
def compare_clip(got, ref, worst=None):
    """Every output of one clip against its reference track, which must be unambiguous: lag and voicing on every frame (an unvoiced row reads
    tt_f0_track's pick: compared where THAT is unambiguous), state where no dip is in doubt, f0 and aper inside their bounds, the cost inside B."""
    assert ref["unambiguous"] and got["status"] == E.F0_OK and got["lag"].shape == ref["lag"].shape
    assert ((got["state"] != 7) == ref["voiced"]).all() and int(got["n_voiced"][0]) == int(ref["voiced"].sum())
    own = ref["voiced"] | ~ref["plain"]["ambiguous"]
    assert (got["lag"][own] == ref["lag"][own]).all()
    sure = ~ref["cand_ambiguous"]
    assert (got["state"][sure] == ref["state"][sure]).all()
    shares = {}
    for key in ("f0", "aper"):
        err, b = np.abs(got[key].astype(np.float64) - ref[key])[own], ref[key + "_bound"][own]
        assert (err <= b).all(), (key, err[err > b], b[err > b])
        shares[key] = float(np.max(err[b > 0] / b[b > 0], initial=0.0))
    err = abs(float(got["cost"][0]) - ref["cost"])
    assert err <= ref["bound"], (err, ref["bound"])
    shares["cost"] = err / ref["bound"]
    if worst is not None:
        for k, v in shares.items():
            worst[k] = max(worst[k], v)


def test_every_length_alone():
    """Every border length is compared in full: the reference shows all twelve to be unambiguous."""
    x = R.harmonic(231.7, n=MAX_SAMPLES, snr_db=40.0, seed=11)
    G = stage().lib.tt_op_f0_group()
    assert G == 4
    worst = dict(f0=0.0, aper=0.0, cost=0.0)
    lengths = (1, 239, 240, 241, 719, 720, 721, G * 240 - 1, G * 240, G * 240 + 1, 500, 2 * G * 240 + 100)
    for n in lengths:
        compare_clip(device_track([x[:n]])[0], V.track_smooth(x[:n]), worst)
    print("[f0v] lengths " + ", ".join(str(n) for n in lengths) + ": all compared; worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------------------- 5. ragged batches
def test_a_ragged_batch_of_16_is_bit_identical_to_solo():
    fam = V.family()
    rng = np.random.default_rng(3)
    clips, pars, thrs, costs = [], [], [], []
    for i in range(14):
        x = fam[(5 * i) % len(fam)][3]
        clips.append(x[:int(rng.integers(1, MAX_SAMPLES + 1))] if i % 3 else x)
        lo = int(rng.integers(24, 200))
        pars.append((lo, int(rng.integers(lo, 481))))
        thrs.append((float(rng.uniform(0.05, 0.5)), float(10.0 ** rng.uniform(-6, 1))))
        costs.append(tuple(float(v) for v in rng.uniform(0.0, 0.6, size=4)))
    for at, x in ((4, np.zeros(0, np.float32)), (9, np.zeros(3001, np.float32))):  # an empty clip, digital silence
        clips.insert(at, x); pars.insert(at, PAR); thrs.insert(at, THR); costs.insert(at, V.COSTS)
    batch = device_track(clips, pars, thrs, costs)
    assert len(batch) == 16
    for i, got in enumerate(batch):
        assert same(got, device_track([clips[i]], [pars[i]], [thrs[i]], [costs[i]])[0]), i
        assert got["status"] == (E.F0_EMPTY if len(clips[i]) == 0 else E.F0_OK)
    assert untouched(batch[4]) and (batch[9]["state"] == 7).all() and (batch[9]["f0"] == 0).all() and (batch[9]["lag"] == 48).all()
    assert batch[9]["cost"][0] == V.viterbi([[]] * len(batch[9]["lag"]), 48)[1]
    live = [i for i in range(16) if len(clips[i])]
    res = stage().track_many([torch.from_numpy(np.array(clips[i])) for i in live], [P.Params(*pars[i], *thrs[i]) for i in live], [P.Costs(*costs[i]) for i in live])
    for i, r in zip(live, res):
        assert all(r[k].tobytes() == batch[i][k].tobytes() for k in ("lag", "f0", "aper", "state")) and r["path_cost"] == float(batch[i]["cost"][0])


# ----------------------------------------------------------------------------------------- 6. refusals
BAD = {
    "cost negative": dict(cost=(0.01, -1e-9, 0.14, 0.30)), "cost not a number": dict(cost=(math.nan, 0.35, 0.14, 0.30)),
    "cost infinite": dict(cost=(0.01, 0.35, 0.14, math.inf)), "frame slice too short": dict(slice_less=1), "over max_samples": dict(n=MAX_SAMPLES + 1),
    "lo below 24": dict(par=(23, 400)), "thr not a number": dict(thr=(math.nan, 0.01)),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_refused_clip_gets_its_status_and_nothing_else(name, fam_tracks):
    fam, bad = V.family(), BAD[name]
    x = R.harmonic(200.0, n=bad.get("n", 5000), snr_db=40.0, seed=13)
    batch = device_track([fam[2][3], x, fam[7][3]], [PAR, bad.get("par", PAR), PAR], [THR, bad.get("thr", THR), THR],
                         [V.COSTS, bad.get("cost", V.COSTS), V.COSTS], [None, R.frames(len(x)) - bad.get("slice_less", 0), None])
    assert batch[1]["status"] == E.F0_REFUSED and untouched(batch[1])
    assert same(batch[0], fam_tracks[2]) and same(batch[2], fam_tracks[7])  # the neighbours, and the handle serves on
    assert same(device_track([fam[2][3]])[0], fam_tracks[2])


def test_argument_checks_come_before_device_work():
    st, fam = stage(), V.family()
    for n in (0, 17):
        rc, out = device_track([fam[2][3]], n_clips=n)
        assert rc == -1 and b"clips (1 .. 16)" in st.lib.tt_last_error() and untouched(out[0]) and out[0]["status"] == SENT
    y = torch.zeros(64, device=DEV)
    assert st.lib.tt_f0v_track(st.h, 1, None, *[E.ptr(y)] * 13, E.stream_ptr()) == -1 and b"null argument" in st.lib.tt_last_error()
    h = E.vp()
    tab = (E.C.c_double * E.F0V_TABLE)(*P.LOG2_TABLE)
    assert st.lib.tt_f0v_create(E.F0_MAX_SAMPLES + 1, 1, tab, h) == -1 and b"max_samples" in st.lib.tt_last_error()
    assert st.lib.tt_f0v_create(100, 1, None, h) == -1 and b"null argument" in st.lib.tt_last_error() and not h
    with pytest.raises(ValueError, match="exceed the F0 path stage's capacity"):
        st.track_many([torch.zeros(MAX_SAMPLES + 1)], [P.params()], [P.smooth_params(True)])
    # the path entry: a clip of more frames than the handle's, and none
    tab1 = random_tables(np.random.default_rng(1), 3)
    got = device_path([tab1, tab1, tab1], frames=[3, 51, 0], slices=[3, 51, 3], st=st)
    assert [g["status"] for g in got] == [E.F0_OK, E.F0_REFUSED, E.F0_EMPTY] and untouched(got[1]) and untouched(got[2])
    assert same(device_track([fam[2][3]])[0], device_track([fam[2][3]])[0])


# ----------------------------------------------------------------------------------------- 7. smooth off
@torch.no_grad()
def test_smooth_none_is_tt_f0_track_bit_for_bit():
    from tests.test_gpu_f0 import device_track as plain_track
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    clips = [V.family()[3][3], named(PLANTED[0])[1][3], named(PLANTED[-1])[1][3]]
    for smooth in (None, False, [None, None, None]):
        tracks = h.f0_many([torch.from_numpy(x.copy()) for x in clips], smooth=smooth)
        for tr, x in zip(tracks, clips):
            want = plain_track([x])[0]
            assert not tr.smoothed and tr.state is None and tr.path_cost is None
            assert tr.hz.tobytes() == want["f0"].tobytes() and tr.lag.tobytes() == want["lag"].tobytes() and tr.aperiodicity.tobytes() == want["aper"].tobytes()
    assert h.f0_path_stage is None  # nothing was built
    mixed = h.f0_many([torch.from_numpy(x.copy()) for x in clips], smooth=[None, True, dict(jump_cost=0.5)])
    assert [t.smoothed for t in mixed] == [False, True, True] and mixed[0].hz.tobytes() == plain_track([clips[0]])[0]["f0"].tobytes()
