"""The Viterbi F0 path without a GPU: the fp64 reference (tests/f0v_reference.py) on the planted clips, the glide, the gap, noise and
silence; its recursion against a brute-force enumeration; the cap on ambiguous inputs; the host code (pitch.smooth_params, F0Track, the
refusals of the public calls on stages backed by the reference, the stage's packing, csrc/f0v_host.h under the sanitizers).

Measured with this reference.  Octave-above clips (odd harmonics at 0.14 over runs of 1, 3 and 2 frames, raised-cosine ramps of 1200
samples, 40 dB SNR): plain track 6 jumps each, smoothed 0, worst error of an inner frame 0.53 (150 Hz) / 0.27 (220 Hz) cents.
Octave-below clips (every other period at 0.7 over about a window of 960 samples, three times; measured at YIN threshold 0.05, where plain
YIN takes the double period in those frames - f0v_reference.planted_below derives why a scaling that jumps at 0.15 cannot be held by the
default costs, and the 0.5 cents that a dip of 0.06 costs): plain track 6 jumps each, smoothed 0, worst inner frame 0.68 / 0.64 cents.
Every inner frame of all four is asserted inside 2 x 0.3692 = 0.74 cents, what tests/test_f0_cpu.py asserts at 40 dB.
The cap: 2 of the family's 32 clips are ambiguous by f0v_reference's rule (62.5 Hz at 20 dB: the margin of its path is inside 2 B; 132.2 Hz
at 20 dB: the last frame's dip lies between two lags); no planted clip is.  Counting any doubt about a frame's candidate
set, 29 would be; the rule sets aside dips in doubt that no cheapest path can hold, and derives the condition."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from tests import f0_reference as R
from tests import f0v_reference as V
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import pitch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTS_40DB = 0.3692  # tests/test_f0_cpu.py WORST_CENTS[40.0], the SNR of the planted clips; asserted at twice, as there


def _named(name):
    return next(f for f in V.family() if f[0] == name)


# ----------------------------------------------------------------------------------------- the reference on known signals
@pytest.mark.parametrize("name", ["above 150", "above 220", "below 150", "below 220"])
def test_planted_clips_jump_plain_and_not_smoothed(name):
    _, f0, _, x, tr = _named(name)
    pj, sj = V.octave_jumps(tr["plain"]["f0"]), V.octave_jumps(tr["f0"])
    inner = R.inner_frames(len(x))
    worst = max(abs(R.cents(tr["f0"][f], f0)) for f in inner if tr["f0"][f] > 0)
    print(f"[f0v] {name}: plain track {pj} jumps, smoothed {sj}; worst inner frame {worst:.3f} cents; planted frames plain "
          f"{np.round(tr['plain']['f0'][V.planted_frames(name)], 1).tolist()}")
    assert pj >= 2 and sj == 0
    assert tr["voiced"][inner].all() and worst <= 2.0 * CENTS_40DB


def test_the_glide_is_followed_with_no_jump():
    _, _, _, x, tr = _named("glide")
    inner = R.inner_frames(len(x))
    worst = max(abs(R.cents(tr["f0"][f], 100.0 + 200.0 * f * R.H / R.SR)) for f in inner)
    assert tr["voiced"][inner].all() and V.octave_jumps(tr["f0"]) == 0 and worst <= 2.0 * 21.70  # (test_f0_cpu.GLIDE_CENTS)
    assert np.all(np.diff(tr["f0"][inner]) > 0)


def test_noise_and_silence_have_no_voiced_frame():
    for name in ("noise", "silence"):
        tr = _named(name)[4]
        assert not tr["voiced"].any() and (tr["state"] == 7).all() and (tr["f0"] == 0).all() and (tr["lag"] == tr["plain"]["lag"]).all()
    sil = _named("silence")[4]
    assert all(c == [] for c in sil["cands"]) and sil["cost"] == V.viterbi([[]] * 50, 48)[1] and sil["unambiguous"]


def test_the_gap_comes_back_unvoiced_with_both_edges_voiced():
    tr = _named("gap")[4]
    v = tr["voiced"]
    silent = [f for f in range(50) if f * R.H - R.LEAD >= 4800 and f * R.H - R.LEAD + R.W <= 7200]  # the windows inside the gap
    assert silent and not v[silent].any() and v[5:15].all() and v[38:45].all() and V.octave_jumps(tr["f0"]) == 0
    edges = np.nonzero(np.diff(v.astype(int)))[0]
    assert len(edges) >= 2


def test_viterbi_equals_brute_force_on_200_tiny_problems():
    rng = np.random.default_rng(7)
    exact = 0
    for i in range(200):
        F = int(rng.integers(1, 6))
        grid = i % 2 == 0  # every quantity exact (lags powers of two, dp and costs on a grid of 1 / 8): ties between unlike paths
        cands = []
        for _ in range(F):
            k = int(rng.integers(0, 4))
            lags = np.sort(rng.choice([32, 64, 128, 256] if grid else np.arange(24, 481), size=k, replace=False))
            cands.append([(int(l), float(rng.integers(0, 4)) / 8.0 if grid else float(rng.uniform(0, 1))) for l in lags])
        costs = tuple(float(v) / 8.0 for v in rng.integers(0, 4, size=4)) if grid else tuple(float(v) for v in rng.uniform(0, 0.5, size=4))
        state, cost = V.viterbi(cands, 32, costs)
        want, paths = V.brute_force(cands, 32, costs)
        assert cost == want and tuple(state.tolist()) in paths, i
        if grid:  # sums are exact: the backtrace's rule is "the smallest state, read from the end"
            exact += len(paths) > 1
            assert tuple(state.tolist()) == min(paths, key=lambda p: p[::-1]), i
    assert exact >= 10  # the ties were there (16 of the 100 exact problems have more than one cheapest path)


def test_the_cap_on_ambiguous_clips():
    """At most 10 % of the family's clips ambiguous, no planted clip among them: a condition on the inputs."""
    fam = V.family()
    amb = [name for name, _, _, _, tr in fam if not tr["unambiguous"]]
    print(f"[f0v] ambiguous clips: {len(amb)} of {len(fam)}: {amb}")
    assert len(fam) == 32 and len(amb) <= 0.10 * len(fam)
    assert not [name for name, _, planted, _, tr in fam if planted and not tr["unambiguous"]]


def test_the_bound_and_the_margin_are_what_the_reference_says():
    _, _, _, x, tr = _named("above 150")
    lag_t, dp_t = V.tables(tr["cands"])
    assert tr["bound"] >= R.E_DP * dp_t.max(axis=1).sum() and tr["bound"] < 0.01 and tr["margin"] > 2 * tr["bound"]
    state, cost, through = V.viterbi_tables(lag_t, dp_t, 48, margin=True)
    on = through[np.arange(len(state)), state]
    assert np.allclose(on, cost, rtol=0, atol=1e-12) and (through[np.isfinite(through)] >= cost - 1e-12).all()


# ----------------------------------------------------------------------------------------- host code
def test_smooth_params_and_the_keyword():
    assert P.smooth_params(None) is None and P.smooth_params(False) is None
    assert P.smooth_params(True) == P.Costs(0.01, 0.35, 0.14, 0.30) == P.smooth_params({})
    assert P.smooth_params(dict(jump_cost=0.5, unvoiced_cost=0)) == P.Costs(0.01, 0.5, 0.14, 0.0)
    assert P.smooth_params(P.Costs(1, 2, 3, 4)) == P.Costs(1.0, 2.0, 3.0, 4.0)
    for bad, what in ((dict(jump=1), "unknown key 'jump'"), (dict(jump_cost=-0.1), "jump_cost=-0.1"), (dict(octave_cost=float("nan")), "octave_cost=nan"),
                      (dict(voicing_cost=float("inf")), "voicing_cost=inf"), (dict(unvoiced_cost="1"), "unvoiced_cost='1'"), ("yes", "smooth='yes'"), (1, "smooth=1")):
        with pytest.raises(ValueError, match=re.escape(what)):
            P.smooth_params(bad)
    kw = dict(f0_smooth=True, other=1)
    assert P.smooth_option(kw, 180.0) == P.smooth_params(True) and kw == dict(other=1) and P.smooth_option({}, None) is None
    assert P.smooth_option(dict(f0_smooth=None), None) is None and P.smooth_option(dict(f0_smooth=False), None) is None
    with pytest.raises(ValueError, match="tts: f0_smooth= smooths the measurement of pitch_hz="):
        P.smooth_option(dict(f0_smooth=True), None)
    with pytest.raises(ValueError, match="shift_pitch: f0_smooth= smooths the measurement of to_hz="):
        P.smooth_option(dict(f0_smooth=dict(jump_cost=1)), None, "shift_pitch")
    for f, who, what in ((P.refuse_streaming, "tts_stream", "for streamed audio"), (P.refuse_long_form, "read_long_form", "for a reading"),
                         (P.refuse_sharded, "tts", "on a sharded job")):
        with pytest.raises(ValueError, match=f"{who}: f0_smooth is not available {what}"):
            f(dict(f0_smooth=True), who)
    assert len(P.LOG2_TABLE) == E.F0V_TABLE == 481 and P.LOG2_TABLE[1] == 0.0 and P.LOG2_TABLE[256] == 8.0 and (np.diff(P.LOG2_TABLE[1:]) > 0).all()
    text = open(os.path.join(ROOT, "include", "tortoise_mi355x_f0v.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (define("TT_F0V_STATES"), define("TT_F0V_UNVOICED"), define("TT_F0V_TABLE")) == (E.F0V_STATES, E.F0V_UNVOICED, E.F0V_TABLE)
    lib = E.load_library()
    assert lib.tt_f0v_abi_version() == E.F0V_ABI_VERSION == 1
    h = E.vp()
    tab = (E.C.c_double * E.F0V_TABLE)(*P.LOG2_TABLE)
    assert lib.tt_f0v_create(0, 1, tab, h) == -1 and b"max_samples 0 (1 .. 8388608)" in lib.tt_last_error() and not h
    assert lib.tt_f0v_create(100, 1, None, h) == -1 and b"null argument" in lib.tt_last_error()
    tab[7] = float("nan")
    assert lib.tt_f0v_create(100, 1, tab, h) == -1 and b"log2 table" in lib.tt_last_error() and not h


def test_f0track_smoothed_and_octave_jumps():
    hz = np.array([0, 150, 151, 300, 152, 0, 150, 75, 75, 150, 225], np.float32)
    tr = P.F0Track(hz, np.zeros(11), np.zeros(11))
    assert not tr.smoothed and tr.state is None and tr.path_cost is None
    assert tr.octave_jumps() == 5 and tr.octave_jumps(7.1) == 4 and tr.octave_jumps(12.5) == 0  # (a fifth, 150 -> 225, is 7.02 semitones)
    sm = P.F0Track(hz, np.zeros(11), np.zeros(11), state=np.zeros(11), path_cost=1.5)
    assert sm.smoothed and sm.state.dtype == np.int32 and sm.path_cost == 1.5
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError, match="min_semitones"):
            tr.octave_jumps(bad)
    with pytest.raises(ValueError, match="state"):
        P.F0Track(hz, np.zeros(11), np.zeros(11), state=np.zeros(3))
    got = P.track_of(dict(f0=hz, aper=np.zeros(11), lag=np.zeros(11), state=np.full(11, 7), path_cost=2.0, n_voiced=0), 2640)
    assert got.smoothed and got.path_cost == 2.0 and got.samples == 2640


class ReferencePathStage:
    """stages.F0ViterbiStage backed by tests/f0v_reference.py (the pattern of tests/f0_fake.py)."""
    made, calls = [], []

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferencePathStage.made.append(max_samples)

    def track_many(self, clips, params, costs):
        ReferencePathStage.calls.append(len(clips))
        out = []
        for x, p, k in zip(clips, params, costs):
            tr = V.track_smooth(x.cpu().numpy(), p.lag_lo, p.lag_hi, p.thr, p.floor_e, tuple(k))
            out.append(dict(lag=tr["lag"].astype(np.int32), f0=tr["f0"].astype(np.float32), aper=tr["aper"].astype(np.float32),
                            state=tr["state"], n_voiced=int(tr["voiced"].sum()), path_cost=tr["cost"]))
        return out

    def close(self):
        pass


def _host(monkeypatch):
    from tests.test_f0_cpu import _host as plain_host
    t, kw, F, St, Rs = plain_host(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "F0ViterbiStage", ReferencePathStage, raising=False)
    ReferencePathStage.made, ReferencePathStage.calls = [], []
    return t, kw, F


@torch.no_grad()
def test_smooth_on_f0_and_shift_pitch(monkeypatch):
    t, _, F = _host(monkeypatch)
    x = torch.from_numpy(_named("above 150")[3].copy())
    plain, sm = t.f0(x), t.f0(x, smooth=True)
    assert not plain.smoothed and plain.octave_jumps() >= 2 and sm.smoothed and sm.octave_jumps() == 0 and sm.path_cost > 0 and sm.state.shape == (50,)
    assert F.calls == [1] and ReferencePathStage.calls == [1] and ReferencePathStage.made == [30 * 24000]
    assert t.f0(x, smooth=None).hz.tobytes() == plain.hz.tobytes() == t.f0(x, smooth=False).hz.tobytes()  # off: today's call, today's bits
    F.calls, ReferencePathStage.calls = [], []
    both = t.f0_many([x, x[:6000], x], smooth=[None, True, dict(jump_cost=0.2)])
    assert [b.smoothed for b in both] == [False, True, True] and F.calls == [1] and ReferencePathStage.calls == [2]
    four = t.f0_many([x[:3000]] * 4, smooth=P.Costs(0.01, 0.2, 0.14, 0.30))  # a Costs is ONE setting, also for four clips
    assert [b.smoothed for b in four] == [True] * 4 and ReferencePathStage.calls[-1] == 4
    F.calls, ReferencePathStage.calls = [1], [2]
    with pytest.raises(ValueError, match="3 clips with 2 smooth settings"):
        t.f0_many([x, x, x], smooth=[True, None])
    with pytest.raises(ValueError, match="unknown key 'jump'"):
        t.f0(x, smooth=dict(jump=1))
    # to_hz with f0_smooth: the ONE measurement runs smoothed; without to_hz it is refused before anything is measured
    F.calls, ReferencePathStage.calls = [], []
    y, info = t.shift_pitch(x, to_hz=180.0, f0_smooth=True, return_info=True)
    assert F.calls == [] and ReferencePathStage.calls == [1] and info["measured_hz"] == sm.median_hz()
    assert torch.equal(y, t.shift_pitch(x, info["semitones"]))
    assert torch.equal(t.shift_pitch(x, to_hz=180.0, f0_smooth=None), t.shift_pitch(x, to_hz=180.0))
    ReferencePathStage.calls = []
    for kw in (dict(semitones=2.0, f0_smooth=True), dict(pitch_map=[(0, 1)], f0_smooth=dict(jump_cost=1.0))):
        with pytest.raises(ValueError, match="shift_pitch: f0_smooth= smooths the measurement of to_hz="):
            t.shift_pitch(x, **kw)
    with pytest.raises(ValueError, match="jump_cost=-1"):
        t.shift_pitch(x, to_hz=180.0, f0_smooth=dict(jump_cost=-1))
    assert ReferencePathStage.calls == []


@torch.no_grad()
def test_f0_smooth_on_tts(monkeypatch):
    from tests.test_api_flow_cpu import HELLO_THERE
    t, kw, F = _host(monkeypatch)
    plain = t.tts(HELLO_THERE, **kw)
    assert torch.equal(t.tts(HELLO_THERE, f0_smooth=None, **kw), plain) and ReferencePathStage.made == [] and t.f0_path_stage is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the fake stages' clip may have no median)
        got = t.tts(HELLO_THERE, pitch_hz=180.0, f0_smooth=True, **kw)
        want = t.shift_pitch_many([plain], to_hz=180.0, f0_smooth=True)[0]
        assert torch.equal(got, want) and ReferencePathStage.calls == [1, 1] and F.calls == []
        many = t.tts_many([HELLO_THERE, HELLO_THERE[:6]], pitch_hz=200.0, f0_smooth=dict(octave_cost=0.02), **kw)
        assert len(many) == 2 and ReferencePathStage.calls[-1] == 2
        t.tts_with_preset(HELLO_THERE, preset="ultra_fast", pitch_hz=180.0, f0_smooth=True, **kw)
    assert torch.equal(t.tts(HELLO_THERE, **kw), plain)  # without the keywords, today's bits
    for call in (lambda **k: t.tts(HELLO_THERE, **k, **kw), lambda **k: t.tts_many([HELLO_THERE], **k, **kw),
                 lambda **k: t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **k, **kw)):
        with pytest.raises(ValueError, match="f0_smooth= smooths the measurement of pitch_hz="):
            call(f0_smooth=True)
        with pytest.raises(ValueError, match="unknown key 'x'"):
            call(pitch_hz=180.0, f0_smooth=dict(x=1))


def test_refusals_on_readings():
    from tortoise_tts_amd import longform
    with pytest.raises(ValueError, match="read_long_form: f0_smooth is not available for a reading"):
        longform.read_long_form(None, "hello there", f0_smooth=True)


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.F0ViterbiStage)  # (no handle: the checks come before any device work)
    st.h, st.lib = None, E.load_library()
    st.max_samples, st.max_clips = 1000, 16
    k = P.smooth_params(True)
    with pytest.raises(ValueError, match="1001 samples exceed the F0 path stage's capacity"):
        st.track_many([torch.zeros(1001)], [P.params()], [k])
    with pytest.raises(ValueError, match="at least one sample"):
        st.track_many([torch.zeros(0)], [P.params()], [k])
    with pytest.raises(ValueError, match="2 clips with 1 parameter sets and 2 sets of costs"):
        st.track_many([torch.zeros(10), torch.zeros(10)], [P.params()], [k, k])


def test_f0_path_packing():
    """_Tables / _Results of stages.F0ViterbiStage._group, pinned as tests/test_stage_packing_cpu.py pins the others."""
    import ctypes as C
    from tests import test_stage_packing_cpu as K
    from tortoise_tts_amd import stages
    real, clips = K._real(), K._clips()
    params = [P.Params(24 + i, 400 + i, 0.1 + i, 50.0 + i) for i in range(4)]
    costs = [P.Costs(0.01 + i, 0.35 + i, 0.14 + i, 0.30 + i) for i in range(4)]
    status = [E.F0_OK] * 4

    def track(c, audio, in_off, par, thr, cost, frm_off, lag, f0, aper, state, n_voiced, path_cost, st):
        io, fo = c.read("io", in_off, c.n + 1), c.read("fo", frm_off, c.n + 1)
        c.read("par", par, 2 * c.n)
        c.read("thr", thr, 2 * c.n, C.c_double)
        c.read("cost", cost, 4 * c.n, C.c_double)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("lag", lag, fo[-1])
        c.fill("f0", f0, fo[-1], C.c_float)
        c.fill("aper", aper, fo[-1], C.c_float)
        c.fill("state", state, fo[-1])
        c.fill("n_voiced", n_voiced, c.n)
        c.fill("path_cost", path_cost, c.n, C.c_double)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    import unittest.mock as mock
    with mock.patch.object(E, "stream_ptr", lambda: 0):
        lib = K._Lib(tt_f0v_track=track)
        res = K._stage(stages.F0ViterbiStage, lib, max_samples=2000).track_many(clips, params, costs)
        assert lib.sizes() == [3, 1] and len(res) == 4
        for c, (a, b) in zip(lib.calls, K.GROUPS):
            io, fo = K._off(K.LENS[a:b]), K._off(real.tt_f0_frames(m) for m in K.LENS[a:b])
            c.tables(io=io, fo=fo, par=K._i32([[p.lag_lo, p.lag_hi] for p in params[a:b]]),
                     thr=np.asarray([[p.thr, p.floor_e] for p in params[a:b]], dtype=np.float64).reshape(-1),
                     cost=np.asarray([list(k) for k in costs[a:b]], dtype=np.float64).reshape(-1))
            c.audio(clips[a:b], io)
            c.outputs_apart()
            for i, d in enumerate(res[a:b]):
                assert sorted(d) == ["aper", "f0", "lag", "n_voiced", "path_cost", "state"]
                K._same(d["lag"], c.out["lag"][fo[i]:fo[i + 1]], np.int32)
                K._same(d["state"], c.out["state"][fo[i]:fo[i + 1]], np.int32)
                K._same(d["f0"], c.out["f0"][fo[i]:fo[i + 1]], np.float32)
                K._same(d["aper"], c.out["aper"][fo[i]:fo[i + 1]], np.float32)
                assert d["n_voiced"] == int(c.out["n_voiced"][i]) and d["path_cost"] == float(c.out["path_cost"][i])
        K._refused(lambda: K._stage(stages.F0ViterbiStage, K._Lib(tt_f0v_track=track), max_samples=2000).track_many(clips, params, costs), status,
                   E.F0_REFUSED, "f0 path: the device stage refused clips it was handed (status [0, 2, 0])")


# ----------------------------------------------------------------------------------------- the host code under the sanitizers
def test_host_check_builds_and_passes_under_the_sanitizers(tmp_path):
    """csrc/checks/f0v_host_check.cpp: a stand-alone program (its own main) over f0v_host.h, compiled with ASan + UBSan and run on the CPU -
    the status and check functions over their borders, f0v_viterbi_host against hand-worked answers."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    src = os.path.join(ROOT, "tortoise_tts_amd", "csrc", "checks", "f0v_host_check.cpp")
    exe = str(tmp_path / "f0v_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "f0v_host_check: ok" in r.stdout, r.stdout + r.stderr
