"""The streaming leveler without a GPU (include/tortoise_mi355x_lvs.h, tests/leveler_reference.py, tortoise_tts_amd/loudness.py, api.py,
api_fast.py): the reference against tests/loudness_reference.py, the gate margin of every prefix, the properties of the definition, an
emulation of the device's scheme through the GPU test's own checks, the host code under the sanitizers, the keywords and the host flow on
fakes."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import leveler_reference as V
from tests import loudness_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import loudness as loud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the reference
def test_every_prefix_of_every_stream_keeps_its_blocks_away_from_the_gates():
    """No clip and no hop is left out of any comparison, so none may sit at a gate: the margin of every prefix, bounds included."""
    least = math.inf
    for i, (x, m) in enumerate(V.streams()):
        tr = V.stream_reference(i, False)
        assert len(tr["q"]) == len(x) // V.H
        least = min(least, float(np.min(tr["margin"], initial=np.inf)))
    assert least >= R.GATE_MARGIN
    assert 0.04 < least < 0.05  # (0.0457 LU: speech 120000 seed 0)
    kinds = {int(s) for i in range(len(V.streams())) for s in V.stream_reference(i, False)["status"]}
    assert kinds == {R.OK, R.SHORT, R.SILENT}


def test_prefix_loudness_is_the_whole_clip_reference_of_the_prefix():
    for i in (8, 12, 14, 18):
        x, _ = V.streams()[i]
        tr = V.stream_reference(i, False)
        for h in sorted({3, 4, len(tr["L"]) // 2, len(tr["L"]) - 1}):
            m = R.measure(x[:(h + 1) * V.H])
            assert m["status"] == tr["status"][h] and (m["blocks_abs"], m["blocks_rel"]) == (tr["blocks_abs"][h], tr["blocks_rel"][h])
            if m["status"] == R.OK:
                assert abs(m["lufs"] - tr["L"][h]) <= 1e-9  # (the prefix is filtered on its own: the same values to the reference's rounding)
            else:
                assert tr["L"][h] == -math.inf
    assert (V.stream_reference(1, False)["status"] == R.SHORT).all() and len(V.stream_reference(0, False)["q"]) == 0


def test_fixed_gain_with_the_limiter_is_the_whole_clip_limiter():
    for i, (x, T, c, m) in enumerate(R.family_reference()):
        o = V.Options(V.FIXED, V.LOOKAHEAD, 1.7, T, c)
        a, b = V.level(x, o, m), R.limiter(x, np.float32(1.7), c)
        assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["free"], b["free"]) and np.allclose(a["bound"], b["bound"], rtol=1e-6, atol=0)
        assert (a["g"] == float(np.float32(1.7))).all() and (a["gb"] == 0).all()  # a gain that does not move is gain0 exactly
        assert (np.abs(a["y"]) <= c + a["bound"]).all()


def test_the_ceiling_holds_and_a_held_gain_is_exact():
    for i, (x, m) in enumerate(V.streams()):
        for fx in (False, True):
            o, ref = V.stream_settings(i)[int(fx)].f32(), V.stream_reference(i, fx)
            if o.limit == V.LOOKAHEAD:
                assert (np.abs(ref["y"]) <= o.ceiling + ref["bound"]).all()
            same = ref["gl"][:-1] == ref["gl"][1:]
            idx = np.arange(len(x)) // V.H
            assert (ref["g"][same[idx]] == ref["gl"][idx][same[idx]]).all()
            if len(ref["G"]):  # SHORT and SILENT hold the gain; the slew limits hold
                d = np.diff(np.concatenate([[ref["G0"]], ref["G"]]))
                assert (d <= 0.1 * o.rise + 1e-12).all() and (d >= -0.1 * o.fall - 1e-12).all()
                assert (d[ref["status"] != R.OK] == 0).all()
                assert (ref["G"] <= o.boost + 1e-12).all() or o.steer == V.FIXED
    sw = V.stream_reference(15, False)  # the 20 - 35 LU swing: both slew limits are reached
    d = np.diff(sw["G"])
    o = V.stream_settings(15)[0]
    assert np.isclose(d.max(), 0.1 * o.rise) and np.isclose(d.min(), -0.1 * o.fall)
    x, m = V.streams()[15]  # and with a narrow range both clamps
    tr = V.hops_trace(x, m)
    assert V.steer(tr, V.Options(V.ADAPT, V.NONE, 1.0, -10.0, 1.0, boost=3.0, cut=2.0, rise=30.0, fall=30.0))["G"].max() == 3.0
    assert V.steer(tr, V.Options(V.ADAPT, V.NONE, 1.0, -30.0, 1.0, boost=3.0, cut=2.0, rise=30.0, fall=30.0))["G"].min() == -2.0


def stationary(seconds=24, seed=5):
    x = (R.voiced(seconds * R.FS, seed) * 0.5).astype(np.float32)
    x.setflags(write=False)
    return x


def test_a_stationary_stream_reads_the_target_over_its_last_ten_seconds():
    """out = g x: were the gain constant at G over the tail, the tail would read L_tail(x) + G exactly (the gates are relative).  The gain
    moves inside [min G_h, max G_h] over the hops whose ramps touch the tail, so the reading lies within
    tol = max_h |L_tail(x) + G_h - T| of the target, computed from the reference's own G_h sequence (0.71 LU here, the reading is 0.55 LU off - the prefix is 0.5 LU louder than its own last ten seconds)."""
    x = stationary()
    T = -23.0
    o = V.Options(V.ADAPT, V.NONE, 1.0, T, 1.0)
    ref = V.level(x, o)
    tail = 10 * R.FS
    h0 = (len(x) - tail) // V.H
    Gs = np.concatenate([[ref["G0"]], ref["G"]])[h0 - 1:]  # gl_(h'-2) .. of the tail's hops (index h' - 2 + 1)
    L_in = R.measure(x[-tail:])["lufs"]
    tol = float(np.max(np.abs(L_in + Gs - T))) + 1e-6
    out = R.measure(ref["y"][-tail:].astype(np.float32))["lufs"]
    print(f"stationary {len(x) / R.FS:.0f} s: input tail {L_in:.3f} LUFS, gain {Gs.min():.3f} .. {Gs.max():.3f} dB, output tail {out:.3f} LUFS, tolerance {tol:.3f} LU")
    assert abs(out - T) <= tol and tol < 1.0  # (a tolerance of a whole LU or more would say nothing)


def test_the_emulation_of_the_device_passes_the_gpu_test_s_checks():
    worst = {}
    for i, (x, m) in enumerate(V.streams()):
        for fx in (0, 1):
            o = V.stream_settings(i)[fx]
            em = V.emulate(x, o)
            for k, v in V.verify(em, V.stream_reference(i, bool(fx)), x, o).items():
                worst[k] = max(worst.get(k, 0.0), v)
            ref = V.stream_reference(i, bool(fx))
            if o.limit == V.LOOKAHEAD:  # the readings' checks
                assert em["limited"] <= int((~ref["free"]).sum())
    assert 0 < max(worst.values()) <= 1.0
    # a broken device is caught: a gain one f32 ulp up at every hop, a sample off by its bound and a bit
    x, o = V.streams()[15][0], V.stream_settings(15)[0]
    ref, em = V.stream_reference(15, False), V.emulate(V.streams()[15][0], V.stream_settings(15)[0])
    bad = dict(em, G=em["G"] + 1e-9)
    with pytest.raises(AssertionError):
        V.verify(bad, ref, x, o)
    k = int(np.argmax(np.abs(ref["y"])))
    y = em["y"].copy()
    y[k] = np.float32(ref["y"][k] + 1.5 * ref["bound"][k] + 1e-7)
    with pytest.raises(AssertionError):
        V.verify(dict(em, y=y), ref, x, o)


def test_chunkings_cover_what_the_issue_lists():
    for n in (1, 700, 19201, 120000):
        ch = V.chunkings(n)
        assert all(sum(c for c, _ in v) == n and v[-1][1] and not any(f for _, f in v[:-1]) for v in ch.values())
        assert {"whole", "random", "empty", "big"} <= set(ch) and ("ones" in ch) == (n <= 700)
        assert ch["empty"][-1] == (0, True) and any(c == 0 for c, _ in ch["empty"][:-1])
    ch = V.chunkings(19201)
    assert {f"by{s}" for s in (149, 150, 151, 2399, 2400, 2401, 247, 248, 249)} <= set(ch) and max(c for c, _ in ch["big"]) > V.HIST
    assert V.ready(0, 248, V.LOOKAHEAD, False) == 0 and V.ready(0, 249, V.LOOKAHEAD, False) == 1 and V.ready(300, 0, V.LOOKAHEAD, True) == 248


# ------------------------------------------------------------------------------------------------- the host code under the sanitizers
def test_host_check_builds_and_passes_under_the_sanitizers(tmp_path):
    """csrc/checks/lvs_host_check.cpp: a stand-alone program (its own main) over loudness_stream_host.h, compiled with ASan + UBSan and run
    on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    src = os.path.join(ROOT, "tortoise_tts_amd", "csrc", "checks", "lvs_host_check.cpp")
    exe = str(tmp_path / "lvs_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lvs_host_check: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------- the header and the library
def test_header_constants_equal_engine_constants():
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_lvs.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert (val("TT_LVS_MAX_STREAMS"), val("TT_LVS_DELAY"), val("TT_LVS_HIST"), val("TT_LVS_TILE")) == (E.LVS_MAX_STREAMS, E.LVS_DELAY, E.LVS_HIST, E.LVS_TILE)
    assert (val("TT_LVS_DEFAULT_HOPS"), val("TT_LVS_MAX_HOPS")) == (E.LVS_DEFAULT_HOPS, E.LVS_MAX_HOPS) and E.LVS_DEFAULT_HOPS * E.LOUD_HOP >= 3600 * 24000
    assert (val("TT_LVS_ADAPT"), val("TT_LVS_FIXED"), val("TT_LVS_NONE"), val("TT_LVS_LOOKAHEAD")) == (E.LVS_ADAPT, E.LVS_FIXED, E.LVS_NONE, E.LVS_LOOKAHEAD)
    assert (V.DELAY, V.HIST, V.TILE, V.ADAPT, V.FIXED, V.NONE, V.LOOKAHEAD) == (E.LVS_DELAY, E.LVS_HIST, E.LVS_TILE, E.LVS_ADAPT, E.LVS_FIXED, E.LVS_NONE, E.LVS_LOOKAHEAD)
    assert E.LVS_DELAY == 2 * E.LOUD_LOOKAHEAD + 8 and "tt_lvs_abi_version" in src and E.LVS_ABI_VERSION == 1
    from tortoise_tts_amd import build
    assert "loudness_stream.hip" in build.SOURCES and any(h.endswith("tortoise_mi355x_lvs.h") for h in build._headers())
    steps = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "loudness_steps.h")).read()
    for name in ("loud_segment", "loud_carry_step", "loud_gates", "loud_peak_at", "loud_ratio", "loud_slide", "loud_smooth", "loud_gain_of_db"):
        for f in ("loudness.hip", "loudness_stream.hip"):  # both forms are built from the steps
            assert name in open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", f)).read() and name in steps, (name, f)


@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="the engine library is not built")
def test_the_library_s_host_functions_equal_the_mirrors():
    lib = E.load_library()
    assert lib.tt_lvs_abi_version() == E.LVS_ABI_VERSION and lib.tt_loud_abi_version() == 1 and lib.tt_abi_version() == 6  # the other headers are untouched
    for limit in (E.LVS_NONE, E.LVS_LOOKAHEAD):
        for before in (0, 1, 247, 248, 249, 5000):
            for c in (0, 1, 247, 248, 249, 2400, 61440):
                for flush in (0, 1):
                    assert lib.tt_lvs_ready(before, c, limit, flush) == loud.stream_ready(before, c, limit, bool(flush)) == V.ready(before, c, limit, flush)
    assert lib.tt_lvs_ready(-1, 5, 0, 0) == -1 and lib.tt_lvs_ready(0, -1, 1, 0) == -1 and lib.tt_lvs_ready(0, 5, 2, 0) == -1
    assert lib.tt_lvs_ready(E.LVS_MAX_HOPS * E.LOUD_HOP - 5, 6, 1, 0) == -1


# ------------------------------------------------------------------------------------------------- the keywords
def test_stream_options():
    for kw in ({}, {"stream_loudness": None}, {"stream_gain": None, "stream_true_peak": None, "stream_limit": None, "stream_level": None}):
        assert loud.stream_options(kw) is None and kw == {}
    kw = {"stream_loudness": -23, "top_k": 3}
    s = loud.stream_options(kw)
    assert kw == {"top_k": 3} and (s.steer, s.limit, s.gain0, s.target) == (E.LVS_ADAPT, E.LVS_LOOKAHEAD, 1.0, -23.0)
    assert s.ceiling == loud.linear(-1.0) and (s.boost, s.cut, s.rise, s.fall) == (12.0, 24.0, 3.0, 12.0)
    s = loud.stream_options({"stream_gain": -6})
    assert (s.steer, s.limit) == (E.LVS_FIXED, E.LVS_NONE) and s.gain0 == loud.linear(-6)
    s = loud.stream_options({"stream_gain": 3, "stream_true_peak": -6})
    assert (s.steer, s.limit) == (E.LVS_FIXED, E.LVS_LOOKAHEAD) and s.ceiling == loud.linear(-6)
    assert loud.stream_options({"stream_loudness": -16, "stream_limit": "none"}).limit == E.LVS_NONE
    s = loud.stream_options({"stream_loudness": -16, "stream_level": dict(assume=-30, boost=6, rise=1)})
    assert s.gain0 == loud.linear(6.0) and (s.boost, s.cut, s.rise, s.fall) == (6.0, 24.0, 1.0, 12.0)  # T - assume = 14, clamped at boost
    assert loud.stream_options({"stream_loudness": -30, "stream_level": dict(assume=-20)}).gain0 == loud.linear(-10.0)
    for bad, what in (({"stream_loudness": -4}, "stream_loudness"), ({"stream_loudness": float("nan")}, "stream_loudness"),
                      ({"stream_loudness": -23, "stream_gain": 0}, "exactly one"), ({"stream_true_peak": -1}, "belong to"),
                      ({"stream_limit": "none"}, "belong to"), ({"stream_level": {}}, "belong to"), ({"stream_gain": 61}, "stream_gain"),
                      ({"stream_gain": float("inf")}, "stream_gain"), ({"stream_loudness": -23, "stream_true_peak": 0.5}, "stream_true_peak"),
                      ({"stream_loudness": -23, "stream_limit": "scale"}, "stream_limit"), ({"stream_loudness": -23, "stream_limit": "none", "stream_true_peak": -1}, "needs the limiter"),
                      ({"stream_loudness": -23, "stream_level": dict(rise=-1)}, "rise"), ({"stream_loudness": -23, "stream_level": dict(fall=float("nan"))}, "fall"),
                      ({"stream_loudness": -23, "stream_level": dict(attack=1)}, "stream_level"), ({"stream_loudness": -23, "stream_level": 3}, "stream_level"),
                      ({"stream_loudness": -23, "stream_level": dict(assume=0)}, "assume"), ({"stream_gain": 0, "stream_level": dict(assume=-20)}, "assume"),
                      ({"stream_loudness": -23, "stream_level": dict(cut=-2)}, "cut")):
        with pytest.raises(ValueError, match=what):
            loud.stream_options(dict(bad))
    with pytest.raises(ValueError, match="loudness is not available for streamed audio"):
        loud.refuse_streaming({"loudness": -23}, "tts_stream")
    assert loud.stream_ready(0, 1000, E.LVS_LOOKAHEAD, False) == 752 and loud.stream_latency(E.LVS_LOOKAHEAD) == 248 and loud.stream_latency(E.LVS_NONE) == 0


# ------------------------------------------------------------------------------------------------- host flow on fakes
def _instances(monkeypatch):
    from tests.test_tsstream_cpu import _instances as base
    api_fast, make = base(monkeypatch)
    V.FakeStreamLevelStage.made = []
    monkeypatch.setattr(api_fast.stages, "StreamLevelStage", V.FakeStreamLevelStage)
    return api_fast, make


from tests.test_tsstream_cpu import TEXTS, _whole  # noqa: E402
from tests import rsstream_reference as RS  # noqa: E402
from tests import tsstream_reference as S  # noqa: E402
from tortoise_tts_amd import resample as rs  # noqa: E402
from tortoise_tts_amd import stretch as tsm  # noqa: E402


def _chain(pieces, level, rate=None, pitch=None, sample_rate=None):
    """The fakes' whole-clip chain in the documented order: stretch, pitch, LEVEL, sample rate."""
    x = _whole(pieces, rate, pitch, None)
    x = V.whole_fake(x, level)
    return RS.whole_hold(x, *rs.ratio(24000, sample_rate)) if sample_rate is not None else x


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_tts_stream_at_a_level_keeps_the_pieces(monkeypatch, stop):
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    for t, s, m, c in TEXTS:
        kw = dict(max_mel_tokens=m, use_deterministic_seed=s, stream_chunk_size=c, overlap_wav_len=128)
        plain = [p.clone() for p in one.tts_stream(t, **kw)]
        again = list(one.tts_stream(t, stream_loudness=None, stream_gain=None, stream_level=None, **kw))
        assert len(again) == len(plain) and all(torch.equal(a, b) for a, b in zip(again, plain))
        if t is TEXTS[0][0]:
            assert one._level_stage is None and not V.FakeStreamLevelStage.made  # nothing was built
        for opts in (dict(stream_loudness=-23), dict(stream_gain=-6), dict(stream_gain=4, stream_true_peak=-3),
                     dict(stream_loudness=-16, stream_speaking_rate=0.8, stream_pitch=-2, stream_sample_rate=16000)):
            got = list(one.tts_stream(t, **opts, **kw))
            lv = loud.stream_options({k: v for k, v in opts.items() if k in loud.STREAM_KEYS})
            want = _chain(plain, lv, opts.get("stream_speaking_rate"), opts.get("stream_pitch"), opts.get("stream_sample_rate"))
            assert len(got) == len(plain) and torch.cat(got).numpy().tobytes() == want.tobytes(), opts
            st = one._level_stage
            assert st.max_streams == 1 and not st.slots and len(V.FakeStreamLevelStage.made) == 1  # one stage, slot freed
            assert [f for call in st.calls[-len(plain):] for _, _, f in call] == [False] * (len(plain) - 1) + [True]
            if "stream_pitch" in opts:  # the order: the leveler takes what the pitch resampler emitted, the rate resampler what the leveler did
                taken = [n for call in st.calls[-len(plain):] for _, n, _ in call]
                assert sum(taken) == len(_whole(plain, opts["stream_speaking_rate"], opts["stream_pitch"], None))
                assert sum(n for call in one._stream_stage.calls[-len(plain):] for _, n, _ in call) == sum(taken)
    g = one.tts_stream(TEXTS[0][0], stream_loudness=-20, max_mel_tokens=70, use_deterministic_seed=4, stream_chunk_size=5, overlap_wav_len=128)
    next(g)
    assert len(one._level_stage.slots) == 1
    g.close()
    assert not one._level_stage.slots


@torch.no_grad()
def test_validation_comes_before_a_slot_is_taken_and_loudness_stays_refused(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    one, many = make(1), make(2)
    t = TEXTS[0][0]
    for bad, what in ((dict(stream_loudness=-2), "stream_loudness"), (dict(stream_loudness=-23, stream_gain=1), "exactly one"),
                      (dict(stream_true_peak=-1), "belong to"), (dict(stream_gain=0, stream_limit="soft"), "stream_limit"),
                      (dict(stream_loudness=-23, stream_level=dict(rise=-3)), "rise")):
        with pytest.raises(ValueError, match=what):
            next(one.tts_stream(t, **bad))
        with pytest.raises(ValueError, match=what):
            many.open_stream(t, **bad)
        with pytest.raises(ValueError, match=what):
            next(many.tts_stream_many([t, t], **bad))
    with pytest.raises(ValueError, match="3 stream_loudness values for 2 texts"):
        next(many.tts_stream_many([t, t], stream_loudness=[-23, None, -16]))
    for fn in (lambda **kw: next(one.tts_stream(t, **kw)), lambda **kw: many.open_stream(t, **kw), lambda **kw: next(many.tts_stream_many([t], **kw))):
        for kw in (dict(loudness=-23.0), dict(loudness=-23.0, stream_loudness=-23), dict(true_peak=-1.0, stream_gain=0), dict(limit="scale")):
            with pytest.raises(ValueError, match="loudness is not available for streamed audio"):
                fn(**kw)
    assert not many._sessions and not V.FakeStreamLevelStage.made


@pytest.mark.parametrize("stop", [False, True])
@torch.no_grad()
def test_sessions_with_their_own_levels(monkeypatch, stop):
    """Three texts on two slots, each with its own settings (one with none): pieces and flags as today, the chains concatenate to the
    whole-clip chain, and a round's due pieces share ONE push of the leveler."""
    api_fast, make = _instances(monkeypatch)
    one = make(1, stop)
    kw = dict(max_mel_tokens=66, stream_chunk_size=5, overlap_wav_len=128)
    plain = [[p.clone() for p in one.tts_stream(t, use_deterministic_seed=s, **kw)] for t, s, _, _ in TEXTS]
    many = make(2, stop)
    targets, gains, srs = [-23.0, None, None], [None, None, -4.0], [None, None, 16000]
    got = {}
    for i, wav, done in many.tts_stream_many([t for t, _, _, _ in TEXTS], use_deterministic_seed=[s for _, s, _, _ in TEXTS], stream_loudness=targets,
                                             stream_gain=gains, stream_sample_rate=srs, **kw):
        got.setdefault(i, []).append((wav.clone(), done))
    st = many._level_stage
    assert len(V.FakeStreamLevelStage.made) == 1 and st.max_streams == 2 and not st.slots and not many._sessions
    for i in range(3):
        assert [d for _, d in got[i]] == [False] * (len(plain[i]) - 1) + [True]
        if targets[i] is None and gains[i] is None:
            assert all(torch.equal(a, b) for (a, _), b in zip(got[i], plain[i]))
        else:
            lv = loud.stream_options({"stream_loudness": targets[i], "stream_gain": gains[i]})
            assert torch.cat([a for a, _ in got[i]]).numpy().tobytes() == _chain(plain[i], lv, sample_rate=srs[i]).tobytes(), i
    assert all(len({s for s, _, _ in call}) == len(call) for call in st.calls) and sum(len(call) for call in st.calls) == len(plain[0]) + len(plain[2])
    # open_stream / stream_pieces directly, three sessions with different settings on three slots
    three = make(3, stop)
    opts = [dict(stream_loudness=-16), dict(stream_gain=2, stream_true_peak=-2), dict(stream_loudness=-30, stream_limit="none")]
    sids = [three.open_stream(t, use_deterministic_seed=s, **o, **kw) for (t, s, _, _), o in zip(TEXTS, opts)]
    out = {sid: [] for sid in sids}
    for sid, wav, done in three.stream_pieces():
        out[sid].append(wav.clone())
    for sid, o, p in zip(sids, opts, plain):
        assert torch.cat(out[sid]).numpy().tobytes() == _chain(p, loud.stream_options(dict(o))).tobytes()
    assert any(len(call) > 1 for call in three._level_stage.calls) and not three._level_stage.slots


@torch.no_grad()
def test_open_leveler_and_level_on_fakes(monkeypatch):
    from tortoise_tts_amd import api
    V.FakeStreamLevelStage.made = []
    monkeypatch.setattr(api.stages, "StreamLevelStage", V.FakeStreamLevelStage)

    class Host(api._Common):
        device = torch.device("cpu")

    h = Host()
    assert h.stream_leveller is None
    x = torch.from_numpy(np.array(V.streams()[8][0]))
    lv = loud.stream_settings(loudness=-20, true_peak=-2)
    with h.open_leveler(loudness=-20, true_peak=-2) as r:
        assert r.latency_seconds == 248 / 24000 and h.stream_leveller.max_streams == 16 and r.settings == lv
        got = [r.push(x[:30]), r.push(x[30:30]), r.push(x[30:1900]), r.push(x[1900:]), r.finish()]
        assert got[0].shape == (0,) and got[2].shape == (1900 - 248,) and (r.n_in, r.n_out) == (len(x), len(x)) and r.slot is None
        assert r.reading().samples_out == len(x)
        with pytest.raises(ValueError, match="closed"):
            r.push(x[:4])
    assert torch.cat(got).numpy().tobytes() == V.whole_fake(x.numpy(), lv).tobytes() and not h.stream_leveller.slots
    with h.open_leveler(gain=-3) as r:
        assert r.latency_seconds == 0 and r.push(x[:100]).shape == (100,)
    y, info = h.level_many([x, x.reshape(1, -1)[:, :500]], gain=-3, return_info=True)
    assert y[0].shape == x.shape and y[1].shape == (1, 500) and y[0].numpy().tobytes() == V.whole_fake(x.numpy(), loud.stream_settings(gain=-3)).tobytes()
    assert [i.samples_in for i in info] == [len(x), 500] and torch.equal(h.level(x, gain=-3), y[0]) and not h.stream_leveller.slots
    for bad in (dict(), dict(loudness=-23, gain=0), dict(loudness=-1), dict(gain=0, limit="scale"), dict(loudness=-23, rise=-1), dict(gain=1, attack=3)):
        with pytest.raises(ValueError):
            h.open_leveler(**bad)
        with pytest.raises(ValueError):
            h.level(x, **bad)
    assert not h.stream_leveller.slots and len(V.FakeStreamLevelStage.made) == 1
