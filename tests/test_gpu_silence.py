"""The silence stage on the MI355X (csrc/silence.hip, include/tortoise_mi355x_sil.h) against the fp64 reference of
tests/silence_reference.py.  The clips are bursts at full level separated by exact zeros or by noise 60 dB down, so every decision sits far
from its threshold: the reference first shows that it has NO undecided frame for any of them, and then frame flags, regions, n_out and
segment lists must be equal, frame energies inside the derived band, and every output sample equal to the reference's - bit for bit where
copied, inside the three-operation f32 bound where cross-faded, the two-operation bound where faded.  Ragged batches are bit-identical to
solo calls, a clip that is not read gets its status and nothing else, and nothing is written outside a clip's own slices."""
import os
import re

import numpy as np
import pytest
import torch

from tests import silence_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import silence as sil
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7          # what every output holds before the call
PAD = 64           # canaries on either side of out, the regions and the segments
MAX_SAMPLES = 250000

_src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tortoise_tts_amd", "csrc", "silence.hip")).read()
CHUNK = int(re.search(r"kSilPlan = (\d+)", _src).group(1))  # frames of a scan chunk = threads of the plan workgroup actually built
TILE = int(re.search(r"kSilOut = (\d+)", _src).group(1))    # outputs of a render tile


def _family():
    fam = []
    add = lambda name, parts, **kw: fam.append((name, parts, R.params(**kw)))
    # the shortest clips: one sample, one either side of a slot, a hop and a frame; all speech, all zeros, and zeros then speech
    for n in (1, 119, 120, 121, 239, 240, 241, 479, 480, 481):
        add(f"speech_{n}", [("s", n)])
        add(f"zeros_{n}", [("z", n)])
        add(f"late_{n}", [("z", 480), ("s", n)], lead=0, pad=0)
    add("n5000", [("z", 1000), ("s", 2000), ("z", 2000)], lead=240, trail=240, pad=1)
    add("n24000", [("l", 3000), ("s", 6000), ("z", 5000), ("s", 4000), ("l", 6000)], max_pause=1200)
    for name, kw in (("lead_off", dict(lead=-1, max_pause=1200)), ("trail_off", dict(trail=-1, max_pause=1200)), ("pause_off", dict(max_pause=-1)),
                     ("all_off", dict(lead=-1, trail=-1, max_pause=-1)), ("tight", dict(lead=0, trail=0, max_pause=120, pad=0, min_sil=0))):
        add("n24000_" + name, [("l", 3000), ("s", 6000), ("z", 5000), ("s", 4000), ("l", 6000)], **kw)
    # a scan-chunk edge: CHUNK - 1, CHUNK and CHUNK + 1 frames, pauses on both sides of the edge
    for F in (CHUNK - 1, CHUNK, CHUNK + 1):
        n = R.HOP * F - 7
        parts = [("z", 24000), ("s", 48000), ("z", 36000), ("s", 24000), ("l", 60000), ("s", 30000), ("z", 20000)]
        parts.append(("s", n - sum(m for _, m in parts) - 1700))
        parts.append(("z", 1700))
        add(f"frames_{F}", parts, max_pause=12000)
    # a render-tile edge: outputs of TILE - 1, TILE, TILE + 1 and 2 TILE - 1 .. 2 TILE + 1 samples (speech to 700 -> the region ends at 720)
    for n_out in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        add(f"out_{n_out}", [("s", 700), ("z", 3000)], lead=-1, trail=n_out - 720, pad=0)
    # the three cut boundaries: the pause between the regions of this clip is 2160 samples (asserted in test_the_family_is_decided)
    for d in (-1, 0, 1):
        add(f"cut_{d:+d}", [("s", 2400), ("z", 2400), ("s", 2400)], pad=0, min_sil=0, lead=-1, trail=-1, max_pause=2160 - R.X - d)
    add("cut_least", [("s", 2400), ("z", 2400), ("s", 2400)], pad=0, min_sil=0, max_pause=R.X)  # M = X: nothing but the cross-fade remains
    add("edges_in_speech", [("s", 3000), ("z", 6000), ("s", 3000)], max_pause=1200)
    add("one_region", [("z", 3000), ("s", 3000), ("z", 3000)], trail=600, max_pause=1200)
    add("pad_merges", [("s", 2400), ("z", 2400), ("s", 2400)], pad=5, min_sil=0, max_pause=240)     # 9 frames apart, 5 + 5 >= 9: one region
    add("pad_does_not", [("s", 2400), ("z", 2400), ("s", 2400)], pad=4, min_sil=0, max_pause=240)   # one frame stays between them
    add("bridged", [("s", 2400), ("z", 2400), ("s", 2400)], pad=0, min_sil=10, max_pause=240)       # 9 < 10: bridged
    add("low_noise_gaps", [("l", 2500), ("s", 5000), ("l", 7000), ("s", 3000), ("l", 2500)], max_pause=3000)
    add("many_pauses", [p for _ in range(12) for p in (("s", 1300), ("z", 1900))], pad=1, min_sil=2, max_pause=600, lead=100, trail=50)
    add("constant", None)
    return fam


FAMILY = _family()
NAMES = [f[0] for f in FAMILY]
_refs = {}


def clip(i):
    name, parts, _ = FAMILY[i]
    return np.full(5000, 0.25, dtype=np.float32) if parts is None else R.build(parts, i)


def reference(i):
    """(x, the reference's result) of family member i, computed once."""
    if i not in _refs:
        x = clip(i)
        _refs[i] = (x, R.trim(x, FAMILY[i][2]))
    return _refs[i]


_stage = []


def stage():
    if not _stage:
        _stage.append(stages.SilenceStage(MAX_SAMPLES, max_clips=32, device=DEV))
    return _stage[0]


def _offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def device_trim(clips, find=False, caps=None, energies=True):
    """One tt_sil_trim (or tt_sil_find) call over clips = [(x f32 [n], params)] with every output pre-filled with SENT and canaries around
    out, the regions and the segments -> per clip the raw status and whatever the call wrote (SENT where it wrote nothing).  caps: per clip
    the entries of its region / segment slices where they are not tt_sil_max_regions(n)."""
    st = stage()
    n = len(clips)
    lens = [len(x) for x, _ in clips]
    caps = [R.max_regions(m) if c is None else c for m, c in zip(lens, caps or [None] * n)]
    io, ro, fo = _offsets(lens), _offsets(caps), _offsets([R.frames(m) for m in lens])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    audio = dev(np.concatenate([np.asarray(x, dtype=np.float32) for x, _ in clips] + [np.zeros(1, np.float32)]))
    io_d, ro_d, fo_d = dev(io), dev(ro), dev(fo)
    thr = dev(np.asarray([p[:2] for _, p in clips], dtype=np.float64))
    par = dev(np.asarray([p[2:4] if find else p[2:7] for _, p in clips], dtype=np.int32))
    full = lambda m, dt: torch.full((m,), SENT, dtype=dt, device=DEV)
    y = full(PAD + int(io[-1]) + PAD, torch.float32)
    reg, seg = full(2 * (PAD + int(ro[-1]) + PAD), torch.int32), full(3 * (PAD + int(ro[-1]) + PAD), torch.int32)
    en = full(PAD + int(fo[-1]) + PAD, torch.float64)
    n_out, n_reg, n_seg, status = (full(n + 1, torch.int32) for _ in range(4))
    peak = full(n + 1, torch.float64)
    if find:
        E.check(st.lib.tt_sil_find(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(thr), E.ptr(par), E.ptr(ro_d), E.ptr(fo_d) if energies else None,
                                   E.ptr(n_reg), reg.data_ptr() + 8 * PAD, E.ptr(peak), en.data_ptr() + 8 * PAD if energies else None,
                                   E.ptr(status), E.stream_ptr()))
    else:
        E.check(st.lib.tt_sil_trim(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(thr), E.ptr(par), E.ptr(ro_d), E.ptr(ro_d), y.data_ptr() + 4 * PAD,
                                   E.ptr(n_out), E.ptr(n_reg), reg.data_ptr() + 8 * PAD, E.ptr(n_seg), seg.data_ptr() + 12 * PAD, E.ptr(peak),
                                   E.ptr(status), E.stream_ptr()))
    y, reg, seg, en, n_out, n_reg, n_seg, status, peak = (t.cpu().numpy() for t in (y, reg, seg, en, n_out, n_reg, n_seg, status, peak))
    reg, seg = reg.reshape(-1, 2), seg.reshape(-1, 3)
    for a, m in ((y, io[-1]), (reg, ro[-1]), (seg, ro[-1]), (en, fo[-1])):  # nothing beyond the batch's slices
        assert (a[:PAD] == SENT).all() and (a[PAD + m:] == SENT).all()
    assert n_out[n] == SENT and n_reg[n] == SENT and n_seg[n] == SENT and status[n] == SENT and peak[n] == SENT
    y, reg, seg, en = y[PAD:], reg[PAD:], seg[PAD:], en[PAD:]
    return [dict(status=int(status[i]), y=y[io[i]:io[i + 1]], reg=reg[ro[i]:ro[i + 1]], seg=seg[ro[i]:ro[i + 1]], en=en[fo[i]:fo[i + 1]],
                 n_out=n_out[i:i + 1], n_reg=n_reg[i:i + 1], n_seg=n_seg[i:i + 1], peak=peak[i:i + 1]) for i in range(n)]


KEYS = ("y", "reg", "seg", "en", "n_out", "n_reg", "n_seg", "peak")


def untouched(r):
    return all((r[k] == SENT).all() for k in KEYS)


def same(a, b):
    return a["status"] == b["status"] and all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


def verify(results, what):
    """Every family member's trim result against the reference: no exemption."""
    worst, faded = 0.0, 0
    for i, r in enumerate(results):
        x, ref = reference(i)
        name = NAMES[i]
        n_out, R_, K = ref["n_out"], len(ref["regions"]), len(ref["segments"])
        assert r["status"] == ref["status"], (name, r["status"], ref["status"])
        assert r["n_reg"][0] == R_ and r["reg"][:R_].tolist() == [list(v) for v in ref["regions"]] and (r["reg"][R_:] == SENT).all(), name
        assert r["n_seg"][0] == K and r["seg"][:K].tolist() == [list(v) for v in ref["segments"]] and (r["seg"][K:] == SENT).all(), name
        assert r["n_out"][0] == n_out and (r["y"][n_out:] == SENT).all(), name
        assert abs(r["peak"][0] - ref["E"]) <= R.band(ref["E"]), name
        y = r["y"][:n_out]
        copied = ref["ops"] == 0
        assert y[copied].tobytes() == ref["y"][copied].astype(np.float32).tobytes(), name  # bit for bit
        assert ref["ops"].max() <= 3, name  # a cross-fade (three operations) and a fade (two) never meet
        if (~copied).any():
            share = np.abs(y[~copied].astype(np.float64) - ref["y"][~copied]) / ref["bound"][~copied]
            assert (share <= 1.0).all(), (name, float(share.max()))
            worst, faded = max(worst, float(share.max())), faded + int((~copied).sum())
        if ref["status"] in (E.SIL_UNCHANGED, E.SIL_SILENT):
            assert y.tobytes() == x.tobytes() and K == 1, name
    print(f"[parity] tt_sil_trim {what}: {len(results)} clips (1 .. {max(len(reference(i)[0]) for i in range(len(FAMILY)))} samples, scan chunks "
          f"of {CHUNK} frames, render tiles of {TILE}); regions, segments and n_out equal, copies bit for bit, {faded} cross-faded or faded "
          f"samples, worst share of the sample bound used {worst:.3f}")


def test_the_family_is_decided_and_covers_the_edges():
    """On the CPU alone: no frame of any clip lies within the band of its threshold, and the shapes are the ones the kernels can go wrong at."""
    by = {}
    for i, name in enumerate(NAMES):
        x, ref = reference(i)
        assert not ref["undecided"].any(), (name, np.flatnonzero(ref["undecided"]).tolist())
        by[name] = ref
    assert CHUNK == 1024 and TILE == 1024
    assert [len(by[f"frames_{F}"]["e"]) for F in (CHUNK - 1, CHUNK, CHUNK + 1)] == [CHUNK - 1, CHUNK, CHUNK + 1]
    assert all(len(by[f"frames_{F}"]["segments"]) >= 3 for F in (CHUNK - 1, CHUNK, CHUNK + 1))
    assert [by[f"out_{m}"]["n_out"] for m in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)] == \
        [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
    gap = lambda r: r["regions"][1][0] - r["regions"][0][1]
    assert all(gap(by[f"cut_{d:+d}"]) == 2160 for d in (-1, 0, 1))
    assert [len(by[f"cut_{d:+d}"]["segments"]) for d in (-1, 0, 1)] == [1, 2, 2]          # G = M + X - 1 stays, M + X and M + X + 1 are cut
    assert [by[f"cut_{d:+d}"]["n_out"] for d in (-1, 0, 1)] == [7200, 7200 - R.X, 7200 - R.X - 1]
    assert by["cut_least"]["segments"][0][2] + by["cut_least"]["segments"][1][2] == by["cut_least"]["n_out"]
    assert len(by["pad_merges"]["regions"]) == 1 and len(by["pad_does_not"]["regions"]) == 2 and len(by["bridged"]["regions"]) == 1
    assert len(by["one_region"]["regions"]) == 1 and by["one_region"]["D0"] > 0 and by["one_region"]["Dt"] > 0
    assert by["edges_in_speech"]["D0"] == 0 and by["edges_in_speech"]["Dt"] == 0 and len(by["edges_in_speech"]["segments"]) == 2
    assert len(by["many_pauses"]["segments"]) == 12 and by["many_pauses"]["Dt"] > 0
    assert by["n24000_lead_off"]["D0"] == 0 and by["n24000_trail_off"]["Dt"] == 0 and len(by["n24000_pause_off"]["segments"]) == 1
    assert by["n24000_all_off"]["status"] == E.SIL_UNCHANGED and by["n24000"]["status"] == E.SIL_OK
    assert all(by[f"zeros_{n}"]["status"] == E.SIL_SILENT for n in (1, 120, 481)) and by["constant"]["status"] == E.SIL_UNCHANGED
    assert by["late_1"]["n_out"] == 241 and by["late_1"]["D0"] == 240  # (the frame before a lone last sample holds it too)
    assert (R.OK, R.UNCHANGED, R.SILENT, R.EMPTY, R.REFUSED) == (E.SIL_OK, E.SIL_UNCHANGED, E.SIL_SILENT, E.SIL_EMPTY, E.SIL_REFUSED)


@pytest.fixture(scope="module")
def solo():
    return [device_trim([(reference(i)[0], FAMILY[i][2])])[0] for i in range(len(FAMILY))]


def _batched(size, seed):
    """The family in shuffled order in calls of `size` clips (parameters mixed within a call) -> results in the family's order."""
    order = np.random.default_rng(seed).permutation(len(FAMILY))
    out = [None] * len(FAMILY)
    for g in range(0, len(FAMILY), size):
        idx = order[g:g + size]
        for i, r in zip(idx, device_trim([(reference(i)[0], FAMILY[i][2]) for i in idx])):
            out[i] = r
    return out


def test_family_solo(solo):
    verify(solo, "solo")


def test_find_flags_energies_and_regions():
    """tt_sil_find: every frame energy inside the band, every activity flag equal (from the device's energies and its E), regions equal."""
    res = [device_trim([(reference(i)[0], FAMILY[i][2])], find=True)[0] for i in range(len(FAMILY))]
    worst = 0.0
    for i, r in enumerate(res):
        x, ref = reference(i)
        rel, floor_e = FAMILY[i][2][:2]
        R_ = len(ref["regions"])
        assert r["status"] == (E.SIL_SILENT if ref["status"] == E.SIL_SILENT else E.SIL_OK), NAMES[i]
        assert r["en"].shape == ref["e"].shape and (np.abs(r["en"] - ref["e"]) <= R.band(ref["e"])).all(), NAMES[i]
        assert r["peak"][0] == r["en"].max()  # E is exactly the maximum of the device's frame energies
        assert ((r["en"] > max(floor_e, rel * r["peak"][0])) == ref["active"]).all(), NAMES[i]
        assert r["n_reg"][0] == R_ and r["reg"][:R_].tolist() == [list(v) for v in ref["regions"]] and (r["reg"][R_:] == SENT).all(), NAMES[i]
        assert (r["y"] == SENT).all() and (r["seg"] == SENT).all() and r["n_out"][0] == SENT and r["n_seg"][0] == SENT  # find edits nothing
        nz = ref["e"] > 0
        worst = max(worst, float((np.abs(r["en"] - ref["e"])[nz] / R.band(ref["e"])[nz]).max()) if nz.any() else 0.0)
    print(f"[parity] tt_sil_find: {len(res)} clips, flags and regions equal; worst share of the energy band (gamma_{R.K_OPS + 1}, u = 2^-53) used {worst:.4f}")
    # without the energies: the same regions
    i = NAMES.index("n24000")
    quiet = device_trim([(reference(i)[0], FAMILY[i][2])], find=True, energies=False)[0]
    assert quiet["reg"].tobytes() == res[i]["reg"].tobytes() and (quiet["en"] == SENT).all() and quiet["peak"].tobytes() == res[i]["peak"].tobytes()


def test_family_ragged_batches_of_17(solo):
    ragged = _batched(17, 1)
    verify(ragged, "ragged batches of 17")
    assert all(same(a, b) for a, b in zip(ragged, solo))  # bit-identical to the solo calls


def test_family_in_pairs_is_bit_identical_to_solo(solo):
    assert all(same(a, b) for a, b in zip(_batched(2, 2), solo))


def _bad():
    x = R.build([("z", 500), ("s", 900), ("z", 500)], 99)
    p = R.params
    swap = lambda q, k, v: q[:k] + (v,) + q[k + 1:]
    return {
        "empty": (np.zeros(0, np.float32), p(), E.SIL_EMPTY, None),
        "too_long": (np.zeros(MAX_SAMPLES + 1, np.float32), p(), E.SIL_REFUSED, None),
        "rel_above": (x, swap(p(), 0, 1.5), E.SIL_REFUSED, None),
        "rel_nan": (x, swap(p(), 0, float("nan")), E.SIL_REFUSED, None),
        "floor_negative": (x, swap(p(), 1, -1.0), E.SIL_REFUSED, None),
        "floor_inf": (x, swap(p(), 1, float("inf")), E.SIL_REFUSED, None),
        "min_sil_negative": (x, p(min_sil=-1), E.SIL_REFUSED, None),
        "pad_too_large": (x, p(pad=R.MAX_FRAMES_PARAM + 1), E.SIL_REFUSED, None),
        "lead_below": (x, p(lead=-2), E.SIL_REFUSED, None),
        "trail_above": (x, p(trail=R.MAX_SAMPLES + 1), E.SIL_REFUSED, None),
        "pause_below_fade": (x, p(max_pause=R.X - 1), E.SIL_REFUSED, None),
        "pause_zero": (x, p(max_pause=0), E.SIL_REFUSED, None),
        "slices_short": (x, p(), E.SIL_REFUSED, R.max_regions(len(x)) - 1),
    }


BAD = _bad()


@pytest.mark.parametrize("name", list(BAD))
def test_a_clip_that_is_not_read_gets_its_status_and_nothing_else(name, solo):
    x, p, status, cap = BAD[name]
    a, b = NAMES.index("n5000"), NAMES.index("late_121")
    res = device_trim([(reference(a)[0], FAMILY[a][2]), (x, p), (reference(b)[0], FAMILY[b][2])], caps=[None, cap, None])
    assert R.trim(x, p)["status"] == status or name in ("too_long", "slices_short")  # (these two are the handle's and the call's limits)
    assert res[1]["status"] == status and untouched(res[1])
    assert same(res[0], solo[a]) and same(res[2], solo[b])  # the neighbours: untouched by it, and correct (test_family_solo)


def test_all_zero_and_constant_clips_come_back_bit_for_bit(solo):
    for name, status in (("zeros_1", E.SIL_SILENT), ("zeros_481", E.SIL_SILENT), ("constant", E.SIL_UNCHANGED)):
        i = NAMES.index(name)
        x, r = reference(i)[0], solo[i]
        assert r["status"] == status and r["n_out"][0] == len(x) and r["y"].tobytes() == x.tobytes() and r["seg"][0].tolist() == [0, 0, len(x)]
    r = solo[NAMES.index("zeros_481")]
    assert r["n_reg"][0] == 0 and r["peak"][0] == 0.0 and (r["reg"] == SENT).all()


def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(8, device=DEV)
    z = torch.zeros(8, device=DEV)
    d = torch.zeros(8, dtype=torch.float64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    P = E.ptr
    trim = lambda n, audio=P(y), out=P(z), io=P(i): st.lib.tt_sil_trim(st.h, n, audio, io, P(d), P(i), P(i), P(i), out, P(i), P(i), P(i), P(i), P(i),
                                                                      P(d), P(i), E.stream_ptr())
    for n in (0, 33):
        assert trim(n) == -1 and b"clips (1 .. 32)" in st.lib.tt_last_error()
        assert st.lib.tt_sil_find(st.h, n, P(y), P(i), P(d), P(i), P(i), None, P(i), P(i), P(d), None, P(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert trim(1, io=None) == -1 and b"null argument" in st.lib.tt_last_error()
    assert trim(1, out=P(y)) == -1 and b"overlap" in st.lib.tt_last_error()
    assert st.lib.tt_sil_find(st.h, 1, P(y), P(i), P(d), P(i), P(i), None, P(i), P(i), P(d), P(d), P(i), E.stream_ptr()) == -1
    assert b"go together" in st.lib.tt_last_error()


def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


def _as_params(p):
    return sil.Params(*p)


@torch.no_grad()
def test_trim_and_speech_regions_through_the_api(solo):
    h = _host()
    # the API's options in seconds are the device's integers: 0.05 s lead = 1200 samples, 0.1 s = 10 frames, ...
    assert sil.params(max_pause=0.05) == _as_params(R.params(max_pause=1200)) and sil.params() == _as_params(R.params())
    i = NAMES.index("n24000")
    x = torch.from_numpy(reference(i)[0].copy())
    want = solo[i]["y"][:solo[i]["n_out"][0]]
    y = h.trim(x, max_pause=0.05)
    assert y.shape == want.shape and y.device.type == "cpu" and y.numpy().tobytes() == want.tobytes()
    y, segs = h.trim_many([x.reshape(1, 1, -1).to(DEV)], max_pause=0.05, return_map=True)
    assert y[0].shape == (1, 1, len(want)) and y[0].device.type == "cuda" and y[0].cpu().numpy().tobytes() == want.tobytes()
    assert segs[0] == reference(i)[1]["segments"] and h.silence_info[0]["status"] == "ok"
    assert abs(h.silence_info[0]["removed_s"] - (24000 - len(want)) / 24000) < 1e-12
    regions, pauses = h.speech_regions(x)
    assert regions == reference(i)[1]["regions"] and pauses == [(regions[0][1], regions[1][0])]
    found = h.load_silence().find_many([x], [sil.params()], energies=True)[0]  # the stage's own call, with the frame energies
    e = reference(i)[1]["e"]
    assert found["regions"] == regions and found["status"] == E.SIL_OK and found["peak"] == float(found["energies"].max())
    assert found["energies"].shape == e.shape and (np.abs(found["energies"].numpy() - e) <= R.band(e)).all()
    assert sil.map_sample(regions[1][0], segs[0]) == R.map_sample(regions[1][0], segs[0]) == regions[0][1] - segs[0][0][1] + 1200
    # more clips than one call takes (16), every clip the bits of its solo call (the family members that use the default detection)
    pick = [k for k, (_, _, p) in enumerate(FAMILY) if p == R.params(max_pause=p[6]) and len(reference(k)[0]) <= 30000]
    assert len(pick) > 16
    mp = lambda k: None if FAMILY[k][2][6] < 0 else FAMILY[k][2][6] / 24000
    for m in sorted({mp(k) for k in pick}, key=str):
        ks = [k for k in pick if mp(k) == m]
        out = h.trim_many([torch.from_numpy(reference(k)[0].copy()) for k in ks], max_pause=m)
        for k, o in zip(ks, out):
            assert o.numpy().tobytes() == solo[k]["y"][:solo[k]["n_out"][0]].tobytes(), NAMES[k]
    assert h.silencer.max_samples == 30 * 24000 and h.silencer.max_clips == 16
    z = h.trim(torch.zeros(1, 777))
    assert z.shape == (1, 777) and not z.any() and h.silence_info[0]["status"] == "silent"
    with pytest.raises(ValueError, match="max_pause=0.001"):
        h.trim(x, max_pause=0.001)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    return TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)


@torch.no_grad()
def test_trim_silence_and_max_pause_on_tts_equal_the_chain_on_the_clip(tts):
    import bench
    text = bench.synthetic_prompt()[0].tolist()
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts(text, **kw)
    again = tts.tts(text, trim_silence=None, max_pause=None, **kw)
    assert torch.equal(again, plain) and tts.silencer is None and "silence_s" not in tts.timings  # today's bits, no stage
    got = tts.tts(text, trim_silence=True, max_pause=0.3, **kw)
    assert tts.timings["silence_s"] > 0 and len(tts.silence_info) == 1
    want = tts.trim(plain, max_pause=0.3)
    assert got.shape == want.shape and torch.equal(got, want) and got.shape[-1] <= plain.shape[-1]
