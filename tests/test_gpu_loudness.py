"""The loudness normalisation on the MI355X (csrc/loudness.hip, include/tortoise_mi355x_loud.h) against the reference of
tests/loudness_reference.py, every number inside the bound derived there.

  measure    hop energies, L and true peak inside their bounds; the gated block counts equal the reference's exactly (no family block lies
             within 1e-6 LU of a gate: tests/test_loudness_cpu.py); statuses; nothing written for a refused clip or beyond the batch.
  normalize  the gain inside its bound; the samples judged against the device's OWN reported gain: NONE / SCALE bit for bit f32(g x),
             LOOKAHEAD inside the bound of the fp64 limiter run with that gain, below the ceiling, and exactly g x where nothing limits;
             out_true_peak inside its bound of the reference's reading of the device's output.
Ragged batches are byte-identical to solo calls, on a second handle too, and the target is met end to end."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0             # what every output holds before the call
CLIP = 131072           # the handles are made for clips of this length
MODES = (R.NONE, R.SCALE, R.LOOKAHEAD)
NAMES = {R.NONE: "none", R.SCALE: "scale", R.LOOKAHEAD: "lookahead"}

_stages = {}


def stage(max_clips=32):
    if max_clips not in _stages:
        _stages[max_clips] = stages.LoudnessStage(CLIP * max(max_clips, 17), max_clips=max_clips, device=DEV)
    return _stages[max_clips]


def device_call(clips, mode=None, hop_spans=None, st=None, in_off=None):
    """One tt_loud_measure (mode None) or tt_loud_normalize call over clips = [(x f32 [n], target, ceiling)] with every output pre-filled
    with SENT -> per clip a dict of what the call left (SENT where it wrote nothing).  hop_spans: per clip the hop_energy entries it is
    handed where that is not tt_loud_hops; in_off: the sample offsets where they are not the running sum of the lengths."""
    st = st or stage()
    n = len(clips)
    hop_spans = hop_spans or [None] * n
    spans = [R.hops(len(x)) if s is None else s for s, (x, _, _) in zip(hop_spans, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x, _, _ in clips]))).astype(np.int32)
    ho = np.concatenate(([0], np.cumsum(spans))).astype(np.int32)
    tail = int(io[-1])
    io = io if in_off is None else np.asarray(in_off, dtype=np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _, _ in clips] + [np.zeros(1, np.float32)])).to(DEV)
    io_d, ho_d = torch.from_numpy(io).to(DEV), torch.from_numpy(ho).to(DEV)
    f32 = lambda k: torch.full((k,), SENT, device=DEV)
    lufs, hop = torch.full((n,), SENT, dtype=torch.float64, device=DEV), torch.full((int(ho[-1]) + 1,), SENT, dtype=torch.float64, device=DEV)
    tp, gain, otp, y = f32(n), f32(n), f32(n), f32(tail + 1)
    ba, br, status = (torch.full((n,), int(SENT), dtype=torch.int32, device=DEV) for _ in range(3))
    if mode is None:
        E.check(st.lib.tt_loud_measure(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(ho_d), E.ptr(lufs), E.ptr(tp), E.ptr(ba), E.ptr(br), E.ptr(hop),
                                       E.ptr(status), E.stream_ptr()))
    else:
        target = torch.tensor([t for _, t, _ in clips], dtype=torch.float32, device=DEV)
        ceiling = torch.tensor([c for _, _, c in clips], dtype=torch.float32, device=DEV)
        E.check(st.lib.tt_loud_normalize(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(ho_d), E.ptr(target), E.ptr(ceiling), mode, E.ptr(y), E.ptr(lufs),
                                         E.ptr(tp), E.ptr(ba), E.ptr(br), E.ptr(hop), E.ptr(gain), E.ptr(otp), E.ptr(status), E.stream_ptr()))
    lufs, hop, tp, gain, otp, y, ba, br, status = (t.cpu().numpy() for t in (lufs, hop, tp, gain, otp, y, ba, br, status))
    assert hop[ho[-1]] == SENT and y[tail] == SENT  # nothing beyond the batch
    if mode is None:
        assert (y == SENT).all() and (gain == SENT).all() and (otp == SENT).all()
    return [dict(status=int(status[i]), lufs=lufs[i], true_peak=tp[i], blocks_abs=int(ba[i]), blocks_rel=int(br[i]), hop_energy=hop[ho[i]:ho[i + 1]],
                 gain=gain[i], out_true_peak=otp[i], y=y[io[i]:io[i + 1]]) for i in range(n)]


KEYS = ("lufs", "true_peak", "hop_energy", "gain", "out_true_peak", "y")


def untouched(r):
    return all((np.asarray(r[k]) == SENT).all() for k in KEYS) and r["blocks_abs"] == r["blocks_rel"] == int(SENT)


def same(a, b):
    return a["status"] == b["status"] and a["blocks_abs"] == b["blocks_abs"] and a["blocks_rel"] == b["blocks_rel"] and \
        all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def share(err, bound):
    """The largest share of its bound any entry uses (inf for an error where the bound is 0)."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0))


def verify_measure(results, what):
    fam = R.family_reference()
    assert len(results) == len(fam)
    worst = dict(hop=0.0, lufs=0.0, peak=0.0)
    for r, (x, _, _, m) in zip(results, fam):
        assert r["status"] == m["status"], (len(x), r["status"])
        worst["hop"] = max(worst["hop"], share(np.abs(r["hop_energy"] - m["hop_energy"]), m["hop_bound"]))
        worst["peak"] = max(worst["peak"], share(abs(float(r["true_peak"]) - m["true_peak"]), m["tp_bound"]))
        assert (r["blocks_abs"], r["blocks_rel"]) == (m["blocks_abs"], m["blocks_rel"]), (len(x), r["blocks_abs"], r["blocks_rel"])
        if m["status"] == R.OK:
            worst["lufs"] = max(worst["lufs"], share(abs(r["lufs"] - m["lufs"]), m["lufs_bound"]))
        else:
            assert r["lufs"] == -math.inf
    print(f"[parity] tt_loud_measure {what}: {len(fam)} clips; worst share of the hop-energy bound used {worst['hop']:.3f}, of the L bound "
          f"{worst['lufs']:.3f}, of the true-peak bound {worst['peak']:.3f}")
    assert max(worst.values()) <= 1.0, worst
    return worst


def verify_normalize(results, mode, what):
    fam = R.family_reference()
    worst = dict(gain=0.0, y=0.0, out_peak=0.0, ceiling=0.0)
    limited = exact = 0
    for r, (x, target, ceiling, m) in zip(results, fam):
        assert r["status"] == m["status"]
        g_ref, g_bound = R.gain(m, target, ceiling, mode)
        g = np.float32(r["gain"])
        worst["gain"] = max(worst["gain"], share(abs(float(g) - g_ref), g_bound))
        if m["status"] != R.OK:
            assert g == 1.0 and r["y"].tobytes() == x.tobytes()  # SHORT and SILENT: the samples, bit for bit
        elif mode != R.LOOKAHEAD:
            assert r["y"].tobytes() == (g * x).tobytes()  # f32(g' x) with the device's own g'
            if mode == R.SCALE:
                over = float(r["out_true_peak"]) / ceiling - 1
                worst["ceiling"] = max(worst["ceiling"], share(max(over, 0.0), R.scale_ceiling_bound(m, float(g), ceiling)))
        else:
            lim = R.limiter(x, g, ceiling)
            worst["y"] = max(worst["y"], share(np.abs(r["y"].astype(np.float64) - lim["y"]), lim["bound"]))
            assert (np.abs(r["y"]) <= ceiling * (1 + 4 * R.U32)).all()
            assert r["y"][lim["free"]].tobytes() == (g * x)[lim["free"]].tobytes()  # exactly g x where nothing limits
            limited += bool((lim["s"] < 1).any())
            exact += bool(lim["free"].all())
        tp, tb, _ = R.true_peak(r["y"])
        worst["out_peak"] = max(worst["out_peak"], share(abs(float(r["out_true_peak"]) - tp), tb))
    if mode == R.LOOKAHEAD:
        assert limited >= 3 and exact >= 3
    print(f"[parity] tt_loud_normalize {NAMES[mode]} {what}: {len(fam)} clips; worst share of the gain bound used {worst['gain']:.3f}, of the sample "
          f"bound {worst['y']:.3f}, of the output true-peak bound {worst['out_peak']:.3f}, of the SCALE ceiling bound {worst['ceiling']:.3f}")
    assert max(worst.values()) <= 1.0, worst
    return worst


@pytest.fixture(scope="module")
def solo():
    fam = R.family_reference()
    out = {None: [device_call([(x, T, c)])[0] for x, T, c, _ in fam]}
    for mode in MODES:
        out[mode] = [device_call([(x, T, c)], mode)[0] for x, T, c, _ in fam]
    return out


def _batched(size, seed, mode, st=None):
    """The family in shuffled order in calls of `size` clips (targets, ceilings and lengths mixed within a call) -> results in the family's order."""
    fam = R.family_reference()
    order = np.random.default_rng(seed).permutation(len(fam))
    out = [None] * len(fam)
    for g in range(0, len(fam), size):
        idx = order[g:g + size]
        for i, r in zip(idx, device_call([fam[i][:3] for i in idx], mode, st=st)):
            out[i] = r
    return out


def test_measure_solo(solo):
    verify_measure(solo[None], "solo")
    # normalize measures the same: every reading the bytes of measure's
    for mode in MODES:
        for a, b in zip(solo[mode], solo[None]):
            assert a["status"] == b["status"] and (a["blocks_abs"], a["blocks_rel"]) == (b["blocks_abs"], b["blocks_rel"])
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("lufs", "true_peak", "hop_energy"))


@pytest.mark.parametrize("mode", MODES, ids=[NAMES[m] for m in MODES])
def test_normalize_solo(solo, mode):
    verify_normalize(solo[mode], mode, "solo")


@pytest.mark.parametrize("mode", (None,) + MODES, ids=["measure"] + [NAMES[m] for m in MODES])
def test_ragged_batches_are_byte_identical_to_solo(solo, mode):
    assert all(same(a, b) for a, b in zip(_batched(17, 1, mode), solo[mode]))  # (the solo results are the verified ones)
    assert all(same(a, b) for a, b in zip(_batched(2, 2, mode), solo[mode]))
    assert all(same(a, b) for a, b in zip(_batched(1, 3, mode, st=stage(2)), solo[mode]))  # a second handle, another max_clips
    assert all(same(a, b) for a, b in zip(_batched(2, 4, mode, st=stage(2)), solo[mode]))


BAD = {
    "empty": (np.zeros(0, np.float32), -23.0, 0.5, E.LOUD_EMPTY, 3),
    "beyond_the_handle": (None, -23.0, 0.5, E.LOUD_REFUSED, None),
    "wrong_hop_span": (R.clip("speech", 12000, 5), -23.0, 0.5, E.LOUD_REFUSED, 4),
    "no_hop_span": (R.clip("speech", 12000, 5), -23.0, 0.5, E.LOUD_REFUSED, 0),
    "target_nan": (R.clip("speech", 12000, 5), float("nan"), 0.5, E.LOUD_REFUSED, None),
    "ceiling_zero": (R.clip("speech", 12000, 5), -23.0, 0.0, E.LOUD_REFUSED, None),
    "ceiling_negative": (R.clip("speech", 12000, 5), -23.0, -0.5, E.LOUD_REFUSED, None),
    "ceiling_inf": (R.clip("speech", 12000, 5), -23.0, float("inf"), E.LOUD_REFUSED, None),
}


@pytest.mark.parametrize("name", list(BAD))
def test_a_clip_that_is_not_measured_gets_its_status_and_nothing_else(name, solo):
    x, target, ceiling, status, span = BAD[name]
    fam = R.family_reference()
    a, b = 6, 10  # (12000 and 16800 samples)
    if name == "beyond_the_handle":  # the clip ends behind the samples the handle was made for: a small handle, nothing else differs
        st = stages.LoudnessStage(len(fam[a][0]) + 20000, max_clips=4, device=DEV)
        x = R.clip("speech", 20001, 5)
        clips, spans = [fam[a][:3], (x, target, ceiling)], [None, None]
    else:
        st = None
        clips, spans = [fam[a][:3], (x, target, ceiling), fam[b][:3]], [None, span, None]
    for mode in (None, R.LOOKAHEAD):
        if mode is None and name.startswith(("target", "ceiling")):
            continue  # (measure has no target)
        res = device_call(clips, mode, hop_spans=spans, st=st)
        assert res[1]["status"] == status and untouched(res[1])
        assert same(res[0], solo[mode][a]) and (len(res) < 3 or same(res[2], solo[mode][b]))  # the neighbours: untouched by it, and correct
    if st is not None:
        st.close()


def test_offsets_that_decrease_refuse_every_clip_behind_them(solo):
    """in_off = 0, 12000, 11000, 27800: clip 1 has a negative length, clip 2 starts before clip 1's start - their workspace would overlap."""
    fam = R.family_reference()
    a, b = 6, 10
    for mode in (None, R.SCALE):
        res = device_call([fam[a][:3], fam[a][:3], fam[b][:3]], mode, in_off=[0, 12000, 11000, 27800])
        assert [r["status"] for r in res[1:]] == [E.LOUD_REFUSED] * 2
        assert (res[1]["hop_energy"] == SENT).all() and res[1]["lufs"] == SENT and (res[2]["hop_energy"] == SENT).all() and res[2]["lufs"] == SENT
        assert same(res[0], solo[mode][a])
        assert (res[2]["y"][1000:] == SENT).all()  # (its slice of out begins at 11000: the first 1000 samples are clip 0's)


def test_argument_checks_come_before_device_work():
    st = stage()
    f, d = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    P = E.ptr
    for n in (0, 33):
        assert st.lib.tt_loud_measure(st.h, n, P(f), P(i), P(i), P(d), P(f), P(i), P(i), P(d), P(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
        assert st.lib.tt_loud_normalize(st.h, n, P(f), P(i), P(i), P(f), P(f), 0, P(f), P(d), P(f), P(i), P(i), P(d), P(f), P(f), P(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert st.lib.tt_loud_measure(st.h, 1, P(f), None, P(i), P(d), P(f), P(i), P(i), P(d), P(i), E.stream_ptr()) == -1
    assert b"null argument" in st.lib.tt_last_error()
    for mode in (-1, 3):
        assert st.lib.tt_loud_normalize(st.h, 1, P(f), P(i), P(i), P(f), P(f), mode, P(f), P(d), P(f), P(i), P(i), P(d), P(f), P(f), P(i), E.stream_ptr()) == -1
        assert b"mode" in st.lib.tt_last_error()
    assert not f.any() and not d.any() and not i.any()


@torch.no_grad()
def test_normalize_then_loudness_reads_the_target(solo):
    """Quantising the output to f32 moves a sample by at most 2^-24 relative, the dB value by far less than 0.01: the tolerance is no knob."""
    from tortoise_tts_amd import api
    from tortoise_tts_amd import loudness as loud

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    fam = R.family_reference()
    pick = [i for i, f in enumerate(fam) if f[3]["status"] == R.OK]
    clips = [torch.from_numpy(fam[i][0].copy()) for i in pick]
    targets = [fam[i][1] for i in pick]
    out, info = h.normalize_many(clips, loudness=targets, true_peak=-1.0, limit="none", return_info=True)
    again = h.loudness_many(out)
    for i, o, a, b, T in zip(pick, out, info, again, targets):
        assert o.numpy().tobytes() == (np.float32(solo[R.NONE][i]["gain"]) * fam[i][0]).tobytes()  # the stage's calls are the solo calls
        assert a.status == b.status == "ok" and abs(b.lufs - T) <= 0.01 and abs(a.lufs + a.gain_db - T) <= 1e-5 and a.shortfall_lu == 0.0
    # SCALE: the ceiling holds, the shortfall is what is missing, and the reading says so
    out, info = h.normalize_many([c.reshape(1, 1, -1).to(DEV) for c in clips], loudness=targets, true_peak=-6.0, limit="scale", return_info=True)
    again = h.loudness_many(out)
    assert any(a.shortfall_lu > 0.1 for a in info) and all(o.device.type == "cuda" and o.dim() == 3 for o in out)
    for a, b, T in zip(info, again, targets):
        assert abs(b.lufs - (T - a.shortfall_lu)) <= 0.01 and a.out_true_peak_db <= -6.0 + 1e-4 and abs(b.true_peak_db - a.out_true_peak_db) < 1e-4
    # short and silent clips come back as they went in
    for i, f in enumerate(fam):
        if f[3]["status"] != R.OK:
            y, inf = h.normalize_many([torch.from_numpy(f[0].copy())], -23.0, return_info=True)
            assert y[0].numpy().tobytes() == f[0].tobytes() and inf[0].status in ("short", "silent") and inf[0].lufs == -math.inf and inf[0].gain_db == 0.0
    assert h.leveller.max_total_samples == 16 * 30 * 24000 and h.leveller.max_clips == 16
    with pytest.raises(ValueError, match="LUFS is outside"):
        h.normalize(clips[0], loudness=0.0)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    return TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)


@torch.no_grad()
def test_tts_many_meets_the_target(tts):
    import bench
    text = bench.synthetic_prompt()[0].tolist()
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts_many([text, text[:-2]], **kw)
    assert tts.leveller is None and "level_s" not in tts.timings
    again = tts.tts_many([text, text[:-2]], loudness=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)) and tts.leveller is None  # today's bits, no stage
    lev = tts.tts_many([text, text[:-2]], loudness=-19.0, limit="none", **kw)
    assert tts.timings["level_s"] > 0 and len(tts.loudness_info) == 2
    for l, p, info in zip(lev, plain, tts.loudness_info):
        assert l.shape == p.shape and torch.equal(l, tts.normalize(p, -19.0, limit="none"))
        assert p.shape[-1] >= R.B and info.status == "ok", (p.shape, info)  # (the clips are longer than a block and above the gate: measured)
        assert abs(tts.loudness(l).lufs - -19.0) <= 0.01
    one = tts.tts(text, **kw)
    assert torch.equal(tts.tts(text, loudness=-19.0, true_peak=-3.0, **kw), tts.normalize(one, -19.0, -3.0))
