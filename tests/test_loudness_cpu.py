"""CPU checks of the loudness normalisation: the reference of tests/loudness_reference.py against BS.1770-4 and EBU Tech 3341, the
conditions the clip family must meet so that the GPU test (tests/test_gpu_loudness.py) cannot hide a failure, the header against its Python
mirror, and the host flow (loudness / normalize / loudness= on tts, tts_many and read_long_form) on a reference-backed stand-in of the stage."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import loudness_reference as R
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import loudness as loud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lufs(x, fs):
    """Integrated loudness of x at any rate: the reference's filter and gates with 100 ms hops of that rate."""
    hop = fs // 10
    y = np.asarray(R.kweight(x, fs), dtype=np.float64)
    nb = (len(y) - 4 * hop) // hop + 1
    z = np.array([np.mean(y[j * hop:j * hop + 4 * hop] ** 2) for j in range(nb)])
    l = -0.691 + 10 * np.log10(np.maximum(z, 1e-300))
    a = l > -70
    r = a & (l > -0.691 + 10 * np.log10(z[a].mean()) - 10)
    return -0.691 + 10 * np.log10(z[r].mean())


def tone(db, seconds, fs=48000, f=997.0):
    return 10.0 ** (db / 20.0) * np.sin(2 * np.pi * f * np.arange(int(seconds * fs)) / fs)


# ----------------------------------------------------------------------------------------- conformance of the reference
def test_coefficients_at_48k_are_the_standards_tables():
    (sb, sa), (hb, ha) = R.coefficients(48000)
    table = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, 1.0, -2.0, 1.0, -1.99004745483398,
             0.99007225036621)  # ITU-R BS.1770-4, tables 1 and 2
    assert np.abs(np.array(sb + sa + hb + ha) - np.array(table)).max() <= 1e-10


def test_the_segmented_recurrence_is_the_recurrence():
    x = R.clip("speech", 2000, 3)
    a, b = R.kweight(x), R.kweight_plain(x)
    assert float(np.abs(a - b).max()) <= 2.0 ** -50 * float(np.abs(a).max())  # (both in extended precision where the platform has it)
    assert np.allclose(R.transition() @ R.transition(), np.linalg.matrix_power(R.transition(), 2))
    assert max(abs(np.linalg.eigvals(R.transition()))) < 0.5  # a segment forgets more than half of its start state


def test_tech_3341_tones_read_minus_23():
    assert abs(lufs(tone(-20.0, 20.0), 48000) - -23.0) <= 0.1  # 997 Hz at -20 dBFS, mono (one channel of the standard's stereo pair: -3.01 dB)
    # Tech 3341 cases 3 and 4 for one channel: each tone 3.01 dB up
    case3 = np.concatenate([tone(d + 3.01, s) for d, s in ((-36, 10), (-23, 60), (-36, 10))])
    case4 = np.concatenate([tone(d + 3.01, s) for d, s in ((-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10))])
    assert abs(lufs(case3, 48000) - -23.0) <= 0.1 and abs(lufs(case4, 48000) - -23.0) <= 0.1
    # and at the engine's rate, through measure() itself
    m = R.measure(tone(-20.0, 5.0, fs=24000).astype(np.float32))
    assert m["status"] == R.OK and abs(m["lufs"] - -23.0) <= 0.1


def test_true_peak_of_the_quarter_rate_sine():
    n = np.arange(4800)
    tp, bound, mag = R.true_peak(np.sin(2 * np.pi * n / 4 + np.pi / 4).astype(np.float32))  # sample peak 0.7071, true peak 1
    assert -0.4 <= 20 * math.log10(tp) <= 0.2 and bound < 1e-5 and mag >= tp
    h = R.taps()
    assert h.shape == (4, 16) and h[0].tolist() == [0.0] * 7 + [1.0] + [0.0] * 8 and np.abs(h.astype(np.float64).sum(axis=1) - 1).max() < 1e-6
    w = R.hann()
    assert w.shape == (241,) and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6 and w.argmax() == 120 and w.min() > 0


def test_the_tabulated_taps_are_the_formulas():
    """The f32 taps are part of the specification: the table the library uploads (csrc/loudness.hip) equals the header's formula, evaluated
    here, bit for bit - so the true-peak bound has no term for them."""
    src = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "loudness.hip")).read()
    body = re.search(r"kLoudTaps\[3\]\[TT_LOUD_TAPS\] = \{(.*?)\};", src, flags=re.S).group(1)
    table = np.array([float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[-+]?\d+", body)]).reshape(3, 16)
    assert table.astype(np.float32).tobytes() == R.taps()[1:].tobytes() and np.array_equal(table, table.astype(np.float32))


def test_limiter_properties():
    fam = R.family_reference()
    limited = 0
    for x, target, ceiling, m in fam:
        if m["status"] != R.OK:
            continue
        g = np.float32(R.gain(m, target, ceiling, R.NONE)[0])
        lim = R.limiter(x, g, ceiling)
        assert (lim["s"] <= lim["r"]).all()
        assert (np.abs(lim["y"]) <= ceiling * (1 + 4 * R.U32)).all()
        gx = float(g) * x.astype(np.float64)
        assert np.array_equal(lim["y"][lim["free"]], gx[lim["free"]])
        # wherever r is 1 within 2 Lh in exact arithmetic too
        pad = np.concatenate([np.ones(2 * R.LH), lim["r"], np.ones(2 * R.LH)])
        quiet = np.lib.stride_tricks.sliding_window_view(pad, 4 * R.LH + 1).min(axis=1) == 1
        assert np.array_equal(lim["y"][quiet], gx[quiet]) and not (lim["free"] & ~quiet).any()
        limited += bool((lim["s"] < 1).any())
    assert limited >= 3


# ----------------------------------------------------------------------------------------- conditions on the family
def test_family_conditions():
    fam = R.family_reference()
    assert len(fam) == len(R.FAMILY) == 20
    lose_abs = lose_rel = 0
    for (kind, n, seed), (x, target, ceiling, m) in zip(R.FAMILY, fam):
        assert len(x) == n and len(m["hop_energy"]) == R.hops(n) and len(m["z"]) == R.blocks(n)
        assert m["margin"] > R.GATE_MARGIN, (kind, n, seed, m["margin"])  # no block within 1e-6 LU of a gate, bounds included
        assert m["lufs_bound"] <= 1e-6, (kind, n, seed, m["lufs_bound"])
        assert m["status"] == (R.SHORT if n < R.B else R.SILENT if kind != "speech" else R.OK)
        lose_abs += m["blocks_abs"] < R.blocks(n) and m["status"] == R.OK
        lose_rel += m["blocks_rel"] < m["blocks_abs"]
    assert lose_abs >= 2 and lose_rel >= 2
    # SCALE binds on some clips and not on others; LOOKAHEAD limits on some and not on others; every target and ceiling occurs
    ok = [(x, T, c, m) for x, T, c, m in fam if m["status"] == R.OK]
    binds = [R.gain(m, T, c, R.SCALE)[0] < R.gain(m, T, c, R.NONE)[0] * (1 - 1e-3) for x, T, c, m in ok]
    assert 3 <= sum(binds) <= len(ok) - 3
    limits = [bool((R.limiter(x, np.float32(R.gain(m, T, c, R.NONE)[0]), c)["s"] < 1).any()) for x, T, c, m in ok]
    assert 3 <= sum(limits) <= len(ok) - 3
    assert {T for _, T, _, _ in ok} == set(R.TARGETS) and len({c for _, _, c, _ in ok}) == 2
    # the gain reaches the target: the gates cut the same blocks of g x (what the GPU test's end-to-end check relies on)
    # (also at the lower gain SCALE takes under a ceiling of -6 dBTP)
    for x, T, c, m in ok:
        for g in (R.gain(m, T, c, R.NONE)[0], R.gain(m, T, float(np.float32(loud.linear(-6.0))), R.SCALE)[0]):
            again = R.measure((np.float32(g) * x).astype(np.float32))
            assert abs(again["lufs"] - (m["lufs"] + 20 * math.log10(g))) <= 1e-3, (len(x), T, g, again["lufs"])
        assert abs(m["lufs"] + 20 * math.log10(R.gain(m, T, c, R.NONE)[0]) - T) <= 1e-9


def test_bounds_come_from_the_formats():
    assert R.U64 == 2.0 ** -53 and R.U32 == 2.0 ** -24 and 1 < R.REF_SHARE <= 2
    x, _, _, m = R.family_reference()[13]  # 72000 samples
    y, e = R.filter_with_bound(x)
    y = np.abs(np.asarray(y, dtype=np.float64))
    assert e.shape == y.shape and (e >= R.gamma(8, R.U64) * y * 0.99).all()      # at least the sample's own roundings
    assert e.max() <= 7e4 * 4 * R.gamma(8, R.U64) * 3 * np.abs(x).max()           # at most the worst-case gain of the recursion (6.9e4) on every term
    assert (m["hop_bound"] >= R.gamma(R.H, R.U64) * m["hop_energy"]).all()
    P, Pb = R.peaks(x)
    assert (P >= np.abs(x)).all() and (Pb >= R.gamma(16, R.U32) * P).all() and (Pb <= R.gamma(16, R.U32) * 2.2 * np.abs(x).max()).all()


def test_an_emulation_in_the_device_formats_passes_the_gpu_checks():
    """tests/test_gpu_loudness.py's own checks on the device's scheme run in numpy (f64 segment passes and carry, f32 peaks and limiter,
    without fused operations): the bounds hold for another rounding order, and the checks do see a wrong number."""
    from tests import test_gpu_loudness as G
    fam = R.family_reference()
    for mode in G.MODES:
        res = [R.emulate(x, T, c, mode) for x, T, c, _ in fam]
        if mode == R.NONE:
            G.verify_measure(res, "emulated")
        G.verify_normalize(res, mode, "emulated")
    # (res: the LOOKAHEAD run)
    hop = res[13]["hop_energy"]
    res[13]["hop_energy"] = hop * (1 + 1e-7)
    with pytest.raises(AssertionError):
        G.verify_measure(res, "emulated, one clip's energies 1e-7 off")
    res[13]["hop_energy"] = hop
    res[15]["y"][60000] *= np.float32(1 + 1e-5)
    with pytest.raises(AssertionError):
        G.verify_normalize(res, R.LOOKAHEAD, "emulated, one sample 1e-5 off")


def test_the_checks_see_an_f32_filter():
    """The filter in f32 misses the hop bounds by orders of magnitude: the bounds do test the precision they are derived for."""
    x, _, _, m = R.family_reference()[13]
    (sb, sa), (hb, ha) = R.coefficients()
    from scipy.signal import lfilter
    y = lfilter(np.float32(hb), np.float32((1.0,) + ha), lfilter(np.float32(sb), np.float32((1.0,) + sa), x)).astype(np.float64)
    q = np.add.reduceat(y * y, np.arange(0, len(y), R.H))
    assert (np.abs(q - m["hop_energy"]) > 100 * m["hop_bound"]).any()


# ----------------------------------------------------------------------------------------- ABI
def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def test_loud_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_loud.h")
    assert set(names) == set(E._LOUD_PROTOS) == {"tt_loud_abi_version", "tt_loud_create", "tt_loud_destroy", "tt_loud_hops", "tt_loud_blocks",
                                                 "tt_loud_measure", "tt_loud_normalize"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_loud_abi_version() == 1 == E.LOUD_ABI_VERSION
    assert lib.tt_tsm_abi_version() == 1 and lib.tt_ctc_abi_version() == 1 and lib.tt_abi_version() == 6  # the other headers are untouched
    assert not [n for n in declared_symbols() if n.startswith("tt_loud")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_loud.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_LOUD_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    mirror = dict(TT_LOUD_SAMPLE_RATE=E.LOUD_SAMPLE_RATE, TT_LOUD_HOP=E.LOUD_HOP, TT_LOUD_BLOCK=E.LOUD_BLOCK, TT_LOUD_SEGMENT=E.LOUD_SEGMENT,
                  TT_LOUD_OVERSAMPLE=E.LOUD_OVERSAMPLE, TT_LOUD_TAPS=E.LOUD_TAPS, TT_LOUD_LOOKAHEAD=E.LOUD_LOOKAHEAD,
                  TT_LOUD_MAX_SAMPLES=E.LOUD_MAX_SAMPLES, TT_LOUD_MAX_CLIPS=E.LOUD_MAX_CLIPS, TT_LOUD_NONE=E.LOUD_NONE, TT_LOUD_SCALE=E.LOUD_SCALE,
                  TT_LOUD_LOOKAHEAD_MODE=E.LOUD_LOOKAHEAD_MODE, TT_LOUD_OK=E.LOUD_OK, TT_LOUD_SHORT=E.LOUD_SHORT, TT_LOUD_SILENT=E.LOUD_SILENT,
                  TT_LOUD_EMPTY=E.LOUD_EMPTY, TT_LOUD_REFUSED=E.LOUD_REFUSED)
    assert defines == mirror
    assert (R.FS, R.H, R.B, R.S, R.LH, R.TAPS, R.OS) == (E.LOUD_SAMPLE_RATE, E.LOUD_HOP, E.LOUD_BLOCK, E.LOUD_SEGMENT, E.LOUD_LOOKAHEAD, E.LOUD_TAPS,
                                                         E.LOUD_OVERSAMPLE)
    assert (R.NONE, R.SCALE, R.LOOKAHEAD, R.OK, R.SHORT, R.SILENT, R.EMPTY, R.REFUSED) == \
        (E.LOUD_NONE, E.LOUD_SCALE, E.LOUD_LOOKAHEAD_MODE, E.LOUD_OK, E.LOUD_SHORT, E.LOUD_SILENT, E.LOUD_EMPTY, E.LOUD_REFUSED)
    for n in (1, 2399, 2400, 2401, 9599, 9600, 9601, 11999, 12000, 120000, E.LOUD_MAX_SAMPLES):
        assert (lib.tt_loud_hops(n), lib.tt_loud_blocks(n)) == (R.hops(n), R.blocks(n))
    for n in (0, -1, E.LOUD_MAX_SAMPLES + 1):
        assert lib.tt_loud_hops(n) == 0 == lib.tt_loud_blocks(n)
    h = E.vp()
    for bad in ((0, 1), (E.LOUD_MAX_SAMPLES + 1, 1), (100, 0), (100, E.LOUD_MAX_CLIPS + 1)):
        assert lib.tt_loud_create(*bad, C.byref(h)) == -1 and b"tt_loud_create" in lib.tt_last_error()
    assert lib.tt_loud_measure(None, 1, *[None] * 10) == -1 and b"tt_loud_measure" in lib.tt_last_error()
    assert lib.tt_loud_normalize(None, 1, None, None, None, None, None, 0, *[None] * 10) == -1 and b"tt_loud_normalize" in lib.tt_last_error()
    rc = lib.tt_loud_create(1000, 2, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_loud_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())
        with pytest.raises(E.EngineError):
            E.check(rc)


# ----------------------------------------------------------------------------------------- options
def test_option_parsing():
    kw = dict(top_k=3)
    assert loud.level_options(kw) is None and kw == dict(top_k=3)
    kw = dict(loudness=None, top_k=3)
    assert loud.level_options(kw) is None and kw == dict(top_k=3)
    kw = dict(loudness=-19, top_k=3)
    lv = loud.level_options(kw)
    assert lv == loud.Level(-19.0, -1.0, "scale") and kw == dict(top_k=3) and lv.mode == E.LOUD_SCALE and abs(lv.ceiling - 10 ** (-1 / 20)) < 1e-15
    lv = loud.level_options(dict(loudness=-16.0, true_peak=-6, limit="lookahead"))
    assert lv == loud.Level(-16.0, -6.0, "lookahead") and lv.mode == E.LOUD_LOOKAHEAD_MODE
    assert loud.level_options(dict(loudness=-30, limit="none")).mode == E.LOUD_NONE
    for bad in (-70.1, -4.9, 0.0, 3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="LUFS is outside"):
            loud.level_options(dict(loudness=bad))
    for bad in (0.1, 3.0, -61.0, float("nan")):
        with pytest.raises(ValueError, match="dBTP is outside"):
            loud.level_options(dict(loudness=-23, true_peak=bad))
    with pytest.raises(ValueError, match="limit="):
        loud.level_options(dict(loudness=-23, limit="hard"))
    for orphan in (dict(true_peak=-2), dict(limit="scale")):
        with pytest.raises(ValueError, match="belong to loudness="):
            loud.level_options(orphan)
    with pytest.raises(ValueError, match="loudness_scope"):
        loud.scope_option(dict(loudness_scope="book"))
    assert loud.scope_option({}) == "chunk" and loud.scope_option(dict(loudness_scope="whole")) == "whole"
    assert loud.db(1.0) == 0.0 and loud.db(0.0) == -math.inf and abs(loud.linear(-6.0) - 0.5011872336272722) < 1e-15
    r = dict(status=E.LOUD_OK, lufs=-20.0, true_peak=0.5, gain=10 ** (-5 / 20), out_true_peak=0.25)
    got = loud.reading(r, -23.0)
    assert got.status == "ok" and abs(got.gain_db + 5) < 1e-12 and abs(got.shortfall_lu - 2) < 1e-9 and abs(got.out_true_peak_db - loud.db(0.25)) < 1e-12
    assert loud.reading(dict(r, gain=10 ** (-3 / 20)), -23.0).shortfall_lu == 0.0
    assert loud.reading(dict(status=E.LOUD_SHORT, lufs=-math.inf, true_peak=0.1)) == loud.Loudness(-math.inf, loud.db(0.1), status="short")


# ----------------------------------------------------------------------------------------- host flow
class ReferenceLoudnessStage:
    """stages.LoudnessStage backed by tests/loudness_reference.py."""
    made = []
    calls = []

    def __init__(self, max_total_samples, max_clips=16, device="cpu"):
        self.max_total_samples, self.max_clips = max_total_samples, max_clips
        ReferenceLoudnessStage.made.append(max_total_samples)

    @staticmethod
    def _dict(m):
        return dict(status=m["status"], lufs=m["lufs"], true_peak=float(np.float32(m["true_peak"])), blocks_abs=m["blocks_abs"],
                    blocks_rel=m["blocks_rel"], hop_energy=torch.from_numpy(m["hop_energy"]))

    def measure_many(self, clips):
        ReferenceLoudnessStage.calls.append(("measure", len(clips)))
        return [self._dict(R.measure(x.numpy())) for x in clips]

    def normalize_many(self, clips, targets, ceilings, mode):
        ReferenceLoudnessStage.calls.append(("normalize", len(clips)))
        out = []
        for x, T, c in zip(clips, targets, ceilings):
            assert x.dim() == 1 and x.shape[0] <= self.max_total_samples
            x = x.numpy()
            m = R.measure(x)
            g = np.float32(R.gain(m, T, c, mode)[0])
            y = R.limiter(x, g, c)["y"].astype(np.float32) if mode == R.LOOKAHEAD and m["status"] == R.OK else g * x
            out.append((torch.from_numpy(y), dict(self._dict(m), gain=float(g), out_true_peak=float(np.float32(R.true_peak(y)[0])))))
        return out

    def close(self):
        pass


def _ref(clip, target, true_peak=-1.0, limit="scale"):
    stage = ReferenceLoudnessStage.__new__(ReferenceLoudnessStage)
    stage.max_total_samples = 1 << 30
    calls = list(ReferenceLoudnessStage.calls)
    y = stage.normalize_many([clip.reshape(-1)], [target], [loud.linear(true_peak)], loud.MODES[limit])[0][0]
    ReferenceLoudnessStage.calls = calls
    return y.reshape(clip.shape)


def _install(monkeypatch, api):
    from tests.test_tsm_cpu import ReferenceStretchStage
    monkeypatch.setattr(api.stages, "LoudnessStage", ReferenceLoudnessStage)
    monkeypatch.setattr(api.stages, "TimeStretchStage", ReferenceStretchStage)
    ReferenceLoudnessStage.made, ReferenceLoudnessStage.calls = [], []
    ReferenceStretchStage.made, ReferenceStretchStage.calls = [], []


def _tts(monkeypatch, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup, voice_latents
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, **kw)
    call = dict(conditioning_latents=voice_latents(cfgs), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
                use_deterministic_seed=7, verbose=False)
    return t, call


def _speech(n=24000, seed=0):
    return torch.from_numpy(R.clip("speech", n, seed))


@torch.no_grad()
def test_loudness_and_normalize(monkeypatch):
    t, _ = _tts(monkeypatch)
    x = _speech()
    m = R.measure(x.numpy())
    got = t.loudness(x.reshape(1, 1, -1))
    assert got == loud.Loudness(m["lufs"], loud.db(float(np.float32(m["true_peak"]))), status="ok") and got.gain_db is None
    assert ReferenceLoudnessStage.made == [16 * 30 * 24000] and ReferenceLoudnessStage.calls == [("measure", 1)]
    for shape in ((24000,), (1, 24000), (1, 1, 24000)):
        y = t.normalize(x.reshape(shape), loudness=-19)
        assert y.shape == shape and y.dtype == torch.float32 and torch.equal(y.reshape(-1), _ref(x, -19.0))
    # several clips, a target and a ceiling each, ONE call, and what it reports
    clips = [x, _speech(12000, 1).reshape(1, -1), _speech(5000, 2)]
    ReferenceLoudnessStage.calls = []
    out, info = t.normalize_many(clips, loudness=[-16, -23, -30], true_peak=[-1, -6, -1], limit="scale", return_info=True)
    assert ReferenceLoudnessStage.calls == [("normalize", 3)] and [o.shape for o in out] == [c.shape for c in clips]
    assert torch.equal(out[1], _ref(clips[1], -23.0, -6.0)) and torch.equal(out[2], clips[2]) and info[2].status == "short" and info[2].gain_db == 0.0
    for i, c in zip(info[:2], (-1.0, -6.0)):
        assert i.status == "ok" and i.out_true_peak_db <= c + 1e-4 and i.shortfall_lu >= 0
    assert abs(info[0].lufs + info[0].gain_db + info[0].shortfall_lu - -16) < 1e-5
    assert torch.equal(t.normalize(x, -16, -6, "lookahead"), _ref(x, -16.0, -6.0, "lookahead"))
    assert torch.equal(t.normalize(x, -16, limit="none"), _ref(x, -16.0, limit="none"))
    assert t.normalize_many([]) == [] and t.loudness_many([]) == []
    # a longer clip than the stage was built for: it is built again, larger
    assert t.load_loudness(16 * 30 * 24000 + 1).max_total_samples == 16 * 30 * 24000 + 1 and t.load_loudness(100) is t.leveller
    assert ReferenceLoudnessStage.made == [16 * 30 * 24000, 16 * 30 * 24000 + 1]
    with pytest.raises(ValueError, match="LUFS is outside"):
        t.normalize(x, loudness=-3)
    with pytest.raises(ValueError, match="dBTP is outside"):
        t.normalize(x, true_peak=1.0)
    with pytest.raises(ValueError, match="3 clips with 2 targets"):
        t.normalize_many(clips, loudness=[-16, -23])
    with pytest.raises(ValueError, match="expected"):
        t.normalize(torch.zeros(2, 100))
    with pytest.raises(ValueError, match="expected"):
        t.loudness(torch.zeros(0))


@torch.no_grad()
def test_loudness_on_tts_and_tts_many(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    from tests.test_tsm_cpu import ReferenceStretchStage, _ref as stretched
    t, kw = _tts(monkeypatch)
    plain = t.tts(HELLO_THERE, **kw)
    # None: no stage, no call, today's bits
    assert torch.equal(t.tts(HELLO_THERE, loudness=None, **kw), plain) and torch.equal(t.tts_many([HELLO_THERE], loudness=None, **kw)[0], plain)
    assert t.leveller is None and ReferenceLoudnessStage.made == [] and ReferenceLoudnessStage.calls == [] and "level_s" not in t.timings
    lev = t.tts(HELLO_THERE, loudness=-19, **kw)
    assert ReferenceLoudnessStage.calls == [("normalize", 1)] and "level_s" in t.timings and "diffusion_s" in t.timings
    assert lev.shape == plain.shape and torch.equal(lev, _ref(plain, -19.0)) and len(t.loudness_info) == 1
    preset = t.tts_with_preset(HELLO_THERE, preset="ultra_fast", **kw)
    assert torch.equal(t.tts_with_preset(HELLO_THERE, preset="ultra_fast", loudness=-23, true_peak=-6, limit="lookahead", **kw),
                       _ref(preset, -23.0, -6.0, "lookahead"))
    # the rate first, then the level; k winners in one call each
    two = t.tts(HELLO_THERE, k=2, **kw)
    ReferenceLoudnessStage.calls, ReferenceStretchStage.calls = [], []
    both, state = t.tts(HELLO_THERE, k=2, speaking_rate=0.8, loudness=-16, return_deterministic_state=True, **kw)
    assert ReferenceLoudnessStage.calls == [("normalize", 2)] and ReferenceStretchStage.calls == [2] and state[0] == 7
    assert all(torch.equal(a, _ref(stretched(b, 0.8), -16.0)) for a, b in zip(both, two))
    # tts_many: one call for the texts
    many = t.tts_many([HELLO_THERE, HELLO], **kw)
    ReferenceLoudnessStage.calls = []
    many_lev = t.tts_many([HELLO_THERE, HELLO], loudness=-23, limit="none", **kw)
    assert ReferenceLoudnessStage.calls == [("normalize", 2)] and "level_s" in t.timings
    assert all(torch.equal(a, _ref(b, -23.0, limit="none")) for a, b in zip(many_lev, many))
    for call in (lambda **k: t.tts(HELLO_THERE, **k, **kw), lambda **k: t.tts_many([HELLO_THERE], **k, **kw)):
        with pytest.raises(ValueError, match="LUFS is outside"):
            call(loudness=-2)
        with pytest.raises(ValueError, match="dBTP is outside"):
            call(loudness=-23, true_peak=2)
        with pytest.raises(ValueError, match="belong to loudness="):
            call(true_peak=-2)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (other unknown kwargs are refused as before)
        t.tts(HELLO_THERE, loudnes=-23, **kw)


@torch.no_grad()
def test_the_order_is_redaction_rate_level(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    from tests.test_redaction_cpu import _flow_tts
    from tests.test_tsm_cpu import ReferenceStretchStage
    t, _ = _flow_tts(monkeypatch)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    order = []
    redact = t._redact_clips
    t._redact_clips = lambda wavs, text: (order.append("redact"), redact(wavs, text))[1]
    monkeypatch.setattr(ReferenceStretchStage, "stretch_many", lambda self, clips, rqs, f=ReferenceStretchStage.stretch_many: (order.append("rate"), f(self, clips, rqs))[1])
    monkeypatch.setattr(ReferenceLoudnessStage, "normalize_many",
                        lambda self, *a, f=ReferenceLoudnessStage.normalize_many: (order.append("level"), f(self, *a))[1])
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    t.tts("[I am so sad,] hello there", speaking_rate=1.25, loudness=-23, **kw)
    assert order == ["redact", "rate", "level"]
    assert "redact_s" in t.timings and "stretch_s" in t.timings and "level_s" in t.timings


@torch.no_grad()
def test_timings_are_unchanged_by_the_gain(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_api_flow_cpu import voice_latents, small_setup
    t, m = CC._flow(monkeypatch)
    from tortoise_tts_amd import api
    _install(monkeypatch, api)
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    plain, al0 = t.tts_with_timings("hello there", **kw)
    res, al = t.tts_with_timings("hello there", loudness=-23, **kw)
    assert torch.equal(res, _ref(plain, -23.0)) and al.samples == al0.samples == res.shape[-1]
    assert al == CC._expected(m, res, "hello there")


@torch.no_grad()
def test_long_form_scopes(monkeypatch):
    from tests.test_api_flow_cpu import HELLO, HELLO_THERE
    from tortoise_tts_amd import longform
    t, kw = _tts(monkeypatch, candidate_sharding=False)
    kw = dict(conditioning_latents=kw["conditioning_latents"], num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, seed=5,
              texts_are_chunks=True, preset="ultra_fast")
    full, clips = longform.read_long_form(t, [HELLO_THERE, HELLO], **kw)
    assert ReferenceLoudnessStage.calls == []
    lfull, lclips = longform.read_long_form(t, [HELLO_THERE, HELLO], loudness=-19, **kw)
    assert ReferenceLoudnessStage.calls == [("normalize", 2)]  # every chunk of the rank in ONE call
    assert all(torch.equal(a, _ref(b, -19.0)) for a, b in zip(lclips, clips)) and torch.equal(lfull, torch.cat([c.squeeze(0) for c in lclips], dim=-1))
    ReferenceLoudnessStage.calls = []
    wfull, wclips = longform.read_long_form(t, [HELLO_THERE, HELLO], loudness=-19, true_peak=-3, loudness_scope="whole", **kw)
    assert ReferenceLoudnessStage.calls == [("normalize", 1)]  # one gain for the concatenation
    assert torch.equal(wfull, _ref(full, -19.0, -3.0)) and [c.shape for c in wclips] == [c.shape for c in clips]
    assert torch.equal(torch.cat([c.squeeze(0) for c in wclips], dim=-1), wfull)
    with pytest.raises(ValueError, match="loudness_scope"):
        longform.read_long_form(t, [HELLO], loudness=-19, loudness_scope="book", **kw)


@torch.no_grad()
def test_fast_path_level_and_streaming_refusals(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    _install(monkeypatch, api_fast)
    one = make(1)
    kw = dict(max_mel_tokens=24, use_deterministic_seed=41)
    plain = one.tts(TEXTS[0], **kw)
    assert torch.equal(one.tts(TEXTS[0], loudness=None, **kw), plain) and ReferenceLoudnessStage.made == [] and one.leveller is None
    assert torch.equal(one.tts(TEXTS[0], loudness=-19, **kw), _ref(plain, -19.0)) and ReferenceLoudnessStage.calls == [("normalize", 1)]
    both = one.tts_many(TEXTS[:2], **kw)
    ReferenceLoudnessStage.calls = []
    assert all(torch.equal(a, _ref(b, -23.0, -6.0)) for a, b in zip(one.tts_many(TEXTS[:2], loudness=-23, true_peak=-6, **kw), both))
    assert ReferenceLoudnessStage.calls == [("normalize", 2)]
    # an integrated loudness needs the whole clip: no level on streamed audio
    with pytest.raises(ValueError, match="loudness is not available for streamed audio .an integrated loudness needs the whole clip"):
        next(one.tts_stream(TEXTS[0], loudness=-19, **KW))
    many = make(3)
    with pytest.raises(ValueError, match="loudness is not available"):
        many.open_stream(TEXTS[0], loudness=-19, **KW)
    with pytest.raises(ValueError, match="loudness is not available"):
        next(many.tts_stream_many(TEXTS[:2], true_peak=-2, **KW))
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.LoudnessStage)  # (no handle: the checks come before any device work)
    st.h = None
    st.max_total_samples, st.max_clips = 1000, 16
    with pytest.raises(ValueError, match="1001 samples"):
        st.measure_many([torch.zeros(1001)])
    with pytest.raises(ValueError, match="at least one sample"):
        st.normalize_many([torch.zeros(0)], [-23.0], [0.9], E.LOUD_SCALE)
    with pytest.raises(ValueError, match="positive linear ceiling"):
        st.normalize_many([torch.zeros(10)], [-23.0], [0.0], E.LOUD_SCALE)
    with pytest.raises(ValueError, match="mode 3"):
        st.normalize_many([torch.zeros(10)], [-23.0], [0.9], 3)
    with pytest.raises(ValueError, match="2 clips with 1 targets"):
        st.normalize_many([torch.zeros(10), torch.zeros(10)], [-23.0], [0.9, 0.9], E.LOUD_SCALE)
