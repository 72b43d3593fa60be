"""The resampler along a pitch map on the MI355X (csrc/resample_warp.hip, include/tortoise_mi355x_rsw.h) against the whole-clip kernel and
the fp64 reference of tests/pitchmap_reference.py.

  1. the table (0, 0, 0, P) gives tt_rs_resample(P, 65536)'s bits, samples and peak;
  2. every sample of every clip of the map family inside the reference's f32 bound (the worst share of the bound is printed), and the peak
     the maximum of the device's own output exactly;
  3. ragged batches bit-identical to solo calls; 4. a clip that is not OK gets its status and nothing else;
  5. the interface: shift_pitch(pitch_map=), tts_with_timings(word_pitches=).
Every clip is at most 5000 samples (two or three tiles of 1024 outputs)."""
import numpy as np
import pytest
import torch

from tests import pitchmap_reference as M
from tests import resample_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0        # what every output holds before the call
MAX_SAMPLES = 5000

_stage = []


def stage():
    if not _stage:
        _stage.append(stages.WarpResampleStage(MAX_SAMPLES, max_clips=32, device=DEV))
    return _stage[0]


def device_resample(clips, spans=None):
    """One tt_rsw_resample call over clips = [(x f32 [n], table rows)] with every output pre-filled with SENT -> per clip the raw status, y
    and peak (SENT where the call wrote nothing).  A table is passed as it is, rule-breaking or not, with any number of rows; spans: per
    clip the entries of out where they are not the table's own integer."""
    st = stage()
    n = len(clips)
    spans = spans or [None] * n
    spans = [M.out_samples(len(x), tb) if s is None else s for s, (x, tb) in zip(spans, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x, _ in clips]))).astype(np.int32)
    so = np.concatenate(([0], np.cumsum([len(tb) for _, tb in clips]))).astype(np.int32)
    oo = np.concatenate(([0], np.cumsum(spans))).astype(np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _ in clips] + [np.zeros(1, np.float32)])).to(DEV)
    seg = torch.tensor([v for _, tb in clips for row in tb for v in row] + [0, 0, 0, 0], dtype=torch.int32, device=DEV)
    io_d, so_d, oo_d = (torch.from_numpy(a).to(DEV) for a in (io, so, oo))
    y = torch.full((int(oo[-1]) + 1,), SENT, device=DEV)
    peak = torch.full((n,), SENT, device=DEV)
    status = torch.full((n,), int(SENT), dtype=torch.int32, device=DEV)
    E.check(st.lib.tt_rsw_resample(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(seg), E.ptr(so_d), E.ptr(y), E.ptr(oo_d), E.ptr(peak), E.ptr(status),
                                   E.stream_ptr()))
    y, peak, status = (t.cpu().numpy() for t in (y, peak, status))
    assert y[oo[-1]] == SENT  # nothing beyond the batch
    return [dict(status=int(status[i]), y=y[oo[i]:oo[i + 1]], peak=peak[i:i + 1]) for i in range(n)]


def untouched(r):
    return (r["y"] == SENT).all() and r["peak"][0] == SENT


def same(a, b):
    return a["status"] == b["status"] and a["y"].tobytes() == b["y"].tobytes() and a["peak"].tobytes() == b["peak"].tobytes()


@pytest.fixture(scope="module")
def solo():
    return [device_resample([(x, table)])[0] for _, x, table, _, _ in M.family_reference()]


# ----------------------------------------------------------------------------------------- 1. the constant ratio
def test_one_segment_gives_the_whole_clip_kernel_s_bits():
    const = stages.ResampleStage(MAX_SAMPLES, max_clips=32, device=DEV)
    cases = [(R.clip(n, 4), P) for n in (1, 37, 1000, 5000) for P in (32768, 55109, 65536, 77936, 131072)]
    want = const.resample_many([torch.from_numpy(x) for x, _ in cases], [(P, 65536) for _, P in cases])
    got = device_resample([(x, [(0, 0, 0, P)]) for x, P in cases])  # one ragged call of 20 clips
    for (x, P), (y, pk), g in zip(cases, want, got):
        assert g["status"] == E.RSW_OK and g["y"].shape == (R.out_samples(len(x), P, 65536),)
        assert np.array_equal(g["y"].view(np.int32), y.cpu().numpy().view(np.int32)), (len(x), P)
        assert np.array_equal(g["peak"].view(np.int32), np.asarray([pk], np.float32).view(np.int32)), (len(x), P)
    const.close()


# ----------------------------------------------------------------------------------------- 2. the map family
def test_family_inside_the_fp64_bound_and_the_peak_is_exact(solo):
    fam = M.family_reference()
    assert len(solo) == len(fam) >= 20
    worst, where = 0.0, None
    for r, (name, x, table, y, b) in zip(solo, fam):
        assert r["status"] == E.RSW_OK and r["y"].shape == y.shape, name
        share = np.abs(r["y"].astype(np.float64) - y) / b
        print(f"[parity] tt_rsw_resample {name}: n {len(x)}, {len(table)} segments, {len(y)} outputs, worst |err| / bound {share.max():.3f}")
        assert (share <= 1.0).all(), (name, int(share.argmax()), float(share.max()))
        assert r["peak"].view(np.int32)[0] == np.abs(r["y"]).max().view(np.int32), name  # the maximum of the device's own output
        if share.max() > worst:
            worst, where = float(share.max()), name
    print(f"[parity] tt_rsw_resample family: {len(fam)} clips, worst share of the fp64 bound {worst:.3f} ({where})")


# ----------------------------------------------------------------------------------------- 3. ragged batches
def test_a_ragged_batch_of_16_is_bit_identical_to_solo(solo):
    fam = M.family_reference()
    for seed in (1, 2):
        idx = np.random.default_rng(seed).permutation(len(fam))[:16]
        assert len({tuple(fam[i][2]) for i in idx}) == 16  # sixteen different tables
        batch = device_resample([(fam[i][1], fam[i][2]) for i in idx])
        assert all(same(r, solo[i]) for r, i in zip(batch, idx)), seed


# ----------------------------------------------------------------------------------------- 4. refusals
GOOD = M.plan(3000, [(0, 81920), (1000, 52429), (1700, 131072)])


def _edit(at, v):
    return [tuple(v if 4 * i + j == at else GOOD[i][j] for j in range(4)) for i in range(3)]


BAD_TABLES = {
    "start_m_not_0": _edit(0, 1), "start_thi_not_0": _edit(1, 1), "start_tlo_not_0": _edit(2, 1),
    "m_not_increasing": _edit(8, GOOD[1][0]), "m_decreasing": _edit(4, -5),
    "continuity_thi_plus_1": _edit(5, GOOD[1][1] + 1), "continuity_tlo_minus_1": _edit(10, (GOOD[2][2] - 1) % 65536),
    "tlo_negative": _edit(6, GOOD[1][2] - 65536), "tlo_65536": _edit(6, GOOD[1][2] + 65536), "thi_negative": _edit(9, -1),
    "ratio_below": _edit(7, M.P_MIN - 1), "ratio_above": _edit(11, M.P_MAX + 1), "ratio_zero": _edit(3, 0), "ratio_negative": _edit(3, -65536),
    "no_segments": [], "too_many_segments": M.plan(3000, [(40 * i, 65536) for i in range(64)]) + [(1, 1, 0, 65536)],
}
BAD = sorted(BAD_TABLES) + ["t_last_at_n", "wrong_out_span_short", "wrong_out_span_long", "empty", "too_long"]


@pytest.mark.parametrize("name", BAD)
def test_a_clip_that_is_not_ok_gets_its_status_and_nothing_else(name, solo):
    x, span, status = R.clip(3000, 5), M.out_samples(3000, GOOD), E.RSW_REFUSED
    if name in BAD_TABLES:
        table = BAD_TABLES[name]
        assert M.out_samples(3000, table) == 0
    elif name == "t_last_at_n":
        x, table = x[:GOOD[2][1]], GOOD  # t_(S-1) >= n 65536
    elif name == "wrong_out_span_short":
        table, span = GOOD, span - 1
    elif name == "wrong_out_span_long":
        table, span = GOOD, span + 1
    elif name == "empty":
        x, table, span, status = np.zeros(0, np.float32), [(0, 0, 0, 65536)], 5, E.RSW_EMPTY
    else:
        x, table, span = R.clip(MAX_SAMPLES + 1, 5), [(0, 0, 0, 65536)], MAX_SAMPLES + 1
    fam = M.family_reference()
    a, b = 1, len(fam) - 3
    res = device_resample([(fam[a][1], fam[a][2]), (x, table), (fam[b][1], fam[b][2])], spans=[None, span, None])
    assert res[1]["status"] == status and untouched(res[1])
    assert same(res[0], solo[a]) and same(res[2], solo[b])  # the neighbours: untouched by it, and correct (the family test)


def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(8, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    for n in (0, 33):
        assert st.lib.tt_rsw_resample(st.h, n, E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(y), E.ptr(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert st.lib.tt_rsw_resample(st.h, 1, E.ptr(y), None, E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(y), E.ptr(i), E.stream_ptr()) == -1
    assert b"null argument" in st.lib.tt_last_error()
    # peak may be NULL: the samples are the same
    x, table = R.clip(1000, 7), M.plan(1000, [(0, 77936), (500, 55109)])
    n_out = M.out_samples(1000, table)
    ints = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    out, stt = torch.full((n_out + 1,), SENT, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV)
    xd, io, seg, so, oo = torch.from_numpy(x).to(DEV), ints([0, 1000]), ints([v for r in table for v in r]), ints([0, 2]), ints([0, n_out])
    E.check(st.lib.tt_rsw_resample(st.h, 1, E.ptr(xd), E.ptr(io), E.ptr(seg), E.ptr(so), E.ptr(out), E.ptr(oo), None, E.ptr(stt), E.stream_ptr()))
    assert int(stt[0]) == E.RSW_OK and out[:n_out].cpu().numpy().tobytes() == device_resample([(x, table)])[0]["y"].tobytes() and float(out[n_out]) == SENT


# ----------------------------------------------------------------------------------------- 5. the interface
@torch.no_grad()
def test_shift_pitch_along_a_map_through_the_api():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    x = torch.from_numpy(R.clip(5000, 0).copy())
    pm = rs.PitchMap.from_segments(5000, [(0, 0), (1500, 3), (3000, -2), (4200, 12)])
    chain = rs.WarpChain(5000, pm.starts, [65536] * 4, pm.pqs)
    y, a = h.shift_pitch(x, pitch_map=pm, return_map=True)
    assert y.device.type == "cpu" and y.shape == (chain.n_out,) and torch.equal(a, chain.anchors)
    for i in range(1, 5):  # the length and every border within the derived bound of where they were
        assert abs(int(a[i, 1]) - int(a[i, 0])) <= rs.duration_bound(i, int(a[i, 0]))
    # the stretch and resample stages called by hand on the same tables: bit for bit
    mid = h.load_warp_stretch().stretch_many([x], [chain.stretch])[0][0]
    assert mid.shape == (chain.n_mid,)
    want = h.load_warp_resample().resample_many([mid], [chain.resample])[0][0]
    assert torch.equal(y.view(torch.int32), want.cpu().view(torch.int32))
    # one segment: the path (and the bits) of semitones=; 0 throughout: the clip itself
    assert torch.equal(h.shift_pitch(x, pitch_map=[(0, 3)]).view(torch.int32), h.shift_pitch(x, 3).view(torch.int32))
    assert h.shift_pitch(x, pitch_map=[(0, 0), (0.1, 0)]) is x
    # clips on the device, a map each
    out = h.shift_pitch_many([x.to(DEV).reshape(1, 1, -1), x[:1000].to(DEV)], pitch_maps=[pm, [(0, -12), (0.02, 12)]])
    assert out[0].device.type == "cuda" and out[0].shape[:2] == (1, 1) and torch.equal(out[0].cpu().reshape(-1).view(torch.int32), y.view(torch.int32))
    assert out[1].shape[-1] == rs.WarpChain(1000, [0, 480], [65536] * 2, [32768, 131072]).n_out
    assert h.warp_resampler.max_samples == 2 * 30 * 24000 and h.warp_resampler.max_clips == 16


@pytest.fixture(scope="module")
def tts():
    import bench
    from tests import w2v_reference as W
    from tests.test_gpu_ctc import _IdsTokenizer
    from tortoise_tts_amd.api import TextToSpeech
    cfg = W.small_config()
    model = W.hf_model(cfg, seed=5)
    src = (cfg, {k: v.detach().cpu() for k, v in model.state_dict().items()}, W.VOCAB, W.TOK_CFG)
    t = TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48, aligner=src)
    t._tokenizer = _IdsTokenizer(bench.synthetic_prompt()[0].tolist())
    return t


@torch.no_grad()
def test_word_pitches_on_tts_with_timings(tts):
    from tortoise_tts_amd import align
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    text = "hello there"
    plain, al0 = tts.tts_with_timings(text, **kw)
    same_, al1 = tts.tts_with_timings(text, word_pitches=[0, None], **kw)
    assert torch.equal(same_, plain) and repr(al1) == repr(al0) and tts.warp_resampler is None  # the plain call's bits, no stage
    word = max(range(len(al0.words)), key=lambda i: al0.words[i][2] - al0.words[i][1])
    assert al0.words[word][2] - al0.words[word][1] >= 4, "the synthetic clip has a word with a span"
    up, al = tts.tts_with_timings(text, word_pitches={word: 2}, **kw)
    pm = tts.pitch_maps[0]
    assert pm.table == rs.PitchMap.from_words(al0, {word: 2}).table and len(pm.starts) >= 2 and tts.timings["pitch_s"] > 0
    assert isinstance(al, align.Alignment) and al.samples == up.shape[-1]
    assert torch.equal(up, tts.shift_pitch(plain, pitch_map=pm))
    assert abs(up.shape[-1] - plain.shape[-1]) <= rs.duration_bound(len(pm.starts), plain.shape[-1])
    again, _ = tts.tts_with_timings(text, **kw)
    assert torch.equal(again, plain)  # without the keyword, the plain call's bits
