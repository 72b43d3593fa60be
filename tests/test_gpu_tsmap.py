"""The WSOLA time-stretch along a rate map on the MI355X (csrc/tsm_warp.hip, include/tortoise_mi355x_tsw.h) against the constant-rate kernel
and the fp64 reference of tests/tsmap_reference.py.

  1. the table (0, 0, rq) gives tt_tsm_stretch's bits;
  2. tests/test_gpu_tsm.py's protocol on the map family: every device choice admissible against the device's own history, every output
     sample inside the 4 u bound of the fp64 overlap-add of the device's offsets, and on the clips whose every frame the reference finds
     unambiguous (at least 50 % of the family: tests/test_tsmap_cpu.py) the offsets equal the reference's exactly;
  3. the edges of a table; 4. ragged batches bit-identical to solo calls; 5. a clip that is not OK gets its status and nothing else;
  6. the interface: stretch(rate_map=), retime, tts_with_timings(word_rates=).
Every clip is at most 12 000 samples."""
import numpy as np
import pytest
import torch

from tests import tsm_reference as T
from tests import tsmap_reference as M
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import stretch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0        # what every output holds before the call
MAX_SAMPLES = 12000

_stage = []


def stage():
    if not _stage:
        _stage.append(stages.WarpStretchStage(MAX_SAMPLES, max_clips=32, device=DEV))
    return _stage[0]


def device_stretch(clips, spans=None):
    """One tt_tsw_stretch call over clips = [(x f32 [n], table rows)] with every output pre-filled with SENT -> per clip the raw status, y and
    offsets (SENT where the call wrote nothing).  A table is passed as it is, rule-breaking or not, with any number of rows; spans: per
    clip (out entries, offsets entries) where they are not the table's own integers."""
    st = stage()
    n = len(clips)
    spans = spans or [None] * n
    spans = [s or (M.out_samples(len(x), tb), M.frames(len(x), tb)) for s, (x, tb) in zip(spans, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x, _ in clips]))).astype(np.int32)
    so = np.concatenate(([0], np.cumsum([len(tb) for _, tb in clips]))).astype(np.int32)
    oo = np.concatenate(([0], np.cumsum([s[0] for s in spans]))).astype(np.int32)
    fo = np.concatenate(([0], np.cumsum([s[1] for s in spans]))).astype(np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _ in clips] + [np.zeros(1, np.float32)])).to(DEV)
    seg = torch.tensor([v for _, tb in clips for row in tb for v in row] + [0, 0, 0], dtype=torch.int32, device=DEV)
    io_d, so_d, oo_d, fo_d = (torch.from_numpy(a).to(DEV) for a in (io, so, oo, fo))
    y = torch.full((int(oo[-1]) + 1,), SENT, device=DEV)
    off = torch.full((int(fo[-1]) + 1,), int(SENT), dtype=torch.int32, device=DEV)
    status = torch.full((n,), int(SENT), dtype=torch.int32, device=DEV)
    E.check(st.lib.tt_tsw_stretch(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(seg), E.ptr(so_d), E.ptr(y), E.ptr(oo_d), E.ptr(off), E.ptr(fo_d),
                                  E.ptr(status), E.stream_ptr()))
    y, off, status = (t.cpu().numpy() for t in (y, off, status))
    assert y[oo[-1]] == SENT and off[fo[-1]] == SENT  # nothing beyond the batch
    return [dict(status=int(status[i]), y=y[oo[i]:oo[i + 1]], offsets=off[fo[i]:fo[i + 1]]) for i in range(n)]


def untouched(r):
    return (r["y"] == SENT).all() and (r["offsets"] == SENT).all()


def same(a, b):
    return a["status"] == b["status"] and a["y"].tobytes() == b["y"].tobytes() and a["offsets"].tobytes() == b["offsets"].tobytes()


def verify(results, fam, what, least=0.0):
    """Steps 1 - 3 of the protocol over [(x, table, reference or None)] -> the worst shares of the two bounds used."""
    assert len(results) == len(fam)
    worst = dict(score=0.0, y=0.0)
    exact = 0
    for r, (x, table, ref) in zip(results, fam):
        assert r["status"] == E.TSW_OK, (len(x), table, r["status"])
        c = M.check(x, table, r["y"], r["offsets"])
        worst["score"], worst["y"] = max(worst["score"], c["score_share"]), max(worst["y"], c["y_share"])
        assert not c["inadmissible"] and not c["bad_samples"], (len(x), table, c)
        if ref is not None and ref["unambiguous"].all():
            assert np.array_equal(r["offsets"], ref["offsets"]), (len(x), table)
            exact += 1
    assert exact >= least * len(fam)
    print(f"[parity] tt_tsw_stretch {what}: {len(fam)} clips, {exact} unambiguous with offsets equal to fp64; worst share of the score bound used "
          f"by a choice {worst['score']:.3f}, of the sample bound {worst['y']:.3f}")
    return worst


@pytest.fixture(scope="module")
def solo():
    return [device_stretch([(x, table)])[0] for x, table, _ in M.family_reference()]


# ----------------------------------------------------------------------------------------- 1. the constant rate
def test_one_segment_gives_the_constant_rate_kernel_s_bits():
    const = stages.TimeStretchStage(MAX_SAMPLES, max_clips=32, device=DEV)
    cases = [(T.clip(n, 4), T.rate_q(r)) for n in (1, 768, 769, 5000, 12000) for r in T.RATES]
    want = const.stretch_many([torch.from_numpy(x) for x, _ in cases], [rq for _, rq in cases])
    got = device_stretch([(x, [(0, 0, rq)]) for x, rq in cases])  # one ragged call of 20 clips
    for (x, rq), (y, off), g in zip(cases, want, got):
        assert g["status"] == E.TSW_OK and g["y"].shape == (T.out_samples(len(x), rq),)
        assert np.array_equal(g["y"].view(np.int32), y.cpu().numpy().view(np.int32)), (len(x), rq)
        assert np.array_equal(g["offsets"], off.numpy()), (len(x), rq)
    const.close()


# ----------------------------------------------------------------------------------------- 2. the map family
def test_family_solo(solo):
    verify(solo, M.family_reference(), "solo", least=0.5)


# ----------------------------------------------------------------------------------------- 3. edges
def _edge_cases():
    q = M.rq_of
    rng = np.random.default_rng(77)
    cases = {
        "n4_two_segments_of_2": (T.clip(4, 1), [(0, q(0.5)), (2, q(2.0))]),
        "n128_64_segments_of_2": (T.clip(128, 1), [(2 * i, int(rng.integers(T.RATE_MIN, T.RATE_MAX + 1))) for i in range(64)]),
        "64_segments_shorter_than_a_hop": (T.clip(6400, 2), [(100 * i, q((0.5, 2.0, 1.0, 0.7)[i % 4])) for i in range(64)]),
        "border_at_2_hops": (T.clip(3000, 3), [(0, q(1.0)), (2 * T.HS, q(0.5))]),
        "border_at_2_hops_minus_1": (T.clip(3000, 3), [(0, q(1.0)), (2 * T.HS - 1, q(0.5))]),
        "border_at_2_hops_plus_1": (T.clip(3000, 3), [(0, q(1.0)), (2 * T.HS + 1, q(2.0))]),
        "last_segment_of_2": (T.clip(2400, 4), [(0, q(0.8)), (2398, q(2.0))]),
        "fast_slow_across_both_ends": (T.clip(900, 5), [(0, q(2.0)), (450, q(0.5))]),
        "slow_fast_across_both_ends": (T.clip(900, 5), [(0, q(0.5)), (450, q(2.0))]),
        "fast_slow_at_the_end": (T.clip(5000, 6), [(0, q(1.0)), (4600, q(2.0)), (4800, q(0.5))]),
        "slow_fast_at_the_start": (T.clip(5000, 6), [(0, q(0.5)), (100, q(2.0)), (300, q(0.5))]),
    }
    return {name: (x, M.plan(len(x), segs)) for name, (x, segs) in cases.items()}


def test_edges_of_a_table():
    cases = _edge_cases()
    fam = [(x, table, M.stretch(x, table)) for x, table in cases.values()]
    assert fam[0][1] == [(0, 0, 32768), (4, 2, 131072)] and len(fam[1][1]) == len(fam[2][1]) == 64
    assert [fam[i][1][1][0] for i in (3, 4, 5)] == [2 * T.HS, 2 * T.HS - 1, 2 * T.HS + 1]  # the border in the output: at a frame's start, one before, one after
    assert fam[2][1][1][0] < T.HS  # segments that own no frame
    results = [device_stretch([(x, table)])[0] for x, table, _ in fam]
    verify(results, fam, "edges")
    batch = device_stretch([(x, table) for x, table, _ in fam])
    assert all(same(a, b) for a, b in zip(batch, results))


# ----------------------------------------------------------------------------------------- 4. ragged batches
def _batched(size, seed):
    fam = M.family_reference()
    order = np.random.default_rng(seed).permutation(len(fam))
    out = [None] * len(fam)
    for g in range(0, len(fam), size):
        idx = order[g:g + size]
        for i, r in zip(idx, device_stretch([(fam[i][0], fam[i][1]) for i in idx])):
            out[i] = r
    return out


def test_ragged_batches_are_bit_identical_to_solo(solo):
    for size, seed in ((17, 1), (2, 2), (1, 3)):
        assert all(same(a, b) for a, b in zip(_batched(size, seed), solo)), size


# ----------------------------------------------------------------------------------------- 5. refusals
def _bad_tables():
    x = T.clip(3000, 5)
    good = M.plan(3000, [(0, 81920), (1000, 52429), (1700, 131072)])
    span = (M.out_samples(3000, good), M.frames(3000, good))
    edit = lambda at, v: [tuple(v if 3 * i + j == at else good[i][j] for j in range(3)) for i in range(3)]
    return x, good, span, {
        "start_m_not_0": edit(0, 1), "start_a_not_0": edit(1, 1), "m_not_increasing": edit(6, good[1][0]), "m_decreasing": edit(3, -5),
        "continuity_plus_1": edit(4, good[1][1] + 1), "continuity_minus_1": edit(7, good[2][1] - 1),
        "rate_below": edit(5, T.RATE_MIN - 1), "rate_above": edit(8, T.RATE_MAX + 1), "rate_zero": edit(2, 0), "rate_negative": edit(2, -65536),
        "no_segments": [], "too_many_segments": M.plan(3000, [(40 * i, 65536) for i in range(64)]) + [(1, 1, 65536)],
    }


BAD = ["start_m_not_0", "start_a_not_0", "m_not_increasing", "m_decreasing", "continuity_plus_1", "continuity_minus_1", "rate_below", "rate_above",
       "rate_zero", "rate_negative", "no_segments", "too_many_segments", "a_last_at_n", "wrong_out_span", "wrong_frame_span", "empty", "too_long"]


@pytest.mark.parametrize("name", BAD)
def test_a_clip_that_is_not_ok_gets_its_status_and_nothing_else(name, solo):
    x, good, span, tables = _bad_tables()
    status = E.TSW_REFUSED
    if name in tables:
        table = tables[name]
    elif name == "a_last_at_n":
        x, table = x[:good[2][1]], good  # a_(S-1) = n
    elif name == "wrong_out_span":
        table, span = good, (span[0] - 1, span[1])
    elif name == "wrong_frame_span":
        table, span = good, (span[0], span[1] + 1)
    elif name == "empty":
        x, table, span, status = np.zeros(0, np.float32), [(0, 0, 65536)], (5, 3), E.TSW_EMPTY
    else:
        x, table = T.clip(MAX_SAMPLES + 1, 5), [(0, 0, 65536)]
        span = (MAX_SAMPLES + 1, T.frames(MAX_SAMPLES + 1, 65536))
    assert set(BAD) == set(tables) | {"a_last_at_n", "wrong_out_span", "wrong_frame_span", "empty", "too_long"}
    fam = M.family_reference()
    a, b = 1, 20
    res = device_stretch([(fam[a][0], fam[a][1]), (x, table), (fam[b][0], fam[b][1])], spans=[None, span, None])
    assert res[1]["status"] == status and untouched(res[1])
    assert same(res[0], solo[a]) and same(res[2], solo[b])  # the neighbours: untouched by it, and correct (test_family_solo)


def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(8, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    for n in (0, 33):
        assert st.lib.tt_tsw_stretch(st.h, n, E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert st.lib.tt_tsw_stretch(st.h, 1, E.ptr(y), None, E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(i), E.stream_ptr()) == -1
    assert b"null argument" in st.lib.tt_last_error()


# ----------------------------------------------------------------------------------------- 6. the interface
@torch.no_grad()
def test_stretch_along_a_map_and_retime_through_the_api(solo):
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    fam = M.family_reference()
    x = torch.from_numpy(T.clip(9001, 0).copy())
    for rate in (0.5, 1.25):  # a map of one segment: the constant rate's bits, through either form of the map
        want = h.stretch(x, rate=rate)
        for rm in (stretch.RateMap.from_segments(9001, [(0, rate)]), [(0.0, rate)]):
            got = h.stretch(x, rate_map=rm)
            assert got.device.type == "cpu" and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # more clips than one call takes (16), a map each: every clip the bits of its solo call, and its anchors those of its offsets
    pick = list(range(0, len(fam), 3))
    maps = [stretch.RateMap(len(fam[i][0]), [b for b, _ in M.FAMILY_SEGMENTS[i]], [rq for _, rq in M.FAMILY_SEGMENTS[i]]) for i in pick]
    assert len(pick) > 16 and all(m.table == fam[i][1] for m, i in zip(maps, pick))
    out, anchors = h.stretch_many([torch.from_numpy(fam[i][0].copy()).reshape(1, 1, -1).to(DEV) for i in pick], rate_maps=maps, return_map=True)
    for i, o, a in zip(pick, out, anchors):
        assert o.device.type == "cuda" and o.shape[:2] == (1, 1) and o.cpu().numpy().tobytes() == solo[i]["y"].tobytes()
        assert a[:, 1].tolist() == M.positions(fam[i][1], solo[i]["offsets"]).tolist()
    assert h.warp_stretcher.max_samples == 30 * 24000 and h.warp_stretcher.max_clips == 16
    # retime: the plan lands within its bound of every anchor, and the frames within the search range of the plan
    pts = [(0.08, 0.12), (0.2, 0.2), (0.3, 0.36)]
    y, a = h.retime(x, anchors=pts, duration=0.42, return_map=True)
    rm = stretch.RateMap.from_anchors(9001, [(round(s * 24000), round(d * 24000)) for s, d in pts] + [(9001, 10080)])
    assert y.shape == (rm.n_out,) and a.shape == (rm.frames, 2)
    ms = [row[0] for row in rm.table[1:]] + [rm.n_out]
    for i, (m, dst) in enumerate(zip(ms, (2880, 4800, 8640, 10080))):
        assert abs(m - dst) <= (dst - rm.table[i][0]) / 65536 + 1
    for k in range(1, rm.frames):
        assert int(a[k, 0]) == (k - 1) * T.HS and abs(int(a[k, 1]) - stretch.table_nominal(k, rm.table)) <= 256 + 1
    c = M.check(x.numpy(), rm.table, y.numpy(), (a[:, 1] - torch.tensor([-T.HS] + [stretch.table_nominal(k, rm.table) for k in range(1, rm.frames)])).numpy())
    assert not c["inadmissible"] and not c["bad_samples"]
    with pytest.raises(ValueError, match="need rate"):
        h.retime(x, duration=1.0)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tests import w2v_reference as R
    from tests.test_gpu_ctc import _IdsTokenizer
    from tortoise_tts_amd.api import TextToSpeech
    cfg = R.small_config()
    model = R.hf_model(cfg, seed=5)
    src = (cfg, {k: v.detach().cpu() for k, v in model.state_dict().items()}, R.VOCAB, R.TOK_CFG)
    t = TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48, aligner=src)
    t._tokenizer = _IdsTokenizer(bench.synthetic_prompt()[0].tolist())
    return t


@torch.no_grad()
def test_word_rates_on_tts_with_timings(tts):
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    text = "hello there"
    plain, al0 = tts.tts_with_timings(text, **kw)
    same_, al1 = tts.tts_with_timings(text, word_rates=[1.0, 1.0], **kw)
    assert torch.equal(same_, plain) and repr(al1) == repr(al0) and tts.warp_stretcher is None  # today's bits, no stage
    word = max(range(len(al0.words)), key=lambda i: al0.words[i][2] - al0.words[i][1])
    span = al0.words[word][2] - al0.words[word][1]
    assert span >= 2, "the synthetic clip has a word with a span"
    slow, al = tts.tts_with_timings(text, word_rates={word: 0.5}, **kw)
    rm = tts.rate_maps[0]
    assert rm.table == stretch.RateMap.from_words(al0, {word: 0.5}).table and tts.timings["stretch_s"] > 0
    assert torch.equal(slow, tts.stretch(plain, rate_map=rm)) and al.samples == slow.shape[-1] == rm.n_out
    assert abs(slow.shape[-1] - plain.shape[-1] - span) <= 2  # longer by about that word's span
    # with a base rate and a pitch: ONE stretch along the folded map and ONE resampling
    both, _ = tts.tts_with_timings(text, word_rates={word: 0.8}, speaking_rate=1.25, pitch=2, **kw)
    from tortoise_tts_amd import resample as rs
    pq = rs.pitch(2)[0]
    eff = stretch.RateMap.from_words(al0, {word: 0.8}, base=1.25).with_pitch(pq)
    want = tts._resample_ratios([tts.stretch(plain, rate_map=eff)], [(pq, 65536)], False)[0]
    assert torch.equal(both, want)
