"""The WSOLA time-stretch on the MI355X (csrc/tsm.hip, include/tortoise_mi355x_tsm.h) against the fp64 reference of tests/tsm_reference.py.

The protocol (near-ties are real: voiced speech correlates almost as well one pitch period further):
  1. every frame against the device's own history: with p_(k-1) from the device's offsets, the device's choice must be admissible;
  2. every output sample against the fp64 overlap-add of the device's offsets, inside the sample bound;
  3. on the clips whose every frame the reference finds unambiguous (at least 40 % of the family: tests/test_tsm_cpu.py), the offsets equal
     the reference's exactly.
Ragged batches are bit-identical to solo calls, a clip that is not OK gets its status and nothing else, and the API end to end."""
import numpy as np
import pytest
import torch

from tests import tsm_reference as T
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0        # what every output holds before the call
MAX_SAMPLES = 12000

_stage = []


def stage():
    if not _stage:
        _stage.append(stages.TimeStretchStage(MAX_SAMPLES, max_clips=32, device=DEV))
    return _stage[0]


def device_stretch(clips, spans=None):
    """One tt_tsm_stretch call over clips = [(x f32 [n], rq)] with every output pre-filled with SENT -> per clip the raw status, y and offsets
    (SENT where the call wrote nothing).  spans: per clip (out entries, offsets entries) where they are not the reference's integers."""
    st = stage()
    n = len(clips)
    spans = spans or [None] * n
    spans = [s or (T.out_samples(len(x), rq), T.frames(len(x), rq)) for s, (x, rq) in zip(spans, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x, _ in clips]))).astype(np.int32)
    oo = np.concatenate(([0], np.cumsum([s[0] for s in spans]))).astype(np.int32)
    fo = np.concatenate(([0], np.cumsum([s[1] for s in spans]))).astype(np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _ in clips] + [np.zeros(1, np.float32)])).to(DEV)
    io_d, oo_d, fo_d = (torch.from_numpy(a).to(DEV) for a in (io, oo, fo))
    rq_d = torch.tensor([rq for _, rq in clips], dtype=torch.int32, device=DEV)
    y = torch.full((int(oo[-1]) + 1,), SENT, device=DEV)
    off = torch.full((int(fo[-1]) + 1,), int(SENT), dtype=torch.int32, device=DEV)
    status = torch.full((n,), int(SENT), dtype=torch.int32, device=DEV)
    E.check(st.lib.tt_tsm_stretch(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(rq_d), E.ptr(y), E.ptr(oo_d), E.ptr(off), E.ptr(fo_d), E.ptr(status),
                                  E.stream_ptr()))
    y, off, status = (t.cpu().numpy() for t in (y, off, status))
    assert y[oo[-1]] == SENT and off[fo[-1]] == SENT  # nothing beyond the batch
    return [dict(status=int(status[i]), y=y[oo[i]:oo[i + 1]], offsets=off[fo[i]:fo[i + 1]]) for i in range(n)]


def untouched(r):
    return (r["y"] == SENT).all() and (r["offsets"] == SENT).all()


def same(a, b):
    return a["status"] == b["status"] and a["y"].tobytes() == b["y"].tobytes() and a["offsets"].tobytes() == b["offsets"].tobytes()


def verify(results, what):
    """Steps 1 - 3 over the family -> the worst shares of the two bounds used."""
    fam = T.family_reference()
    assert len(results) == len(fam)
    worst = dict(score=0.0, y=0.0)
    exact = 0
    for r, (x, rq, ref) in zip(results, fam):
        assert r["status"] == E.TSM_OK
        c = T.check(x, rq, r["y"], r["offsets"])
        worst["score"], worst["y"] = max(worst["score"], c["score_share"]), max(worst["y"], c["y_share"])
        assert not c["inadmissible"] and not c["bad_samples"], (len(x), rq, c)
        if ref["unambiguous"].all():
            assert np.array_equal(r["offsets"], ref["offsets"]), (len(x), rq)
            exact += 1
    assert exact >= 0.4 * len(fam)
    print(f"[parity] tt_tsm_stretch {what}: {len(fam)} clips, {exact} unambiguous with offsets equal to fp64; worst share of the score bound used "
          f"by a choice {worst['score']:.3f}, of the sample bound {worst['y']:.3f}")
    return worst


@pytest.fixture(scope="module")
def solo():
    return [device_stretch([(x, rq)])[0] for x, rq, _ in T.family_reference()]


def _batched(size, seed):
    """The family in shuffled order in calls of `size` clips (rates mixed within a call) -> results in the family's order."""
    fam = T.family_reference()
    order = np.random.default_rng(seed).permutation(len(fam))
    out = [None] * len(fam)
    for g in range(0, len(fam), size):
        idx = order[g:g + size]
        for i, r in zip(idx, device_stretch([(fam[i][0], fam[i][1]) for i in idx])):
            out[i] = r
    return out


def test_family_solo(solo):
    verify(solo, "solo")


def test_family_ragged_batches_of_17(solo):
    ragged = _batched(17, 1)
    verify(ragged, "ragged batches of 17")
    assert all(same(a, b) for a, b in zip(ragged, solo))  # bit-identical to the solo calls


def test_family_in_pairs_is_bit_identical_to_solo(solo):
    assert all(same(a, b) for a, b in zip(_batched(2, 2), solo))
    assert all(same(a, b) for a, b in zip(_batched(1, 3), solo))


BAD = {
    "empty": (np.zeros(0, np.float32), 65536, E.TSM_EMPTY, (5, 3)),
    "too_long": (T.clip(MAX_SAMPLES + 1, 5), 65536, E.TSM_REFUSED, None),
    "rate_below": (T.clip(900, 5), T.RATE_MIN - 1, E.TSM_REFUSED, (900, 4)),
    "rate_above": (T.clip(900, 5), T.RATE_MAX + 1, E.TSM_REFUSED, (900, 4)),
    "rate_zero": (T.clip(900, 5), 0, E.TSM_REFUSED, (900, 4)),
    "rate_negative": (T.clip(900, 5), -65536, E.TSM_REFUSED, (900, 4)),
    "wrong_out_span": (T.clip(900, 5), 65536, E.TSM_REFUSED, (899, 4)),
    "wrong_frame_span": (T.clip(900, 5), 65536, E.TSM_REFUSED, (900, 5)),
}


@pytest.mark.parametrize("name", list(BAD))
def test_a_clip_that_is_not_ok_gets_its_status_and_nothing_else(name, solo):
    x, rq, status, span = BAD[name]
    if name == "too_long":
        span = (T.out_samples(len(x), rq), T.frames(len(x), rq))
    fam = T.family_reference()
    a, b = 4 * 4 + 1, 7 * 4 + 2  # (769 samples at 0.8, 9001 at 1.25)
    res = device_stretch([(fam[a][0], fam[a][1]), (x, rq), (fam[b][0], fam[b][1])], spans=[None, span, None])
    assert res[1]["status"] == status and untouched(res[1])
    assert same(res[0], solo[a]) and same(res[2], solo[b])  # the neighbours: untouched by it, and correct (test_family_solo)


def test_all_zero_audio_takes_offset_zero():
    for n, rate in ((3000, 0.8), (768, 1.25), (1, 2.0)):
        r = device_stretch([(np.zeros(n, np.float32), T.rate_q(rate))])[0]
        assert r["status"] == E.TSM_OK and not r["offsets"].any() and not r["y"].any()
        assert r["y"].tobytes() == np.zeros(len(r["y"]), np.float32).tobytes()  # (+0, not -0)


def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(8, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    for n in (0, 33):
        assert st.lib.tt_tsm_stretch(st.h, n, E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert st.lib.tt_tsm_stretch(st.h, 1, E.ptr(y), None, E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(i), E.stream_ptr()) == -1
    assert b"null argument" in st.lib.tt_last_error()


@torch.no_grad()
def test_stretch_through_the_api(solo):
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    h = Host()
    fam = T.family_reference()
    x = torch.from_numpy(fam[7 * 4][0].copy())  # 9001 samples (at rate 0.5 in the family)
    for d in (0.25, 0.4, 0.7):
        rq = T.rate_q(9001 / (d * 24000))
        y = h.stretch(x, duration=d)
        assert y.shape == (h.load_stretch().lib.tt_tsm_out_samples(9001, rq),) and y.device.type == "cpu"
    y = h.stretch(x.reshape(1, 1, -1).to(DEV), rate=0.5)
    assert y.shape == (1, 1, 18002) and y.device.type == "cuda" and y.cpu().numpy().tobytes() == solo[7 * 4]["y"].tobytes()
    # more clips than one call takes (16), a rate each: every clip the bits of its solo call, and its anchors those of its offsets
    pick = list(range(0, 72, 2))
    out, maps = h.stretch_many([torch.from_numpy(fam[i][0].copy()) for i in pick], rates=[fam[i][1] / 65536 for i in pick], return_map=True)
    for i, o, m in zip(pick, out, maps):
        assert o.numpy().tobytes() == solo[i]["y"].tobytes()
        assert m[:, 1].tolist() == T.positions(fam[i][1], solo[i]["offsets"]).tolist()
    assert h.stretcher.max_samples == 30 * 24000 and h.stretcher.max_clips == 16
    with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
        h.stretch(x, rate=2.5)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    return TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)


@torch.no_grad()
def test_speaking_rate_equals_stretching_the_clip(tts):
    import bench
    text = bench.synthetic_prompt()[0].tolist()
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts(text, k=2, **kw)
    assert tts.stretcher is None and "stretch_s" not in tts.timings
    again = tts.tts(text, k=2, speaking_rate=1.0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)) and tts.stretcher is None  # today's bits, no stage
    fast = tts.tts(text, k=2, speaking_rate=1.25, **kw)
    assert tts.timings["stretch_s"] > 0
    for f, p in zip(fast, plain):
        want = tts.stretch(p, rate=1.25)
        assert f.shape == want.shape == (1, 1, T.out_samples(p.shape[-1], 81920)) and torch.equal(f, want)
        c = T.check(p.reshape(-1).numpy(), 81920, f.reshape(-1).numpy(), tts.stretch_many([p], rates=1.25, return_map=True)[1][0][:, 1].numpy()
                    - np.array([-T.HS] + [T.nominal(k, 81920) for k in range(1, T.frames(p.shape[-1], 81920))]))
        assert not c["inadmissible"] and not c["bad_samples"]
