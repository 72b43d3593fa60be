"""The arbitrary-ratio resampler on the MI355X (csrc/resample.hip, include/tortoise_mi355x_rs.h) against the fp64 reference of
tests/resample_reference.py: every output sample inside its derived bound, ragged batches bit-identical to solo calls, a clip that is not OK
gets its status and nothing else, nothing is written outside a clip's own slice, the peak is the maximum of what was written, and the
API end to end (resample, shift_pitch, pitch= and sample_rate= on tts)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_reference as R
from tests import tsm_reference as T
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0        # what every output holds before the call
PAD = 64           # canaries on either side of `out`
MAX_SAMPLES = 5000

_src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tortoise_tts_amd", "csrc", "resample.hip")).read()
TILE = int(re.search(r"kRsTile == (\d+)", _src).group(1))  # outputs per tile (the source's static_assert)


def _length_for(n_out, P, Q):
    """A clip length whose output has exactly n_out samples."""
    n = next(n for n in range(1, 8 * n_out + 9) if R.out_samples(n, P, Q) == n_out)
    assert n <= MAX_SAMPLES
    return n


# the issue's lengths at its six ratios, the extreme ratios on short clips, and clips that end one short of, on and one past a tile (the
# downward ratios reach every output length; around the same border, three neighbouring lengths at two upward ones)
FAMILY = [(n, P, Q) for P, Q in R.RATIOS for n in R.LENGTHS] + [(n, P, Q) for P, Q in R.EXTREME_RATIOS for n in R.EXTREME_LENGTHS] + \
    [(_length_for(TILE + d, P, Q), P, Q) for P, Q in ((3, 2), (77936, 65536)) for d in (-1, 0, 1)] + \
    [(TILE * P // Q + d, P, Q) for P, Q in ((80, 147), (55109, 65536)) for d in (-1, 0, 1)] + \
    [(_length_for(2 * TILE + d, 1, 1), 1, 1) for d in (-1, 0, 1)]  # (P = Q is the low-pass, not a copy)

_stage = []


def stage():
    if not _stage:
        _stage.append(stages.ResampleStage(MAX_SAMPLES, max_clips=32, device=DEV))
    return _stage[0]


def device_resample(clips, spans=None, with_peak=True):
    """One tt_rs_resample call over clips = [(x f32 [n], P, Q)] with every output pre-filled with SENT and canaries around `out` -> per clip
    the raw status, y and peak (SENT where the call wrote nothing).  spans: per clip the out entries where they are not the reference's."""
    st = stage()
    n = len(clips)
    spans = spans or [None] * n
    spans = [R.out_samples(len(x), P, Q) if s is None else s for s, (x, P, Q) in zip(spans, clips)]
    io = np.concatenate(([0], np.cumsum([len(x) for x, _, _ in clips]))).astype(np.int32)
    oo = np.concatenate(([0], np.cumsum(spans))).astype(np.int32)
    audio = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _, _ in clips] + [np.zeros(1, np.float32)])).to(DEV)
    io_d, oo_d = torch.from_numpy(io).to(DEV), torch.from_numpy(oo).to(DEV)
    p_d = torch.tensor([P for _, P, _ in clips], dtype=torch.int32, device=DEV)
    q_d = torch.tensor([Q for _, _, Q in clips], dtype=torch.int32, device=DEV)
    y = torch.full((PAD + int(oo[-1]) + PAD,), SENT, device=DEV)
    peak = torch.full((n + 1,), SENT, device=DEV)
    status = torch.full((n + 1,), int(SENT), dtype=torch.int32, device=DEV)
    E.check(st.lib.tt_rs_resample(st.h, n, E.ptr(audio), E.ptr(io_d), E.ptr(p_d), E.ptr(q_d), y.data_ptr() + 4 * PAD, E.ptr(oo_d),
                                  E.ptr(peak) if with_peak else None, E.ptr(status), E.stream_ptr()))
    y, peak, status = (t.cpu().numpy() for t in (y, peak, status))
    assert (y[:PAD] == SENT).all() and (y[PAD + oo[-1]:] == SENT).all() and peak[n] == SENT and status[n] == SENT  # nothing beyond the batch
    y = y[PAD:]
    return [dict(status=int(status[i]), y=y[oo[i]:oo[i + 1]], peak=peak[i:i + 1]) for i in range(n)]


def untouched(r):
    return (r["y"] == SENT).all() and (r["peak"] == SENT).all()


def same(a, b):
    return a["status"] == b["status"] and a["y"].tobytes() == b["y"].tobytes() and a["peak"].tobytes() == b["peak"].tobytes()


_refs = {}


def reference(i):
    """(x, y fp64, bound) of family member i, computed once."""
    if i not in _refs:
        n, P, Q = FAMILY[i]
        x = R.clip(n, i)
        _refs[i] = (x,) + R.resample(x, P, Q)
    return _refs[i]


def verify(results, what):
    worst = 0.0
    for i, (r, (n, P, Q)) in enumerate(zip(results, FAMILY)):
        x, y, b = reference(i)
        assert r["status"] == E.RS_OK and r["y"].shape == y.shape == (R.out_samples(n, P, Q),), (n, P, Q)
        share = np.abs(r["y"].astype(np.float64) - y) / b
        assert (share <= 1.0).all(), (n, P, Q, int(share.argmax()), float(share.max()))
        assert r["peak"].tobytes() == np.abs(r["y"]).max(keepdims=True).tobytes(), (n, P, Q)  # exactly max |y| of what was written
        worst = max(worst, float(share.max()))
    print(f"[parity] tt_rs_resample {what}: {len(FAMILY)} clips (lengths 1 .. {MAX_SAMPLES}, {len(set(f[1:] for f in FAMILY))} ratios, tiles of {TILE}); "
          f"worst share of the sample bound used {worst:.3f}")
    return worst


@pytest.fixture(scope="module")
def solo():
    return [device_resample([(reference(i)[0], P, Q)])[0] for i, (_, P, Q) in enumerate(FAMILY)]


def _batched(size, seed):
    """The family in shuffled order in calls of `size` clips (ratios mixed within a call) -> results in the family's order."""
    order = np.random.default_rng(seed).permutation(len(FAMILY))
    out = [None] * len(FAMILY)
    for g in range(0, len(FAMILY), size):
        idx = order[g:g + size]
        for i, r in zip(idx, device_resample([(reference(i)[0],) + FAMILY[i][1:] for i in idx])):
            out[i] = r
    return out


def test_family_solo(solo):
    assert TILE == 1024 and {R.out_samples(*f) for f in FAMILY} >= {TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1}
    verify(solo, "solo")


def test_family_ragged_batches_of_17(solo):
    ragged = _batched(17, 1)
    verify(ragged, "ragged batches of 17")
    assert all(same(a, b) for a, b in zip(ragged, solo))  # bit-identical to the solo calls


def test_family_in_pairs_is_bit_identical_to_solo(solo):
    assert all(same(a, b) for a, b in zip(_batched(2, 2), solo))


def test_a_ragged_batch_with_an_empty_and_a_refused_clip(solo):
    a, b, c = FAMILY.index((5000, 80, 147)), FAMILY.index((1000, 3, 1)), FAMILY.index((2000, 1, 8))
    res = device_resample([(reference(a)[0], 80, 147), (np.zeros(0, np.float32), 3, 2), (reference(b)[0], 3, 1), (R.clip(900, 5), 6, 4),
                           (reference(c)[0], 1, 8)], spans=[None, 5, None, 600, None])
    assert [r["status"] for r in res] == [E.RS_OK, E.RS_EMPTY, E.RS_OK, E.RS_REFUSED, E.RS_OK]
    assert untouched(res[1]) and untouched(res[3])
    assert same(res[0], solo[a]) and same(res[2], solo[b]) and same(res[4], solo[c])
    # without a peak array: the same samples
    quiet = device_resample([(reference(a)[0], 80, 147), (reference(b)[0], 3, 1)], with_peak=False)
    assert all(q["y"].tobytes() == solo[i]["y"].tobytes() and (q["peak"] == SENT).all() for q, i in zip(quiet, (a, b)))


BAD = {
    "empty": (np.zeros(0, np.float32), 3, 2, E.RS_EMPTY, 5),
    "too_long": (R.clip(MAX_SAMPLES + 1, 5), 3, 2, E.RS_REFUSED, None),
    "ratio_above": (R.clip(900, 5), 9, 1, E.RS_REFUSED, 100),
    "ratio_below": (R.clip(900, 5), 1, 9, E.RS_REFUSED, 8100),
    "term_zero": (R.clip(900, 5), 0, 1, E.RS_REFUSED, 900),
    "term_negative": (R.clip(900, 5), -3, 2, E.RS_REFUSED, 600),
    "term_too_large": (R.clip(900, 5), (1 << 20) + 1, 1 << 20, E.RS_REFUSED, 900),
    "not_reduced": (R.clip(900, 5), 6, 4, E.RS_REFUSED, 600),
    "out_span_short": (R.clip(900, 5), 3, 2, E.RS_REFUSED, 599),
    "out_span_long": (R.clip(900, 5), 3, 2, E.RS_REFUSED, 601),
}


@pytest.mark.parametrize("name", list(BAD))
def test_a_clip_that_is_not_ok_gets_its_status_and_nothing_else(name, solo):
    x, P, Q, status, span = BAD[name]
    a, b = FAMILY.index((1000, 77936, 65536)), FAMILY.index((37, 1, 2))
    res = device_resample([(reference(a)[0],) + FAMILY[a][1:], (x, P, Q), (reference(b)[0],) + FAMILY[b][1:]],
                          spans=[None, R.out_samples(len(x), 3, 2) if span is None else span, None])
    assert res[1]["status"] == status and untouched(res[1])
    assert same(res[0], solo[a]) and same(res[2], solo[b])  # the neighbours: untouched by it, and correct (test_family_solo)


def test_a_pitch_ratio_need_not_be_reduced():
    x = R.clip(700, 9)
    r = device_resample([(x, 98304, 65536)])[0]  # 3/2 as 16.16: other integers (cq is the same, r and Q are not), the same filter
    y, b = R.resample(x, 98304, 65536)
    assert r["status"] == E.RS_OK and (np.abs(r["y"] - y) <= b).all()


def test_all_zero_audio_gives_all_zero_output():
    for n, P, Q in ((3000, 3, 2), (1025, 1, 2), (1, 8, 1), (1, 1, 8)):
        r = device_resample([(np.zeros(n, np.float32), P, Q)])[0]
        assert r["status"] == E.RS_OK and r["y"].tobytes() == np.zeros(R.out_samples(n, P, Q), np.float32).tobytes()  # (+0, not -0)
        assert r["peak"].tobytes() == np.zeros(1, np.float32).tobytes()


def test_argument_checks_come_before_device_work():
    st = stage()
    y = torch.zeros(8, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    for n in (0, 33):
        assert st.lib.tt_rs_resample(st.h, n, E.ptr(y), E.ptr(i), E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(y), E.ptr(i), E.stream_ptr()) == -1
        assert b"clips (1 .. 32)" in st.lib.tt_last_error()
    assert st.lib.tt_rs_resample(st.h, 1, E.ptr(y), None, E.ptr(i), E.ptr(i), E.ptr(y), E.ptr(i), E.ptr(y), E.ptr(i), E.stream_ptr()) == -1
    assert b"null argument" in st.lib.tt_last_error()


def _host():
    from tortoise_tts_amd import api

    class Host(api._Common):
        device = torch.device(DEV)

    return Host()


@torch.no_grad()
def test_resample_and_shift_pitch_through_the_api(solo):
    h = _host()
    i = FAMILY.index((5000, 3, 2))
    x = torch.from_numpy(reference(i)[0].copy())
    y = h.resample(x, 16000)
    assert y.shape == (3334,) and y.device.type == "cpu" and y.numpy().tobytes() == solo[i]["y"].tobytes()
    y = h.resample(x.reshape(1, 1, -1).to(DEV), 16000)
    assert y.shape == (1, 1, 3334) and y.device.type == "cuda" and y.cpu().numpy().tobytes() == solo[i]["y"].tobytes()
    # more clips than one call takes (16), a ratio each: every clip the bits of its solo call, and its peak
    pick = [k for k, (n, P, Q) in enumerate(FAMILY) if (P, Q) in ((3, 1), (3, 2), (1, 2), (80, 147))]
    assert len(pick) > 16
    rates = {(3, 1): 8000, (3, 2): 16000, (1, 2): 48000, (80, 147): 44100}
    out, peaks = h.resample_many([torch.from_numpy(reference(k)[0].copy()) for k in pick], [rates[FAMILY[k][1:]] for k in pick], return_info=True)
    for k, o, pk in zip(pick, out, peaks):
        assert o.numpy().tobytes() == solo[k]["y"].tobytes() and np.float32(pk).tobytes() == solo[k]["peak"].tobytes()
    assert h.resampler.max_samples == 30 * 24000 and h.resampler.max_clips == 16
    # a 220 Hz tone, three semitones up and down: the duration the integers predict, the pitch where it belongs
    n = 24000
    tone = torch.from_numpy((0.5 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 24000)).astype(np.float32))
    for s, shifted in zip((3, -3), h.shift_pitch_many([tone, tone], [3, -3])):
        pq, rq_eff = rs.pitch(s)
        n2 = rs.out_samples(T.out_samples(n, rq_eff), pq, 65536)
        assert shifted.shape == (n2,) and abs(n2 - n) <= 2  # (the two roundings: test_resample_cpu.py derives < 3)
        spec = np.abs(np.fft.rfft(shifted.numpy().astype(np.float64) * np.hanning(n2)))
        f_bin = 24000.0 / n2  # one analysis bin, 1 Hz
        got, want = spec.argmax() * f_bin, 220.0 * 2.0 ** (s / 12)
        print(f"[parity] shift_pitch {s:+d} semitones of a 220 Hz tone: {n2} samples, dominant frequency {got:.2f} Hz (wanted {want:.2f})")
        assert abs(got - want) <= f_bin
    with pytest.raises(ValueError, match="ratio 12/1"):
        h.resample(x, 2000)


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    return TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48)


@torch.no_grad()
def test_pitch_and_sample_rate_on_tts_equal_the_chain_on_the_clip(tts):
    import bench
    text = bench.synthetic_prompt()[0].tolist()
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    plain = tts.tts(text, k=2, **kw)
    again = tts.tts(text, k=2, pitch=0, sample_rate=24000, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)) and tts.resampler is None and tts.stretcher is None  # today's bits, no stage
    assert "pitch_s" not in tts.timings and "resample_s" not in tts.timings
    got = tts.tts(text, k=2, pitch=3, sample_rate=16000, **kw)
    assert tts.timings["pitch_s"] > 0 and tts.timings["resample_s"] > 0 and len(tts.resample_info) == 2
    for o, p, pk in zip(got, plain, tts.resample_info):
        mid = tts.shift_pitch(p, 3)
        want = tts.resample(mid, 16000)
        assert o.shape == want.shape == (1, 1, rs.out_samples(mid.shape[-1], 3, 2)) and torch.equal(o, want) and pk == float(o.abs().max())
        y, b = R.resample(mid.reshape(-1).numpy(), 3, 2)
        assert (np.abs(o.reshape(-1).numpy() - y) <= b).all()
