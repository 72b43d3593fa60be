"""CPU checks of the time-varying pitch (include/tortoise_mi355x_rsw.h, tortoise_tts_amd/resample.py): the table's integers in their three
spellings (tests/pitchmap_reference.py, resample.py, the built library), the plan's bound, every refusal, the fp64 reference along a table
against the constant-ratio reference and on stepped tones, PitchMap.from_words, the chain's duration bound, the host flow
(shift_pitch(pitch_map=), tts_with_timings(word_pitches=)) on reference-backed stand-ins of the device stages, and the stand-alone
sanitizer check of the host code.  The kernel is tests/test_gpu_pitchmap.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import pitchmap_reference as M
from tests import resample_reference as R
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import stretch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def _arr(values):
    return (C.c_int * max(1, len(values)))(*[int(v) for v in values])


def _lib_plan(lib, n, starts, ps):
    out = (C.c_int * (4 * max(1, len(starts))))(*([-7] * (4 * max(1, len(starts)))))
    rc = lib.tt_rsw_plan(n, len(starts), _arr(starts), _arr(ps), out)
    return rc, [tuple(out[4 * i:4 * i + 4]) for i in range(len(starts))]


def _flat(table):
    return _arr([v for row in table for v in row])


GOOD = M.plan(3000, [(0, 81920), (1000, 52429), (1700, 131072)])


def _edit(at, v):
    return [tuple(v if 4 * i + j == at else GOOD[i][j] for j in range(4)) for i in range(3)]


BAD_TABLES = {
    "start_m_not_0": _edit(0, 1), "start_thi_not_0": _edit(1, 1), "start_tlo_not_0": _edit(2, 1),
    "m_not_increasing": _edit(8, GOOD[1][0]), "m_decreasing": _edit(4, -5),
    "continuity_thi_plus_1": _edit(5, GOOD[1][1] + 1), "continuity_tlo_minus_1": _edit(10, (GOOD[2][2] - 1) % 65536),
    "tlo_negative": _edit(6, GOOD[1][2] - 65536), "tlo_65536": _edit(6, GOOD[1][2] + 65536), "thi_negative": _edit(9, -1),
    "ratio_below": _edit(7, M.P_MIN - 1), "ratio_above": _edit(11, M.P_MAX + 1), "ratio_zero": _edit(3, 0), "ratio_negative": _edit(3, -65536),
}


# ----------------------------------------------------------------------------------------- the integers
def test_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_rsw.h")
    assert set(names) == set(E._RSW_PROTOS) == {"tt_rsw_abi_version", "tt_rsw_plan", "tt_rsw_out_samples", "tt_rsw_create", "tt_rsw_destroy",
                                                "tt_rsw_resample"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_rsw_abi_version() == 1 == E.RSW_ABI_VERSION
    assert lib.tt_rs_abi_version() == 1 and lib.tt_rss_abi_version() == 1 and lib.tt_tsw_abi_version() == 1  # the other headers are untouched
    assert not [n for n in declared_symbols() if n.startswith("tt_rsw")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_rsw.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_RSW_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert defines == dict(TT_RSW_MAX_SEGMENTS=E.RSW_MAX_SEGMENTS, TT_RSW_MIN_SEGMENT=E.RSW_MIN_SEGMENT, TT_RSW_P_MIN=E.RSW_P_MIN,
                           TT_RSW_P_MAX=E.RSW_P_MAX, TT_RSW_OK=E.RSW_OK, TT_RSW_EMPTY=E.RSW_EMPTY, TT_RSW_REFUSED=E.RSW_REFUSED)
    assert (M.MAX_SEGMENTS, M.MIN_SEGMENT, M.P_MIN, M.P_MAX) == (E.RSW_MAX_SEGMENTS, E.RSW_MIN_SEGMENT, E.RSW_P_MIN, E.RSW_P_MAX)
    assert (E.RSW_P_MIN, E.RSW_P_MAX) == (rs.pitch_ratio(-12)[0], rs.pitch_ratio(12)[0])  # the range of pitch=
    from tortoise_tts_amd import build
    assert "resample_warp.hip" in build.SOURCES and any(h.endswith("tortoise_mi355x_rsw.h") for h in build._headers())
    kernel = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "resample_warp.hip")).read()
    for name in ("rs_output", "rs_cq", "rs_half_width", "rs_c32", "rsw_row_ok", "rsw_tail", "rsw_position"):
        assert name + "(" in kernel, name  # the kernel is built from the shared steps, and checks the table with the host's code
    assert "fmaf" not in kernel  # no arithmetic of its own
    h = E.vp()
    for bad in ((0, 1, 1), (E.RS_MAX_SAMPLES + 1, 1, 1), (100, 0, 1), (100, E.RS_MAX_CLIPS + 1, 1), (100, 1, 0), (100, 1, E.RSW_MAX_SEGMENTS + 1)):
        assert lib.tt_rsw_create(*bad, C.byref(h)) == -1 and b"tt_rsw_create" in lib.tt_last_error()
    assert lib.tt_rsw_resample(None, 1, None, None, None, None, None, None, None, None, None) == -1 and b"tt_rsw_resample" in lib.tt_last_error()
    rc = lib.tt_rsw_create(1000, 2, 8, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_rsw_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())


def test_library_python_and_reference_agree():
    lib = _lib()
    rng = np.random.default_rng(12)
    for _ in range(400):
        S = int(rng.integers(1, E.RSW_MAX_SEGMENTS + 1))
        n = int(max(2 * S, rng.integers(2, 4000)))
        segs = M.random_segments(rng, n, S)
        starts, ps = [b for b, _ in segs], [p for _, p in segs]
        rc, table = _lib_plan(lib, n, starts, ps)
        assert rc == 0 and table == rs.map_plan(n, starts, ps) == M.plan(n, segs)
        assert lib.tt_rsw_out_samples(n, S, _flat(table)) == rs.map_out_samples(n, table) == M.out_samples(n, table) > 0
    # the longest clip: the 64-bit products, t beyond 2^32
    n = E.RS_MAX_SAMPLES
    for segs in ([(0, M.P_MIN), (n // 3, M.P_MAX), (n - 2, 98765)], [(0, M.P_MAX)] + [(n - 2 * (64 - i), (M.P_MIN, M.P_MAX)[i % 2]) for i in range(1, 64)]):
        rc, table = _lib_plan(lib, n, [b for b, _ in segs], [p for _, p in segs])
        assert rc == 0 and table == rs.map_plan(n, [b for b, _ in segs], [p for _, p in segs]) == M.plan(n, segs)
        assert M.t_of(table[-1]) > 1 << 38
        assert lib.tt_rsw_out_samples(n, len(segs), _flat(table)) == rs.map_out_samples(n, table) == M.out_samples(n, table) > 0
    # the family's tables (some are not plans) are tables for all three
    for name, n, _, table in M.FAMILY:
        assert lib.tt_rsw_out_samples(n, len(table), _flat(table)) == rs.map_out_samples(n, table) == M.out_samples(n, table) > 0, name


def test_every_table_rule_is_refused_one_at_a_time():
    lib = _lib()
    assert lib.tt_rsw_out_samples(3000, 3, _flat(GOOD)) == rs.map_out_samples(3000, GOOD) == M.out_samples(3000, GOOD) > 0
    for name, table in BAD_TABLES.items():
        assert lib.tt_rsw_out_samples(3000, 3, _flat(table)) == 0 == rs.map_out_samples(3000, table) == M.out_samples(3000, table), name
    assert lib.tt_rsw_out_samples(GOOD[2][1], 3, _flat(GOOD)) == 0 == rs.map_out_samples(GOOD[2][1], GOOD) == M.out_samples(GOOD[2][1], GOOD)  # t_(S-1) < n 65536
    assert lib.tt_rsw_out_samples(GOOD[2][1] + 1, 3, _flat(GOOD)) == rs.map_out_samples(GOOD[2][1] + 1, GOOD) == GOOD[2][0] + 1
    assert lib.tt_rsw_out_samples(3000, 0, _flat(GOOD)) == 0 == rs.map_out_samples(3000, [])
    assert lib.tt_rsw_out_samples(3000, 65, _flat(GOOD * 22)) == 0 == rs.map_out_samples(3000, GOOD * 22)
    assert lib.tt_rsw_out_samples(0, 3, _flat(GOOD)) == 0 == lib.tt_rsw_out_samples(3000, 3, None)
    assert lib.tt_rsw_out_samples(E.RS_MAX_SAMPLES + 1, 3, _flat(GOOD)) == 0 == rs.map_out_samples(E.RS_MAX_SAMPLES + 1, GOOD)
    # the plan: -1 with a message that names the segment, and nothing written
    for n, starts, ps, what in ((100, [0, 1], [65536, 65536], b"at least 2 samples"), (100, [0, 99], [65536, 65536], b"at least 2 samples"),
                                (100, [0, 60, 40], [65536] * 3, b"segment 1 starts at sample 60 and ends at 40"), (100, [5], [65536], b"not at 0"),
                                (100, [0, 50], [65536, 32767], b"segment 1: ratio 32767"), (100, [0], [131073], b"segment 0: ratio 131073"),
                                (100, [], [], b"0 segments"), (1000, [2 * i for i in range(65)], [65536] * 65, b"65 segments (1 .. 64)"),
                                (0, [0], [65536], b"a clip of 0 samples"), (E.RS_MAX_SAMPLES + 1, [0], [65536], b"samples (1 ..")):
        rc, table = _lib_plan(lib, n, starts, ps)
        assert rc == -1 and what in lib.tt_last_error() and all(row == (-7, -7, -7, -7) for row in table), what
        with pytest.raises(ValueError, match="pitch map"):
            rs.map_plan(n, starts, ps)
    assert lib.tt_rsw_plan(100, 1, None, _arr([65536]), _arr([0, 0, 0, 0])) == -1 and b"null argument" in lib.tt_last_error()
    F = rs.PitchMap.from_segments
    for n, segs, what in ((100, [(0, 0), (1, 2)], "at least 2 samples"), (100, [(0, 0), (60, 1), (40, 2)], "segment 1 starts at sample 60 and ends at 40"),
                          (100, [(5, 0)], "not at 0"), (100, [], r"0 segments \(1 \.\. 64\)"), (1000, [(2 * i, i % 2) for i in range(65)], r"65 segments"),
                          (100, [(0, 12.5)], r"segment 0: pitch 12\.5"), (100, [(0, 0), (50, -13)], r"segment 1: pitch -13"),
                          (100, [(0, float("nan"))], "segment 0"), (100, [(0, "x")], "segment 0")):
        with pytest.raises(ValueError, match=what):
            F(n, segs)
    assert F(1000, [(2 * i, 0) for i in range(64)]).n_out == 1000 and F(4, [(0, -12), (2, 12)]).table == [(0, 0, 0, 32768), (4, 2, 0, 131072)]


def test_plan_stays_within_its_bound():
    """5 000 random plans (csrc/checks/rsw_host_check.cpp runs 20 000 of the library's), up to 64 segments, ratios including both ends:
    0 <= t_i - 65536 b_i < P_(i-1) (under two input samples, and it does not accumulate), the position increases, and the last output
    reads inside the clip."""
    rng = np.random.default_rng(22)
    worst = 0
    for _ in range(5000):
        S = int(rng.integers(1, E.RSW_MAX_SEGMENTS + 1))
        n = int(max(2 * S, rng.integers(2, 4000)))
        segs = M.random_segments(rng, n, S)
        table = rs.map_plan(n, [b for b, _ in segs], [p for _, p in segs])
        for i, (row, (b, _)) in enumerate(zip(table, segs)):
            over = M.t_of(row) - 65536 * b
            assert 0 <= over < (segs[i - 1][1] if i else 1), (n, segs)
            worst = max(worst, over)
        n_out = rs.map_out_samples(n, table)
        assert n_out > table[-1][0] and n // 2 <= n_out <= 2 * n
        last = M.t_of(table[-1]) + (n_out - 1 - table[-1][0]) * table[-1][3]
        assert last < n * 65536 <= last + table[-1][3]
        assert rs.map_position(n_out - 1, table) == (last >> 16, last & 65535) and rs.map_position(0, table) == (0, 0)
    assert 65536 < worst < 131072


# ----------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("P", [32768, 55109, 65536, 77936, 131072])
def test_one_segment_is_the_constant_ratio_reference_exactly(P):
    for n in (37, 1000):
        x = R.clip(n, 0)
        y, b = M.resample_map(x, [(0, 0, 0, P)])
        y0, b0 = R.resample(x, P, 65536)
        assert np.array_equal(y, y0) and np.array_equal(b, b0) and M.out_samples(n, [(0, 0, 0, P)]) == R.out_samples(n, P, 65536)
        assert rs.map_plan(n, [0], [P]) == M.plan(n, [(0, P)]) == [(0, 0, 0, P)]


def _tone_fit(y, f):
    """amplitude of the best fit of a tone at f cycles per sample, and the residual's rms relative to it"""
    m = np.arange(len(y))
    A = np.stack([np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)], axis=1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.hypot(*c)), float(np.sqrt(np.mean((y - A @ c) ** 2)) / np.hypot(*c))


def test_each_segment_of_a_stepped_map_carries_its_tone():
    """A tone at f through the map (P_0, P_1): segment i holds a tone at f P_i / 65536 at unit gain, and the step across the border is no
    larger than the largest step elsewhere (the position is continuous; only the filter changes)."""
    n, f = 6000, 0.05
    x = np.sin(2 * np.pi * f * np.arange(n)).astype(np.float32)
    for ps in ((55109, 77936), (131072, 32768), (32768, 98304)):
        table = M.plan(n, [(0, ps[0]), (3000, ps[1])])
        y, _ = M.resample_map(x, table, bound=False)
        border = table[1][0]
        for lo, hi, P in ((100, border - 100, ps[0]), (border + 100, len(y) - 100, ps[1])):
            amp, res = _tone_fit(y[lo:hi], f * P / 65536)
            assert abs(amp - 1.0) < 1e-3 and res < 1e-3, (ps, P, amp, res)
            other = ps[1] if P == ps[0] else ps[0]
            assert _tone_fit(y[lo:hi], f * other / 65536)[1] > 0.5  # and not the other segment's tone
        steps = np.abs(np.diff(y))
        assert steps[border - 1] <= steps[100:-100].max() * (1 + 1e-9), ps


# ----------------------------------------------------------------------------------------- PitchMap
def _alignment(n, spans):
    from tortoise_tts_amd import align
    words = [("w%d" % i, a, b, 1.0) for i, (a, b) in enumerate(spans)]
    return align.Alignment("", [], words, 0.0, n)


def test_pitch_map_from_words():
    q = lambda s: rs.pitch_ratio(s)[0]
    al = _alignment(24000, [(1000, 5000), (5000, 9000), (12000, 12003), (15000, 20000)])
    F = rs.PitchMap.from_words
    m = F(al, [2, None, None, -1])
    assert list(zip(m.starts, m.pqs)) == [(0, 65536), (1000, q(2)), (5000, 65536), (15000, q(-1)), (20000, 65536)]
    assert F(al, {0: 2, 3: -1}).table == m.table
    up = F(al, {1: -3}, base=2.0)
    assert list(zip(up.starts, up.pqs)) == [(0, q(2)), (5000, q(-3)), (9000, q(2))]
    assert F(al, [2, 2, None, None]).starts == [0, 1000, 9000]  # neighbours at one pitch are one segment
    assert F(al, {2: 5}).table == [(0, 0, 0, 65536)] == F(al, [None] * 4).table == F(al, [0] * 4).table  # a span under 4 samples owns nothing
    assert stretch.RateMap.from_words(al, {2: 0.5}).starts == [0, 12000, 12003]  # (the rate map's limit is 2: the one difference)
    assert F(_alignment(24000, [(1000, 5000), (5000, 9000), (12000, 12004), (15000, 20000)]), {2: 5}).starts == [0, 12000, 12004]
    assert F(al, [3] * 4, base=3).table == [(0, 0, 0, q(3))]
    assert F(_alignment(9000, [(0, 5000), (5000, 9000)]), [-12, 12]).pqs == [32768, 131072]  # words from the first sample to the last
    assert F(_alignment(9000, [(0, 5000), (5003, 9000)]), [1, 2]).starts == [0, 5003]  # a gap under 4 samples joins the word before it
    for bad, what in (([2], "1 pitches for the 4 words"), ({4: 2}, "word index 4"), ({-1: 2}, "word index -1"), ({0: 12.5}, r"word 0 \('w0'\)"),
                      ([None, "x", None, None], r"word 1 \('w1'\)"), ({True: 1}, "word index True")):
        with pytest.raises(ValueError, match=what):
            F(al, bad)
    with pytest.raises(ValueError, match=r"the base: pitch 13\.0"):
        F(al, {}, base=13)
    al.rate = 16000
    with pytest.raises(ValueError, match="16000 Hz"):
        F(al, {})
    # pitch_map(): a PitchMap of the clip, or (start_seconds, semitones)
    pm = rs.PitchMap.from_segments(5000, [(0, 0), (2400, 3)])
    assert rs.pitch_map(5000, pm) is pm and rs.pitch_map(5000, [(0, 0), (0.1, 3)]).table == pm.table
    with pytest.raises(ValueError, match="made for a clip of 5000 samples, this one has 300"):
        rs.pitch_map(300, pm)
    with pytest.raises(ValueError, match="a PitchMap, or a list"):
        rs.pitch_map(5000, 3.0)
    assert "2400" in repr(pm) and "3.0" in repr(pm)


# ----------------------------------------------------------------------------------------- the chain
def test_the_chain_keeps_every_duration_within_its_bound():
    """Random maps of words with rates and pitches: every border and the end land within resample.duration_bound of sum len_i / rate_i.
    The bound is derived in its docstring from the two plans' roundings; the worst distance seen is printed."""
    rng = np.random.default_rng(31)
    worst, worst_share, tried = 0.0, 0.0, 0
    for _ in range(3000):
        S = int(rng.integers(1, 65))
        n = int(max(4 * S + 4, rng.integers(8, 250000)))
        cuts = np.sort(rng.choice(np.arange(1, n - 3 * S - 1), S - 1, replace=False)) + 3 * np.arange(1, S) if S > 1 else []
        starts = [0] + [int(c) for c in cuts]
        pqs = [int(rng.choice([M.P_MIN, M.P_MAX, 65536])) if rng.random() < 0.3 else int(rng.integers(M.P_MIN, M.P_MAX + 1)) for _ in range(S)]
        rqs = []
        for pq in pqs:  # a speaking rate whose time-stretch stays in range (half of the segments at rate 1.0 where that is one)
            lo, hi = max(32768, (32768 * pq + 65535) // 65536 + 1), min(131072, 131072 * pq // 65536 - 1)
            rqs.append(65536 if rng.random() < 0.5 and lo <= 65536 <= hi else int(rng.integers(lo, hi + 1)))
        ch = rs.WarpChain(n, starts, rqs, pqs)
        assert all(32768 <= e <= 131072 for e in ch.rq_effs) and ch.anchors.shape == (S + 1, 2) and ch.anchors.dtype == torch.int64
        assert ch.anchors[:, 0].tolist() == starts + [n] and ch.anchors[0].tolist() == [0, 0] and int(ch.anchors[-1, 1]) == ch.n_out
        assert rs.map_out_samples(ch.n_mid, ch.resample) == ch.n_out and [r[3] for r in ch.resample] == pqs
        if ch.stretch is not None:
            assert stretch.table_out_samples(n, ch.stretch) == ch.n_mid and [r[0] for r in ch.stretch] == ch.mid_starts
        else:
            assert ch.n_mid == n and ch.mid_starts == starts
        for i in range(1, S + 1):
            ideal = ch.ideal(i)
            dist = abs(int(ch.anchors[i, 1]) - ideal)
            assert dist <= rs.duration_bound(i, ideal), (n, starts, rqs, pqs, i)
            worst, worst_share = max(worst, dist), max(worst_share, dist / rs.duration_bound(i, ideal))
        tried += 1
    print(f"[pitchmap] chain: {tried} maps, worst distance from the ideal {worst:.2f} samples, worst share of the bound {worst_share:.3f}")
    # a pitch alone on eight words of a 5 s clip
    ch = rs.WarpChain(120000, [15000 * i for i in range(8)], [65536] * 8, [rs.pitch_ratio(s)[0] for s in (0, 2, 0, -1, 0, 3, 0, -2)])
    assert abs(ch.n_out - 120000) <= rs.duration_bound(8, 120000) < 74
    # segments under 4 samples are named
    with pytest.raises(ValueError, match="segment 1 starts at sample 100 and ends at 103"):
        rs.WarpChain(1000, [0, 100, 103], [65536] * 3, [65536, 77936, 65536])
    # merge_maps: the union of the borders, short pieces joined, the word named, at most 64
    assert rs.merge_maps(1000, [(0, 65536), (100, 49152), (500, 65536)], [(0, 65536), (300, 77936), (700, 65536)]) == \
        ([0, 100, 300, 500, 700], [65536, 49152, 49152, 65536, 65536], [65536, 65536, 77936, 77936, 65536])
    assert rs.merge_maps(1000, [(0, 65536), (100, 32768), (500, 65536)], [(0, 65536), (502, 77936), (998, 65536)])[0] == [0, 100, 502]
    with pytest.raises(ValueError, match=r"segment 1: speaking rate 0\.5000 at pitch ratio 1\.1892 needs a time-stretch at rate 0\.4204"):
        rs.merge_maps(1000, [(0, 65536), (100, 32768)], [(0, 65536), (100, 77936)])
    with pytest.raises(ValueError, match="65 segments.*at most 64"):
        rs.merge_maps(10000, [(100 * i, (65536, 60000)[i % 2]) for i in range(33)], [(0, 65536)] + [(50 + 100 * i, (70000, 65536)[i % 2]) for i in range(32)])


# ----------------------------------------------------------------------------------------- host flow
class ReferenceWarpResampleStage:
    """stages.WarpResampleStage backed by tests/pitchmap_reference.py."""
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, max_segments=64, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceWarpResampleStage.made.append(max_samples)

    def resample_many(self, clips, tables):
        ReferenceWarpResampleStage.calls.append(len(clips))
        out = []
        for x, table in zip(clips, tables):
            assert x.dim() == 1 and x.shape[0] <= self.max_samples and len({r[3] for r in table}) > 1
            y = torch.from_numpy(M.resample_map(x.numpy(), table, bound=False)[0]).float()
            out.append((y, float(y.abs().max())))
        return out

    def close(self):
        pass


def _by_hand(clip, chain):
    """the chain's two tables applied with the references"""
    from tests import tsmap_reference as TM
    x = clip.reshape(-1).numpy()
    if chain.stretch is not None:
        x = TM.stretch(x, chain.stretch)["y"].astype(np.float32)
    if len(set(chain.pqs)) > 1:
        x = M.resample_map(x, chain.resample, bound=False)[0]
    elif chain.pqs[0] != 65536:
        x = R.resample(x, chain.pqs[0], 65536, bound=False)[0]
    return torch.from_numpy(np.asarray(x)).float().reshape(clip.shape[:-1] + (-1,))


def _host(monkeypatch):
    from tests.test_resample_cpu import ReferenceResampleStage, _tts
    from tests.test_tsm_cpu import ReferenceStretchStage
    from tests.test_tsmap_cpu import ReferenceWarpStage
    t, kw = _tts(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "WarpStretchStage", ReferenceWarpStage)
    monkeypatch.setattr(api.stages, "WarpResampleStage", ReferenceWarpResampleStage)
    ReferenceWarpStage.made, ReferenceWarpStage.calls = [], []
    ReferenceWarpResampleStage.made, ReferenceWarpResampleStage.calls = [], []
    return t, kw, ReferenceWarpStage, ReferenceStretchStage, ReferenceResampleStage


@torch.no_grad()
def test_shift_pitch_along_a_map(monkeypatch):
    t, _, Warp, Const, ConstRs = _host(monkeypatch)
    x = torch.from_numpy(R.clip(5000, 0))
    pm = rs.PitchMap.from_segments(5000, [(0, 0), (1500, 3), (3000, -2)])
    chain = rs.WarpChain(5000, pm.starts, [65536] * 3, pm.pqs)
    for shape in ((5000,), (1, 5000), (1, 1, 5000)):
        y, a = t.shift_pitch(x.reshape(shape), pitch_map=pm, return_map=True)
        assert y.shape == shape[:-1] + (chain.n_out,) and torch.equal(y.reshape(-1), _by_hand(x, chain)) and torch.equal(a, chain.anchors)
        for i in range(1, 4):
            assert abs(int(a[i, 1]) - int(a[i, 0])) <= rs.duration_bound(i, int(a[i, 0]))  # every border and the length stay where they were
    assert Warp.calls == [1, 1, 1] and ReferenceWarpResampleStage.calls == [1, 1, 1] and Const.calls == [] and ConstRs.calls == []
    assert ReferenceWarpResampleStage.made == [2 * 30 * 24000] and t.pitch_maps[0] is pm
    assert torch.equal(t.shift_pitch(x, pitch_map=[(0.0, 0), (1500 / 24000, 3), (3000 / 24000, -2)]), _by_hand(x, chain))
    # 0 semitones throughout: the clip as it is, nothing runs; one segment: the path of semitones=
    Warp.calls, ReferenceWarpResampleStage.calls = [], []
    assert t.shift_pitch(x, pitch_map=[(0, 0)]) is x and t.shift_pitch(x, pitch_map=[(0, 0), (0.1, 0.0)]) is x
    assert torch.equal(t.shift_pitch(x, pitch_map=[(0, 3)]), t.shift_pitch(x, 3)) and torch.equal(t.shift_pitch(x, pitch_map=[(0, 3), (0.1, 3)]), t.shift_pitch(x, 3))
    assert Warp.calls == [] and ReferenceWarpResampleStage.calls == [] and len(Const.calls) == 4 and len(ConstRs.calls) == 4
    # several clips, a map each, ONE call of either stage; peaks and anchors on request
    clips = [x, torch.from_numpy(R.clip(1000, 1)).reshape(1, -1), torch.from_numpy(R.clip(5000, 2))]
    maps = [pm, [(0, 12), (0.02, -12)], [(0, 2)]]
    out, peaks, anchors = t.shift_pitch_many(clips, pitch_maps=maps, return_info=True, return_map=True)
    assert Warp.calls == [2] and ReferenceWarpResampleStage.calls == [2]
    for o, c, m, p, a in zip(out, clips, maps, peaks, anchors):
        m = rs.pitch_map(c.shape[-1], m)
        ch = rs.WarpChain(m.n, m.starts, [65536] * len(m.starts), m.pqs)
        assert torch.equal(o, _by_hand(c, ch)) and p == float(o.abs().max()) and torch.equal(a, ch.anchors)
    # exactly one of semitones and pitch_map; the refusals
    for kw in (dict(), dict(semitones=2, pitch_map=pm)):
        with pytest.raises(ValueError, match="exactly one of semitones and pitch_map"):
            t.shift_pitch(x, **kw)
    with pytest.raises(ValueError, match="return_map=True goes with pitch_map"):
        t.shift_pitch(x, 2, return_map=True)
    with pytest.raises(ValueError, match="3 clips with 2 pitch maps"):
        t.shift_pitch_many(clips, pitch_maps=maps[:2])
    with pytest.raises(ValueError, match="made for a clip of 5000 samples, this one has 1000"):
        t.shift_pitch(clips[1], pitch_map=pm)
    with pytest.raises(ValueError, match=r"segment 1: pitch 13"):
        t.shift_pitch(x, pitch_map=[(0, 0), (0.1, 13)])
    with pytest.raises(ValueError, match="formants='keep' / formant_shift= do not go with a pitch that changes inside the clip"):
        t.shift_pitch(x, pitch_map=pm, formants="keep")
    assert torch.equal(t.shift_pitch(x, pitch_map=pm, formants="follow"), _by_hand(x, chain))
    with pytest.raises(ValueError, match="expected"):
        t.shift_pitch(torch.zeros(2, 100), pitch_map=[(0, 1)])
    assert torch.equal(t.shift_pitch(x, 2), t.shift_pitch_many([x], 2)[0])  # the positional form of today


@torch.no_grad()
def test_word_pitches_on_tts_with_timings(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_resample_cpu import ReferenceResampleStage
    from tests.test_tsm_cpu import ReferenceStretchStage
    from tests.test_tsmap_cpu import ReferenceWarpStage
    from tests.test_api_flow_cpu import small_setup, voice_latents
    t, m = CC._flow(monkeypatch)
    from tortoise_tts_amd import api
    for name, cls in (("TimeStretchStage", ReferenceStretchStage), ("WarpStretchStage", ReferenceWarpStage), ("ResampleStage", ReferenceResampleStage),
                      ("WarpResampleStage", ReferenceWarpResampleStage)):
        monkeypatch.setattr(api.stages, name, cls)
        cls.made, cls.calls = [], []
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    text = "hello there"
    plain, al0 = t.tts_with_timings(text, **kw)
    # all pitches 0 (or none) and no rates: today's bits, nothing built
    for wp in ([0, None], {}):
        res, al = t.tts_with_timings(text, word_pitches=wp, **kw)
        assert torch.equal(res, plain) and CC._same(al, al0) and "stretch_s" not in t.timings and "pitch_s" not in t.timings
    assert ReferenceWarpResampleStage.made == [] and ReferenceWarpStage.made == [] and t.warp_resampler is None and t.warp_stretcher is None
    # one word two semitones up: ONE stretch and ONE resampling along the map of the plain clip's words; the timings are the returned clip's
    span = al0.words[1][2] - al0.words[1][1]
    assert span >= 4
    pm = rs.PitchMap.from_words(al0, {1: 2})
    chain = rs.WarpChain(pm.n, pm.starts, [65536] * len(pm.starts), pm.pqs)
    for wp in ({1: 2}, [None, 2]):
        ReferenceWarpStage.calls, ReferenceWarpResampleStage.calls = [], []
        res, al = t.tts_with_timings(text, word_pitches=wp, **kw)
        assert ReferenceWarpStage.calls == [1] and ReferenceWarpResampleStage.calls == [1] and t.pitch_maps[0].table == pm.table
        assert torch.equal(res, _by_hand(plain, chain)) and al.samples == res.shape[-1] == chain.n_out and CC._same(al, CC._expected(m, res, text))
        assert abs(res.shape[-1] - plain.shape[-1]) <= rs.duration_bound(len(pm.starts), plain.shape[-1]) and t.timings["pitch_s"] >= 0
    # with word_rates, a base rate and a base pitch: the segments are the union, the durations len_i / rate_i
    res, _ = t.tts_with_timings(text, word_pitches={1: 3}, word_rates={0: 0.8}, speaking_rate=1.25, pitch=1, **kw)
    rm, pm = stretch.RateMap.from_words(al0, {0: 0.8}, base=1.25), rs.PitchMap.from_words(al0, {1: 3}, base=1)
    assert t.rate_maps[0].table == rm.table and t.pitch_maps[0].table == pm.table
    chain = rs.WarpChain(al0.samples, *rs.merge_maps(al0.samples, list(zip(rm.starts, rm.rqs)), list(zip(pm.starts, pm.pqs))))
    assert torch.equal(res, _by_hand(plain, chain))
    S = len(chain.starts)
    assert abs(res.shape[-1] - chain.ideal(S)) <= rs.duration_bound(S, chain.ideal(S))
    # k winners and return_deterministic_state
    (two, state), als = t.tts_with_timings(text, word_pitches={0: -2}, k=2, return_deterministic_state=True, **kw)
    plain2, als2 = t.tts_with_timings(text, k=2, **kw)
    assert state[0] == 7 and len(two) == len(als) == 2
    for y, p, a in zip(two, plain2, als2):
        pm = rs.PitchMap.from_words(a, {0: -2})
        assert torch.equal(y, _by_hand(p, rs.WarpChain(pm.n, pm.starts, [65536] * len(pm.starts), pm.pqs)))
    # refusals
    for bad, what in ((1.5, "a list with one pitch in semitones per word"), ([2], "1 pitches for the 2 words"), ({2: 1}, "word index 2"),
                      ({0: 12.5}, "word 0")):
        with pytest.raises(ValueError, match=what):
            t.tts_with_timings(text, word_pitches=bad, **kw)
    with pytest.raises(ValueError, match=r"word 1 \('there'\): speaking rate 0\.5000 at pitch ratio 1\.1892"):
        t.tts_with_timings(text, word_pitches={1: 3}, word_rates={1: 0.5}, **kw)
    for extra in (dict(formants="keep"), dict(formant_shift=2)):
        with pytest.raises(ValueError, match="do not go with a pitch that changes inside the clip"):
            t.tts_with_timings(text, word_pitches={1: 2}, **extra, **kw)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (tts() itself has no word timings to go by)
        t.tts(text, word_pitches={0: 2}, **kw)
    with pytest.raises(ValueError, match="tts_many: word_pitches is not available"):
        t.tts_many([text], word_pitches={0: 2}, **kw)
    from tortoise_tts_amd import longform
    with pytest.raises(ValueError, match="read_long_form: word_pitches is not available"):
        longform.read_long_form(t, text, word_pitches={0: 2})
    t.world = 2
    with pytest.raises(ValueError, match="sharded job"):
        t.tts_with_timings(text, word_pitches={0: 2}, **kw)


@torch.no_grad()
def test_streams_refuse_word_pitches(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    one = make(1)
    with pytest.raises(ValueError, match="word_pitches is not available"):
        next(one.tts_stream(TEXTS[0], word_pitches={0: 2}, **KW))
    with pytest.raises(ValueError, match="tts_many: word_pitches is not available"):
        one.tts_many(TEXTS[:1], word_pitches={0: 2}, **KW)
    many = make(3)
    with pytest.raises(ValueError, match="word_pitches is not available"):
        many.open_stream(TEXTS[0], word_pitches={0: 2}, **KW)
    with pytest.raises(ValueError, match="word_pitches is not available"):
        next(many.tts_stream_many(TEXTS[:2], word_pitches=[2], **KW))
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.WarpResampleStage)  # (no handle: the checks come before any device work)
    st.h = None
    st.max_samples, st.max_clips, st.max_segments = 1000, 16, 2
    with pytest.raises(ValueError, match="1001 samples"):
        st.resample_many([torch.zeros(1001)], [[(0, 0, 0, 65536)]])
    with pytest.raises(ValueError, match="at least one sample"):
        st.resample_many([torch.zeros(0)], [[(0, 0, 0, 65536)]])
    with pytest.raises(ValueError, match=r"3 segments \(1 \.\. 2\)"):
        st.resample_many([torch.zeros(10)], [rs.map_plan(10, [0, 3, 6], [65536] * 3)])
    with pytest.raises(ValueError, match="breaks a rule"):
        st.resample_many([torch.zeros(10)], [[(0, 0, 0, 65536), (5, 6, 0, 65536)]])
    with pytest.raises(ValueError, match="2 clips with 1 pitch maps"):
        st.resample_many([torch.zeros(10), torch.zeros(10)], [[(0, 0, 0, 65536)]])


# ----------------------------------------------------------------------------------------- the host code under the sanitizers
def test_host_check_builds_and_passes_under_the_sanitizers(tmp_path):
    """csrc/checks/rsw_host_check.cpp: a stand-alone program (its own main) over resample_warp_host.h, compiled with ASan + UBSan and run on
    the CPU - random plans against the rules, every refusal, the 64-bit edges."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    src = os.path.join(ROOT, "tortoise_tts_amd", "csrc", "checks", "rsw_host_check.cpp")
    exe = str(tmp_path / "rsw_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rsw_host_check: ok" in r.stdout, r.stdout + r.stderr
