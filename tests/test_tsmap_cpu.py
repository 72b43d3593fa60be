"""CPU checks of the time-varying speaking rate (include/tortoise_mi355x_tsw.h, tortoise_tts_amd/stretch.py): the table's integers in
their three spellings (tests/tsmap_reference.py, stretch.py, the built library), the plan's bounds by brute force, every refusal, the fp64
reference along a table against the constant-rate reference, the shared map family, and the host flow (stretch(rate_map=), retime,
tts_with_timings(word_rates=)) on a reference-backed stand-in of the device stage.  The kernel is tests/test_gpu_tsmap.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import tsm_reference as T
from tests import tsmap_reference as M
from tests.test_abi import declared_symbols
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stretch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES_Q = [T.rate_q(r) for r in T.RATES]


def _lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def _arr(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


def _lib_plan(lib, n, starts, rqs):
    out = (C.c_int * (3 * max(1, len(starts))))(*([-7] * (3 * max(1, len(starts)))))
    rc = lib.tt_tsw_plan(n, len(starts), _arr(starts), _arr(rqs), out)
    return rc, [tuple(out[3 * i:3 * i + 3]) for i in range(len(starts))]


def _flat(table):
    return _arr([v for row in table for v in row])


def _random_segments(rng, n, S):
    """S input-domain segments of a clip of n >= 2 S samples, every one (the last too) of at least 2 samples, rates including both ends."""
    cuts = np.sort(rng.choice(np.arange(1, n - S), S - 1, replace=False)) + np.arange(1, S) if S > 1 else np.zeros(0, np.int64)
    pick = lambda: int(rng.choice([T.RATE_MIN, T.RATE_MAX])) if rng.random() < 0.25 else int(rng.integers(T.RATE_MIN, T.RATE_MAX + 1))
    return [(int(b), pick()) for b in [0] + cuts.tolist()]


# ----------------------------------------------------------------------------------------- the integers
def test_one_segment_is_the_constant_rate():
    for n in (1, 300, 769, 5000):
        for rq in RATES_Q:
            table = [(0, 0, rq)]
            assert M.out_samples(n, table) == stretch.table_out_samples(n, table) == T.out_samples(n, rq)
            assert M.frames(n, table) == stretch.table_frames(n, table) == T.frames(n, rq)
            for k in range(1, T.frames(n, rq) + 3):
                assert M.nominal(k, table) == stretch.table_nominal(k, table) == T.nominal(k, rq) == stretch.nominal(k, rq)
            if n >= 2:
                assert M.plan(n, [(0, rq)]) == stretch.plan(n, [0], [rq]) == table
                m = stretch.RateMap.from_segments(n, [(0, rq / 65536)])
                assert (m.table, m.n_out, m.frames) == (table, T.out_samples(n, rq), T.frames(n, rq))


def test_header_is_exported_and_mirrored():
    lib = _lib()
    names = declared_symbols("tortoise_mi355x_tsw.h")
    assert set(names) == set(E._TSW_PROTOS) == {"tt_tsw_abi_version", "tt_tsw_plan", "tt_tsw_out_samples", "tt_tsw_frames", "tt_tsw_create",
                                                "tt_tsw_destroy", "tt_tsw_stretch"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_tsw_abi_version() == 1 == E.TSW_ABI_VERSION
    assert lib.tt_tsm_abi_version() == 1 and lib.tt_tss_abi_version() == 1 and lib.tt_abi_version() == 6  # the other headers are untouched
    assert not [n for n in declared_symbols() if n.startswith("tt_tsw")]
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_tsw.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_TSW_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert defines == dict(TT_TSW_MAX_SEGMENTS=E.TSW_MAX_SEGMENTS, TT_TSW_MIN_SEGMENT=E.TSW_MIN_SEGMENT, TT_TSW_OK=E.TSW_OK,
                           TT_TSW_EMPTY=E.TSW_EMPTY, TT_TSW_REFUSED=E.TSW_REFUSED)
    assert (M.MAX_SEGMENTS, M.MIN_SEGMENT) == (E.TSW_MAX_SEGMENTS, E.TSW_MIN_SEGMENT)
    from tortoise_tts_amd import build
    assert "tsm_warp.hip" in build.SOURCES and any(h.endswith("tortoise_mi355x_tsw.h") for h in build._headers())
    kernel = open(os.path.join(ROOT, "tortoise_tts_amd", "csrc", "tsm_warp.hip")).read()
    for name in ("tsm_store_region", "tsm_search", "tsm_argmax", "tsm_overlap_add", "tsm_next_template", "tsm_fetch_inside", "tsw_out_samples"):
        assert name + "(" in kernel, name  # the kernel is built from the shared steps, and checks the table with the host's code
    h = E.vp()
    for bad in ((0, 1, 1), (E.TSM_MAX_SAMPLES + 1, 1, 1), (100, 0, 1), (100, E.TSM_MAX_CLIPS + 1, 1), (100, 1, 0), (100, 1, E.TSW_MAX_SEGMENTS + 1)):
        assert lib.tt_tsw_create(*bad, C.byref(h)) == -1 and b"tt_tsw_create" in lib.tt_last_error()
    assert lib.tt_tsw_stretch(None, 1, None, None, None, None, None, None, None, None, None, None) == -1 and b"tt_tsw_stretch" in lib.tt_last_error()
    rc = lib.tt_tsw_create(1000, 2, 8, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_tsw_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())


def test_python_mirrors_equal_the_library():
    lib = _lib()
    rng = np.random.default_rng(11)
    for _ in range(400):
        S = int(rng.integers(1, E.TSW_MAX_SEGMENTS + 1))
        n = int(max(2 * S, rng.integers(2, 4000)))
        segs = _random_segments(rng, n, S)
        starts, rqs = [b for b, _ in segs], [rq for _, rq in segs]
        rc, table = _lib_plan(lib, n, starts, rqs)
        assert rc == 0 and table == stretch.plan(n, starts, rqs) == M.plan(n, segs)
        assert lib.tt_tsw_out_samples(n, S, _flat(table)) == stretch.table_out_samples(n, table) == M.out_samples(n, table)
        assert lib.tt_tsw_frames(n, S, _flat(table)) == stretch.table_frames(n, table) == M.frames(n, table)
    # a long clip: the 64-bit products
    n = E.TSM_MAX_SAMPLES
    segs = [(0, T.RATE_MIN), (n // 3, T.RATE_MAX), (n - 2, 98765)]
    rc, table = _lib_plan(lib, n, [b for b, _ in segs], [rq for _, rq in segs])
    assert rc == 0 and table == stretch.plan(n, [b for b, _ in segs], [rq for _, rq in segs]) == M.plan(n, segs)
    assert lib.tt_tsw_out_samples(n, 3, _flat(table)) == stretch.table_out_samples(n, table) == M.out_samples(n, table) > 0
    # tables that break a rule: 0 from all of them
    good = stretch.plan(3000, [0, 1000, 1700], [81920, 52429, 131072])
    edit = lambda at, v: [tuple(v if 3 * i + j == at else good[i][j] for j in range(3)) for i in range(3)]
    bad = [edit(0, 1), edit(1, 1), edit(3, 0), edit(6, good[1][0]), edit(4, good[1][1] + 1), edit(4, good[1][1] - 1), edit(7, good[2][1] + 1),
           edit(2, T.RATE_MIN - 1), edit(5, T.RATE_MAX + 1), edit(8, 0), edit(8, -65536)]
    for table in bad:
        assert lib.tt_tsw_out_samples(3000, 3, _flat(table)) == 0 == stretch.table_out_samples(3000, table), table
        assert lib.tt_tsw_frames(3000, 3, _flat(table)) == 0 == stretch.table_frames(3000, table)
    assert lib.tt_tsw_out_samples(good[2][1], 3, _flat(good)) == 0 == stretch.table_out_samples(good[2][1], good)  # a_(S-1) < n
    assert lib.tt_tsw_out_samples(good[2][1] + 1, 3, _flat(good)) == stretch.table_out_samples(good[2][1] + 1, good) == good[2][0] + 1
    assert lib.tt_tsw_out_samples(3000, 0, _flat(good)) == 0 == stretch.table_out_samples(3000, [])
    assert lib.tt_tsw_out_samples(3000, 65, _flat(good * 22)) == 0 == stretch.table_out_samples(3000, good * 22)
    assert lib.tt_tsw_out_samples(0, 3, _flat(good)) == 0 == lib.tt_tsw_out_samples(3000, 3, None)


def test_plan_stays_within_a_sample_and_positions_do_not_decrease():
    """20 000 random plans, n < 4000, up to 64 segments, rates including both ends: |a_i - b_i| <= 1, and a_k does not decrease."""
    rng = np.random.default_rng(20)
    worst = 0
    for _ in range(20000):
        S = int(rng.integers(1, E.TSW_MAX_SEGMENTS + 1))
        n = int(max(2 * S, rng.integers(2, 4000)))
        segs = _random_segments(rng, n, S)
        table = stretch.plan(n, [b for b, _ in segs], [rq for _, rq in segs])
        dev = max(abs(row[1] - b) for row, (b, _) in zip(table, segs))
        assert dev <= 1, (n, segs)
        worst = max(worst, dev)
        assert stretch.table_out_samples(n, table) > 0  # the plan obeys the table's rules
        K = stretch.table_frames(n, table)
        a = [stretch.table_nominal(k, table) for k in range(1, K)]
        assert all(p <= q for p, q in zip(a, a[1:])) and (not a or a[0] == 0), (n, segs)
    assert worst == 1


def test_anchor_plan_lands_within_its_bound():
    """|m_(i+1) - dst_(i+1)| <= (dst_(i+1) - m_i) / 65536 + 1, from the rounding of the rate and the rounding of the length."""
    rng = np.random.default_rng(21)
    tried = 0
    for _ in range(3000):
        P = int(rng.integers(1, 12))
        n = int(rng.integers(40 * P, 200000))
        src = np.sort(rng.choice(np.arange(10, n - 10), P - 1, replace=False)).tolist() + [n] if P > 1 else [n]
        if any(b - a < 4 for a, b in zip([0] + src, src)):
            continue
        dst, m = [], 0
        for a, b in zip([0] + src, src):
            m += max(2, int(round((b - a) / rng.uniform(0.55, 1.9))))
            dst.append(m)
        try:
            rm = stretch.RateMap.from_anchors(n, list(zip(src, dst)))
        except ValueError as err:  # (the rate is measured from the achieved position: a pair at the edge of the range can leave it)
            assert "need rate" in str(err)
            continue
        tried += 1
        ms = [row[0] for row in rm.table[1:]] + [rm.n_out]
        assert len(ms) == len(dst) and rm.starts == [0] + src[:-1]
        for i, (got, want) in enumerate(zip(ms, dst)):
            assert abs(got - want) <= (want - rm.table[i][0]) / 65536 + 1, (n, src, dst, rm.table)
        assert all(abs(row[1] - b) <= 1 for row, b in zip(rm.table, rm.starts))
    assert tried > 2000
    # a last anchor inside the clip: the rest at rate 1.0; (0, 0) may be given
    rm = stretch.RateMap.from_anchors(5000, [(0, 0), (1000, 1500), (3000, 2800)])
    assert rm.starts == [0, 1000, 3000] and rm.rqs[2] == 65536 and abs(rm.n_out - 4800) <= 2


def test_every_refusal_of_the_plan():
    lib = _lib()
    F, A = stretch.RateMap.from_segments, stretch.RateMap.from_anchors
    cases = [
        (100, [(0, 1.0), (1, 1.0)], "at least 2 samples"), (100, [(0, 1.0), (99, 1.0)], "at least 2 samples"), (1, [(0, 1.0)], "at least 2 samples"),
        (100, [(0, 1.0), (60, 1.0), (40, 1.0)], "segment 1 starts at sample 60 and ends at 40"), (100, [(0, 1.0), (40, 1.0), (40, 1.5)], "at least 2 samples"),
        (100, [(5, 1.0)], "not at 0"), (100, [], r"0 segments \(1 \.\. 64\)"), (1000, [(2 * i, 1.0) for i in range(65)], r"65 segments \(1 \.\. 64\)"),
        (100, [(0, 0.49)], r"segment 0: speaking rate 0\.49"), (100, [(0, 1.0), (50, 2.01)], r"segment 1: speaking rate 2\.01"),
        (100, [(0, float("nan"))], "segment 0"), (0, [(0, 1.0)], "a clip of 0 samples"), (E.TSM_MAX_SAMPLES + 1, [(0, 1.0)], "samples"),
    ]
    for n, segs, what in cases:
        with pytest.raises(ValueError, match=what):
            F(n, segs)
    assert F(1000, [(2 * i, 1.0) for i in range(64)]).n_out == 1000 and F(4, [(0, 1.0), (2, 2.0)]).table == [(0, 0, 65536), (2, 2, 131072)]
    # the library refuses the same plans and writes nothing
    for n, starts, rqs, what in ((100, [0, 1], [65536, 65536], b"at least 2 samples"), (100, [0, 99], [65536, 65536], b"at least 2 samples"),
                                 (100, [0, 60, 40], [65536] * 3, b"at least 2 samples"), (100, [5], [65536], b"not at 0"),
                                 (100, [0, 50], [65536, 32767], b"segment 1: rate 32767"), (100, [0], [131073], b"segment 0: rate 131073"),
                                 (100, [], [], b"0 segments"), (1000, [2 * i for i in range(65)], [65536] * 65, b"65 segments (1 .. 64)"),
                                 (0, [0], [65536], b"a clip of 0 samples")):
        rc, table = _lib_plan(lib, n, starts, rqs)
        assert rc == -1 and what in lib.tt_last_error() and all(row == (-7, -7, -7) for row in table)
        with pytest.raises(ValueError):
            stretch.plan(n, starts, rqs)
    assert lib.tt_tsw_plan(100, 1, None, _arr([65536]), _arr([0, 0, 0])) == -1 and b"null argument" in lib.tt_last_error()
    # anchors: the pair is named
    with pytest.raises(ValueError, match=r"anchors \(0, 0\) -> \(1000, 400\) need rate 2\.5"):
        A(5000, [(1000, 400), (5000, 4400)])
    with pytest.raises(ValueError, match=r"anchors \(1000, 1000\) -> \(2000, 4000\) need rate 0\.33"):
        A(5000, [(1000, 1000), (2000, 4000)])
    with pytest.raises(ValueError, match="both increase"):
        A(5000, [(1000, 1000), (900, 2000)])
    with pytest.raises(ValueError, match="both increase"):
        A(5000, [(1000, 1000), (2000, 1000)])
    with pytest.raises(ValueError, match="beyond the clip"):
        A(5000, [(6000, 6000)])
    with pytest.raises(ValueError, match="no anchors"):
        A(5000, [(0, 0)])
    # with_pitch: the segment is named
    rm = F(5000, [(0, 0.6), (2000, 1.8), (4000, 1.0)])
    assert rm.with_pitch(65536).table == rm.table
    up = rm.with_pitch(77936)  # +3 semitones
    assert up.rqs == [(rq * 65536 + 77936 // 2) // 77936 for rq in rm.rqs] and up.starts == rm.starts
    with pytest.raises(ValueError, match=r"segment 0 \(speaking rate 0\.6000\).*outside"):
        rm.with_pitch(98304)  # 0.6 / 1.5 = 0.4
    with pytest.raises(ValueError, match=r"segment 1 \(speaking rate 1\.8000\).*outside"):
        rm.with_pitch(49152)  # 1.8 / 0.75 = 2.4


# ----------------------------------------------------------------------------------------- the reference
def test_reference_on_one_segment_equals_the_constant_rate_reference():
    for n in (1, 300, 769, 5000):
        for rq in RATES_Q:
            x = T.clip(n, 0)
            a, b = T.stretch(x, rq), M.stretch(x, [(0, 0, rq)])
            assert np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["unambiguous"], b["unambiguous"])
            assert a["y"].shape == b["y"].shape and np.abs(a["y"] - b["y"]).max() <= 1e-12
            c = M.check(x, [(0, 0, rq)], a["y"], a["offsets"])
            assert not c["inadmissible"] and not c["bad_samples"]


def test_map_family_has_enough_unambiguous_clips():
    fam = M.family_reference()
    assert len(fam) == len(M.FAMILY) == 58
    clear = sum(bool(r["unambiguous"].all()) for _, _, r in fam)
    frames_, clear_frames = sum(len(r["offsets"]) - 1 for _, _, r in fam), sum(int(r["unambiguous"][1:].sum()) for _, _, r in fam)
    print(f"[tsmap] family: {len(fam)} clips, {clear} unambiguous in every frame; {clear_frames} of {frames_} frames unambiguous")
    assert clear >= 0.5 * len(fam)
    for (n, seed, name), (x, table, r) in zip(M.FAMILY, fam):
        assert len(x) == n and stretch.table_out_samples(n, table) == len(r["y"]) and stretch.table_frames(n, table) == len(r["offsets"])
        c = M.check(x, table, r["y"], r["offsets"])  # the reference passes its own protocol
        assert not c["inadmissible"] and not c["bad_samples"] and c["y_share"] == 0
    assert max(len(t) for _, t, _ in fam) == 64 and {len(t) for _, t, _ in fam} >= {2, 3, 4}


# ----------------------------------------------------------------------------------------- host flow
class ReferenceWarpStage:
    """stages.WarpStretchStage backed by tests/tsmap_reference.py."""
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, max_segments=64, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceWarpStage.made.append(max_samples)

    def stretch_many(self, clips, tables):
        ReferenceWarpStage.calls.append(len(clips))
        out = []
        for x, table in zip(clips, tables):
            assert x.dim() == 1 and x.shape[0] <= self.max_samples and stretch.table_out_samples(x.shape[0], table) > 0
            r = M.stretch(x.numpy(), table)
            out.append((torch.from_numpy(r["y"]).float(), torch.from_numpy(r["offsets"])))
        return out

    def close(self):
        pass


def _ref(clip, table):
    return torch.from_numpy(M.stretch(clip.reshape(-1).numpy(), table)["y"]).float().reshape(clip.shape[:-1] + (-1,))


def _host(monkeypatch):
    from tests.test_tsm_cpu import ReferenceStretchStage, _tts
    t, kw = _tts(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "WarpStretchStage", ReferenceWarpStage)
    ReferenceWarpStage.made, ReferenceWarpStage.calls = [], []
    return t, kw, ReferenceStretchStage


@torch.no_grad()
def test_stretch_along_a_map_and_retime(monkeypatch):
    t, _, Const = _host(monkeypatch)
    x = torch.from_numpy(T.clip(5000, 0))
    rm = stretch.RateMap.from_segments(5000, [(0, 0.5), (2500, 2.0)])
    for shape in ((5000,), (1, 5000), (1, 1, 5000)):
        y = t.stretch(x.reshape(shape), rate_map=rm)
        assert y.shape == shape[:-1] + (rm.n_out,) and torch.equal(y.reshape(-1), _ref(x, rm.table))
    assert ReferenceWarpStage.made == [30 * 24000] and ReferenceWarpStage.calls == [1, 1, 1] and Const.made == []
    # a list of (start_seconds, rate) is from_segments at 24 kHz; one segment is the constant rate
    assert torch.equal(t.stretch(x, rate_map=[(0.0, 0.5), (2500 / 24000, 2.0)]), _ref(x, rm.table))
    assert torch.equal(t.stretch(x, rate_map=[(0, 1.25)]), t.stretch(x, rate=1.25))
    # several clips, a map each, ONE call; the anchors follow the table
    clips = [x, torch.from_numpy(T.clip(769, 1)).reshape(1, -1), torch.from_numpy(T.clip(300, 1))]
    maps = [rm, [(0, 2.0), (0.01, 0.8)], stretch.RateMap.from_segments(300, [(0, 0.8)])]
    ReferenceWarpStage.calls = []
    out, anchors = t.stretch_many(clips, rate_maps=maps, return_map=True)
    assert ReferenceWarpStage.calls == [3]
    for o, c, m, a in zip(out, clips, maps, anchors):
        m = stretch.rate_map(c.shape[-1], m)
        ref = M.stretch(c.reshape(-1).numpy(), m.table)
        assert torch.equal(o, _ref(c, m.table)) and a.dtype == torch.int64 and a.shape == (m.frames, 2)
        assert a[:, 0].tolist() == [(k - 1) * T.HS for k in range(m.frames)] and a[:, 1].tolist() == M.positions(m.table, ref["offsets"]).tolist()
        assert torch.equal(a, stretch.table_anchors(m.table, ref["offsets"]))
    # exactly one of rate, duration, rate_map
    for kw in (dict(rate=1.25, rate_map=rm), dict(duration=0.2, rate_map=rm), dict(rate=1.25, duration=0.2, rate_map=rm), dict()):
        with pytest.raises(ValueError, match="exactly one"):
            t.stretch(x, **kw)
    with pytest.raises(ValueError, match="3 clips with 2 rate maps"):
        t.stretch_many(clips, rate_maps=maps[:2])
    with pytest.raises(ValueError, match="made for a clip of 5000 samples, this one has 300"):
        t.stretch(clips[2], rate_map=rm)
    with pytest.raises(ValueError, match="a RateMap, or a list"):
        t.stretch(x, rate_map=1.25)
    with pytest.raises(ValueError, match=r"segment 1: speaking rate 3"):
        t.stretch(x, rate_map=[(0, 1.0), (0.1, 3)])
    with pytest.raises(ValueError, match="expected"):
        t.stretch(torch.zeros(2, 100), rate_map=[(0, 1.0)])
    # retime: the dubbing call
    y, a = t.retime(x, anchors=[(1000 / 24000, 1500 / 24000), (3000 / 24000, 2800 / 24000)], duration=5000 / 24000, return_map=True)
    want = stretch.RateMap.from_anchors(5000, [(1000, 1500), (3000, 2800), (5000, 5000)])
    assert torch.equal(y, _ref(x, want.table)) and abs(y.shape[-1] - 5000) <= 2 and a.shape == (want.frames, 2)
    assert all(abs(row[0] - d) <= 1 for row, d in zip(want.table, (0, 1500, 2800)))
    y = t.retime(x, duration=0.25)  # a duration alone: one segment, the rate of stretch(duration=) to a rounding
    assert abs(y.shape[-1] - 6000) <= 1 and y.shape == t.stretch(x, duration=0.25).shape
    outs = t.retime_many([x, clips[2]], [[(0.1, 0.15)], None], durations=[None, 0.02])
    assert torch.equal(outs[0], _ref(x, stretch.RateMap.from_anchors(5000, [(2400, 3600)]).table)) and abs(outs[1].shape[-1] - 480) <= 1
    with pytest.raises(ValueError, match="anchors, a duration or both"):
        t.retime(x)
    with pytest.raises(ValueError, match="positive"):
        t.retime(x, duration=0)
    with pytest.raises(ValueError, match="need rate"):
        t.retime(x, duration=1.0)  # 5000 samples cannot last a second
    with pytest.raises(ValueError, match="2 clips with 1 anchor lists"):
        t.retime_many([x, x], [[(0.1, 0.1)]])


def _alignment(n, spans):
    from tortoise_tts_amd import align
    words = [("w%d" % i, a, b, 1.0) for i, (a, b) in enumerate(spans)]
    return align.Alignment("", [], words, 0.0, n)


def test_rate_map_from_words():
    al = _alignment(24000, [(1000, 5000), (5000, 9000), (12000, 12001), (15000, 20000)])
    F = stretch.RateMap.from_words
    m = F(al, [0.5, None, None, 2.0])
    assert list(zip(m.starts, m.rqs)) == [(0, 65536), (1000, 32768), (5000, 65536), (15000, 131072), (20000, 65536)]
    assert F(al, {0: 0.5, 3: 2.0}).table == m.table
    assert list(zip(F(al, {1: 0.8}, base=1.25).starts, F(al, {1: 0.8}, base=1.25).rqs)) == [(0, 81920), (5000, 52429), (9000, 81920)]
    assert F(al, [0.5, 0.5, None, None]).starts == [0, 1000, 9000]  # neighbours at one rate are one segment
    assert F(al, {2: 0.5}).table == [(0, 0, 65536)] == F(al, [None] * 4).table == F(al, [1.0] * 4).table  # a span under 2 samples owns nothing
    assert F(al, [1.5] * 4, base=1.5).table == [(0, 0, 98304)]
    assert F(_alignment(9000, [(0, 5000), (5000, 9000)]), [0.5, 2.0]).starts == [0, 5000]  # words from the first sample to the last
    for bad, what in (([0.5], "1 rates for the 4 words"), ({4: 0.5}, "word index 4"), ({-1: 0.5}, "word index -1"), ({0: 2.5}, r"word 0 \('w0'\)"),
                      ([None, "x", None, None], r"word 1 \('w1'\)")):
        with pytest.raises(ValueError, match=what):
            F(al, bad)
    with pytest.raises(ValueError, match=r"\[0\.5, 2\.0\]"):
        F(al, {}, base=3.0)
    al.rate = 16000
    with pytest.raises(ValueError, match="16000 Hz"):
        F(al, {})


@torch.no_grad()
def test_word_rates_on_tts_with_timings(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_tsm_cpu import ReferenceStretchStage
    from tests.test_api_flow_cpu import small_setup, voice_latents
    t, m = CC._flow(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "TimeStretchStage", ReferenceStretchStage)
    monkeypatch.setattr(api.stages, "WarpStretchStage", ReferenceWarpStage)
    ReferenceStretchStage.made, ReferenceStretchStage.calls, ReferenceWarpStage.made, ReferenceWarpStage.calls = [], [], [], []
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    text = "hello there"
    plain, al0 = t.tts_with_timings(text, **kw)
    # all rates 1.0 (or none): today's bits, nothing built
    for wr in ([1.0, 1.0], [None, None], {}, {1: 1.0}):
        res, al = t.tts_with_timings(text, word_rates=wr, **kw)
        assert torch.equal(res, plain) and CC._same(al, al0) and "stretch_s" not in t.timings
    assert ReferenceWarpStage.made == [] and t.warp_stretcher is None
    # one word at half speed: ONE stretch along the map of the plain clip's words, and the timings are the returned clip's
    assert al0.words[1][2] - al0.words[1][1] >= 2
    want_map = stretch.RateMap.from_words(al0, {1: 0.5})
    for wr in ({1: 0.5}, [None, 0.5]):
        ReferenceWarpStage.calls = []
        res, al = t.tts_with_timings(text, word_rates=wr, **kw)
        assert ReferenceWarpStage.calls == [1] and ReferenceStretchStage.calls == [] and t.rate_maps[0].table == want_map.table
        assert torch.equal(res, _ref(plain, want_map.table)) and al.samples == res.shape[-1] and CC._same(al, CC._expected(m, res, text))
        assert abs(res.shape[-1] - plain.shape[-1] - (al0.words[1][2] - al0.words[1][1])) <= 2 and "stretch_s" in t.timings
    # with speaking_rate= (the base) and k winners, return_deterministic_state
    (two, state), als = t.tts_with_timings(text, word_rates={0: 2.0}, speaking_rate=0.8, k=2, return_deterministic_state=True, **kw)
    plain2, als2 = t.tts_with_timings(text, k=2, **kw)
    assert state[0] == 7 and len(two) == len(als) == 2
    for y, p, a in zip(two, plain2, als2):
        assert torch.equal(y, _ref(p, stretch.RateMap.from_words(a, {0: 2.0}, base=0.8).table))
    # refusals
    for bad, what in ((1.5, "a list with one rate per word"), ([0.5], "1 rates for the 2 words"), ({2: 0.5}, "word index 2"), ({0: 2.5}, "word 0")):
        with pytest.raises(ValueError, match=what):
            t.tts_with_timings(text, word_rates=bad, **kw)
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (tts() itself has no word timings to go by)
        t.tts(text, word_rates={0: 0.5}, **kw)
    t.world = 2
    with pytest.raises(ValueError, match="sharded job"):
        t.tts_with_timings(text, word_rates={0: 0.5}, **kw)


@torch.no_grad()
def test_pitch_is_folded_into_the_map(monkeypatch):
    from tests import test_ctc_cpu as CC
    from tests.test_api_flow_cpu import small_setup, voice_latents
    from tortoise_tts_amd import resample as rs
    t, _ = CC._flow(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "WarpStretchStage", ReferenceWarpStage)
    ReferenceWarpStage.calls = []
    seen = []
    monkeypatch.setattr(type(t), "_resample_ratios", lambda self, audios, ratios, info: (seen.append(list(ratios)), setattr(self, "_resample_s", 0.0), list(audios))[2])
    kw = dict(conditioning_latents=voice_latents(small_setup()[1]), num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32,
              use_deterministic_seed=7, verbose=False)
    plain, al0 = t.tts_with_timings("hello there", **kw)
    pq = rs.pitch(3)[0]
    res, _ = t.tts_with_timings("hello there", word_rates={1: 0.8}, pitch=3, **kw)
    eff = stretch.RateMap.from_words(al0, {1: 0.8}).with_pitch(pq)
    assert ReferenceWarpStage.calls == [1] and seen == [[(pq, 65536)]] and torch.equal(res, _ref(plain, eff.table))
    with pytest.raises(ValueError, match=r"segment 1 \(speaking rate 0\.5000\)"):  # 0.5 / 2^(3/12) = 0.42: validated per segment
        t.tts_with_timings("hello there", word_rates={1: 0.5}, pitch=3, **kw)


@torch.no_grad()
def test_streams_refuse_word_rates(monkeypatch):
    from tests.test_wide_sessions_cpu import _instances, TEXTS, KW
    api_fast, make = _instances(monkeypatch)
    one = make(1)
    with pytest.raises(ValueError, match="word_rates is not available"):
        next(one.tts_stream(TEXTS[0], word_rates={0: 0.5}, **KW))
    many = make(3)
    with pytest.raises(ValueError, match="word_rates is not available"):
        many.open_stream(TEXTS[0], word_rates={0: 0.5}, **KW)
    with pytest.raises(ValueError, match="word_rates is not available"):
        next(many.tts_stream_many(TEXTS[:2], word_rates=[0.5], **KW))
    assert not many._sessions


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.WarpStretchStage)  # (no handle: the checks come before any device work)
    st.h = None
    st.max_samples, st.max_clips, st.max_segments = 1000, 16, 2
    with pytest.raises(ValueError, match="1001 samples"):
        st.stretch_many([torch.zeros(1001)], [[(0, 0, 65536)]])
    with pytest.raises(ValueError, match="at least one sample"):
        st.stretch_many([torch.zeros(0)], [[(0, 0, 65536)]])
    with pytest.raises(ValueError, match=r"3 segments \(1 \.\. 2\)"):
        st.stretch_many([torch.zeros(10)], [stretch.plan(10, [0, 3, 6], [65536] * 3)])
    with pytest.raises(ValueError, match="breaks a rule"):
        st.stretch_many([torch.zeros(10)], [[(0, 0, 65536), (5, 6, 65536)]])
    with pytest.raises(ValueError, match="2 clips with 1 rate maps"):
        st.stretch_many([torch.zeros(10), torch.zeros(10)], [[(0, 0, 65536)]])
