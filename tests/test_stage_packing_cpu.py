"""What the clip stages' _group methods hand to the library, pinned without a GPU.  Each stage is built with object.__new__ on the CPU, where
a tensor's data_ptr() is a host address, with a `lib` that forwards the host length functions to the real library and replaces the one
device entry point by a Python stand-in.  The stand-in reads every table at the address it was given ((C.c_int32 * k).from_address(p)),
writes recognisable values (an arange from a base of its own) into every output array, and the test finds those values back in the per-clip
results.  Four clips with max_clips = 3: every call splits into groups of 3 and 1."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tortoise_tts_amd import engine as E
from tortoise_tts_amd import formant as fmt
from tortoise_tts_amd import pitch as f0m
from tortoise_tts_amd import resample as rs
from tortoise_tts_amd import silence as sil
from tortoise_tts_amd import stages
from tortoise_tts_amd import stretch as tsm

LENS = (700, 1, 1300, 960)
GROUPS = ((0, 3), (3, 4))
_NP = {C.c_int32: np.int32, C.c_float: np.float32, C.c_double: np.float64}


def _real():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


@pytest.fixture(autouse=True)
def _no_stream(monkeypatch):
    monkeypatch.setattr(E, "stream_ptr", lambda: 0)


def _view(p, k, ct):
    """k elements of C type ct at the host address p, as a writable numpy view."""
    k = int(k)
    return np.frombuffer((ct * k).from_address(p), dtype=_NP[ct]) if k else np.zeros(0, _NP[ct])


class _Call:
    """One call of a stand-in: the tables it read, the values it wrote and where it wrote them."""

    def __init__(self, index, first, n):
        self.index, self.first, self.n, self.tab, self.out, self.spans = index, first, n, {}, {}, []

    def read(self, name, p, k, ct=C.c_int32):
        self.tab[name] = _view(p, k, ct).copy()
        return self.tab[name]

    def fill(self, name, p, k, ct=C.c_int32, values=None):
        """`values`, or an arange from a base that no other output array and no other call shares, into the k elements at p."""
        v = _view(p, k, ct)
        v[:] = 1000000 * (self.index + 1) + 20000 * len(self.out) + np.arange(int(k)) if values is None else values
        self.out[name] = v.copy()
        self.spans.append((p, int(k) * C.sizeof(ct), name))
        return self.out[name]

    def outputs_apart(self):
        """Every output array that holds anything has an address of its own and overlaps no other."""
        live = sorted(s for s in self.spans if s[1])
        assert len({p for p, _, _ in live}) == len(live)
        for (p0, b0, n0), (p1, _, n1) in zip(live, live[1:]):
            assert p0 + b0 <= p1, f"{n0} runs into {n1}"

    def tables(self, **want):
        for name, v in want.items():
            assert self.tab[name].dtype == np.asarray(v).dtype and self.tab[name].tolist() == np.asarray(v).tolist(), name

    def audio(self, clips, io, width=1):
        """Clip i stands at audio + 4 * width * io[i], and one pad element (of `width` values) follows the last clip."""
        a = self.tab["audio"]
        assert a.shape[0] == width * (int(io[-1]) + 1) and not a[width * int(io[-1]):].any()
        for i, x in enumerate(clips):
            assert np.array_equal(a[width * io[i]:width * io[i + 1]], x.reshape(-1).numpy())


class _Lib:
    """The real library for everything but `entries`: name -> stand-in(call, *arguments between n_clips and the stream)."""

    def __init__(self, **entries):
        self._real_lib, self.calls = _real(), []
        for name, fn in entries.items():
            setattr(self, name, self._entry(fn))

    def __getattr__(self, name):
        return getattr(self._real_lib, name)

    def _entry(self, fn):
        def entry(h, n, *args):
            assert h is None and args[-1] == 0  # (the stage's handle and E.stream_ptr())
            self.calls.append(_Call(len(self.calls), sum(c.n for c in self.calls), n))
            fn(self.calls[-1], *args[:-1])
            return 0
        return entry

    def sizes(self):
        return [c.n for c in self.calls]


def _stage(cls, lib, **attrs):
    st = object.__new__(cls)
    st.h, st.lib, st.device, st.max_clips = None, lib, torch.device("cpu"), 3
    for k, v in attrs.items():
        setattr(st, k, v)
    return st


def _clips(lens=LENS):
    return [torch.arange(m, dtype=torch.float32) + 10000 * (i + 1) for i, m in enumerate(lens)]


def _off(counts):
    return np.concatenate(([0], np.cumsum(list(counts)))).astype(np.int32)


def _i32(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1)


def _same(got, want, dtype):
    """A returned slice (tensor or numpy) is `want` to the bit, in the dtype the stage returns."""
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == dtype and got.shape == np.asarray(want).shape and np.array_equal(got, want)


def _refused(run, status, bad, text):
    """A status the stage does not accept, written by the stand-in for clip 1, raises the stage's RuntimeError."""
    status[1] = bad
    with pytest.raises(RuntimeError, match=re.escape(text)):
        run()


# ----------------------------------------------------------------------------------------- time-stretch
def test_time_stretch_packing():
    real, clips, rqs = _real(), _clips(), [49152, 65536, 98304, 131072]
    status = [E.TSM_OK] * 4

    def stretch(c, audio, in_off, rq, out, out_off, offsets, frame_off, st):
        io, oo, fo = c.read("io", in_off, c.n + 1), c.read("oo", out_off, c.n + 1), c.read("fo", frame_off, c.n + 1)
        c.read("rq", rq, c.n)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("y", out, oo[-1], C.c_float)
        c.fill("offsets", offsets, fo[-1])
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    lib = _Lib(tt_tsm_stretch=stretch)
    res = _stage(stages.TimeStretchStage, lib, max_samples=2000).stretch_many(clips, rqs)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io = _off(LENS[a:b])
        oo = _off(real.tt_tsm_out_samples(m, r) for m, r in zip(LENS[a:b], rqs[a:b]))
        fo = _off(real.tt_tsm_frames(m, r) for m, r in zip(LENS[a:b], rqs[a:b]))
        assert all(np.diff(oo) > 0) and all(np.diff(fo) > 0)
        c.tables(io=io, oo=oo, fo=fo, rq=_i32(rqs[a:b]))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        for i, (y, off) in enumerate(res[a:b]):
            _same(y, c.out["y"][oo[i]:oo[i + 1]], np.float32)
            _same(off, c.out["offsets"][fo[i]:fo[i + 1]], np.int32)
    _refused(lambda: _stage(stages.TimeStretchStage, _Lib(tt_tsm_stretch=stretch), max_samples=2000).stretch_many(clips, rqs), status,
             E.TSM_REFUSED, "time-stretch: the device stage refused clips it was handed (status [0, 2, 0])")


def test_warp_stretch_packing():
    real, clips = _real(), _clips()
    tables = [[(0, 0, 49152)], [(0, 0, 65536)], tsm.plan(1300, [0, 600], [98304, 40000]), [(0, 0, 131072)]]
    assert [len(tb) for tb in tables] == [1, 1, 2, 1]
    status = [E.TSW_OK] * 4

    def stretch(c, audio, in_off, seg, seg_off, out, out_off, offsets, frame_off, st):
        io, so = c.read("io", in_off, c.n + 1), c.read("so", seg_off, c.n + 1)
        oo, fo = c.read("oo", out_off, c.n + 1), c.read("fo", frame_off, c.n + 1)
        c.read("seg", seg, 3 * so[-1])
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("y", out, oo[-1], C.c_float)
        c.fill("offsets", offsets, fo[-1])
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    def flat(tb):
        return (C.c_int * (3 * len(tb)))(*[v for row in tb for v in row])

    lib = _Lib(tt_tsw_stretch=stretch)
    res = _stage(stages.WarpStretchStage, lib, max_samples=2000, max_segments=4).stretch_many(clips, tables)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io, so = _off(LENS[a:b]), _off(len(tb) for tb in tables[a:b])
        oo = _off(real.tt_tsw_out_samples(m, len(tb), flat(tb)) for m, tb in zip(LENS[a:b], tables[a:b]))
        fo = _off(real.tt_tsw_frames(m, len(tb), flat(tb)) for m, tb in zip(LENS[a:b], tables[a:b]))
        assert all(np.diff(oo) > 0) and all(np.diff(fo) > 0)
        c.tables(io=io, so=so, oo=oo, fo=fo, seg=_i32([row for tb in tables[a:b] for row in tb]))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        for i, (y, off) in enumerate(res[a:b]):
            _same(y, c.out["y"][oo[i]:oo[i + 1]], np.float32)
            _same(off, c.out["offsets"][fo[i]:fo[i + 1]], np.int32)
    _refused(lambda: _stage(stages.WarpStretchStage, _Lib(tt_tsw_stretch=stretch), max_samples=2000, max_segments=4).stretch_many(clips, tables),
             status, E.TSW_REFUSED, "time-stretch along a rate map: the device stage refused clips it was handed (status [0, 2, 0])")


# ----------------------------------------------------------------------------------------- resampling
def test_resample_packing():
    real, clips, ratios = _real(), _clips(), [(3, 2), (1, 2), (160, 147), (70000, 65536)]
    status = [E.RS_OK] * 4

    def resample(c, audio, in_off, P, Q, out, out_off, peak, st):
        io, oo = c.read("io", in_off, c.n + 1), c.read("oo", out_off, c.n + 1)
        c.read("P", P, c.n)
        c.read("Q", Q, c.n)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("y", out, oo[-1], C.c_float)
        c.fill("peak", peak, c.n, C.c_float)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    lib = _Lib(tt_rs_resample=resample)
    res = _stage(stages.ResampleStage, lib, max_samples=2000).resample_many(clips, ratios)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io = _off(LENS[a:b])
        oo = _off(real.tt_rs_out_samples(m, P, Q) for m, (P, Q) in zip(LENS[a:b], ratios[a:b]))
        assert all(np.diff(oo) > 0)
        c.tables(io=io, oo=oo, P=_i32([P for P, _ in ratios[a:b]]), Q=_i32([Q for _, Q in ratios[a:b]]))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        for i, (y, pk) in enumerate(res[a:b]):
            _same(y, c.out["y"][oo[i]:oo[i + 1]], np.float32)
            assert isinstance(pk, float) and pk == float(c.out["peak"][i])
    _refused(lambda: _stage(stages.ResampleStage, _Lib(tt_rs_resample=resample), max_samples=2000).resample_many(clips, ratios), status,
             E.RS_REFUSED, "resample: the device stage refused clips it was handed (status [0, 2, 0])")


def test_warp_resample_packing():
    real, clips = _real(), _clips()
    tables = [[(0, 0, 0, 98304)], [(0, 0, 0, 40000)], rs.map_plan(1300, [0, 600], [70000, 50000]), [(0, 0, 0, 131072)]]
    assert [len(tb) for tb in tables] == [1, 1, 2, 1]
    status = [E.RSW_OK] * 4

    def resample(c, audio, in_off, seg, seg_off, out, out_off, peak, st):
        io, so, oo = c.read("io", in_off, c.n + 1), c.read("so", seg_off, c.n + 1), c.read("oo", out_off, c.n + 1)
        c.read("seg", seg, 4 * so[-1])
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("y", out, oo[-1], C.c_float)
        c.fill("peak", peak, c.n, C.c_float)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    def flat(tb):
        return (C.c_int * (4 * len(tb)))(*[v for row in tb for v in row])

    lib = _Lib(tt_rsw_resample=resample)
    res = _stage(stages.WarpResampleStage, lib, max_samples=2000, max_segments=4).resample_many(clips, tables)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io, so = _off(LENS[a:b]), _off(len(tb) for tb in tables[a:b])
        oo = _off(real.tt_rsw_out_samples(m, len(tb), flat(tb)) for m, tb in zip(LENS[a:b], tables[a:b]))
        assert all(np.diff(oo) > 0)
        c.tables(io=io, so=so, oo=oo, seg=_i32([row for tb in tables[a:b] for row in tb]))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        for i, (y, pk) in enumerate(res[a:b]):
            _same(y, c.out["y"][oo[i]:oo[i + 1]], np.float32)
            assert isinstance(pk, float) and pk == float(c.out["peak"][i])
    _refused(lambda: _stage(stages.WarpResampleStage, _Lib(tt_rsw_resample=resample), max_samples=2000, max_segments=4).resample_many(clips, tables),
             status, E.RSW_REFUSED, "resample along a pitch map: the device stage refused clips it was handed (status [0, 2, 0])")


# ----------------------------------------------------------------------------------------- silence
_SIL_PARAMS = [sil.Params(0.25 + i, 100.0 + i, 3 + i, 10 + i, 20 + i, 30 + i, 40 + i) for i in range(4)]


def _sil_counts(real, lens):
    """Per clip (n_out, n_regions, n_segments) as the stand-ins report them: within the clip's capacity and not all alike."""
    caps = [real.tt_sil_max_regions(m) for m in lens]
    return ([m - m // 7 for m in lens], [cap - (cap > 1 and i % 2 == 0) for i, cap in enumerate(caps)],
            [cap - (cap > 1 and i % 2 == 1) for i, cap in enumerate(caps)])


def test_silence_find_packing():
    real, clips = _real(), _clips()
    status = [E.SIL_OK, E.SIL_SILENT, E.SIL_OK, E.SIL_SILENT]

    def find(c, audio, in_off, thr, par, reg_off, frm_off, n_regions, regions, peak, energies, st):
        io, ro = c.read("io", in_off, c.n + 1), c.read("ro", reg_off, c.n + 1)
        c.read("thr", thr, 2 * c.n, C.c_double)
        c.read("par", par, 2 * c.n)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        assert (frm_off is None) == (energies is None)
        if energies is not None:
            c.fill("energies", energies, c.read("fo", frm_off, c.n + 1)[-1], C.c_double)
        c.fill("n_regions", n_regions, c.n, values=_sil_counts(real, np.diff(io).tolist())[1])
        c.fill("regions", regions, 2 * ro[-1])
        c.fill("peak", peak, c.n, C.c_double)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    for energies in (False, True):
        lib = _Lib(tt_sil_find=find)
        res = _stage(stages.SilenceStage, lib, max_samples=2000).find_many(clips, _SIL_PARAMS, energies=energies)
        assert lib.sizes() == [3, 1] and len(res) == 4
        for c, (a, b) in zip(lib.calls, GROUPS):
            io, ro = _off(LENS[a:b]), _off(real.tt_sil_max_regions(m) for m in LENS[a:b])
            fo = _off(real.tt_sil_frames(m) for m in LENS[a:b])
            n_reg = _sil_counts(real, LENS[a:b])[1]
            assert b - a == 1 or len(set(n_reg)) > 1
            c.tables(io=io, ro=ro, par=_i32([[p.min_sil, p.pad] for p in _SIL_PARAMS[a:b]]),
                     thr=np.asarray([[p.rel, p.floor_e] for p in _SIL_PARAMS[a:b]], dtype=np.float64).reshape(-1))
            c.audio(clips[a:b], io)
            c.outputs_apart()
            regs = c.out["regions"].reshape(-1, 2)
            for i, d in enumerate(res[a:b]):
                assert sorted(d) == sorted(["status", "peak", "regions"] + ["energies"] * energies)
                assert d["status"] == status[a + i] and d["peak"] == float(c.out["peak"][i])
                assert d["regions"] == [tuple(r) for r in regs[ro[i]:ro[i] + n_reg[i]].tolist()]
                if energies:
                    c.tables(fo=fo)
                    _same(d["energies"], c.out["energies"][fo[i]:fo[i + 1]], np.float64)
    _refused(lambda: _stage(stages.SilenceStage, _Lib(tt_sil_find=find), max_samples=2000).find_many(clips, _SIL_PARAMS), status, E.SIL_REFUSED,
             "silence: the device stage refused clips it was handed (status [0, 4, 0])")


def test_silence_trim_packing():
    real, clips = _real(), _clips()
    status = [E.SIL_OK, E.SIL_UNCHANGED, E.SIL_SILENT, E.SIL_OK]

    def trim(c, audio, in_off, thr, par, reg_off, seg_off, out, n_out, n_regions, regions, n_segments, segments, peak, st):
        io, ro = c.read("io", in_off, c.n + 1), c.read("ro", reg_off, c.n + 1)
        c.read("so", seg_off, c.n + 1)
        c.read("thr", thr, 2 * c.n, C.c_double)
        c.read("par", par, 5 * c.n)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        counts = _sil_counts(real, np.diff(io).tolist())
        c.fill("y", out, io[-1], C.c_float)
        c.fill("n_out", n_out, c.n, values=counts[0])
        c.fill("n_regions", n_regions, c.n, values=counts[1])
        c.fill("regions", regions, 2 * ro[-1])
        c.fill("n_segments", n_segments, c.n, values=counts[2])
        c.fill("segments", segments, 3 * ro[-1])
        c.fill("peak", peak, c.n, C.c_double)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    lib = _Lib(tt_sil_trim=trim)
    res = _stage(stages.SilenceStage, lib, max_samples=2000).trim_many(clips, _SIL_PARAMS)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io, ro = _off(LENS[a:b]), _off(real.tt_sil_max_regions(m) for m in LENS[a:b])
        n_out, n_reg, n_seg = _sil_counts(real, LENS[a:b])
        assert b - a == 1 or (len(set(n_reg)) > 1 and len(set(n_seg)) > 1 and n_reg != n_seg)
        c.tables(io=io, ro=ro, so=ro, par=_i32([[p.min_sil, p.pad, p.lead, p.trail, p.max_pause] for p in _SIL_PARAMS[a:b]]),
                 thr=np.asarray([[p.rel, p.floor_e] for p in _SIL_PARAMS[a:b]], dtype=np.float64).reshape(-1))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        regs, segs = c.out["regions"].reshape(-1, 2), c.out["segments"].reshape(-1, 3)
        for i, (y, d) in enumerate(res[a:b]):
            _same(y, c.out["y"][io[i]:io[i] + n_out[i]], np.float32)
            assert sorted(d) == ["peak", "regions", "segments", "status"]
            assert d["status"] == status[a + i] and d["peak"] == float(c.out["peak"][i])
            assert d["regions"] == [tuple(r) for r in regs[ro[i]:ro[i] + n_reg[i]].tolist()]
            assert d["segments"] == [tuple(s) for s in segs[ro[i]:ro[i] + n_seg[i]].tolist()]
    _refused(lambda: _stage(stages.SilenceStage, _Lib(tt_sil_trim=trim), max_samples=2000).trim_many(clips, _SIL_PARAMS), status, E.SIL_EMPTY,
             "silence: the device stage refused clips it was handed (status [0, 3, 2])")


# ----------------------------------------------------------------------------------------- F0
@pytest.mark.parametrize("dprime", [False, True])
def test_f0_packing(dprime):
    real, clips = _real(), _clips()
    params = [f0m.Params(24 + i, 400 + i, 0.1 + i, 50.0 + i) for i in range(4)]
    status = [E.F0_OK] * 4
    W = E.F0_LAG_MAX + 1

    def track(c, audio, in_off, par, thr, frm_off, lag, f0, aper, n_voiced, st, dpr=None):
        io, fo = c.read("io", in_off, c.n + 1), c.read("fo", frm_off, c.n + 1)
        c.read("par", par, 2 * c.n)
        c.read("thr", thr, 2 * c.n, C.c_double)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("lag", lag, fo[-1])
        c.fill("f0", f0, fo[-1], C.c_float)
        c.fill("aper", aper, fo[-1], C.c_float)
        c.fill("n_voiced", n_voiced, c.n)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])
        if dpr is not None:
            c.fill("dprime", dpr, fo[-1] * W, C.c_double)

    entry = {"tt_op_f0_track" if dprime else "tt_f0_track": track}
    lib = _Lib(**entry)
    res = _stage(stages.F0Stage, lib, max_samples=2000).track_many(clips, params, dprime=dprime)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        io, fo = _off(LENS[a:b]), _off(real.tt_f0_frames(m) for m in LENS[a:b])
        assert all(np.diff(fo) > 0) and ("dprime" in c.out) == dprime
        c.tables(io=io, fo=fo, par=_i32([[p.lag_lo, p.lag_hi] for p in params[a:b]]),
                 thr=np.asarray([[p.thr, p.floor_e] for p in params[a:b]], dtype=np.float64).reshape(-1))
        c.audio(clips[a:b], io)
        c.outputs_apart()
        for i, d in enumerate(res[a:b]):
            assert sorted(d) == sorted(["lag", "f0", "aper", "n_voiced"] + ["dprime"] * dprime)
            _same(d["lag"], c.out["lag"][fo[i]:fo[i + 1]], np.int32)
            _same(d["f0"], c.out["f0"][fo[i]:fo[i + 1]], np.float32)
            _same(d["aper"], c.out["aper"][fo[i]:fo[i + 1]], np.float32)
            assert d["n_voiced"] == int(c.out["n_voiced"][i])
            if dprime:
                _same(d["dprime"], c.out["dprime"].reshape(-1, W)[fo[i]:fo[i + 1]], np.float64)
    _refused(lambda: _stage(stages.F0Stage, _Lib(**entry), max_samples=2000).track_many(clips, params, dprime=dprime), status, E.F0_REFUSED,
             "f0: the device stage refused clips it was handed (status [0, 2, 0])")


# ----------------------------------------------------------------------------------------- loudness
# max_total_samples = 1500: 700 + 1 fit, 1300 does not fit behind them and 960 does not fit behind 1300 -> calls of 2, 1 and 1 clips
@pytest.mark.parametrize("max_total,groups", [(4000, GROUPS), (1500, ((0, 2), (2, 3), (3, 4)))])
def test_loudness_packing(max_total, groups):
    real, clips = _real(), _clips()
    targets, ceilings = [-23.0, -16.5, -30.25, -20.0], [0.5, 0.75, 0.875, 0.25]
    status = [E.LOUD_OK, E.LOUD_SHORT, E.LOUD_SILENT, E.LOUD_OK]

    def measure(c, audio, in_off, hop_off, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, st, more=()):
        io, ho = c.read("io", in_off, c.n + 1), c.read("ho", hop_off, c.n + 1)
        c.read("audio", audio, io[-1] + 1, C.c_float)
        c.fill("lufs", lufs, c.n, C.c_double)
        c.fill("true_peak", true_peak, c.n, C.c_float)
        c.fill("blocks_abs", blocks_abs, c.n)
        c.fill("blocks_rel", blocks_rel, c.n)
        c.fill("hop_energy", hop_energy, ho[-1], C.c_double)
        for name, p in more:
            c.fill(name, p, io[-1] if name == "y" else c.n, C.c_float)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    def normalize(c, audio, in_off, hop_off, target, ceiling, mode, out, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, gain, out_true_peak, st):
        assert mode == E.LOUD_LOOKAHEAD_MODE
        c.read("target", target, c.n, C.c_float)
        c.read("ceiling", ceiling, c.n, C.c_float)
        measure(c, audio, in_off, hop_off, lufs, true_peak, blocks_abs, blocks_rel, hop_energy, st,
                (("y", out), ("gain", gain), ("out_true_peak", out_true_peak)))

    def stage(lib):
        return _stage(stages.LoudnessStage, lib, max_total_samples=max_total)

    for norm in (False, True):
        lib = _Lib(tt_loud_measure=measure, tt_loud_normalize=normalize)
        if norm:
            res = stage(lib).normalize_many(clips, targets, ceilings, E.LOUD_LOOKAHEAD_MODE)
        else:
            res = [(None, r) for r in stage(lib).measure_many(clips)]
        assert lib.sizes() == [b - a for a, b in groups] and len(res) == 4
        for c, (a, b) in zip(lib.calls, groups):
            io, ho = _off(LENS[a:b]), _off(real.tt_loud_hops(m) for m in LENS[a:b])
            c.tables(io=io, ho=ho)
            if norm:
                c.tables(target=np.asarray(targets[a:b], dtype=np.float32), ceiling=np.asarray(ceilings[a:b], dtype=np.float32))
            c.audio(clips[a:b], io)
            c.outputs_apart()
            for i, (y, d) in enumerate(res[a:b]):
                assert sorted(d) == sorted(["status", "lufs", "true_peak", "blocks_abs", "blocks_rel", "hop_energy"] + ["gain", "out_true_peak"] * norm)
                assert d["status"] == status[a + i] and d["lufs"] == float(c.out["lufs"][i]) and d["true_peak"] == float(c.out["true_peak"][i])
                assert d["blocks_abs"] == int(c.out["blocks_abs"][i]) and d["blocks_rel"] == int(c.out["blocks_rel"][i])
                _same(d["hop_energy"], c.out["hop_energy"][ho[i]:ho[i + 1]], np.float64)
                if norm:
                    _same(y, c.out["y"][io[i]:io[i + 1]], np.float32)
                    assert d["gain"] == float(c.out["gain"][i]) and d["out_true_peak"] == float(c.out["out_true_peak"][i])
    lib = _Lib(tt_loud_measure=measure, tt_loud_normalize=normalize)
    _refused(lambda: stage(lib).measure_many(clips), status, E.LOUD_REFUSED,
             f"loudness: the device stage refused clips it was handed (status {[0, 4, 2][:groups[0][1]]})")


# ----------------------------------------------------------------------------------------- formants
def test_formant_packing():
    lens, alphas = (513, 700, 1300, 960), [1.5, 0.75, 1.25, 2.0]
    assert lens[0] == fmt.MIN_SAMPLES
    clips, calls = _clips(lens), []

    def run(h, wav, clip_offsets, clip_lengths, warp_index, k, out, out_offsets, stream):
        assert h is None and stream == 0
        c = _Call(len(calls), sum(x.n for x in calls), k)
        calls.append(c)
        c.tab.update(offs=np.asarray(list(clip_offsets)), lens=np.asarray(list(clip_lengths)), idx=np.asarray(list(warp_index)),
                     out_offs=np.asarray(list(out_offsets)))
        assert C.sizeof(clip_offsets) == C.sizeof(out_offsets) == 8 * k and C.sizeof(clip_lengths) == C.sizeof(warp_index) == 4 * k
        total = int(c.tab["offs"][-1] + c.tab["lens"][-1])
        c.read("wav", wav, total, C.c_float)
        c.fill("y", out, total, C.c_float)
        return 0

    lib = _Lib()
    lib.tt_fmt_run = run
    q = fmt.lifter_q()
    st = _stage(stages.FormantStage, lib, max_samples=2000, fmt=fmt, q=q, slots={}, clock=0,
                t={"warps": torch.zeros(E.FMT_MAX_WARPS, E.FMT_Q_PAD, fmt.BINS_PAD)})
    res = st.correct_many(clips, alphas)
    assert [c.n for c in calls] == [3, 1] and len(res) == 4
    for c, (a, b) in zip(calls, GROUPS):
        offs = _off(lens[a:b])
        assert c.tab["offs"].tolist() == c.tab["out_offs"].tolist() == offs[:-1].tolist() and c.tab["lens"].tolist() == list(lens[a:b])
        assert c.tab["idx"].tolist() == list(range(a, b))  # (a fresh stage fills its warp slots in order)
        for i, (x, y) in enumerate(zip(clips[a:b], res[a:b])):
            assert np.array_equal(c.tab["wav"][offs[i]:offs[i + 1]], x.numpy())
            _same(y, c.out["y"][offs[i]:offs[i + 1]], np.float32)
    for slot, alpha in enumerate(alphas):
        assert st.slots[alpha][0] == slot and torch.equal(st.t["warps"][slot], fmt.warp_table(alpha, q).float())


# ----------------------------------------------------------------------------------------- CTC forced alignment
def test_ctc_packing():
    V, frames, targets = 5, (7, 1, 13, 9), [[1, 2, 3], [4], [2, 1, 4, 3, 2], []]
    logits = [(torch.arange(T * V, dtype=torch.float32) + 10000 * (i + 1)).reshape(T, V) for i, T in enumerate(frames)]
    status = [E.CTC_OK] * 4

    def align(c, lg, frame_off, tg, tok_off, path, spans, conf, score, st):
        fo, to = c.read("fo", frame_off, c.n + 1), c.read("to", tok_off, c.n + 1)
        c.read("targets", tg, to[-1])
        c.read("audio", lg, V * (fo[-1] + 1), C.c_float)
        c.fill("path", path, fo[-1])
        c.fill("spans", spans, 2 * to[-1])
        c.fill("conf", conf, to[-1], C.c_float)
        c.fill("score", score, c.n, C.c_float)
        c.fill("status", st, c.n, values=status[c.first:c.first + c.n])

    def stage(lib):
        return _stage(stages.CtcAlignStage, lib, vocab=V, blank=0, max_frames=20, max_tokens=8)

    lib = _Lib(tt_ctc_align=align)
    res = stage(lib).align_many(logits, targets)
    assert lib.sizes() == [3, 1] and len(res) == 4
    for c, (a, b) in zip(lib.calls, GROUPS):
        fo, to = _off(frames[a:b]), _off(len(t) for t in targets[a:b])
        c.tables(fo=fo, to=to, targets=_i32([t for tg in targets[a:b] for t in tg]))
        c.audio(logits[a:b], fo, width=V)
        c.outputs_apart()
        for i, d in enumerate(res[a:b]):
            assert sorted(d) == ["conf", "path", "score", "spans", "status"] and d["status"] == E.CTC_OK
            _same(d["path"], c.out["path"][fo[i]:fo[i + 1]], np.int32)
            _same(d["spans"], c.out["spans"].reshape(-1, 2)[to[i]:to[i + 1]], np.int32)
            _same(d["conf"], c.out["conf"][to[i]:to[i + 1]], np.float32)
            assert isinstance(d["score"], float) and d["score"] == float(c.out["score"][i])
    # a clip the device could not align comes back with its status alone, the others as before
    status[:] = [E.CTC_OK, E.CTC_INFEASIBLE, E.CTC_REFUSED, E.CTC_EMPTY]
    res = stage(_Lib(tt_ctc_align=align)).align_many(logits, targets)
    assert [sorted(d) for d in res[1:]] == [["status"]] * 3 and [d["status"] for d in res] == status and len(res[0]) == 5
