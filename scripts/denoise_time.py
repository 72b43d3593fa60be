"""What the spectral-subtraction denoiser (csrc/denoise.hip) costs beside the formant correction, with which it shares three of its five
launches.  A record, not a gate.

    python scripts/denoise_time.py [--out profiles/rNN_denoise.txt] [--against <the parent commit's libtortoise_mi355x.so>] [--digests FILE]

Children of ONE run, each under its own time limit (scripts/formant_time.py's method):
  time     tt_nr_run on 1 and 16 clips of 9.28 s (222,720 samples: 871 frames, the select's register form) INTERLEAVED in the same process
           with tt_fmt_run on the same samples, and with tt_nr_run with the select's long form forced (TTX_NR_SELECT_LONG); then one clip
           of 24 s (2,251 frames: the long form by itself).  Device events around the call alone, inputs resident on the device, a FRESH
           input buffer for every repeat and entry, median and min .. max of 25 repeats after 3 warm-up calls.
  trace    the same calls, three each, under `rocprofv3 --kernel-trace --stats`: every launch alone.
  against  tt_fmt_run through this build and through another build of the library (the parent commit's), alternating in one process with
           plain ctypes: sha256 of every output of formant's test family (tests/test_gpu_formant.py: lengths x warps x clamps) and the
           timing of the 9.28 s clips.  --digests writes the OTHER build's digests as JSON (tests/golden/formant_parent_digests.json).
"""
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts import formant_time as FT  # noqa: E402
from scripts import stretch_time as ST  # noqa: E402

SAMPLES, LONG_SAMPLES = FT.SAMPLES, 576000
REPEATS, WARM = FT.REPEATS, FT.WARM
PEAK_L2, PEAK_HBM = 34.5e12, 8.0e12
# per frame, padded dimensions: forward 2 * 1024 * 1088, inverse 2 * 1088 * 1024 (the select and the gain are not MFMA work)
FLOP_PER_FRAME = 2 * 1024 * 1088 + 2 * 1088 * 1024


def spread(v):
    return "%.3f  (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def nr_call(st, n, samples, base, p):
    import torch
    from tortoise_tts_amd import denoise as nr, engine as E
    audio, y = FT.batch(n, base[:samples]), torch.zeros(n * samples).cuda()
    floor = torch.zeros(n, nr.BINS_PAD).cuda()
    offs, lens, zero = (C.c_longlong * n)(*[i * samples for i in range(n)]), (C.c_int * n)(*[samples] * n), (C.c_int * n)()
    status, cp = (C.c_int * n)(), nr.c_params(p)
    return lambda: E.check(st.lib.tt_nr_run(st.h, E.ptr(audio), offs, lens, zero, zero, C.byref(cp), n, E.ptr(y), offs, E.ptr(floor), status, E.stream_ptr()))


def child(timing):
    import numpy as np
    import torch
    from tortoise_tts_amd import denoise as nr, engine as E, stages
    p = nr.params()
    fm = stages.FormantStage(SAMPLES)
    slot = fm._slot(2.0 ** (FT.SEMITONES / 12.0), set())
    st = stages.DenoiseStage(LONG_SAMPLES)
    lib = E.init()
    bases = [FT.long_clip(s) for s in range(4)]
    long_bases = [np.concatenate([b, np.roll(b, 5003), np.roll(b, 9001)])[:LONG_SAMPLES] for b in bases]
    res = {}

    def with_form(form, f):
        def g():
            prev = lib.ttx_kernel_variant(E.TTX_NR_SELECT_LONG, form)
            try:
                f()
            finally:
                lib.ttx_kernel_variant(E.TTX_NR_SELECT_LONG, prev)
        return g
    reps = REPEATS + WARM if timing else 3
    for n, samples, src in ((1, SAMPLES, bases), (16, SAMPLES, bases), (1, LONG_SAMPLES, long_bases)):
        frames = 1 + samples // nr.HOP
        sets = []
        for r in range(reps):
            base = np.roll(src[r % 4], 4099 * r)
            calls = {"tt_nr_run": with_form(0, nr_call(st, n, samples, base, p)), "tt_nr_run, long select": with_form(1, nr_call(st, n, samples, base, p))}
            if samples == SAMPLES:
                calls["tt_fmt_run"] = FT.fmt_call(fm, n, slot, base)
            sets.append(calls)
        torch.cuda.synchronize()
        ms = {}
        for r, calls in enumerate(sets):  # interleaved: denoise, denoise with the long select, formant, denoise, ...
            for name, f in calls.items():
                t = FT.timed(f)
                if r >= WARM:
                    ms.setdefault(name, []).append(t)
        del sets
        if not timing:
            continue
        key = "%d x %d samples (%d frames)" % (n, samples, frames)
        for name, v in ms.items():
            res["%s: %s ms" % (key, name)] = spread(v)
        med = statistics.median(ms["tt_nr_run"])
        floor_ms = 1e3 * max(n * frames * FLOP_PER_FRAME / FT.PEAK_F32_MFMA, 2 * 4 * n * samples / PEAK_HBM)
        res["%s: floor ms (two GEMMs at peak f32 MFMA, or the clip in and out at HBM peak)" % key] = "%.4f, tt_nr_run is %.1f x" % (floor_ms, med / floor_ms)
        if "tt_fmt_run" in ms:
            res["%s: tt_nr_run / tt_fmt_run" % key] = "%.2f" % (med / statistics.median(ms["tt_fmt_run"]))
        p_bytes = 4.0 * n * frames * nr.BINS
        res["%s: the power once, %.2f MB, from L2 at %.1f TB/s / from HBM at %.0f TB/s" % (key, p_bytes / 1e6, PEAK_L2 / 1e12, PEAK_HBM / 1e12)] = \
            "%.5f / %.5f ms" % (1e3 * p_bytes / PEAK_L2, 1e3 * p_bytes / PEAK_HBM)
        res["%s: long select - register select, ms (medians)" % key] = "%.3f" % (statistics.median(ms["tt_nr_run, long select"]) - med)
    st.close()
    fm.close()
    print("RESULT " + json.dumps(res))


def against(other, digests_out):
    """tt_fmt_run through two builds of the library, alternating, with plain ctypes (the other build need not have this build's entry
    points): the family's outputs byte for byte, and the timing of the 9.28 s clips."""
    import numpy as np
    import torch
    from tests.melfront_reference import probe_signal
    from tortoise_tts_amd import engine as E, formant as fmt
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    Q, lengths, warps, clamps = 48, (513, 1024, 1279, 1280, 4096, 24000), (2.0 ** (4 / 12.0), 2.0 ** (7 / 12.0), 0.5, 2.0, 1.0), (24.0, 6.0)
    tabs = {k: v.cuda().contiguous() for k, v in fmt.tables(Q, list(warps)).items()}
    libs = {}
    for name, path in (("this", E.LIB_PATH), ("other", os.path.abspath(other))):
        lib = C.CDLL(path)
        lib.tt_fmt_create.argtypes, lib.tt_fmt_create.restype = [C.POINTER(E.FmtConfig), C.POINTER(E.FmtTables), C.POINTER(vp)], i
        lib.tt_fmt_run.argtypes, lib.tt_fmt_run.restype = [vp, vp, C.POINTER(ll), C.POINTER(i), C.POINTER(i), i, vp, C.POINTER(ll), vp], i
        lib.tt_fmt_destroy.argtypes, lib.tt_fmt_destroy.restype = [vp], None
        hs = {}
        for db in clamps:
            c = E.FmtConfig()
            c.n_fft, c.hop, c.bins_pad, c.q, c.max_gain_db, c.max_samples, c.max_clips, c.n_warps = fmt.N_FFT, fmt.HOP, fmt.BINS_PAD, Q, db, FT.SAMPLES, 16, len(warps)
            t = E.FmtTables()
            t.basis, t.inverse, t.cepstrum, t.warps = (E.ptr(tabs[k]) for k in ("basis", "inverse", "cepstrum", "warps"))
            h = vp()
            assert lib.tt_fmt_create(C.byref(c), C.byref(t), C.byref(h)) == 0
            hs[db] = h
        libs[name] = (lib, hs)

    def run(name, db, wav, n_clips, samples, wi):
        lib, hs = libs[name]
        y = torch.full((n_clips * samples,), -7.0).cuda()
        offs, lens, w = (ll * n_clips)(*[k * samples for k in range(n_clips)]), (i * n_clips)(*[samples] * n_clips), (i * n_clips)(*[wi] * n_clips)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.tt_fmt_run(hs[db], E.ptr(wav), offs, lens, w, n_clips, E.ptr(y), offs, None)
        b.record()
        b.synchronize()
        assert rc == 0
        return y, a.elapsed_time(b)
    res, digests, same = {}, {}, True
    for db in clamps:
        for n in lengths:
            wav = probe_signal(n, seed=n % 7, sr=24000.0).cuda()
            for wi in range(len(warps)):
                d = {name: hashlib.sha256(run(name, db, wav, 1, n, wi)[0].cpu().numpy().tobytes()).hexdigest() for name in ("this", "other")}
                digests["%d,%d,%g" % (n, wi, db)] = d["other"]
                same = same and d["this"] == d["other"]
    res["tt_fmt_run, %d outputs of the family (lengths x warps x clamps)" % len(digests)] = "BYTE-IDENTICAL in both builds" if same else "DIFFERENT"
    bases = [FT.long_clip(s) for s in range(2)]
    for n in FT.CLIPS:
        ms, dig = {"this": [], "other": []}, {}
        for r in range(WARM + REPEATS):
            wav = FT.batch(n, np.roll(bases[r % 2], 4099 * (r % 2)))
            for name in (("this", "other") if r % 2 == 0 else ("other", "this")):  # (alternating, and in alternating order)
                y, t = run(name, 24.0, wav, n, FT.SAMPLES, 0)
                if r >= WARM:
                    ms[name].append(t)
                if r < 2:
                    dig[(name, r)] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
        same = same and all(dig[("this", r)] == dig[("other", r)] for r in range(2))
        for name in ("this", "other"):
            res["tt_fmt_run, %2d x %d samples, ms, %s build" % (n, FT.SAMPLES, name)] = spread(ms[name])
        res["tt_fmt_run, %2d x %d samples, outputs" % (n, FT.SAMPLES)] = "BYTE-IDENTICAL in both builds" if all(dig[("this", r)] == dig[("other", r)] for r in range(2)) else "DIFFERENT"
    for lib, hs in libs.values():
        for h in hs.values():
            lib.tt_fmt_destroy(h)
    if digests_out:
        with open(digests_out, "w") as f:
            json.dump(digests, f, indent=0, sort_keys=True)
            f.write("\n")
    print("RESULT " + json.dumps(res))
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--against")
    ap.add_argument("--digests")
    ap.add_argument("--child", choices=("time", "trace", "against"))
    a = ap.parse_args()
    if a.child:
        return {"time": lambda: child(True), "trace": lambda: child(False), "against": lambda: against(a.against, a.digests)}[a.child]()
    out = a.out or os.path.join(ROOT, "profiles", ST.next_round_prefix() + "_denoise.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# spectral-subtraction denoiser (tt_nr_run, the defaults, auto mode) beside tt_fmt_run (warp 2^(%d/12)) on the same samples" % FT.SEMITONES)
    log("## one process, the entries interleaved, device events around the call, a fresh input buffer per repeat and entry: median (min .. max) of "
        "%d repeats after %d warm-up calls" % (REPEATS, WARM))
    ST.run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: the same calls, three each - every launch alone (nr_floor_kernel: both forms of the select together)")
    with tempfile.TemporaryDirectory() as d:
        ST.run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "nr_" in row or "fmt_" in row:
                    log(row)
    if a.against:
        log("## tt_fmt_run after its kernels moved to csrc/stft_kernels.h: this build and the parent commit's build alternating in one process")
        ST.run_child(me + ["--child", "against", "--against", a.against] + (["--digests", a.digests] if a.digests else []), log)


if __name__ == "__main__":
    main()
