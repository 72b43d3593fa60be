"""What the formant correction (csrc/formant.hip) costs against the forward STFT alone and against the time-stretch it follows.  A record,
not a gate.

    python scripts/formant_time.py [--out profiles/rNN_formant.txt]      (default: the next free round prefix)

ONE process, DESIGN.md 5.24's method: tt_fmt_run on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the speech-like clips of
tests/tsm_reference.py) at warp 2^(4/12), INTERLEAVED in the same run with tt_mel_spectrum on the same samples (the forward GEMM alone) and
tt_tsm_stretch at rate 1 / 2^(4/12) (the step the correction follows in a pitch shift): device events around the call alone, inputs
resident on the device, a FRESH input buffer for every repeat and for each of the three, median and min .. max of 25 repeats after 3
warm-up calls on buffers of their own.  The child runs under its own time limit.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = 222720  # 9.28 s
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400
SEMITONES = 4
# per frame, padded dimensions: forward 2 * 1024 * 1088, cepstrum 2 * 544 * 64, gain 2 * 64 * 544, inverse 2 * 1088 * 1024
FLOP_PER_FRAME = 2 * 1024 * 1088 + 2 * 544 * 64 + 2 * 64 * 544 + 2 * 1088 * 1024
PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12


def long_clip(seed):
    import numpy as np
    from tests import tsm_reference as T
    return np.concatenate([T.clip(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES]


def batch(n, base):
    import numpy as np
    import torch
    return torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()


def fmt_call(st, n, slot, base):
    import torch
    from tortoise_tts_amd import engine as E
    audio, y = batch(n, base), torch.zeros(n * SAMPLES).cuda()
    offs, lens, wi = (C.c_longlong * n)(*[i * SAMPLES for i in range(n)]), (C.c_int * n)(*[SAMPLES] * n), (C.c_int * n)(*[slot] * n)
    return lambda: E.check(st.lib.tt_fmt_run(st.h, E.ptr(audio), offs, lens, wi, n, E.ptr(y), offs, E.stream_ptr()))


def spectrum_call(lib, h, n, base):
    import torch
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import formant as fmt
    T = 1 + SAMPLES // fmt.HOP
    audio, spec = batch(n, base), torch.zeros(n * T * fmt.BINS_PAD).cuda()
    offs, lens = (C.c_longlong * n)(*[i * SAMPLES for i in range(n)]), (C.c_int * n)(*[SAMPLES] * n)
    ooffs = (C.c_longlong * n)(*[i * T * fmt.BINS_PAD for i in range(n)])
    return lambda: E.check(lib.tt_mel_spectrum(h, E.ptr(audio), offs, lens, n, E.ptr(spec), ooffs, E.stream_ptr()))


def stretch_call(st, n, rq, base):
    import torch
    from tests import tsm_reference as T
    from tortoise_tts_amd import engine as E
    n_out, K = T.out_samples(SAMPLES, rq), T.frames(SAMPLES, rq)
    audio = batch(n, base)
    io, oo, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, n_out, K))
    rqs = torch.full((n,), rq, dtype=torch.int32).cuda()
    y, off, status = torch.zeros(n * n_out).cuda(), torch.zeros(n * K, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()
    return lambda: E.check(st.lib.tt_tsm_stretch(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(rqs), E.ptr(y), E.ptr(oo), E.ptr(off), E.ptr(fo),
                                                 E.ptr(status), E.stream_ptr()))


def timed(call):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def child():
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import formant as fmt
    from tortoise_tts_amd import stages
    p = 2.0 ** (SEMITONES / 12.0)
    st = stages.FormantStage(SAMPLES)
    slot = st._slot(p, set())
    const = stages.TimeStretchStage(SAMPLES, max_clips=16)
    rq = int(round(65536 / p))
    lib = E.init()
    fb = torch.zeros(80, fmt.BINS_PAD).cuda()
    c = E.MelConfig()
    c.n_fft, c.hop, c.n_mels, c.bins_pad, c.power, c.clamp_input = fmt.N_FFT, fmt.HOP, 80, fmt.BINS_PAD, 2, 0
    c.floor, c.max_samples, c.max_clips = 1e-5, SAMPLES, 16
    t = E.MelTables()
    t.basis, t.fb, t.scale = E.ptr(st.t["basis"]), E.ptr(fb), None
    mel = E.vp()
    E.check(lib.tt_mel_create(C.byref(c), C.byref(t), C.byref(mel)))
    bases = [long_clip(s) for s in range(4)]
    frames = 1 + SAMPLES // fmt.HOP
    rows = []
    for n in CLIPS:
        trios = []
        for r in range(REPEATS + WARM):
            base = np.roll(bases[r % 4], 4099 * r)
            trios.append((fmt_call(st, n, slot, base), spectrum_call(lib, mel, n, base), stretch_call(const, n, rq, base)))
        torch.cuda.synchronize()
        ms = [[], [], []]
        for r, trio in enumerate(trios):  # interleaved: correction, spectrum, stretch, correction, ...
            got = [timed(f) for f in trio]
            if r >= WARM:
                for v, g in zip(ms, got):
                    v.append(g)
        del trios
        show = lambda v: "%.3f  (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
        floor_ms = 1e3 * max(n * frames * FLOP_PER_FRAME / PEAK_F32_MFMA, 2 * 4 * n * SAMPLES / PEAK_HBM)
        rows.append(dict(clips=n, frames=frames, formant=show(ms[0]), spectrum=show(ms[1]), stretch=show(ms[2]),
                         us_per_frame=round(1e3 * statistics.median(ms[0]) / (n * frames), 3), floor_ms=round(floor_ms, 4),
                         over_floor=round(statistics.median(ms[0]) / floor_ms, 1), over_spectrum=round(statistics.median(ms[0]) / statistics.median(ms[1]), 2)))
    lib.tt_mel_destroy(mel)
    st.close()
    const.close()
    print("RESULT " + json.dumps(rows))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_formant.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# formant correction (tt_fmt_run, warp 2^(%d/12)) on clips of %d samples (%.2f s at 24 kHz), beside tt_mel_spectrum on the same samples "
        "(the forward GEMM alone) and tt_tsm_stretch at rate 2^(-%d/12) (the step it follows)" % (SEMITONES, SAMPLES, SAMPLES / 24000, SEMITONES))
    log("# ms per call: median (min .. max) of %d repeats after %d warm-up calls, device events around the call alone, a fresh input buffer per "
        "repeat and entry; the three interleaved in one process" % (REPEATS, WARM))
    log("# floor: %.2f MFLOP per frame (padded dimensions) at %.1f TFLOP/s of f32 MFMA, or the clip's bytes in and out at %.0f TB/s, whichever is "
        "larger" % (FLOP_PER_FRAME / 1e6, PEAK_F32_MFMA / 1e12, PEAK_HBM / 1e12))
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    log("%5s %7s  %-28s %-28s %-28s %12s %9s %10s %13s" % ("clips", "frames", "tt_fmt_run: ms", "tt_mel_spectrum: ms", "tt_tsm_stretch: ms", "us / frame",
                                                         "floor ms", "x floor", "x spectrum"))
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            for row in json.loads(line[7:]):
                log("%5d %7d  %-28s %-28s %-28s %12.3f %9.4f %10.1f %13.2f" % (row["clips"], row["frames"], row["formant"], row["spectrum"], row["stretch"],
                                                                              row["us_per_frame"], row["floor_ms"], row["over_floor"], row["over_spectrum"]))


if __name__ == "__main__":
    main()
