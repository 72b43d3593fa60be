"""What the resampler along a pitch map (csrc/resample_warp.hip) costs against the whole-clip resampler (csrc/resample.hip), and what the
whole shift_pitch(pitch_map=) chain costs beside shift_pitch(semitones=).  A record, not a gate.

    python scripts/pitchmap_time.py [--out profiles/rNN_pitchmap.txt] [--append "heading"]     (default: the next free round prefix)

ONE process, scripts/tsmap_time.py's method: tt_rsw_resample on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the clips of
tests/resample_reference.py) along maps of 1, 8 and 64 segments around a mean of +3 semitones, INTERLEAVED in the same run with tt_rs_resample
on the same samples at the map's mean ratio (n 65536 / n_out): device events around the call alone, inputs resident on the device, a FRESH
input buffer for every repeat and for each of the two kernels, median and min .. max of 25 repeats after 3 warm-up calls on buffers of
their own.  tt_rs_resample is the only baseline.  The chain is timed on the host around the call with a device synchronisation on either
side (it copies its results' sizes back, so it synchronises anyway).  The child runs under its own time limit.  --append adds the run
under a heading to an existing file (an A/B library selected with TORTOISE_MI355X_LIB).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = 222720  # 9.28 s
SEGMENTS = (1, 8, 64)
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400


def long_clip(seed):
    import numpy as np
    from tests import resample_reference as R
    return np.concatenate([R.clip(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES]


def semitones(S):
    """S equal segments at +3 (one segment) or at +1 / +5 / +2 / +4 in turn: a mean of +3."""
    pattern = (3,) if S == 1 else (1, 5, 2, 4)
    return [(SAMPLES * i // S, pattern[i % len(pattern)]) for i in range(S)]


def map_call(st, n, table, n_out, base):
    """One tt_rsw_resample call over n clips along table -> (closure, status tensor); its buffers are its own."""
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    S = len(table)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, so, oo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, S, n_out))
    seg = torch.tensor([v for row in table for v in row] * n, dtype=torch.int32).cuda()
    y, peak, status = torch.zeros(n * n_out).cuda(), torch.zeros(n).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_rsw_resample(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(seg), E.ptr(so), E.ptr(y), E.ptr(oo), E.ptr(peak), E.ptr(status),
                                       E.stream_ptr()))
    return call, status


def const_call(st, n, P, base):
    """One tt_rs_resample call over n clips at (P, 65536), on the same samples in buffers of its own."""
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import resample as rs
    n_out = rs.out_samples(SAMPLES, P, 65536)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, oo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, n_out))
    Ps, Qs = torch.full((n,), P, dtype=torch.int32).cuda(), torch.full((n,), 65536, dtype=torch.int32).cuda()
    y, peak, status = torch.zeros(n * n_out).cuda(), torch.zeros(n).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_rs_resample(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(Ps), E.ptr(Qs), E.ptr(y), E.ptr(oo), E.ptr(peak), E.ptr(status),
                                      E.stream_ptr()))
    return call, status


def timed(call, status, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    assert status.cpu().tolist() == [0] * n
    return a.elapsed_time(b)


def child():
    import numpy as np
    import torch
    from tortoise_tts_amd import api, resample as rs, stages
    warp = stages.WarpResampleStage(SAMPLES, max_clips=16)
    const = stages.ResampleStage(SAMPLES, max_clips=16)
    bases = [long_clip(s) for s in range(4)]
    med = statistics.median
    fmt = lambda v: "%.1f  (%.1f .. %.1f)" % (med(v), min(v), max(v))
    rows = []
    for S in SEGMENTS:
        pm = rs.PitchMap.from_segments(SAMPLES, semitones(S))
        P = int(round(SAMPLES * 65536 / pm.n_out))
        for n in CLIPS:
            pairs = [(map_call(warp, n, pm.table, pm.n_out, np.roll(bases[r % 4], 4099 * r)), const_call(const, n, P, np.roll(bases[r % 4], 4099 * r)))
                     for r in range(REPEATS + WARM)]
            torch.cuda.synchronize()
            us_map, us_const = [], []
            for r, (m, c) in enumerate(pairs):  # interleaved: map, whole-clip, map, whole-clip, ...
                tm, tc = timed(*m, n), timed(*c, n)
                if r >= WARM:
                    us_map.append(1e3 * tm)
                    us_const.append(1e3 * tc)
            del pairs
            spread = (max(us_const) - min(us_const)) / med(us_const)
            rows.append(dict(segments=S, clips=n, outputs=pm.n_out, mean_ratio=round(P / 65536, 4), map=fmt(us_map), const=fmt(us_const),
                             ratio=round(med(us_map) / med(us_const), 4), spread=round(spread, 4)))
    warp.close()
    const.close()

    class Host(api._Common):
        device = torch.device("cuda")

    h = Host()
    chain = []
    for S in SEGMENTS:
        pm = rs.PitchMap.from_segments(SAMPLES, semitones(S))
        for n in CLIPS:
            clips = [torch.from_numpy(np.roll(bases[i % 4], 997 * i)).cuda() for i in range(n)]
            ms_map, ms_const = [], []
            for r in range(10 + WARM):
                for which, into in ((lambda: h.shift_pitch_many(clips, pitch_maps=[pm] * n), ms_map), (lambda: h.shift_pitch_many(clips, 3), ms_const)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    which()
                    torch.cuda.synchronize()
                    if r >= WARM:
                        into.append(1e3 * (time.perf_counter() - t0))
            chain.append(dict(segments=S, clips=n, map="%.2f  (%.2f .. %.2f)" % (med(ms_map), min(ms_map), max(ms_map)),
                              const="%.2f  (%.2f .. %.2f)" % (med(ms_const), min(ms_const), max(ms_const)), ratio=round(med(ms_map) / med(ms_const), 4)))
    print("RESULT " + json.dumps(dict(kernel=rows, chain=chain)))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--append", metavar="HEADING")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_pitchmap.txt")
    lines = open(out).read().splitlines() + ["", "## " + a.append] if a.append else []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# the resampler along a pitch map (tt_rsw_resample) against the whole-clip resampler (tt_rs_resample): clips of %d samples (%.2f s at "
        "24 kHz), maps around a mean of +3 semitones" % (SAMPLES, SAMPLES / 24000))
    log("# us per call: median (min .. max) of %d repeats after %d warm-up calls, device events around the call alone, a fresh input buffer per "
        "repeat and kernel; the two kernels interleaved in one process, the whole-clip kernel at the map's mean ratio n 65536 / n_out; spread = "
        "(max - min) / median of the whole-clip kernel in that run" % (REPEATS, WARM))
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
            log("%8s %5s %10s %8s  %-26s %-26s %7s %7s" % ("segments", "clips", "mean ratio", "outputs", "map: us / call", "whole-clip: us / call", "ratio",
                                                          "spread"))
            for row in res["kernel"]:
                log("%8d %5d %10.4f %8d  %-26s %-26s %7.4f %7.4f" % (row["segments"], row["clips"], row["mean_ratio"], row["outputs"], row["map"],
                                                                   row["const"], row["ratio"], row["spread"]))
            log("# the whole chain on the host, ms per call (stretch, resample, copies of sizes and peaks): shift_pitch_many(pitch_maps=) beside "
                "shift_pitch_many(semitones=3), median (min .. max) of 10 after %d warm-up calls" % WARM)
            log("%8s %5s  %-26s %-26s %7s" % ("segments", "clips", "pitch_maps=: ms", "semitones=3: ms", "ratio"))
            for row in res["chain"]:
                log("%8d %5d  %-26s %-26s %7.4f" % (row["segments"], row["clips"], row["map"], row["const"], row["ratio"]))


if __name__ == "__main__":
    main()
