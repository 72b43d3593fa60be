"""What the time-stretch along a rate map (csrc/tsm_warp.hip) costs per frame against the constant-rate kernel (csrc/tsm.hip).  A record, not
a gate.

    python scripts/tsmap_time.py [--out profiles/rNN_tsmap.txt]      (default: the next free round prefix)

ONE process, scripts/stretch_time.py's method: tt_tsw_stretch on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the speech-like clips
of tests/tsm_reference.py) along maps of 1, 8 and 64 segments, INTERLEAVED in the same run with tt_tsm_stretch on the same samples at the
map's mean rate (n / n_out): device events around the call alone, inputs resident on the device, a FRESH input buffer for every repeat and
for each of the two kernels, median and min .. max of 25 repeats after 3 warm-up calls on buffers of their own.  Per-frame time = call
time / frames of one clip (the clips of a call run side by side, one workgroup each).  The child runs under its own time limit.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = 222720  # 9.28 s
SEGMENTS = (1, 8, 64)
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400


def long_clip(seed):
    import numpy as np
    from tests import tsm_reference as T
    return np.concatenate([T.clip(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES]


def rate_map(S):
    """S equal segments at 0.75 (one segment) or at 0.6 / 1.5 / 0.9 / 1.25 in turn."""
    from tortoise_tts_amd import stretch
    rates = (0.75,) if S == 1 else (0.6, 1.5, 0.9, 1.25)
    return stretch.RateMap.from_segments(SAMPLES, [(SAMPLES * i // S, rates[i % len(rates)]) for i in range(S)])


def map_call(st, n, rm, base):
    """One tt_tsw_stretch call over n clips along rm -> (closure, status tensor); its buffers are its own."""
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    S = len(rm.table)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, so, oo, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, S, rm.n_out, rm.frames))
    seg = torch.tensor([v for row in rm.table for v in row] * n, dtype=torch.int32).cuda()
    y, off, status = torch.zeros(n * rm.n_out).cuda(), torch.zeros(n * rm.frames, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_tsw_stretch(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(seg), E.ptr(so), E.ptr(y), E.ptr(oo), E.ptr(off), E.ptr(fo),
                                      E.ptr(status), E.stream_ptr()))
    return call, status


def const_call(st, n, rq, base):
    """One tt_tsm_stretch call over n clips at rq, on the same samples in buffers of its own."""
    import numpy as np
    import torch
    from tests import tsm_reference as T
    from tortoise_tts_amd import engine as E
    n_out, K = T.out_samples(SAMPLES, rq), T.frames(SAMPLES, rq)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, oo, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, n_out, K))
    rqs = torch.full((n,), rq, dtype=torch.int32).cuda()
    y, off, status = torch.zeros(n * n_out).cuda(), torch.zeros(n * K, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_tsm_stretch(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(rqs), E.ptr(y), E.ptr(oo), E.ptr(off), E.ptr(fo), E.ptr(status),
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
    from tests import tsm_reference as T
    from tortoise_tts_amd import stages
    warp = stages.WarpStretchStage(SAMPLES, max_clips=16)
    const = stages.TimeStretchStage(SAMPLES, max_clips=16)
    bases = [long_clip(s) for s in range(4)]
    rows = []
    for S in SEGMENTS:
        rm = rate_map(S)
        rq = int(round(SAMPLES * 65536 / rm.n_out))
        K_map, K_const = rm.frames, T.frames(SAMPLES, rq)
        for n in CLIPS:
            pairs = [(map_call(warp, n, rm, np.roll(bases[r % 4], 4099 * r)), const_call(const, n, rq, np.roll(bases[r % 4], 4099 * r)))
                     for r in range(REPEATS + WARM)]
            torch.cuda.synchronize()
            us_map, us_const = [], []
            for r, (m, c) in enumerate(pairs):  # interleaved: map, constant, map, constant, ...
                tm, tc = timed(*m, n), timed(*c, n)
                if r >= WARM:
                    us_map.append(1e3 * tm / K_map)
                    us_const.append(1e3 * tc / K_const)
            del pairs
            med = lambda v: statistics.median(v)
            rows.append(dict(segments=S, clips=n, frames_map=K_map, frames_const=K_const, mean_rate=round(rq / 65536, 4),
                             map="%.3f  (%.3f .. %.3f)" % (med(us_map), min(us_map), max(us_map)),
                             const="%.3f  (%.3f .. %.3f)" % (med(us_const), min(us_const), max(us_const)),
                             ratio=round(med(us_map) / med(us_const), 4),
                             inside=bool(min(us_const) <= med(us_map) <= max(us_const))))
    warp.close()
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
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_tsmap.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# WSOLA along a rate map (tt_tsw_stretch) against the constant rate (tt_tsm_stretch): clips of %d samples (%.2f s at 24 kHz), one "
        "workgroup per clip" % (SAMPLES, SAMPLES / 24000))
    log("# us per frame: median (min .. max) of %d repeats after %d warm-up calls, device events around the call alone, a fresh input buffer per "
        "repeat and kernel; the two kernels interleaved in one process, the constant rate at the map's mean rate n / n_out" % (REPEATS, WARM))
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    log("%8s %5s %10s %7s  %-28s %-28s %7s  %s" % ("segments", "clips", "mean rate", "frames", "map: us / frame", "constant: us / frame", "ratio",
                                                 "map's median inside the constant's min .. max"))
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            for row in json.loads(line[7:]):
                log("%8d %5d %10.4f %7d  %-28s %-28s %7.4f  %s" % (row["segments"], row["clips"], row["mean_rate"], row["frames_map"], row["map"],
                                                                 row["const"], row["ratio"], "yes" if row["inside"] else "no"))


if __name__ == "__main__":
    main()
