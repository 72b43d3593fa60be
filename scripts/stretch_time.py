"""What the WSOLA time-stretch (csrc/tsm.hip) costs on a rendered clip.  A record, not a gate.

    python scripts/stretch_time.py [--out profiles/rNN_tsm_stretch.txt]      (default: the next free round prefix)

  time     ONE process: tt_tsm_stretch on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the speech-like clips of
           tests/tsm_reference.py) at rates 0.75 and 1.5, in isolation: device events around the call alone, inputs resident on the
           device, a FRESH input buffer for every repeat (no repeat finds its audio in a cache because the one before read it), median
           and spread of 25 repeats after 3 warm-up calls on buffers of their own.  Per-frame time = call time / frames of one clip (the
           clips of a call run side by side, one workgroup each).  Then the same batches through TextToSpeech.stretch_many from host
           tensors (upload, call, offsets back; host clock around a call that ends synchronised).
  trace    the same calls, three each, under `rocprofv3 --kernel-trace --stats`: the kernel's own time.
Each child runs under its own time limit; the first failure ends the run.
"""
import argparse
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = 222720  # 9.28 s
RATES = (0.75, 1.5)
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400


def long_clip(seed):
    """9.28 s of the test family's speech-like audio (pieces of 12,000 samples with their own pitch contours)."""
    import numpy as np
    from tests import tsm_reference as T
    return np.concatenate([T.clip(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES]


def batch_call(st, n, rq, base):
    """One tt_tsm_stretch call over n clips -> (closure, status tensor); its buffers are its own."""
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


def child(timed):
    import numpy as np
    import torch
    from tests import tsm_reference as T
    from tortoise_tts_amd import stages
    res = {}
    st = stages.TimeStretchStage(SAMPLES, max_clips=16)
    repeats, warm = (REPEATS, WARM) if timed else (3, 0)
    bases = [long_clip(s) for s in range(4)]
    for rate in RATES:
        rq = T.rate_q(rate)
        for n in CLIPS:
            calls = [batch_call(st, n, rq, np.roll(bases[r % 4], 4099 * r)) for r in range(repeats + warm)]
            torch.cuda.synchronize()
            ms = []
            for r, (call, status) in enumerate(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                assert status.cpu().tolist() == [0] * n
                if r >= warm:
                    ms.append(a.elapsed_time(b))
            key = "rate%.2f_x%d" % (rate, n)
            res["call_ms_" + key] = "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(ms), min(ms), max(ms), len(ms))
            res["us_per_frame_" + key] = round(1e3 * statistics.median(ms) / T.frames(SAMPLES, rq), 3)
            res["frames_" + key] = T.frames(SAMPLES, rq)
            del calls
    st.close()
    if timed:
        from tortoise_tts_amd import api

        class Host(api._Common):
            device = torch.device("cuda")

        h = Host()
        for rate in RATES:
            for n in CLIPS:
                ms = []
                for r in range(WARM + 10):
                    clips = [torch.from_numpy(np.roll(bases[(r + i) % 4], 811 * r + 13 * i).copy()) for i in range(n)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h.stretch_many(clips, rates=rate)
                    torch.cuda.synchronize()
                    if r >= WARM:
                        ms.append(1e3 * (time.perf_counter() - t0))
                res["stretch_many_host_ms_rate%.2f_x%d" % (rate, n)] = "median %.3f  min %.3f  max %.3f  (10 repeats, CPU tensors in and out)" % (
                    statistics.median(ms), min(ms), max(ms))
    print("RESULT " + json.dumps(res))


def run_child(args, log):
    cmd = ["timeout", "-k", "10", str(LIMIT)] + args
    log("$ " + " ".join("python" if c == sys.executable else os.path.relpath(c, ROOT) if c.endswith(".py") else "<tmp>" if c.startswith(tempfile.gettempdir()) else c
                        for c in cmd))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            for k, v in json.loads(line[7:]).items():
                log("%-44s %s" % (k, v))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("time", "trace"))
    a = ap.parse_args()
    if a.child:
        return child(a.child == "time")
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_tsm_stretch.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# WSOLA time-stretch (tt_tsm_stretch) of clips of %d samples (%.2f s at 24 kHz); one workgroup per clip" % (SAMPLES, SAMPLES / 24000))
    log("## one process, device events around the call, a fresh input buffer per repeat: rate<speaking rate>_x<clips per call>")
    run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every batch above, three calls each")
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "tsm_" in row:
                    log(row)


if __name__ == "__main__":
    main()
