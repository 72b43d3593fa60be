"""What the silence stage (csrc/silence.hip) costs on a rendered clip.  A record, not a gate.

    python scripts/silence_time.py [--out profiles/rNN_silence.txt]      (default: the next free round prefix)

  time     ONE process: tt_sil_find and tt_sil_trim on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz: bursts of speech-like signal,
           pauses of exact zeros and of noise 60 dB down, tests/silence_reference.py) in isolation: device events around the call alone,
           inputs resident on the device, a FRESH input buffer for every repeat (no repeat finds its audio in a cache because the one before
           read it), median and spread of 25 repeats after 3 warm-up calls on buffers of their own.  With every case the bytes it moves
           (DESIGN.md 5.28 computes the floor from them).  Then the same batches through TextToSpeech.trim_many / speech_regions_many from
           host tensors (upload, call, results back; host clock around a call that ends synchronised), and what a tts() call that gives
           neither keyword pays: silence.options on its kwargs.
  trace    the same calls, three each, under `rocprofv3 --kernel-trace --stats`: the kernels' own time.
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
PARTS = [("l", 9000), ("s", 40000), ("z", 12000), ("s", 30000), ("l", 20000), ("s", 50000), ("z", 6000), ("s", 35000), ("l", 20720)]
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400


def batch_call(st, n, trim, base, p):
    """One tt_sil_trim / tt_sil_find call over n clips -> (closure, status tensor); its buffers are its own."""
    import numpy as np
    import torch
    from tests import silence_reference as R
    from tortoise_tts_amd import engine as E
    cap = R.max_regions(SAMPLES)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 240 * 7 * i) for i in range(n)])).cuda()
    io, ro = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, cap))
    thr = torch.tensor([p[:2]] * n, dtype=torch.float64).cuda()
    par = torch.tensor([p[2:7] if trim else p[2:4]] * n, dtype=torch.int32).cuda()
    y = torch.zeros(n * SAMPLES).cuda()
    ints = [torch.zeros(n, dtype=torch.int32).cuda() for _ in range(3)]
    reg, seg = torch.zeros(2 * n * cap, dtype=torch.int32).cuda(), torch.zeros(3 * n * cap, dtype=torch.int32).cuda()
    peak, status = torch.zeros(n, dtype=torch.float64).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        if trim:
            E.check(st.lib.tt_sil_trim(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(thr), E.ptr(par), E.ptr(ro), E.ptr(ro), E.ptr(y), E.ptr(ints[0]),
                                       E.ptr(ints[1]), E.ptr(reg), E.ptr(ints[2]), E.ptr(seg), E.ptr(peak), E.ptr(status), E.stream_ptr()))
        else:
            E.check(st.lib.tt_sil_find(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(thr), E.ptr(par), E.ptr(ro), None, E.ptr(ints[1]), E.ptr(reg),
                                       E.ptr(peak), None, E.ptr(status), E.stream_ptr()))
    return call, status, ints[0]


def child(timed):
    import numpy as np
    import torch
    from tests import silence_reference as R
    from tortoise_tts_amd import silence as sil
    from tortoise_tts_amd import stages
    res = {}
    st = stages.SilenceStage(SAMPLES, max_clips=16)
    repeats, warm = (REPEATS, WARM) if timed else (3, 0)
    bases = [R.build(PARTS, s) for s in range(4)]
    assert all(len(b) == SAMPLES for b in bases)
    p = R.params(max_pause=7200)
    ref = R.analyse(bases[0], p)
    for what, trim in (("find", False), ("trim", True)):
        for n in CLIPS:
            calls = [batch_call(st, n, trim, np.roll(bases[r % 4], 240 * 11 * r), p) for r in range(repeats + warm)]
            torch.cuda.synchronize()
            ms = []
            for r, (call, status, n_out) in enumerate(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                assert status.cpu().tolist() == [0] * n
                if r >= warm:
                    ms.append(a.elapsed_time(b))
            key = "%s_x%d" % (what, n)
            res["call_ms_" + key] = "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(ms), min(ms), max(ms), len(ms))
            out = int(n_out.sum()) if trim else 0
            moved = 4 * (n * SAMPLES * (2 if trim else 1) + out)  # the audio read once (find) or twice (trim), the output written
            res["bytes_" + key] = "%d clips x %d samples read %s, %d samples written = %.2f MB; %.1f GB/s at the median" % (
                n, SAMPLES, "twice" if trim else "once", out, 1e-6 * moved, 1e-6 * moved / statistics.median(ms))
            del calls
    res["clip"] = "%d regions, %d segments, %d of %d samples kept (default detection, lead 0.05 s, trail 0.1 s, max_pause 0.3 s)" % (
        len(ref["regions"]), len(ref["segments"]), ref["n_out"], SAMPLES)
    st.close()
    if timed:
        from tortoise_tts_amd import api

        class Host(api._Common):
            device = torch.device("cuda")

        h = Host()
        for what in ("trim_many", "speech_regions_many"):
            for n in CLIPS:
                ms = []
                for r in range(WARM + 10):
                    clips = [torch.from_numpy(np.roll(bases[(r + i) % 4], 240 * (5 * r + i)).copy()) for i in range(n)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if what == "trim_many":
                        h.trim_many(clips, max_pause=0.3)
                    else:
                        h.speech_regions_many(clips)
                    torch.cuda.synchronize()
                    if r >= WARM:
                        ms.append(1e3 * (time.perf_counter() - t0))
                res["%s_host_ms_x%d" % (what, n)] = "median %.3f  min %.3f  max %.3f  (10 repeats, CPU tensors in and out)" % (
                    statistics.median(ms), min(ms), max(ms))
        t0 = time.perf_counter()
        for _ in range(100000):
            sil.options({})
        res["keywords_off_us_per_tts_call"] = "%.3f (silence.options on kwargs without trim_silence= / max_pause=: two dict lookups; no stage is built)" % (
            1e6 * (time.perf_counter() - t0) / 100000)
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
                log("%-36s %s" % (k, v))


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
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_silence.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# silence stage (tt_sil_find / tt_sil_trim) on clips of %d samples (%.2f s at 24 kHz); slot tiles of 64 x 120 samples, one plan "
        "workgroup per clip, render tiles of 1024 outputs" % (SAMPLES, SAMPLES / 24000))
    log("## one process, device events around the call, a fresh input buffer per repeat: <call>_x<clips per call>")
    run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every batch above, three calls each")
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "sil_" in row:
                    log(row)


if __name__ == "__main__":
    main()
