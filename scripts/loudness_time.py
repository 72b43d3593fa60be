"""What the loudness stage (csrc/loudness.hip) costs on a rendered clip.  A record, not a gate.

    python scripts/loudness_time.py [--out profiles/rNN_loudness.txt]      (default: the next free round prefix)

  time     ONE process: tt_loud_measure and tt_loud_normalize in each mode on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the
           speech-like clips of tests/loudness_reference.py) in isolation: device events around the call alone, inputs resident on the
           device, a FRESH input buffer for every repeat (no repeat finds its audio in a cache because the one before read it), median
           and spread of 25 repeats after 3 warm-up calls on buffers of their own.  Then the same batches through
           TextToSpeech.normalize_many from host tensors (upload, call, readings back; host clock around a call that ends synchronised).
  trace    the same calls, three each, under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
Each child runs under its own time limit; the first failure ends the run.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_time as ST  # noqa: E402  (run_child and next_round_prefix: the same protocol, the same limits)
SAMPLES = 222720  # 9.28 s
CLIPS = (1, 16)
WHAT = ("measure", "none", "scale", "lookahead")
TARGET, CEILING = -16.0, 0.5  # a ceiling of -6 dBTP: the limiter has work to do
REPEATS, WARM = 25, 3


def long_clip(seed):
    """9.28 s of the test family's speech-like audio (pieces of 12,000 samples with their own pitch contours)."""
    import numpy as np
    from tests import loudness_reference as R
    return np.concatenate([R.voiced(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES].astype(np.float32)


def batch_call(st, n, what, base):
    """One call over n clips -> (closure, status tensor); its buffers are its own."""
    import numpy as np
    import torch
    from tests import loudness_reference as R
    from tortoise_tts_amd import engine as E
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, ho = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, R.hops(SAMPLES)))
    f32 = lambda k: torch.zeros(k).cuda()
    target, ceiling = torch.full((n,), TARGET).cuda(), torch.full((n,), CEILING).cuda()
    y, lufs, hop = f32(n * SAMPLES), torch.zeros(n, dtype=torch.float64).cuda(), torch.zeros(n * R.hops(SAMPLES), dtype=torch.float64).cuda()
    tp, gain, otp = f32(n), f32(n), f32(n)
    ba, br, status = (torch.full((n,), -1, dtype=torch.int32).cuda() for _ in range(3))
    P = E.ptr

    def call():
        if what == "measure":
            E.check(st.lib.tt_loud_measure(st.h, n, P(audio), P(io), P(ho), P(lufs), P(tp), P(ba), P(br), P(hop), P(status), E.stream_ptr()))
        else:
            E.check(st.lib.tt_loud_normalize(st.h, n, P(audio), P(io), P(ho), P(target), P(ceiling), WHAT.index(what) - 1, P(y), P(lufs), P(tp), P(ba),
                                             P(br), P(hop), P(gain), P(otp), P(status), E.stream_ptr()))
    return call, status


def child(timed):
    import numpy as np
    import torch
    from tortoise_tts_amd import stages
    res = {}
    st = stages.LoudnessStage(16 * SAMPLES, max_clips=16)
    repeats, warm = (REPEATS, WARM) if timed else (3, 0)
    bases = [long_clip(s) for s in range(4)]
    for what in WHAT:
        for n in CLIPS:
            calls = [batch_call(st, n, what, np.roll(bases[r % 4], 4099 * r)) for r in range(repeats + warm)]
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
            res["call_ms_%s_x%d" % (what, n)] = "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(ms), min(ms), max(ms), len(ms))
            del calls
    st.close()
    if timed:
        from tortoise_tts_amd import api

        class Host(api._Common):
            device = torch.device("cuda")

        h = Host()
        for what in WHAT[1:]:
            for n in CLIPS:
                ms = []
                for r in range(WARM + 10):
                    clips = [torch.from_numpy(np.roll(bases[(r + i) % 4], 811 * r + 13 * i).copy()) for i in range(n)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h.normalize_many(clips, TARGET, -6.0, what)
                    torch.cuda.synchronize()
                    if r >= WARM:
                        ms.append(1e3 * (time.perf_counter() - t0))
                res["normalize_many_host_ms_%s_x%d" % (what, n)] = "median %.3f  min %.3f  max %.3f  (10 repeats, CPU tensors in and out)" % (
                    statistics.median(ms), min(ms), max(ms))
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("time", "trace"))
    a = ap.parse_args()
    if a.child:
        return child(a.child == "time")
    out = a.out or os.path.join(ROOT, "profiles", ST.next_round_prefix() + "_loudness.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# loudness stage (tt_loud_measure / tt_loud_normalize) on clips of %d samples (%.2f s at 24 kHz), target %.0f LUFS, ceiling %.1f" % (
        SAMPLES, SAMPLES / 24000, TARGET, CEILING))
    log("## one process, device events around the call, a fresh input buffer per repeat: <call>_x<clips per call>")
    ST.run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every batch above, three calls each")
    with tempfile.TemporaryDirectory() as d:
        ST.run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "loud_" in row:
                    log(row)


if __name__ == "__main__":
    main()
