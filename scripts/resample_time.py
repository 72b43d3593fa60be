"""What the arbitrary-ratio resampler (csrc/resample.hip) costs on a rendered clip.  A record, not a gate.

    python scripts/resample_time.py [--out profiles/rNN_resample.txt]      (default: the next free round prefix)

  time     ONE process: tt_rs_resample on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the noise-and-tones clips of
           tests/resample_reference.py) from 24 kHz to 8 / 16 / 44.1 / 48 kHz and at +3 semitones (77936 / 65536), in isolation: device events
           around the call alone, inputs resident on the device, a FRESH input buffer for every repeat (no repeat finds its audio in a cache
           because the one before read it), median and spread of 25 repeats after 3 warm-up calls on buffers of their own.  With every case
           its taps (outputs x (2 H + 2)): DESIGN.md 5.27 computes the FMA and LDS-traffic floors from them.  Then the same batches through
           TextToSpeech.resample_many / shift_pitch_many from host tensors (upload, call, peaks back; host clock around a call that ends
           synchronised).
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
CASES = (("8k", (3, 1)), ("16k", (3, 2)), ("44k1", (80, 147)), ("48k", (1, 2)), ("+3st", (77936, 65536)))
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400


def batch_call(st, n, P, Q, base):
    """One tt_rs_resample call over n clips -> (closure, status tensor); its buffers are its own."""
    import numpy as np
    import torch
    from tests import resample_reference as R
    from tortoise_tts_amd import engine as E
    n_out = R.out_samples(SAMPLES, P, Q)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, oo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, n_out))
    ps, qs = torch.full((n,), P, dtype=torch.int32).cuda(), torch.full((n,), Q, dtype=torch.int32).cuda()
    y, peak, status = torch.zeros(n * n_out).cuda(), torch.zeros(n).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_rs_resample(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(ps), E.ptr(qs), E.ptr(y), E.ptr(oo), E.ptr(peak), E.ptr(status),
                                      E.stream_ptr()))
    return call, status


def child(timed):
    import numpy as np
    import torch
    from tests import resample_reference as R
    from tortoise_tts_amd import stages
    res = {}
    st = stages.ResampleStage(SAMPLES, max_clips=16)
    repeats, warm = (REPEATS, WARM) if timed else (3, 0)
    bases = [R.clip(SAMPLES, s) for s in range(4)]
    for name, (P, Q) in CASES:
        n_out, taps = R.out_samples(SAMPLES, P, Q), 2 * R.half_width(R.cutoff_q(P, Q)) + 2
        for n in CLIPS:
            calls = [batch_call(st, n, P, Q, np.roll(bases[r % 4], 4099 * r)) for r in range(repeats + warm)]
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
            key = "%s_x%d" % (name, n)
            res["call_ms_" + key] = "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(ms), min(ms), max(ms), len(ms))
            res["taps_" + key] = "%d outputs x %d taps x %d clips = %.1f M; %.2f ns per 1000 taps" % (
                n_out, taps, n, 1e-6 * n_out * taps * n, 1e9 * statistics.median(ms) / (n_out * taps * n))
            del calls
    st.close()
    if timed:
        from tortoise_tts_amd import api

        class Host(api._Common):
            device = torch.device("cuda")

        h = Host()
        rates = {"8k": 8000, "16k": 16000, "44k1": 44100, "48k": 48000}
        for name, _ in CASES:
            for n in CLIPS:
                ms = []
                for r in range(WARM + 10):
                    clips = [torch.from_numpy(np.roll(bases[(r + i) % 4], 811 * r + 13 * i).copy()) for i in range(n)]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name in rates:
                        h.resample_many(clips, rates[name])
                    else:
                        h.shift_pitch_many(clips, 3)  # (the time-stretch at rate 65536^2 / 77936, then the resampling)
                    torch.cuda.synchronize()
                    if r >= WARM:
                        ms.append(1e3 * (time.perf_counter() - t0))
                what = "resample_many" if name in rates else "shift_pitch_many"
                res["%s_host_ms_%s_x%d" % (what, name, n)] = "median %.3f  min %.3f  max %.3f  (10 repeats, CPU tensors in and out)" % (
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
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_resample.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# arbitrary-ratio resampler (tt_rs_resample) of clips of %d samples (%.2f s at 24 kHz); tiles of 1024 outputs, one workgroup per CU" % (
        SAMPLES, SAMPLES / 24000))
    log("## one process, device events around the call, a fresh input buffer per repeat: <target>_x<clips per call>")
    run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every batch above, three calls each")
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "rs_" in row:
                    log(row)


if __name__ == "__main__":
    main()
