"""What a push of the streaming resampler (csrc/resample_stream.hip) costs at piece size, against resampling the piece alone with
tt_rs_resample (what a caller who resamples a stream piece by piece pays today).  A record, not a gate.

    python scripts/rsstream_time.py [--out profiles/rNN_rsstream.txt] [--first-chunk]      (default: the next free round prefix)

  push     ONE process: tt_rss_push of a 40-token piece (40 960 samples at 24 kHz) and of the 60-token first piece (61 440) for 1 and 16
           sessions in one call, to 8 / 16 / 32 / 44.1 / 48 kHz, on a bank-form and on a table-form handle (44.1 kHz has 147 phases: its bank is
           measured too), in isolation: device events around the call alone, inputs resident on the device, a FRESH input buffer for every
           repeat, median and spread of 25 repeats after 3 warm-up calls; the streams continue from push to push.  Beside each, the host
           clock from before the call until the stream has drained.  With every case its taps (outputs x (2 H + 2)) and the call as a
           multiple of the bank form's floors: one FMA and two LDS dwords per tap, 7.9e13 lane-operations and 7.9e13 LDS bytes per second
           on 256 CUs: 0.0127 us and 0.101 us per million taps.
  whole    the same samples through tt_rs_resample in the same run: device events around the call, and the host clock including the copy
           back of the status that the stage needs before it can hand the clips out.
  first    (--first-chunk) the first-chunk latency of tts_stream with and without stream_sample_rate=8000, on the setup of bench.py
           --workload stream.
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
PIECES = (("40tok", 40960), ("60tok", 61440))
CASES = (("8k", (3, 1)), ("16k", (3, 2)), ("32k", (3, 4)), ("44k1", (80, 147)), ("48k", (1, 2)))
SESSIONS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 500
FMA_US_PER_MTAP, LDS_US_PER_MTAP = 1e12 / 7.9e13, 8e12 / 7.9e13  # us per million taps: one lane-operation, eight LDS bytes


def spread(ms):
    return "median %.4f  min %.4f  max %.4f" % (statistics.median(ms), min(ms), max(ms))


def child():
    import ctypes as C
    import numpy as np
    import torch
    from tests import resample_reference as R
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    res = {}
    bases = [R.clip(61440, s) for s in range(4)]
    whole = stages.ResampleStage(61440, max_clips=16)
    streams = {form: stages.StreamResampleStage(16, form=form) for form in ("bank", "table")}
    for piece, n_in in PIECES:
        for name, (P, Q) in CASES:
            taps = 2 * R.half_width(R.cutoff_q(P, Q)) + 2
            for n in SESSIONS:
                key = "%s_%s_x%d" % (piece, name, n)
                audios = [torch.from_numpy(np.concatenate([np.roll(bases[(r + i) % 4][:n_in], 997 * i + 4099 * r) for i in range(n)])).cuda()
                          for r in range(REPEATS + WARM)]
                n_out = R.out_samples(n_in, P, Q)
                mtaps = 1e-6 * n_out * taps * n
                res["taps_" + key] = "%d outputs x %d taps x %d sessions = %.2f M; bank-form floors: FMA %.4f ms, LDS %.4f ms" % (
                    n_out, taps, n, mtaps, 1e-3 * mtaps * FMA_US_PER_MTAP, 1e-3 * mtaps * LDS_US_PER_MTAP)
                for form, st in streams.items():
                    for s in list(st.slots):
                        st.close(s)
                    slots = [st.open(P, Q) for _ in range(n)]
                    arr = C.c_int * n
                    y = torch.zeros(n * (n_out + 8)).cuda()
                    torch.cuda.synchronize()
                    dev, host = [], []
                    for r, audio in enumerate(audios):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        a.record()
                        E.check(st.lib.tt_rss_push(st.h, n, arr(*slots), arr(*[n_in] * n), arr(*[0] * n), E.ptr(audio), E.ptr(y), E.stream_ptr()))
                        b.record()
                        b.synchronize()
                        t1 = time.perf_counter()
                        if r >= WARM:
                            dev.append(a.elapsed_time(b))
                            host.append(1e3 * (t1 - t0))
                    med = statistics.median(dev)
                    res["push_%s_ms_%s" % (form, key)] = "%s  (x %.1f of the LDS floor; host clock until drained: median %.4f)" % (
                        spread(dev), med / (1e-3 * mtaps * LDS_US_PER_MTAP), statistics.median(host))
                io, oo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (n_in, n_out))
                ps, qs = torch.full((n,), P, dtype=torch.int32).cuda(), torch.full((n,), Q, dtype=torch.int32).cuda()
                y, peak, status = torch.zeros(n * n_out).cuda(), torch.zeros(n).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()
                torch.cuda.synchronize()
                dev, host = [], []
                for r, audio in enumerate(audios):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    E.check(whole.lib.tt_rs_resample(whole.h, n, E.ptr(audio), E.ptr(io), E.ptr(ps), E.ptr(qs), E.ptr(y), E.ptr(oo), E.ptr(peak),
                                                     E.ptr(status), E.stream_ptr()))
                    b.record()
                    ok = status.cpu().tolist() == [0] * n  # the copy back a piece-by-piece caller waits for
                    t1 = time.perf_counter()
                    b.synchronize()
                    assert ok
                    if r >= WARM:
                        dev.append(a.elapsed_time(b))
                        host.append(1e3 * (t1 - t0))
                res["whole_ms_" + key] = "%s  (host clock with the status copied back: median %.4f)" % (spread(dev), statistics.median(host))
    print("RESULT " + json.dumps(res))


def first_chunk():
    """The time from the call until the first piece of tts_stream is on the host, plain and at 8 kHz: bench.py --workload stream's setup
    (synthetic weights with the stop token suppressed, bf16, 200 mel tokens, the committed prompt, pieces of 40 after a first of 60)."""
    import torch
    import bench
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    a_cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(a_cfg), 1234), a_cfg),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    tts = TextToSpeech(state_dicts=sds, dtype="bf16", max_mel_tokens=200, kv_cache=True)
    text, (auto, _) = bench.bench_prompt()
    res, ms = {}, {"plain": [], "8k": []}
    for r in range(WARM + 10):
        for name, extra in (("plain", {}), ("8k", {"stream_sample_rate": 8000})):  # (interleaved: both see the same machine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = tts.tts_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=1000 + r, stream_chunk_size=40,
                               overlap_wav_len=1024, verbose=False, **extra)
            piece = next(g).cpu()
            t1 = time.perf_counter()
            g.close()
            if r >= WARM:
                ms[name].append(1e3 * (t1 - t0))
            res["first_chunk_samples_" + name] = str(piece.shape[0])
    for name in ms:
        res["first_chunk_ms_" + name] = spread(ms[name]) + "  (10 repeats)"
    res["first_chunk_ms_difference"] = "%.3f (medians)" % (statistics.median(ms["8k"]) - statistics.median(ms["plain"]))
    print("RESULT " + json.dumps(res))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--first-chunk", action="store_true")
    ap.add_argument("--child", choices=("push", "first"))
    a = ap.parse_args()
    if a.child:
        return child() if a.child == "push" else first_chunk()
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_rsstream.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# streaming resampler (tt_rss_push) at piece size against tt_rs_resample of the same samples; bank tiles of 256 outputs, table tiles of 1024")
    log("## one process, device events around the call, a fresh input buffer per repeat: <piece>_<target>_x<sessions per call>")
    for what in ["push"] + (["first"] if a.first_chunk else []):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", what]
        log("$ python scripts/rsstream_time.py --child " + what)
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            log(r.stdout[-2000:] + r.stderr[-4000:])
            log("exit status %d: the run ends here" % r.returncode)
            sys.exit(1)
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                for k, v in json.loads(line[7:]).items():
                    log("%-36s %s" % (k, v))


if __name__ == "__main__":
    main()
