"""What a push of the streaming time-stretch (csrc/tsm_stream.hip) costs at piece size, against tt_tsm_stretch of the same samples (the
whole-clip kernel, csrc/tsm.hip).  A record, not a gate.

    python scripts/tsstream_time.py [--out profiles/rNN_tsstream.txt] [--first-chunk]      (default: the next free round prefix)

  push     ONE process: tt_tss_push of a 40-token piece (40 960 samples at 24 kHz) and of the 60-token first piece (61 440) for 1 and 16
           sessions in one call, at rates 0.5 / 0.8 / 1.25 / 2.0, in isolation: device events around the call alone, inputs resident on the
           device, a FRESH input buffer for every repeat, median and spread of 25 repeats after 3 warm-up calls; the streams continue from
           push to push.  Beside each, the host clock from before the call until the stream has drained, the frames a push ran (the
           median over the repeats) and the call per frame.
  whole    the same samples through tt_tsm_stretch in the same run: device events around the call, its frames K - 1 and the call per frame,
           and the host clock including the copy back of the status that the stage needs before it can hand the clips out.
  first    (--first-chunk) the first-chunk latency of tts_stream plain, with stream_speaking_rate=1.25, and with stream_speaking_rate,
           stream_pitch and stream_sample_rate together, on the setup of bench.py --workload stream.
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
RATES = (0.5, 0.8, 1.25, 2.0)
SESSIONS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 500


def spread(ms):
    return "median %.4f  min %.4f  max %.4f" % (statistics.median(ms), min(ms), max(ms))


def child():
    import ctypes as C
    import numpy as np
    import torch
    from tests import tsm_reference as T
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    from tortoise_tts_amd import stretch as tsm
    res = {}
    bases = [T.clip(61440, s) for s in range(4)]
    whole = stages.TimeStretchStage(61440, max_clips=16)
    st = stages.StreamStretchStage(16)
    for piece, n_in in PIECES:
        for rate in RATES:
            rq = T.rate_q(rate)
            for n in SESSIONS:
                key = "%s_r%s_x%d" % (piece, rate, n)
                audios = [torch.from_numpy(np.concatenate([np.roll(bases[(r + i) % 4][:n_in], 997 * i + 4099 * r) for i in range(n)])).cuda()
                          for r in range(REPEATS + WARM)]
                for s in list(st.slots):
                    st.close(s)
                slots = [st.open(rq) for _ in range(n)]
                arr = C.c_int * n
                y = torch.zeros(n * (2 * n_in + 8 * 384)).cuda()
                torch.cuda.synchronize()
                dev, host, frames = [], [], []
                for r, audio in enumerate(audios):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    E.check(st.lib.tt_tss_push(st.h, n, arr(*slots), arr(*[n_in] * n), arr(*[0] * n), E.ptr(audio), E.ptr(y), None, E.stream_ptr()))
                    b.record()
                    b.synchronize()
                    t1 = time.perf_counter()
                    if r >= WARM:
                        dev.append(a.elapsed_time(b))
                        host.append(1e3 * (t1 - t0))
                        frames.append(tsm.stream_frames_done((r + 1) * n_in, rq) - tsm.stream_frames_done(r * n_in, rq))
                f = statistics.median(frames)
                res["push_ms_" + key] = "%s  (%d frames per stream: %.3f us per frame; min %.3f max %.3f; host clock until drained: median %.4f)" % (
                    spread(dev), f, 1e3 * statistics.median(dev) / f, 1e3 * min(dev) / f, 1e3 * max(dev) / f, statistics.median(host))
                n_out, K = T.out_samples(n_in, rq), T.frames(n_in, rq)
                io, oo, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (n_in, n_out, K))
                rqs = torch.full((n,), rq, dtype=torch.int32).cuda()
                y2, off, status = torch.zeros(n * n_out).cuda(), torch.zeros(n * K, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()
                torch.cuda.synchronize()
                dev, host = [], []
                for r, audio in enumerate(audios):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    E.check(whole.lib.tt_tsm_stretch(whole.h, n, E.ptr(audio), E.ptr(io), E.ptr(rqs), E.ptr(y2), E.ptr(oo), E.ptr(off), E.ptr(fo),
                                                     E.ptr(status), E.stream_ptr()))
                    b.record()
                    ok = status.cpu().tolist() == [0] * n  # the copy back a piece-by-piece caller waits for
                    t1 = time.perf_counter()
                    b.synchronize()
                    assert ok
                    if r >= WARM:
                        dev.append(a.elapsed_time(b))
                        host.append(1e3 * (t1 - t0))
                res["whole_ms_" + key] = "%s  (%d frames per clip: %.3f us per frame; min %.3f max %.3f; host clock with the status copied back: median %.4f)" % (
                    spread(dev), K - 1, 1e3 * statistics.median(dev) / (K - 1), 1e3 * min(dev) / (K - 1), 1e3 * max(dev) / (K - 1), statistics.median(host))
    print("RESULT " + json.dumps(res))


def first_chunk():
    """The time from the call until the first piece of tts_stream is on the host, plain and with the streaming keywords: bench.py --workload
    stream's setup (synthetic weights with the stop token suppressed, bf16, 200 mel tokens, the committed prompt, pieces of 40 after a first
    of 60)."""
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
    cases = (("plain", {}), ("rate", {"stream_speaking_rate": 1.25}),
             ("all", {"stream_speaking_rate": 1.25, "stream_pitch": 3, "stream_sample_rate": 16000}))
    res, ms = {}, {name: [] for name, _ in cases}
    for r in range(WARM + 10):
        for name, extra in cases:  # (interleaved: all see the same machine)
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
    for name in ("rate", "all"):
        res["first_chunk_ms_difference_" + name] = "%.3f (medians, against plain)" % (statistics.median(ms[name]) - statistics.median(ms["plain"]))
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
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_tsstream.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# streaming time-stretch (tt_tss_push) at piece size against tt_tsm_stretch of the same samples; one workgroup per stream / clip")
    log("## one process, device events around the call, a fresh input buffer per repeat: <piece>_r<rate>_x<sessions per call>")
    for what in ["push"] + (["first"] if a.first_chunk else []):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", what]
        log("$ python scripts/tsstream_time.py --child " + what)
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
