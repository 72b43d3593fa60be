"""What the wav -> mel front-end of the voice_samples path costs, mel_front_end="torch" (audio.MelFrontEnd: rocFFT, MIOpen, rocBLAS) against
"device" (stages.MelFrontStage: csrc/melfront.hip).  A record, not a gate.

    python scripts/melfront_time.py [--out profiles/rNN_melfront.txt]      (default: the next free round prefix)

The driver starts one fresh child process per measurement, each under its own time limit; the first failure ends the run.
  cond     api.TextToSpeech.get_conditioning_latents for 1, 2 and 4 six-second clips: the first call of a fresh process (1 clip), then the
           warm median of 20 calls per clip count.  Full-width conditioning encoders; the stages that play no part are built two layers deep.
  stream   api_fast.tts_stream(voice_samples=[clip]): time to the first chunk, first call and warm median of 5, full-size synthetic
           weights as scripts/stream_sessions.py uses.
  trace    one device-path get_conditioning_latents call under `rocprofv3 --kernel-trace --stats`: launches and per-kernel times.
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
CLIP_SAMPLES = 132300  # six seconds at 22.05 kHz
LIMIT = {"cond": 300, "stream": 300, "trace": 300}


def clip(i):
    import math
    import torch
    g = torch.Generator().manual_seed(50 + i)
    t = torch.arange(CLIP_SAMPLES, dtype=torch.float64) / 22050.0
    x = 0.3 * torch.sin(2 * math.pi * (180.0 + 40.0 * i) * t) + 0.2 * torch.sin(2 * math.pi * 3000.0 * t) + 0.05 * torch.randn(CLIP_SAMPLES, generator=g, dtype=torch.float64)
    return x.float().reshape(1, -1)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    (out[0] if isinstance(out, (tuple, list)) else out).cpu()
    return (time.perf_counter() - t0) * 1e3


def mel_norms():
    import torch
    return -(2.0 + 6.0 * torch.rand(80, generator=torch.Generator().manual_seed(3)))


def front_end(kind):
    from tortoise_tts_amd import audio, stages
    return stages.MelFrontStage(mel_norms=mel_norms()) if kind == "device" else audio.MelFrontEnd(mel_norms=mel_norms())


def child_cond(kind, calls, counts):
    import torch
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, VocoderConfig
    ar, diff, clvp = ARConfig(layers=2), DiffusionConfig(num_layers=2), CLVPConfig()
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(ar), 1234), "diffusion": W.synthetic_state_dict(W.diffusion_manifest(diff), 1235),
           "clvp": W.synthetic_state_dict(W.clvp_manifest(clvp), 1236),
           "vocoder": W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(VocoderConfig()), 1237))}
    with torch.no_grad():
        tts = TextToSpeech(state_dicts=sds, configs={"ar": ar, "diffusion": diff, "clvp": clvp}, max_candidates=4, max_mel_tokens=32, mel_front_end=kind)
        clips = [clip(i).cuda() for i in range(max(counts))]
        # the conditioning encoders are warmed with ready mels, so that the first call below is the front-end's first call alone
        tts.get_conditioning_latents([(torch.zeros(1, 80, 517), torch.zeros(1, 100, 401))])
        tts.mel_front_end = front_end(kind)
        res = {"path": kind, "first_call_ms_1_clip": timed(lambda: tts.get_conditioning_latents(clips[:1]))}
        for n in counts:
            tts.get_conditioning_latents(clips[:n])
            res["warm_median_ms_%d_clips" % n] = statistics.median(timed(lambda: tts.get_conditioning_latents(clips[:n])) for _ in range(calls))
        res["encoders_only_ms_1_clip"] = statistics.median(timed(lambda: tts.get_conditioning_latents([(torch.zeros(1, 80, 517), torch.zeros(1, 100, 401))]))
                                                           for _ in range(calls))
    print("RESULT " + json.dumps(res))


def child_stream(kind, calls):
    import torch
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    text = list(range(10, 60))
    with torch.no_grad():
        tts = TextToSpeech(state_dicts=sds, dtype="bf16", max_mel_tokens=200, kv_cache=True, mel_front_end=kind)
        tts.mel_front_end = front_end(kind)
        x = clip(0).cuda()

        def first_chunk(**kw):
            gen = tts.tts_stream(text, max_mel_tokens=200, use_deterministic_seed=1, verbose=False, **kw)
            ms = timed(lambda: next(gen))
            for _ in gen:
                pass
            return ms
        auto = torch.randn(1, cfg.model_dim, generator=torch.Generator().manual_seed(9)) * 0.5
        first_chunk(conditioning_latents=(auto,))  # warms the decode and the vocoder: the first voice_samples call below is the front-end's
        res = {"path": kind, "first_chunk_ms_first_call": first_chunk(voice_samples=[x]),
               "first_chunk_ms_warm_median": statistics.median(first_chunk(voice_samples=[x]) for _ in range(calls)),
               "first_chunk_ms_latents_given": statistics.median(first_chunk(conditioning_latents=(auto,)) for _ in range(calls))}
    print("RESULT " + json.dumps(res))


def run_child(args, limit, log, env=None):
    cmd = ["timeout", "-k", "10", str(limit)] + args
    log("$ " + " ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            log(line[7:])
            return json.loads(line[7:])
    return None


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("cond", "stream"))
    ap.add_argument("--path", default="device")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--counts", default="1,2,4")
    ap.add_argument("--skip", default="", help="comma list of cond, stream, trace")
    a = ap.parse_args()
    if a.child == "cond":
        return child_cond(a.path, a.calls, [int(c) for c in a.counts.split(",")])
    if a.child == "stream":
        return child_stream(a.path, a.calls)
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_melfront.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    skip = a.skip.split(",")
    log("# mel front-end: mel_front_end='torch' (audio.MelFrontEnd) vs 'device' (stages.MelFrontStage); six-second clips, times in ms")
    if "cond" not in skip:
        log("## api.TextToSpeech.get_conditioning_latents")
        for kind in ("torch", "device"):
            run_child(me + ["--child", "cond", "--path", kind], LIMIT["cond"], log)
    if "stream" not in skip:
        log("## api_fast.tts_stream(voice_samples=[clip]): time to the first chunk")
        for kind in ("torch", "device"):
            run_child(me + ["--child", "stream", "--path", kind, "--calls", "5"], LIMIT["stream"], log)
    if "trace" not in skip:
        log("## rocprofv3 --kernel-trace --stats of one process: device path, 1 clip, first call + 3 calls + 1 ready-mel call")
        with tempfile.TemporaryDirectory() as d:
            run_child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + me + ["--child", "cond", "--path", "device", "--calls", "1", "--counts", "1"],
                      LIMIT["trace"], log)
            for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
                rows = open(path).read().splitlines()
                log(rows[0])
                for row in rows[1:]:
                    if "mel_" in row:
                        log(row)
                log("(%d kernels in all; mel_* rows shown)" % (len(rows) - 1))


if __name__ == "__main__":
    main()
