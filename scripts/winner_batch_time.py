"""tts(k > 1) with TextToSpeech(winner_batch=W) against the serial winner loop of ANOTHER source tree (the parent commit, checked out and
built next to this one), 'standard' preset at the benchmark's prompt with bench.py's full-size synthetic weights.  One worker process per
tree holds its engines; the driver alternates them round by round in the same run, so both see the same device and the same moment.
Also: VocoderStage.inference_many against per-clip inference() (this tree), and --voc-once for a kernel trace of one call.

    python scripts/winner_batch_time.py --parent /path/to/parent/tree [--rounds 3] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python scripts/winner_batch_time.py --voc-once batched|single
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((3, 3), (2, 2), (5, 5))  # (k, winner_batch)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def voc_stage(max_frames):
    from oracle import make_golden as G
    from tortoise_tts_amd import engine as E, stages, weights as W
    from tortoise_tts_amd.config import VocoderConfig
    cfg = VocoderConfig()
    sd = W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(cfg), seed=G.VOC_SEED))
    return stages.VocoderStage(sd, cfg, dtype=E.TT_F16, max_frames=max_frames), cfg


def voc_items(cfg, n, S=870):
    import torch
    g = torch.Generator().manual_seed(5)
    return [((torch.randn(1, 100, S, generator=g) * 2 - 5).cuda(), torch.randn(1, cfg.noise_dim, S + 10, generator=g).cuda()) for _ in range(n)]


def voc_once(form):
    """One warm call, then ONE call of the given form between two synchronisations (the kernels a trace should show last)."""
    import torch
    with torch.no_grad():
        st, cfg = voc_stage(3 * 880 - 10)
        items = voc_items(cfg, 3)
        run = (lambda: st.inference_many(items)) if form == "batched" else (lambda: [st.inference(m, z) for m, z in items])
        run()
        print(json.dumps({"voc_once": form, "seconds": round(timed(run), 6)}))
        st.close()


def voc_bench(rounds):
    import torch
    out = []
    with torch.no_grad():
        st, cfg = voc_stage(16 * 880 - 10)
        for n in (3, 16):
            items = voc_items(cfg, n)
            for (m, z), w in zip(items, st.inference_many(items)):  # warm-up + bit check
                assert torch.equal(w, st.inference(m, z))
            single, batched = [], []
            for r in range(rounds):
                for form in (("single", "batched") if r % 2 == 0 else ("batched", "single")):
                    if form == "single":
                        single.append(timed(lambda: [st.inference(m, z) for m, z in items]))
                    else:
                        batched.append(timed(lambda: st.inference_many(items)))
            out.append({"univnet": f"{n}x870 frames fp16", "single_s": [round(x, 5) for x in single], "batched_s": [round(x, 5) for x in batched]})
        st.close()
    return out


def worker(batched):
    """Serves 'k W' lines on stdin: one tts_with_preset('standard', k) per line on an instance with winner_batch=W (this tree) or on the
    plain instance (a tree without the keyword) -> one JSON line with the wall time and the stage seconds."""
    import torch
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    sds = bench.synthetic_weights()
    text, latents = bench.bench_prompt()
    inst = {}
    print(json.dumps({"ready": True}), flush=True)
    with torch.no_grad():
        for line in sys.stdin:
            k, W, seed = (int(v) for v in line.split())
            key = W if batched else 1
            if key not in inst:
                extra = {"winner_batch": W} if batched else {}
                inst[key] = TextToSpeech(state_dicts=sds, max_candidates=256, max_mel_tokens=200, **extra)
            tts = inst[key]
            s = timed(lambda: tts.tts_with_preset(text, preset="standard", conditioning_latents=latents, max_mel_tokens=200,
                                                  use_deterministic_seed=seed, k=k, verbose=False))
            print(json.dumps({"k": k, "winner_batch": key, "total_s": round(s, 4), "stages": {n: round(v, 4) for n, v in tts.timings.items()}}), flush=True)


def start(tree, batched):
    env = dict(os.environ, PYTHONPATH=tree)
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "batched" if batched else "serial"], cwd=tree, env=env,
                         stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    assert json.loads(p.stdout.readline())["ready"]
    return p


def ask(p, k, W, seed):
    p.stdin.write(f"{k} {W} {seed}\n")
    p.stdin.flush()
    line = p.stdout.readline()
    if not line:
        raise RuntimeError("a worker ended early (exit status %s)" % p.wait())
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its serial tts(k) is the baseline)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=["batched", "serial"])
    ap.add_argument("--voc-once", default=None, choices=["batched", "single"])
    args = ap.parse_args()
    sys.path.insert(0, os.environ.get("PYTHONPATH") or HERE)
    if args.worker:
        return worker(args.worker == "batched")
    if args.voc_once:
        return voc_once(args.voc_once)
    lines = []
    if args.parent:
        base, new = start(os.path.abspath(args.parent), False), start(HERE, True)
        try:
            for k, W in CASES:
                for p in (base, new):  # warm-up (graph captures, first-use allocations): not reported
                    ask(p, k, W, 999)
                for r in range(args.rounds):
                    pair = ((base, "parent_serial"), (new, "winner_batch")) if r % 2 == 0 else ((new, "winner_batch"), (base, "parent_serial"))
                    for p, label in pair:
                        lines.append(dict(ask(p, k, W, 1000 + r), run=label, round=r))
        finally:
            for p in (base, new):
                p.stdin.close()
                p.wait()
    lines += voc_bench(args.rounds)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
