"""Batched HiFi-GAN decoding against one call per sequence (full-size synthetic weights, bf16): n inference() calls vs one
inference_many() at 16 x 60, 16 x 280, 16 x 500 latents and ragged mixes, three alternating rounds in one process.  The handle is made
with max_latents = 16 * 508 (a per-call budget of padded slots) so that sixteen 500-latent sequences fit one call.

    python scripts/hifi_batch_time.py [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tortoise_tts_amd import engine as E  # noqa: E402
from tortoise_tts_amd import stages  # noqa: E402
from tortoise_tts_amd import weights as W  # noqa: E402
from tortoise_tts_amd.config import HifiganConfig  # noqa: E402

MIXES = {"16x60": [60] * 16, "16x280": [280] * 16, "16x500": [500] * 16, "1x500+15x60": [500] + [60] * 15,
         "ragged16": [60, 100, 140, 180, 220, 260, 300, 340, 380, 420, 460, 500, 60, 60, 120, 240]}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = HifiganConfig()
    sd = W.fold_weight_norm(W.synthetic_state_dict(W.hifigan_manifest(cfg), seed=31))
    st = stages.HifiganStage(sd, cfg, dtype=E.TT_BF16, max_latents=16 * 508)
    gen = torch.Generator().manual_seed(5)
    lines = []
    with torch.no_grad():
        data = {k: [(torch.randn(1, T, cfg.in_channels, generator=gen).cuda(), torch.randn(1, cfg.cond_channels, generator=gen).cuda() * 0.5)
                    for T in v] for k, v in MIXES.items()}
        for k, items in data.items():  # warm-up + bit check
            for (lat, g), w in zip(items, st.inference_many(items)):
                assert torch.equal(w, st.inference(lat, g)), k
        res = {k: {"single": [], "batched": []} for k in MIXES}
        for r in range(args.rounds):
            for k, items in data.items():
                order = ("single", "batched") if r % 2 == 0 else ("batched", "single")
                for form in order:
                    if form == "single":
                        res[k][form].append(timed(lambda: [st.inference(lat, g) for lat, g in items]))
                    else:
                        res[k][form].append(timed(lambda: st.inference_many(items)))
        for k in MIXES:
            s, b = res[k]["single"], res[k]["batched"]
            line = dict(mix=k, groups=len(st.batch_groups(MIXES[k])), single_s=[round(x, 5) for x in s], batched_s=[round(x, 5) for x in b],
                        speedup_median=round(sorted(s)[len(s) // 2] / sorted(b)[len(b) // 2], 3))
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    st.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
