"""Tortoise detector (csrc/classify.hip) at the reference architecture (synthetic weights): ms per tt_cls_run on a 220 000-sample clip (what
is_this_from_tortoise.py keeps) and a 60 s clip at 24 kHz, fp16 and bf16, device events after warm-up.  --once: one 220 000-sample
classification only (for a kernel trace)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import w2v_reference as R  # noqa: E402
from tortoise_tts_amd import engine as E, stages, weights as W  # noqa: E402

sd = W.synthetic_state_dict(W.classifier_manifest(), seed=1234)
once = "--once" in sys.argv
for name, dt in ((("fp16", E.TT_F16),) if once else (("fp16", E.TT_F16), ("bf16", E.TT_BF16))):
    st = stages.ClassifierStage(sd, "cuda", dt, max_samples=24000 * 60)
    for n in ((220000,) if once else (220000, 24000 * 60)):
        clip = R.test_clip(n / 24000.0 + 1e-3)[:, :n].contiguous().cuda()
        if once:
            st.run(clip)
            torch.cuda.synchronize()
            break
        for _ in range(3):
            st.run(clip)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        a.record()
        for _ in range(reps):
            st.run(clip)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / reps
        L, C, flops = n, 32, 2 * n * 32 * 3
        for _ in range(5):
            flops += 2 * 2 * (2 * L * C * 5 * C)              # two ResBlocks of two k5 convs
            L = (L + 3) // 4
            flops += 2 * L * 2 * C * 5 * C                    # Downsample
            C *= 2
        flops += 2 * L * 1024 * 512 + 4 * (2 * L * 512 * 2048 + 4 * L * L * 512)
        print(f"classify_time {name}: {n} samples ({n / 24000:.1f} s, {L} frames): {ms:.3f} ms per clip ({flops / 1e9:.1f} GFLOP, "
              f"guard {st.guard()})", flush=True)
    st.close()
