"""Redaction aligner (csrc/align.hip) at the reference checkpoint's architecture (24 x 1024, random weights): ms per tt_w2v_run on clips
of 9.3 s and 23 s at 24 kHz, device events after warm-up.  --once: one 9.3 s alignment only (for a kernel trace)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import w2v_reference as R  # noqa: E402
from tortoise_tts_amd import engine as E, stages  # noqa: E402

cfg = R.large_config()
m = R.hf_model(cfg, seed=11)
src = (cfg, {k: v.detach() for k, v in m.state_dict().items()}, R.VOCAB, R.TOK_CFG)
del m
once = "--once" in sys.argv
for name, dt in ((("fp16", E.TT_F16),) if once else (("fp16", E.TT_F16), ("bf16", E.TT_BF16))):
    st = stages.AlignerStage(src, "cuda", dt, max_samples=24000 * 24)
    for sec in ((9.3,) if once else (9.3, 23.0)):
        clip = R.test_clip(sec).cuda()
        if once:
            st.run(clip)
            torch.cuda.synchronize()
            break
        for _ in range(3):
            st.run(clip)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 10
        a.record()
        for _ in range(n):
            st.run(clip)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / n
        T = st.frames(clip.shape[-1])
        D, F = 1024, 4096
        enc = 24 * (2 * T * D * (3 * D + D + 2 * F) + 4 * T * T * D)  # the 24 layers: projections + attention
        pos = 2 * T * D * 128 * (D // 16)                                # grouped positional conv
        n, conv = (2 * clip.shape[-1] + 2) // 3, 0
        for i, (k, s_) in enumerate(zip(cfg["conv_kernel"], cfg["conv_stride"])):
            n = (n - k) // s_ + 1
            conv += 2 * n * 512 * k * (1 if i == 0 else 512)
        print(f"align_time {name}: {sec:.1f} s clip ({clip.shape[-1]} samples, {T} frames): {ms:.3f} ms per alignment "
              f"(encoder {enc / 1e12:.3f} TFLOP, positional conv {pos / 1e12:.4f}, conv stack {conv / 1e12:.4f})", flush=True)
    st.close()
