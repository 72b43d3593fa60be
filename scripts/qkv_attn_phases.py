#!/usr/bin/env python
"""Phase stamps of the LAST decode_qkv_attn_kernel launch of a real generation (layer 30 of the last step, graph replay, cold KV cache), from a
-DTT_ATTN_STAMPS variant build: waves 0 (a projector) and 15 of every workgroup file entry / staged rows landed / projection done / q, k, v in
the LDS / exit.
    python -m tortoise_tts_amd.build --variant astamps -DTT_ATTN_STAMPS
    TORTOISE_MI355X_LIB=tortoise_tts_amd/lib/libtortoise_mi355x_astamps.so python scripts/qkv_attn_phases.py"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench import bench_prompt  # noqa: E402
from tortoise_tts_amd import engine as E, stages, weights as W  # noqa: E402
from tortoise_tts_amd.config import ARConfig  # noqa: E402

lib = E.init()
lib.ttx_attn_stamps.restype = C.c_int
lib.ttx_attn_stamps.argtypes = [C.c_void_p, C.c_int]
cfg = ARConfig()
sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg)
B = 256
ar = stages.ArStage(sd, cfg, dtype=E.TT_F16, max_batch=B, max_new_tokens=200, max_latent_candidates=1)
assert ar.ccfg.max_batch == B
text, (auto, _) = bench_prompt()
tt = F.pad(text.int()[None], (0, 1)).cuda()
nwg = 16 * (B // 16)
for NT in (100, 190):
    ar.prefill(auto.cuda(), tt)
    ar.generate(B, NT, seed=1)
    torch.cuda.synchronize()
    assert ar.stat(2) == 6 * cfg.layers + 4, "this batch does not take the fused launch"
    buf = (C.c_ulonglong * (768 * 10))()
    assert lib.ttx_attn_stamps(buf, 768) == 0
    full = np.array(buf, dtype=np.float64).reshape(768, 10)
    st = full[:nwg]
    arrive = np.concatenate([full[256:256 + nwg, :10], full[512:512 + nwg, :6]], axis=1)  # [workgroup][wave]: arrival at the second barrier
    t0 = min(st[:, 0].min(), st[:, 5].min())
    p = (st[:, :5] - t0) * 0.01   # wave 0: a projector
    s = (st[:, 5:] - t0) * 0.01   # wave 15
    mb = (B * NT + 59) * 16 * 64 * 2 * 2 / 1e6
    print("in situ: last fused launch of a %d-token generation (K / V stream %.1f MB -> %.1f us at 6.4 TB/s)" % (NT, mb, mb / 6.4))
    print("  workgroup entry p50 %.2f max %.2f | exit p50 %.2f p90 %.2f max %.2f us" % (np.median(p[:, 0]), p[:, 0].max(), np.median(s[:, 4]), np.percentile(s[:, 4], 90),
                                                                                     max(s[:, 4].max(), p[:, 4].max())))
    print("  arrival at barrier 2 after the workgroup's entry, mean per wave (0 .. 11 projectors: q q q q k k k k v v v v; 12 .. 15 stream): %s" %
          " ".join("%.1f" % v for v in ((arrive - st[:, :1]) * 0.01).mean(axis=0)))
    for name, a, b in (("entry -> staged rows landed (barrier 1)", p[:, 0], p[:, 1]), ("projection (wave 0: barrier 1 -> its tiles stored)", p[:, 1], p[:, 2]),
                       ("wave 0: tiles stored -> every wave's tiles in the LDS (barrier 2)", p[:, 2], p[:, 3]), ("attention, wave 0 (barrier 2 -> exit)", p[:, 3], p[:, 4]),
                       ("attention, wave 15 (barrier 2 -> exit)", s[:, 3], s[:, 4]), ("whole workgroup (entry -> last exit)", np.minimum(p[:, 0], s[:, 0]), np.maximum(p[:, 4], s[:, 4]))):
        d = b - a
        print("  %-70s mean %6.2f  p90 %6.2f  max %6.2f us" % (name, d.mean(), np.percentile(d, 90), d.max()))
