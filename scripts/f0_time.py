"""What the F0 tracker (csrc/f0.hip) and its Viterbi path (csrc/f0_viterbi.hip) cost on a rendered clip, and how far tt_f0_track is from
its floors.  A record, not a gate.

    python scripts/f0_time.py [--out profiles/rNN_f0.txt]      (default: the next free round prefix)

ONE process: tt_f0_track, tt_f0v_track (the Viterbi path: both launches) and each of its launches alone (tt_op_f0v_candidates,
tt_op_f0v_path) on 1 and 16 clips of 9.28 s (222,720 samples at 24 kHz, the time-stretch family's speech-like audio with its own
pitch contours) and, for scale, tt_sil_find and tt_tsm_stretch (rate 0.75) of the same samples.  The calls are INTERLEAVED: every
repeat runs each of them once, in turn, with device events around the call alone, inputs resident on the device and a FRESH input buffer
for every repeat; median and spread of 25 repeats after 3 warm-up rounds on buffers of their own.

The floors of tt_f0_track come from what the kernel does, counted from the shapes: every workgroup of G frames (tt_op_f0_group) sums G + 3 slots x 240 samples
x 480 lags terms (x[j] - x[j + tau])^2 (a clip needs F + 3 slots; frame by frame is 4 F), a term is one f32 subtraction and one f32 FMA = 2 lane
operations against the f32 vector peak (157.3 TFLOP/s with an FMA counted as two: 78.65e12 lane operations a second), and reads 2 bytes
of LDS (two ds_read_b128 per lane for 16 terms) against the LDS bandwidth (150 TB/s with every CU streaming).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLES = 222720  # 9.28 s
CLIPS = (1, 16)
REPEATS, WARM = 25, 3
LIMIT = 400
VALU_LANE_OPS = 157.3e12 / 2   # f32 vector peak, an FMA counted once
LDS_BYTES = 150e12             # aggregate LDS read bandwidth
SLOT, LAGS = 240, 480


def long_clip(seed):
    import numpy as np
    from tests import tsm_reference as T
    return np.concatenate([T.clip(12000, 100 * seed + i) for i in range(-(-SAMPLES // 12000))])[:SAMPLES]


def f0_call(st, n, base):
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import pitch
    F = pitch.frames(SAMPLES)
    p = pitch.params()
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, F))
    par = torch.tensor([[p.lag_lo, p.lag_hi]] * n, dtype=torch.int32).cuda()
    thr = torch.tensor([[p.thr, p.floor_e]] * n, dtype=torch.float64).cuda()
    lag, f0, aper = torch.zeros(n * F, dtype=torch.int32).cuda(), torch.zeros(n * F).cuda(), torch.zeros(n * F).cuda()
    nv, status = torch.zeros(n, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_f0_track(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(par), E.ptr(thr), E.ptr(fo), E.ptr(lag), E.ptr(f0), E.ptr(aper), E.ptr(nv),
                                   E.ptr(status), E.stream_ptr()))
    return call, status, nv


def f0v_call(which):
    """The Viterbi path's rows (csrc/f0_viterbi.hip) on the same samples and parameters: "track" the whole call tt_f0v_track, "candidates" the
    first launch alone (tt_op_f0v_candidates: f0_track_kernel's geometry and steps, beside tt_f0_track's launch), "path" the second launch
    alone (tt_op_f0v_path on the tables the first launch made of these samples: a chain of F frames, one wave a clip)."""
    def make(st, n, base):
        import numpy as np
        import torch
        from tortoise_tts_amd import engine as E
        from tortoise_tts_amd import pitch
        F = pitch.frames(SAMPLES)
        p, k = pitch.params(), pitch.smooth_params(True)
        audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
        io, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, F))
        par = torch.tensor([[p.lag_lo, p.lag_hi]] * n, dtype=torch.int32).cuda()
        thr = torch.tensor([[p.thr, p.floor_e]] * n, dtype=torch.float64).cuda()
        cost = torch.tensor([list(k)] * n, dtype=torch.float64).cuda()
        frames = torch.full((n,), F, dtype=torch.int32).cuda()
        lag, f0, aper, state = torch.zeros(n * F, dtype=torch.int32).cuda(), torch.zeros(n * F).cuda(), torch.zeros(n * F).cuda(), torch.zeros(n * F, dtype=torch.int32).cuda()
        c_lag, c_dp, c_f0 = torch.zeros(8 * n * F, dtype=torch.int32).cuda(), torch.zeros(8 * n * F, dtype=torch.float64).cuda(), torch.zeros(8 * n * F).cuda()
        nv, pc, status = torch.zeros(n, dtype=torch.int32).cuda(), torch.zeros(n, dtype=torch.float64).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()
        keep = (audio, io, fo, par, thr, cost, frames, lag, f0, aper, state, c_lag, c_dp, c_f0, nv, pc)  # (alive as long as the call is)

        def candidates():
            E.check(st.lib.tt_op_f0v_candidates(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(par), E.ptr(thr), E.ptr(fo), E.ptr(c_lag), E.ptr(c_dp), E.ptr(c_f0),
                                                E.ptr(status), E.stream_ptr()))

        def path(keep=keep):
            E.check(st.lib.tt_op_f0v_path(st.h, n, E.ptr(frames), E.ptr(par), E.ptr(cost), E.ptr(fo), E.ptr(c_lag), E.ptr(c_dp), E.ptr(c_f0), E.ptr(lag),
                                          E.ptr(f0), E.ptr(aper), E.ptr(state), E.ptr(nv), E.ptr(pc), E.ptr(status), E.stream_ptr()))

        def track(keep=keep):
            E.check(st.lib.tt_f0v_track(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(par), E.ptr(thr), E.ptr(cost), E.ptr(fo), E.ptr(lag), E.ptr(f0), E.ptr(aper),
                                        E.ptr(state), E.ptr(nv), E.ptr(pc), E.ptr(status), E.stream_ptr()))
        if which == "path":
            candidates()  # (the tables the path launch reads, made before the events)
        return {"track": track, "candidates": candidates, "path": path}[which], status, None
    return make


def sil_call(st, n, base):
    import numpy as np
    import torch
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import silence as sil
    cap = sil.max_regions(SAMPLES)
    p = sil.params()
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, ro = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, cap))
    thr = torch.tensor([[p.rel, p.floor_e]] * n, dtype=torch.float64).cuda()
    par = torch.tensor([[p.min_sil, p.pad]] * n, dtype=torch.int32).cuda()
    nreg, reg = torch.zeros(n, dtype=torch.int32).cuda(), torch.zeros(2 * n * cap, dtype=torch.int32).cuda()
    peak, status = torch.zeros(n, dtype=torch.float64).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_sil_find(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(thr), E.ptr(par), E.ptr(ro), None, E.ptr(nreg), E.ptr(reg), E.ptr(peak), None,
                                   E.ptr(status), E.stream_ptr()))
    return call, status, None


def tsm_call(st, n, base):
    import numpy as np
    import torch
    from tests import tsm_reference as T
    from tortoise_tts_amd import engine as E
    rq = T.rate_q(0.75)
    n_out, K = T.out_samples(SAMPLES, rq), T.frames(SAMPLES, rq)
    audio = torch.from_numpy(np.concatenate([np.roll(base, 997 * i) for i in range(n)])).cuda()
    io, oo, fo = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (SAMPLES, n_out, K))
    rqs = torch.full((n,), rq, dtype=torch.int32).cuda()
    y, off, status = torch.zeros(n * n_out).cuda(), torch.zeros(n * K, dtype=torch.int32).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_tsm_stretch(st.h, n, E.ptr(audio), E.ptr(io), E.ptr(rqs), E.ptr(y), E.ptr(oo), E.ptr(off), E.ptr(fo), E.ptr(status),
                                      E.stream_ptr()))
    return call, status, None


def child():
    import numpy as np
    import torch
    from tortoise_tts_amd import pitch
    from tortoise_tts_amd import stages
    makers = (("tt_f0_track", stages.F0Stage(SAMPLES, max_clips=16), f0_call), ("tt_sil_find", stages.SilenceStage(SAMPLES, max_clips=16), sil_call),
              ("tt_tsm_stretch_0.75", stages.TimeStretchStage(SAMPLES, max_clips=16), tsm_call))
    if hasattr(makers[0][1].lib, "tt_f0v_track"):  # (a library from before the Viterbi path - the parent's, for tt_f0_track's own figure - has none)
        makers += tuple((name, stages.F0ViterbiStage(SAMPLES, max_clips=16), f0v_call(which)) for name, which in (
            ("tt_f0v_track", "track"), ("tt_op_f0v_candidates", "candidates"), ("tt_op_f0v_path", "path")))
    bases = [long_clip(s) for s in range(4)]
    ms = {(name, n): [] for name, _, _ in makers for n in CLIPS}
    voiced = None
    for r in range(REPEATS + WARM):
        calls = [(name, n, make(st, n, np.roll(bases[r % 4], 4099 * r))) for n in CLIPS for name, st, make in makers]
        torch.cuda.synchronize()
        for name, n, (call, status, nv) in calls:  # interleaved: each of the six once per round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            assert status.cpu().tolist() == [0] * n, (name, status.cpu().tolist())
            if nv is not None and n == 1:
                voiced = int(nv[0])
            if r >= WARM:
                ms[(name, n)].append(a.elapsed_time(b))
        del calls
    res = {}
    for (name, n), v in ms.items():
        res["call_ms_%s_x%d" % (name, n)] = "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(v), min(v), max(v), len(v))
    F = pitch.frames(SAMPLES)
    GROUP = makers[0][1].lib.tt_op_f0_group()
    groups = -(-F // GROUP)
    slots = (groups - 1) * (GROUP + 3) + (F - (groups - 1) * GROUP + 3)  # the last group sums only the slots of its frames
    for n in CLIPS:
        terms = n * slots * SLOT * LAGS
        valu, lds = 1e3 * 2 * terms / VALU_LANE_OPS, 1e3 * 2 * terms / LDS_BYTES
        med = statistics.median(ms[("tt_f0_track", n)])
        res["floors_tt_f0_track_x%d" % n] = ("%d frames in %d workgroups of %d a clip, %.3e terms (%.3f x the F + 3 slots a clip needs; frame by frame is 4 F); f32 VALU floor %.4f ms, "
                                             "LDS floor %.4f ms; the call is %.1f x its VALU floor, %.1f x its LDS floor" % (
                                                 F, groups, GROUP, terms, slots / (F + 3.0), valu, lds, med / valu, med / lds))
    for n in CLIPS:
        if ("tt_f0v_track", n) in ms:  # the path launch is a chain of F frames, one wave a clip: what the call adds over tt_f0_track, a frame
            extra = statistics.median(ms[("tt_f0v_track", n)]) - statistics.median(ms[("tt_f0_track", n)])
            res["chain_tt_f0v_track_x%d" % n] = "%d frames a clip: the call is %.4f ms over tt_f0_track's, %.3f us a frame of the chain" % (F, extra, 1e3 * extra / F)
            med = statistics.median(ms[("tt_op_f0v_path", n)])
            res["chain_tt_op_f0v_path_x%d" % n] = "the path launch alone: %.3f us a frame, %.2f frames a us" % (1e3 * med / F, F / (1e3 * med))
    res["clip"] = "%d of %d frames voiced in the first clip of the last repeat (defaults: 60 .. 500 Hz, threshold 0.15, floor -50 dB)" % (voiced, F)
    for _, st, _ in makers:
        st.close()
    print("RESULT " + json.dumps(res))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_f0.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    log("# F0 tracker (tt_f0_track) on clips of %d samples (%.2f s at 24 kHz): workgroups of 256 threads, 4 lags a thread; with "
        "tt_sil_find and tt_tsm_stretch of the same samples for scale%s" % (
            SAMPLES, SAMPLES / 24000, "; library " + os.path.basename(os.environ["TORTOISE_MI355X_LIB"]) if os.environ.get("TORTOISE_MI355X_LIB") else ""))
    log("## one process, the calls interleaved, device events around each call, a fresh input buffer per repeat: <call>_x<clips per call>")
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"]
    log("$ timeout -k 10 %d python scripts/f0_time.py --child" % LIMIT)
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
