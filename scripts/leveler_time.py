"""What the streaming leveler (csrc/loudness_stream.hip) costs on a piece of a stream.  A record, not a gate.

    python scripts/leveler_time.py [--out profiles/rNN_leveler.txt] [--first-chunk] [--against OTHER_LIBRARY]

  push     ONE process: tt_lvs_push of a 40-token piece (40 960 samples at 24 kHz) and of the 60-token first piece (61 440) for 1 and 16
           sessions, ADAPT + LOOKAHEAD and FIXED + NONE, in isolation: device events around the call alone, a FRESH input buffer for every
           repeat, median and min .. max of 25 repeats after 3 warm-up pushes.  Beside each, tt_loud_normalize(LOOKAHEAD) of the same
           samples in the same run.
  trace    a few of the same pushes under `rocprofv3 --kernel-trace --stats`: the measure launch and the apply launch, each alone.
  first    --first-chunk: tts_stream's first piece on the host, with and without stream_loudness=, alternating.
  against  --against PATH: the whole-clip calls (tt_loud_measure, tt_loud_normalize in each mode) on tests/loudness_reference.py's family
           with this build and with another build of the library (the parent commit's), ONE process, the two alternating: every output
           compared byte for byte, and the calls' device times side by side.
Each child runs under its own time limit; the first failure ends the run.
"""
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stretch_time as ST  # noqa: E402  (run_child and next_round_prefix: the same protocol, the same limits)
PIECES = (("piece40", 40960), ("first60", 61440))
SESSIONS = (1, 16)
MODES = (("adapt_lookahead", 0, 1), ("fixed_none", 1, 0))
TARGET, CEILING = -16.0, 0.5
REPEATS, WARM = 25, 3


def spread(ms):
    return "median %.4f  min %.4f  max %.4f  (%d repeats)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def piece(n, seed):
    import numpy as np
    from tests import loudness_reference as R
    return np.concatenate([R.voiced(12000, 100 * seed + i) for i in range(-(-n // 12000))])[:n].astype(np.float32)


def child(timed):
    import numpy as np
    import torch
    from tests import loudness_reference as R
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    res = {}
    repeats, warm = (REPEATS, WARM) if timed else (3, 0)
    st = stages.StreamLevelStage(16, max_hops=(repeats + warm + 1) * 26)
    whole = stages.LoudnessStage(16 * 61440, max_clips=16)
    bases = [piece(61440, s) for s in range(4)]
    f = C.c_float
    for name, n_in in PIECES:
        for n in SESSIONS:
            audios = [torch.from_numpy(np.concatenate([np.roll(bases[(r + i) % 4][:n_in], 997 * i + 4099 * r) for i in range(n)])).cuda()
                      for r in range(repeats + warm)]
            arr = C.c_int * n
            y = torch.zeros(n * n_in + 1).cuda()
            for mode, steer, limit in MODES:
                for s in range(n):
                    E.check(st.lib.tt_lvs_open(st.h, s, steer, limit, f(1.0), f(TARGET), f(CEILING), f(12.0), f(24.0), f(3.0), f(12.0)))
                torch.cuda.synchronize()
                ms = []
                for r, audio in enumerate(audios):  # (the stream goes on: every push continues the one before, as a session's pieces do)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    E.check(st.lib.tt_lvs_push(st.h, n, arr(*range(n)), arr(*[n_in] * n), arr(*[0] * n), E.ptr(audio), E.ptr(y), E.stream_ptr()))
                    b.record()
                    b.synchronize()
                    if r >= warm:
                        ms.append(a.elapsed_time(b))
                res["push_ms_%s_%s_x%d" % (name, mode, n)] = spread(ms)
            if timed:
                io, ho = (torch.arange(n + 1, dtype=torch.int32).cuda() * v for v in (n_in, R.hops(n_in)))
                target, ceiling = torch.full((n,), TARGET).cuda(), torch.full((n,), CEILING).cuda()
                lufs, hop = torch.zeros(n, dtype=torch.float64).cuda(), torch.zeros(n * R.hops(n_in), dtype=torch.float64).cuda()
                tp, gain, otp = torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
                ba, br, status = (torch.full((n,), -1, dtype=torch.int32).cuda() for _ in range(3))
                P = E.ptr
                torch.cuda.synchronize()
                ms = []
                for r, audio in enumerate(audios):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    E.check(whole.lib.tt_loud_normalize(whole.h, n, P(audio), P(io), P(ho), P(target), P(ceiling), 2, P(y), P(lufs), P(tp), P(ba), P(br),
                                                        P(hop), P(gain), P(otp), P(status), E.stream_ptr()))
                    b.record()
                    b.synchronize()
                    if r >= warm:
                        ms.append(a.elapsed_time(b))
                res["whole_normalize_lookahead_ms_%s_x%d" % (name, n)] = spread(ms)
    print("RESULT " + json.dumps(res))


def first_chunk():
    """The time from the call until the first piece of tts_stream is on the host, plain and with stream_loudness=: scripts/tsstream_time.py's
    setup (synthetic weights with the stop token suppressed, bf16, 200 mel tokens, the committed prompt)."""
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
    cases = (("plain", {}), ("level", {"stream_loudness": -23.0}))
    res, ms = {}, {name: [] for name, _ in cases}
    for r in range(WARM + 10):
        for name, extra in cases:  # (alternating: both see the same machine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = tts.tts_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=1000 + r, stream_chunk_size=40,
                               overlap_wav_len=1024, verbose=False, **extra)
            first = next(g).cpu()
            t1 = time.perf_counter()
            g.close()
            if r >= WARM:
                ms[name].append(1e3 * (t1 - t0))
            res["first_chunk_samples_" + name] = str(first.shape[0])
    for name in ms:
        res["first_chunk_ms_" + name] = spread(ms[name])
    res["first_chunk_ms_difference"] = "%.3f (medians, level against plain)" % (statistics.median(ms["level"]) - statistics.median(ms["plain"]))
    print("RESULT " + json.dumps(res))


def against(other):
    """tt_loud_measure / tt_loud_normalize of the family through two builds of the library, alternating, with plain ctypes (the other
    build need not have this build's entry points)."""
    import numpy as np
    import torch
    from tests import loudness_reference as R
    from tortoise_tts_amd import engine as E
    vp, i = C.c_void_p, C.c_int
    libs = {}
    for name, path in (("this", E.LIB_PATH), ("other", os.path.abspath(other))):
        lib = C.CDLL(path)
        lib.tt_loud_create.argtypes, lib.tt_loud_create.restype = [i, i, C.POINTER(vp)], i
        lib.tt_loud_measure.argtypes, lib.tt_loud_measure.restype = [vp, i] + [vp] * 10, i
        lib.tt_loud_normalize.argtypes, lib.tt_loud_normalize.restype = [vp, i, vp, vp, vp, vp, vp, i] + [vp] * 10, i
        h = vp()
        assert lib.tt_loud_create(4 * 1048576, 32, C.byref(h)) == 0
        libs[name] = (lib, h)
    fam = R.family_reference()
    n = len(fam)
    lens = [len(x) for x, _, _, _ in fam]
    audio = torch.from_numpy(np.concatenate([x for x, _, _, _ in fam] + [np.zeros(1, np.float32)])).cuda()
    io = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32).cuda()
    ho = torch.tensor(np.concatenate(([0], np.cumsum([R.hops(m) for m in lens]))), dtype=torch.int32).cuda()
    target = torch.tensor([T for _, T, _, _ in fam], dtype=torch.float32).cuda()
    ceiling = torch.tensor([c for _, _, c, _ in fam], dtype=torch.float32).cuda()
    P = lambda t: t.data_ptr()
    res, ms, digest = {}, {}, {}
    for r in range(WARM + 15):
        for what in ("measure", "none", "scale", "lookahead"):
            for name in (("this", "other") if r % 2 == 0 else ("other", "this")):  # (alternating, and in alternating order)
                lib, h = libs[name]
                y = torch.full((int(io[-1]) + 1,), -7.0).cuda()
                lufs, hop = torch.full((n,), -7.0, dtype=torch.float64).cuda(), torch.full((int(ho[-1]) + 1,), -7.0, dtype=torch.float64).cuda()
                tp, gain, otp = (torch.full((n,), -7.0).cuda() for _ in range(3))
                ba, br, status = (torch.full((n,), -7, dtype=torch.int32).cuda() for _ in range(3))
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if what == "measure":
                    rc = lib.tt_loud_measure(h, n, P(audio), P(io), P(ho), P(lufs), P(tp), P(ba), P(br), P(hop), P(status), None)
                else:
                    rc = lib.tt_loud_normalize(h, n, P(audio), P(io), P(ho), P(target), P(ceiling), ("none", "scale", "lookahead").index(what), P(y),
                                               P(lufs), P(tp), P(ba), P(br), P(hop), P(gain), P(otp), P(status), None)
                b.record()
                b.synchronize()
                assert rc == 0
                if r >= WARM:
                    ms.setdefault((what, name), []).append(a.elapsed_time(b))
                d = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in (y, lufs, hop, tp, gain, otp, ba, br, status))).hexdigest()
                assert digest.setdefault((what, name), d) == d  # every repeat gives the same bytes
    for what in ("measure", "none", "scale", "lookahead"):
        same = digest[(what, "this")] == digest[(what, "other")]
        res["family_%s_outputs" % what] = "%s  sha256 %s" % ("BYTE-IDENTICAL in both builds" if same else "DIFFERENT", digest[(what, "this")][:16])
        for name in ("this", "other"):
            res["family_%s_ms_%s_build" % (what, name)] = spread(ms[(what, name)])
    print("RESULT " + json.dumps(res))
    assert all(digest[(w, "this")] == digest[(w, "other")] for w in ("measure", "none", "scale", "lookahead"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--first-chunk", action="store_true")
    ap.add_argument("--against")
    ap.add_argument("--child", choices=("time", "trace", "first", "against"))
    a = ap.parse_args()
    if a.child:
        return {"time": lambda: child(True), "trace": lambda: child(False), "first": first_chunk, "against": lambda: against(a.against)}[a.child]()
    out = a.out or os.path.join(ROOT, "profiles", ST.next_round_prefix() + "_leveler.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# streaming leveler (tt_lvs_push: a measure launch and an apply launch) at piece size, target %.0f LUFS, ceiling %.1f" % (TARGET, CEILING))
    log("## one process, device events around the call, a fresh input buffer per repeat: <piece>_<mode>_x<sessions per call>")
    ST.run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every push above, three each - the two launches, each alone")
    with tempfile.TemporaryDirectory() as d:
        ST.run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "lvs_" in row:
                    log(row)
    if a.first_chunk:
        log("## tts_stream's first piece on the host, plain and with stream_loudness=-23, alternating")
        ST.run_child(me + ["--child", "first"], log)
    if a.against:
        log("## the whole-clip calls on the family, this build and the parent commit's build alternating in one process")
        ST.run_child(me + ["--child", "against", "--against", a.against], log)


if __name__ == "__main__":
    main()
