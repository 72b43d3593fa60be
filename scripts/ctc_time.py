"""What the CTC forced alignment (csrc/ctc_align.hip) costs beside the aligner forward that produces its logits.  A record, not a gate.

    python scripts/ctc_time.py [--out profiles/rNN_ctc_align.txt]      (default: the next free round prefix)

  time     ONE process: tt_ctc_align at T = 500 and 1499 frames, L = 100 and 400 tokens, 1 and 16 clips per call (warm median of 30 calls,
           device events), then tt_w2v_run (24 x 1024, fp16, random weights) on clips of the same frame counts; the alignment's share of
           the forward.  Also the worst |error| / bound ratios of score and conf over the accuracy families of tests/test_gpu_ctc.py.
  trace    the same alignments, three calls each, under `rocprofv3 --kernel-trace --stats`: per-kernel times of the three K forms.
Each child runs under its own time limit; the first failure ends the run.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(T, L) for T in (500, 1499) for L in (100, 400)]
CLIPS = (1, 16)
LIMIT = 400


def samples_for(frames):
    """24 kHz samples of a clip that gives exactly `frames` frames."""
    from tortoise_tts_amd import align
    n = frames * 480
    while align.frames_for(n) < frames:
        n += 24
    return n


def events_ms(fn, warm, calls):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def ctc_call(st, T, L, n):
    """A closure that makes one tt_ctc_align call over n planted-path clips of T frames and L tokens (inputs resident on the device)."""
    import numpy as np
    import torch
    from tests import ctc_reference as CR
    from tortoise_tts_amd import engine as E
    clips = [CR.planted_clip(7 * T + L + i, tmin=T, tmax=T) for i in range(n)]
    rng = np.random.default_rng(T + L)
    clips = [(x, CR.random_targets(rng, L, 32, 0)) for x, _ in clips]  # (the planted path is of another target: a hard, not a peaked, input)
    lg = torch.from_numpy(np.concatenate([x for x, _ in clips])).cuda()
    fo = torch.arange(n + 1, dtype=torch.int32).cuda() * T
    to = torch.arange(n + 1, dtype=torch.int32).cuda() * L
    tg = torch.tensor([t for _, g in clips for t in g], dtype=torch.int32).cuda()
    path, spans = torch.zeros(n * T, dtype=torch.int32).cuda(), torch.zeros(n * L * 2, dtype=torch.int32).cuda()
    conf, score, status = torch.zeros(n * L).cuda(), torch.zeros(n).cuda(), torch.full((n,), -1, dtype=torch.int32).cuda()

    def call():
        E.check(st.lib.tt_ctc_align(st.h, n, E.ptr(lg), E.ptr(fo), E.ptr(tg), E.ptr(to), E.ptr(path), E.ptr(spans), E.ptr(conf), E.ptr(score),
                                    E.ptr(status), E.stream_ptr()))
    call()
    assert status.cpu().tolist() == [0] * n
    return call


def child_time(with_forward):
    import torch
    from tests import w2v_reference as R
    from tortoise_tts_amd import engine as E, stages
    res = {}
    st = stages.CtcAlignStage(32, 0, max_frames=1499, max_clips=16)
    calls, warm = (30, 5) if with_forward else (3, 0)
    for T, L in SHAPES:
        for n in CLIPS:
            res["ctc_ms_T%d_L%d_x%d" % (T, L, n)] = round(events_ms(ctc_call(st, T, L, n), warm, calls), 4)
    st.close()
    if with_forward:
        cfg = R.large_config()
        m = R.hf_model(cfg, seed=11)
        src = (cfg, {k: v.detach() for k, v in m.state_dict().items()}, R.VOCAB, R.TOK_CFG)
        del m
        al = stages.AlignerStage(src, "cuda", E.TT_F16, max_samples=24000 * 30 + 480)
        for T in sorted({T for T, _ in SHAPES}):
            clip = R.test_clip(samples_for(T) / 24000.0 + 0.01)[:, :samples_for(T)].contiguous().cuda()
            assert al.frames(clip.shape[-1]) == T
            res["w2v_ms_T%d" % T] = round(events_ms(lambda: al.run(clip, logits=True), 3, 10), 3)
        al.close()
        for T, L in SHAPES:
            for n in CLIPS:  # the aligner runs clip by clip: n forwards beside one alignment call
                res["share_T%d_L%d_x%d" % (T, L, n)] = round(res["ctc_ms_T%d_L%d_x%d" % (T, L, n)] / (n * res["w2v_ms_T%d" % T]), 5)
        res.update(child_accuracy())
    print("RESULT " + json.dumps(res))


def child_accuracy():
    """Worst |error| / bound of score and conf over the 40 + 40 clips of the GPU test's accuracy families."""
    import torch
    from tests import ctc_reference as CR
    from tortoise_tts_amd import stages
    st = stages.CtcAlignStage(32, 0, max_frames=1499, max_clips=16)
    out = {}
    for name, fam in (("random", CR.random_clip), ("planted", CR.planted_clip)):
        clips = [fam(seed) for seed in range(40)]
        res = st.align_many([torch.from_numpy(x) for x, _ in clips], [tg for _, tg in clips])
        ws = wc = 0.0
        same = 0
        for r, (x, tg) in zip(res, clips):
            ref = CR.viterbi(x, tg, 0)
            path = r["path"].numpy()
            same += path.tolist() == ref["path"].tolist()
            spans, conf64 = CR.spans_conf(path, ref["lp"], tg)
            ws = max(ws, abs(r["score"] - CR.path_score(ref["lp"], path, tg, 0)) / CR.score_bound(len(x), ref["lp"], x, CR.labels(tg, 0)[path]))
            wc = max(wc, float((abs(r["conf"].numpy() - conf64) / CR.conf_bound(ref["lp"], x, tg, spans)).max()))
        out.update({name + "_paths_equal_fp64": "%d of 40" % same, name + "_worst_score_error_over_bound": round(ws, 4),
                    name + "_worst_conf_error_over_bound": round(wc, 4)})
    st.close()
    return out


def run_child(args, log):
    cmd = ["timeout", "-k", "10", str(LIMIT)] + args
    log("$ " + " ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        log(r.stdout[-2000:] + r.stderr[-4000:])
        log("exit status %d: the run ends here" % r.returncode)
        sys.exit(1)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            for k, v in json.loads(line[7:]).items():
                log("%-40s %s" % (k, v))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("time", "trace"))
    a = ap.parse_args()
    if a.child:
        return child_time(a.child == "time")
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_ctc_align.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    me = [sys.executable, os.path.abspath(__file__)]
    log("# CTC forced alignment (tt_ctc_align) beside the aligner forward (tt_w2v_run, 24 x 1024, fp16); vocab 32; times in ms, warm medians")
    log("## one process: ctc_ms_T<frames>_L<tokens>_x<clips per call>, w2v_ms_T<frames> (one clip), share = ctc / (clips * w2v)")
    run_child(me + ["--child", "time"], log)
    log("## rocprofv3 --kernel-trace --stats: every shape above, three calls each")
    with tempfile.TemporaryDirectory() as d:
        run_child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + me + ["--child", "trace"], log)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = open(path).read().splitlines()
            log(rows[0])
            for row in rows[1:]:
                if "ctc_" in row:
                    log(row)


if __name__ == "__main__":
    main()
